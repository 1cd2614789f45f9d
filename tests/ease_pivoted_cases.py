"""Cases of the pivoted EASE_R inverse and a NumPy restatement of the device method (csrc/ease_pivot.hip): blocked Gauss-Jordan
elimination with partial (row) pivoting, everything in float64.  Per block column: the swaps come from an LU elimination of a
scratch copy of the panel, they are applied to whole rows, the permuted diagonal block is inverted without pivoting and the block
step of the unpivoted scheme follows; at the end the swaps are undone on the columns, last swap first."""
import functools

import numpy as np

import ease_cases as EC

ELIMINATION_BOUND = 1e-7        # of max |W64|, restatement in float64 (largest measured 4.2e-9)
ROUNDED_BOUND = 1e-6            # the same after W is rounded to float32 (three float32 roundings per cell: 1.8e-7)
BLOCKS = (64, 128)


def panel_swaps(panel, first):
    """LU elimination with partial pivoting of a copy of `panel` (rows first .. n - 1 of the block column): the pivot row of every
    column, the largest |value| with ties towards the lowest row (a NaN counts as the largest).  FloatingPointError on a pivot that is
    0 or NaN."""
    a = np.array(panel, dtype=np.float64)
    rows, width = a.shape
    swaps = []
    for j in range(min(rows, width)):
        mag = np.abs(a[j:, j])
        p = j + (int(np.flatnonzero(np.isnan(mag))[0]) if np.isnan(mag).any() else int(np.argmax(mag)))
        pivot = a[p, j]
        if not abs(pivot) > 0.0:
            raise FloatingPointError("pivot %r in column %d" % (pivot, first + j))
        if p != j:
            a[[j, p]] = a[[p, j]]
        swaps.append((first + j, first + p, abs(pivot)))
        a[j + 1:, j + 1:] -= np.outer(a[j + 1:, j] / pivot, a[j, j + 1:])
    return swaps


def _diagonal_block_inverse(block, step):
    a = np.array(block, dtype=np.float64)
    for j in range(len(a)):
        p = a[j, j]
        if not abs(p) > 0.0:
            raise FloatingPointError("pivot %r in elimination step %d" % (p, step))
        inv = 1.0 / p
        col, row = a[:, j].copy(), a[j, :] * inv
        a -= np.outer(col, row)
        a[j, :] = row
        a[:, j] = -col * inv
        a[j, j] = inv
    return a


def pivoted_inverse_f64(G, block, info=None):
    """G^-1 by the device's method, float64 throughout.  `info`, a dict, receives the number of swaps that moved a row and the
    smallest |pivot|."""
    A = np.array(G, dtype=np.float64)
    n = len(A)
    order = np.arange(n)                                    # order[i]: the row of G that stands in row i
    moved, smallest = 0, np.inf
    for step, k0 in enumerate(range(0, n, block)):
        k1 = min(n, k0 + block)
        for g, p, mag in panel_swaps(A[k0:, k0:k1], k0):
            smallest = min(smallest, mag)
            if p != g:
                A[[g, p]] = A[[p, g]]
                order[[g, p]] = order[[p, g]]
                moved += 1
        D = _diagonal_block_inverse(A[k0:k1, k0:k1], step)
        C = A[:, k0:k1].copy()
        R = D @ A[k0:k1, :]
        A -= C @ R
        A[k0:k1, :] = R
        A[:, k0:k1] = -(C @ D)
        A[k0:k1, k0:k1] = D
    if info is not None:
        info.update(moved=moved, smallest_pivot=smallest)
    out = np.empty_like(A)
    out[:, order] = A                                       # (P G)^-1 = G^-1 P^T: column order[l] of G^-1 is column l of what was computed
    return out


def restated_weights(G, block):
    return EC.weights_from_precision(pivoted_inverse_f64(G, block))


def symmetric_sizes(block):
    return [1, 2, block - 1, block, block + 1, 2 * block + 3, 5 * 128 + 7]


def random_symmetric(n, seed=0):
    """(M + M^T) / 2 with M standard normal float32 (n x n), seeded: symmetric indefinite."""
    M = np.random.RandomState(2000 * seed + n).standard_normal((n, n)).astype(np.float32)
    return ((M + M.T) / 2).astype(np.float32)


@functools.lru_cache(maxsize=None)
def real_mid_gram():
    """The 1 111-item explicit-rating case: named_urm("ml1m", "real", scale=0.3) with l2 = 1."""
    return EC.gram_f32(EC.urm("real", 0.3), 1.0)


MID_CASE = ("ml1m-0.3-real-l2=1", dict(topK=None, l2_norm=1.0, normalize_matrix=False))


def fit_cases():
    """name -> (URM, fit keywords) of the explicit-rating fits: both indefinite cases of ease_cases and the 1 111-item one."""
    out = dict(EC.indefinite_cases())
    out[MID_CASE[0]] = (EC.urm("real", 0.3), MID_CASE[1])
    return out


@functools.lru_cache(maxsize=None)
def _matrices(block):
    out = []
    for name, (X, kw) in EC.indefinite_cases().items():
        out.append((name, EC.gram_f32(X, kw["l2_norm"], kw["normalize_matrix"])))
    out.append((MID_CASE[0], real_mid_gram()))
    for n in symmetric_sizes(block):
        out.append(("symmetric-%d" % n, random_symmetric(n)))
    return tuple(out)


def all_matrices(block):
    """(name, float32 matrix) of every indefinite case for one block size; the arrays are shared: do not modify them."""
    return _matrices(block)


@functools.lru_cache(maxsize=None)
def weights_f64_of(name, block):
    """W64 of one named matrix, computed once."""
    return EC.weights_f64(dict(_matrices(block))[name])


def scaled_permutation(n=200, seed=5):
    """A non-symmetric permutation matrix whose entries are powers of two (either sign): its inverse is exact in any precision."""
    rng = np.random.RandomState(seed)
    perm = rng.permutation(n)
    assert (perm != np.arange(n)).any() and (perm[perm] != np.arange(n)).any()
    G = np.zeros((n, n), np.float32)
    G[np.arange(n), perm] = (rng.choice([-1.0, 1.0], n) * 2.0 ** rng.randint(-6, 7, n)).astype(np.float32)
    return G


def reversal(n):
    """Ones on the anti-diagonal: every pivot comes from the far end."""
    return np.ascontiguousarray(np.eye(n, dtype=np.float32)[::-1])


def diagonally_dominant(n, seed=3):
    M = np.random.RandomState(seed).standard_normal((n, n)).astype(np.float32)
    return (M + 4.0 * n * np.eye(n, dtype=np.float32)).astype(np.float32)


def structured_matrices(block):
    """(name, float32 matrix) of the cases with an exact answer or a known swap count, for one block size."""
    return (("scaled-permutation-200", scaled_permutation()), ("reversal-%d" % (block + 1), reversal(block + 1)),
            ("reversal-%d" % (2 * block + 3), reversal(2 * block + 3)),
            ("diagonally-dominant-%d" % (2 * block + 3), diagonally_dominant(2 * block + 3)))


def exact_inverse_f32(G):
    return np.linalg.inv(G.astype(np.float64)).astype(np.float32)
