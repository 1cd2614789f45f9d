"""Shared cases of the device EASE_R tests, the float64 closed form they are measured against, and a NumPy restatement of the
device method (csrc/ease.hip): blocked Gauss-Jordan elimination without pivoting in float32, the diagonal block inverted in
float64, a pivot that is not positive refused.  The shapes are small on purpose: less than one block, one block exactly, one
cell more, several 128-cell tiles with a ragged edge."""
import functools

import numpy as np
import scipy.sparse as sps

from recsys2019_deeplearning_evaluation_amd.ease_r import _unit_l2
from recsys2019_deeplearning_evaluation_amd.synthetic import named_urm
from _util import load_golden, unpack_csr

BAR = 1e-4          # of max |W64|: the bar tests/test_ease_gpu.py sets for this model


def prepared_urm(X, normalize_matrix):
    X = sps.csr_matrix(X, dtype=np.float32)
    if normalize_matrix:
        X = sps.csr_matrix(_unit_l2(_unit_l2(X, axis=1), axis=0))
    return X


def gram_f32(X, l2_norm, normalize_matrix=False):
    """The matrix the reference inverts (EASE_R_Recommender.py:55-65), float32: X^T X with popularity + l2 on the diagonal.  Every
    cell is the float64 sum of the float32 URM's products rounded ONCE to float32 -- what the device build returns (exact integer,
    fixed-point or float64 sums).  A float32 accumulation differs from it in the last bits, and on the ill-conditioned
    explicit-rating case (condition number 8e4) that alone moves the float64 closed form by 2.1e-4 of max |W|, twice the bar: it
    would not be a truth to hold anything against.  For binary URMs all three are the same integers."""
    X = prepared_urm(X, normalize_matrix)
    X64 = X.astype(np.float64)
    G = np.asarray((X64.T @ X64).toarray(), dtype=np.float64).astype(np.float32)
    np.fill_diagonal(G, (np.diff(X.tocsc().indptr) + l2_norm).astype(np.float32))
    return G


def weights_from_precision(P):
    W = P / -np.diag(P)
    np.fill_diagonal(W, 0.0)
    return W


def weights_f64(G):
    """The closed form in float64 from the float32 Gram matrix."""
    return weights_from_precision(np.linalg.inv(np.asarray(G, dtype=np.float64)))


def _diagonal_block_inverse(block, step):
    a = np.array(block, dtype=np.float64)
    for j in range(len(a)):
        p = a[j, j]
        if not p > 0.0:
            raise FloatingPointError("pivot %r in elimination step %d" % (p, step))
        inv = 1.0 / p
        col, row = a[:, j].copy(), a[j, :] * inv
        a -= np.outer(col, row)
        a[j, :] = row
        a[:, j] = -col * inv
        a[j, j] = inv
    return a.astype(np.float32)


def blocked_inverse_f32(G, block):
    """G^-1 by the device's method: per block column k, D = A[k,k]^-1 (float64), R = D A[k,:], A -= A[:,k] R, then A[k,:] = R,
    A[:,k] = -A[:,k] D, A[k,k] = D; all float32 outside the diagonal block.  FloatingPointError on a pivot <= 0 or NaN."""
    A = np.array(G, dtype=np.float32)
    n = len(A)
    for step, k0 in enumerate(range(0, n, block)):
        k1 = min(n, k0 + block)
        D = _diagonal_block_inverse(A[k0:k1, k0:k1], step)
        C = A[:, k0:k1].copy()
        R = D @ A[k0:k1, :]
        ND = -(C @ D)
        A -= C @ R
        A[k0:k1, :] = R
        A[:, k0:k1] = ND
        A[k0:k1, k0:k1] = D
    return A


def restated_weights(G, block):
    return weights_from_precision(blocked_inverse_f32(G, block))


@functools.lru_cache(maxsize=None)
def fixture():
    z, cases = load_golden("ease_r")
    return unpack_csr(z, "X"), cases, [z["W_%d" % n] for n in range(len(cases))]


@functools.lru_cache(maxsize=None)
def urm(values, scale):
    return named_urm("ml1m", values, scale=scale)


# name -> (URM, fit keywords); every one of them positive definite
def fit_cases():
    X, cases, _ = fixture()
    out = {"fixture-%d" % n: (X, kw) for n, kw in enumerate(cases) if n > 0}
    small, mid = urm("binary", 0.1), urm("binary", 0.3)
    for l2 in (1.0, 100.0):
        for topK in (None, 50):
            out["ml1m-0.1-l2=%g-topK=%s" % (l2, topK)] = (small, dict(topK=topK, l2_norm=l2, normalize_matrix=False))
    for topK in (None, 50):
        out["ml1m-0.1-normalised-l2=10-topK=%s" % topK] = (small, dict(topK=topK, l2_norm=10.0, normalize_matrix=True))
    for l2 in (1.0, 1000.0):
        for topK in (None, 50):
            out["ml1m-0.3-l2=%g-topK=%s" % (l2, topK)] = (mid, dict(topK=topK, l2_norm=l2, normalize_matrix=False))
    return out


# the cases whose matrix is symmetric INDEFINITE (explicit ratings: counts, not sums of squares, on the diagonal)
def indefinite_cases():
    X, cases, _ = fixture()
    return {"fixture-0": (X, cases[0]), "ml1m-0.1-real-l2=100": (urm("real", 0.1), dict(topK=None, l2_norm=100.0, normalize_matrix=False))}


def slice_sizes(block):
    return [1, 2, block - 1, block, block + 1, 2 * block]


def slice_urm(n):
    return sps.csr_matrix(urm("binary", 0.1)[:, :n])


def random_spd_sizes(block):
    return [1, 2, block - 1, block, block + 1, 2 * block + 3, 5 * 128 + 7]


def random_spd(n, seed=0):
    """G = M^T M + n I with M standard normal float32 (n x n), seeded."""
    M = np.random.RandomState(1000 * seed + n).standard_normal((n, n)).astype(np.float32)
    return (M.T @ M + n * np.eye(n, dtype=np.float32)).astype(np.float32)


def all_gram_matrices(block):
    """(name, float32 matrix) of every positive-definite case above for one block size."""
    seen = set()
    for name, (X, kw) in fit_cases().items():
        key = (id(X), kw["l2_norm"], kw["normalize_matrix"])
        if key not in seen:
            seen.add(key)
            yield name, gram_f32(X, kw["l2_norm"], kw["normalize_matrix"])
    for n in slice_sizes(block):
        yield "slice-%d" % n, gram_f32(slice_urm(n), 1.0)
    for n in random_spd_sizes(block):
        yield "spd-%d" % n, random_spd(n)
