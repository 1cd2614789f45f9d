"""Exact sparse scoring test helper (NumPy / SciPy only): the order contract of csrc/spexact.hip as a NumPy restatement and the
shared cases of tests/test_sparse_exact_spec.py (CPU) and tests/test_sparse_exact_gpu.py (device).

Contract: scores[u, :] is SciPy's `(A[users] @ B).toarray()` for float32 CSR operands -- every cell from
+0.0, over the stored cells (m, w) of row u of A IN STORAGE ORDER and, for each, over the stored cells (j, b) of row m of B,
s[j] = s[j] + (w * b) in float32 with the product rounded before the add.  `restate` below is that recurrence;
test_sparse_exact_spec.py pins it to the SciPy that is installed, the device tests compare with the SciPy product itself, as uint32.

Cases: values normal x 10^U(-3, 3) with both signs (order and rounding matter) or all ones; rows of A unsorted, one with an explicit
0.0 first, one with a column stored twice, one empty, profile lengths around a wavefront and a long one; rows of B shuffled, of 0, 1,
63, 64, 65 and n_items cells; score rows of 1, 65 and 1000 items, of the first width that leaves LDS and of three tiles; both operand
orders (A = URM, B = W and A = W, B = URM).
"""
import functools

import numpy as np
import scipy.sparse as sps

import ranking_cases as RC

LENGTHS = (0, 1, 2, 3, 63, 64, 65, 700)     # profile length of the first users (capped at n_mid)
EMPTY_USER = 0
ZERO_USER = 4                   # its first stored cell holds an explicit 0.0
DUPLICATE_USER = 6              # its second stored cell repeats the column of its first
B_LENGTHS = (1, 0, 63, 64, 65, None)        # None: n_items, a full row
TILE = 32256                    # columns of the exact kernel's tile: the widest row the ranking keeps in LDS
NARROW_USERS, WIDE_USERS = 40, 8
USER_BASE = 800                 # users of the user-based cases: A = W is USER_BASE x USER_BASE, the first ones are scored

# name -> (operand order, n_items, values)
CASES = {
    "item_n1": ("item", 1, "range"), "item_n65": ("item", 65, "range"), "item_n1000": ("item", 1000, "range"),
    "item_n1000_binary": ("item", 1000, "binary"),
    "user_n1": ("user", 1, "range"), "user_n65": ("user", 65, "range"), "user_n1000": ("user", 1000, "range"),
    "user_n65_binary": ("user", 65, "binary"),
    "item_first_wide": ("item", TILE + 1, "range"), "item_three_tiles": ("item", 2 * TILE + 5, "range"),
    "user_first_wide": ("user", TILE + 1, "range"), "user_three_tiles": ("user", 2 * TILE + 5, "range"),
}
WIDE_RANGE = tuple(sorted(n for n, c in CASES.items() if c[2] == "range" and c[1] > 1))
NARROW = tuple(sorted(n for n, c in CASES.items() if c[1] <= TILE))
assert not RC.fits_lds_rank(TILE + 1, 10) and RC.fits_lds_rank(TILE, 10)


def bits(a):
    """float32 array -> its uint32 view: +0.0 and -0.0 differ, NaNs compare by payload."""
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def restate(A, users, B, reverse=False, fused=False):
    """The recurrence of the contract, one user at a time; float32 (len(users), n_out).  reverse: the profile walked backwards;
    fused: the product formed exactly (float64) and rounded once with the add, as a fused multiply-add does -- the two wrong kernels
    the device tests must be able to tell from the right one."""
    assert A.dtype == np.float32 and B.dtype == np.float32
    out = np.zeros((len(users), B.shape[1]), np.float32)
    for r, u in enumerate(users):
        s = out[r]
        cells = range(A.indptr[u], A.indptr[u + 1])
        for q in (reversed(cells) if reverse else cells):
            m, w = A.indices[q], A.data[q]
            cols, vals = B.indices[B.indptr[m]:B.indptr[m + 1]], B.data[B.indptr[m]:B.indptr[m + 1]]
            if fused:
                s[cols] = (s[cols].astype(np.float64) + np.float64(w) * vals.astype(np.float64)).astype(np.float32)
            else:
                product = w * vals                  # float32 * float32: rounded to float32 ...
                s[cols] = s[cols] + product         # ... before the add (no row of B holds a column twice)
    return out


def scipy_scores(A, users, B):
    return (A[users] @ B).toarray()


def _values(rng, n, kind):
    if kind == "binary":
        return np.ones(n, np.float32)
    return (rng.normal(size=n) * 10.0 ** rng.uniform(-3, 3, n)).astype(np.float32)


def _rows(rng, lengths, n_cols, kind):
    """CSR with the given row lengths, every row's columns distinct and in a random order."""
    indptr = np.concatenate([[0], np.cumsum(lengths)]).astype(np.int32)
    indices = np.concatenate([rng.permutation(n_cols)[:n] if 2 * n > n_cols else rng.choice(n_cols, n, replace=False) for n in lengths]
                             + [np.empty(0, np.int64)]).astype(np.int32)
    M = sps.csr_matrix((_values(rng, len(indices), kind), indices, indptr), shape=(len(lengths), n_cols))
    assert M.dtype == np.float32 and (max(lengths) <= 3 or not M.has_sorted_indices)
    return M


def _profiles(rng, n_rows, n_cols, kind, other_lengths):
    """A: the first rows have LENGTHS (capped), one explicit zero, one duplicated column; the others `other_lengths`."""
    lengths = [min(n, n_cols) for n in LENGTHS] + list(other_lengths[:n_rows - len(LENGTHS)])
    A = _rows(rng, lengths, n_cols, kind)
    A.data[A.indptr[ZERO_USER]] = 0.0
    if lengths[DUPLICATE_USER] >= 2:
        A.indices[A.indptr[DUPLICATE_USER] + 1] = A.indices[A.indptr[DUPLICATE_USER]]
    A.has_canonical_format = False
    return A


def _b_lengths(n_rows, n_cols, sparse):
    """Row lengths of B: the cycle of B_LENGTHS; sparse (wide rows): one full row only, at row 5."""
    out = []
    for r in range(n_rows):
        n = B_LENGTHS[r % len(B_LENGTHS)]
        if n is None:
            n = n_cols if (not sparse or r == 5) else 2
        out.append(min(n, n_cols))
    return out


@functools.lru_cache(maxsize=None)
def case(name):
    """dict(A, B, seen, users, n_items): the scorer's operands (float32 CSR), the seen matrix (the URM) and the users to score."""
    order, n_items, kind = CASES[name]
    rng = np.random.default_rng(20261020 + sum(name.encode()) * 977 + n_items)
    wide = n_items > TILE
    n_scored = WIDE_USERS if wide else NARROW_USERS
    if order == "item":         # A = URM (n_scored x n_items), B = W (n_items x n_items)
        A = _profiles(rng, n_scored, n_items, kind, list(rng.integers(0, min(n_items, 40) + 1, n_scored)))
        B = _rows(rng, _b_lengths(n_items, n_items, wide), n_items, kind)
        seen = A
    else:                       # A = W (USER_BASE x USER_BASE), B = URM (USER_BASE x n_items)
        A = _profiles(rng, USER_BASE, USER_BASE, kind, list(rng.integers(0, 4, USER_BASE)))
        B = _rows(rng, _b_lengths(USER_BASE, n_items, wide), n_items, kind)
        seen = B
    assert not B.has_sorted_indices or n_items <= 2
    return dict(A=A, B=B, seen=seen, users=np.arange(n_scored, dtype=np.int32), n_items=n_items)


def some_mask(n_items, seed):
    allowed = (np.random.default_rng(seed).random(n_items) < 0.7).astype(np.uint8)
    allowed[:2] = (0, 1)[:n_items]
    return allowed


def exact_lists(filtered, cutoff):
    """The tie rule on filtered float32 rows: np.lexsort((ids, -scores)) cut at the cutoff, -inf cells never listed, -1 padded."""
    out = np.full((len(filtered), cutoff), -1, np.int32)
    ids = np.arange(filtered.shape[1])
    for r, row in enumerate(filtered):
        order = np.lexsort((ids, -row))
        k = min(cutoff, int((row > -np.inf).sum()))
        out[r, :k] = order[:k]
    return out
