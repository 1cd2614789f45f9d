"""The problems of the sparse scorer's update and SLIM hand-off tests (test_spscorer_update_gpu.py, test_slim_hand_off_*.py):
hand_off_cases.URM_TRAIN (300 x 200, a user without a profile, an item nobody has) and the same cut to its first 199 columns -- a row
count of B that the four rows of a csr_adopt_kernel workgroup do not divide -- plus the weight matrices of the update tests."""
import numpy as np
import scipy.sparse as sps

from hand_off_cases import N_ITEMS, N_USERS, URM_NEGATIVE, URM_TEST, URM_TRAIN, candidate_rows

PROBLEMS = {N_ITEMS: dict(train=URM_TRAIN, test=URM_TEST, negative=URM_NEGATIVE, candidates=candidate_rows())}
_CUT = N_ITEMS - 1
PROBLEMS[_CUT] = {name: sps.csr_matrix(m[:, :_CUT]) for name, m in PROBLEMS[N_ITEMS].items()}
ITEM_COUNTS = (N_ITEMS, _CUT)
ALL_USERS = np.arange(N_USERS)


def weights(seed, density, n=N_ITEMS, long_row=None, row_of_64=None, empty_row=None, empty_column=None, shuffle_rows=False):
    """A random sparse n x n float32 matrix whose values are non-zero multiples of 1/64 in [-4, 4]: with ratings 1 .. 5 every product is
    a multiple of 1/64 below 2^5 and every score a sum of at most a few thousand of them -- an exact float32 sum in any order.
    long_row / row_of_64: rows given more than 64 (2 * 64 + 7) / exactly 64 cells; shuffle_rows: every row's cells in a random order."""
    rng = np.random.default_rng(seed)
    mask = rng.random((n, n)) < density
    columns = np.setdiff1d(np.arange(n), [] if empty_column is None else [empty_column])
    for row, count in ((long_row, 2 * 64 + 7), (row_of_64, 64)):
        if row is not None:
            mask[row] = False
            mask[row, rng.choice(columns, count, replace=False)] = True
    if empty_row is not None:
        mask[empty_row] = False
    if empty_column is not None:
        mask[:, empty_column] = False
    steps = rng.integers(1, 257, (n, n)) * rng.choice([-1, 1], (n, n))
    W = sps.csr_matrix(np.where(mask, steps / 64.0, 0.0).astype(np.float32))
    W.sort_indices()
    if shuffle_rows:
        for r in range(n):
            s, e = W.indptr[r], W.indptr[r + 1]
            order = rng.permutation(e - s)
            W.indices[s:e], W.data[s:e] = W.indices[s:e][order], W.data[s:e][order]
        W.has_sorted_indices = False
    return W


W1 = weights(1, 0.05, long_row=3, empty_row=8, empty_column=5)
W2 = weights(2, 0.12, row_of_64=11, empty_row=0, empty_column=N_ITEMS - 1)         # more cells than W1: the spare buffers grow
W3 = weights(3, 0.02, long_row=N_ITEMS - 1, row_of_64=64, empty_row=7, empty_column=0)   # fewer
W_EMPTY = sps.csr_matrix((N_ITEMS, N_ITEMS), dtype=np.float32)
assert W3.nnz < W1.nnz < W2.nnz and W_EMPTY.nnz == 0
assert np.diff(W1.indptr)[3] == 135 and np.diff(W2.indptr)[11] == 64 and np.diff(W3.indptr)[64] == 64 and np.diff(W3.indptr)[-1] == 135
