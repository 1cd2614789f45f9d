"""The one small problem of the validation hand-off tests (test_validation_hand_off_*.py): a 300 x 200 URM of about 3 000 cells with
a user that has no profile and an item nobody has, a train / test split of it, sampled negatives and fixed candidate rows."""
import numpy as np
import scipy.sparse as sps

N_USERS, N_ITEMS = 300, 200
EMPTY_USER, UNSEEN_ITEM = 17, 123


def _urm():
    rng = np.random.default_rng(20241)
    X = sps.random(N_USERS, N_ITEMS, density=0.052, format="lil", dtype=np.float32, random_state=np.random.RandomState(7))
    X[EMPTY_USER, :] = 0
    X[:, UNSEEN_ITEM] = 0
    X = sps.csr_matrix(X)
    X.eliminate_zeros()
    X.data = rng.integers(1, 6, X.nnz).astype(np.float32)          # ratings 1 .. 5 (FunkSVD reads them, BPR and IALS as they like)
    X.sort_indices()
    return X


URM_ALL = _urm()


def _split():
    rng = np.random.default_rng(5)
    coo = URM_ALL.tocoo()
    test = rng.random(coo.nnz) < 0.2
    make = lambda m: sps.csr_matrix((coo.data[m], (coo.row[m], coo.col[m])), shape=URM_ALL.shape)
    return make(~test), make(test)


URM_TRAIN, URM_TEST = _split()


def _negatives(per_user=30):
    rng = np.random.default_rng(11)
    rows, cols = [], []
    for u in range(N_USERS):
        free = np.setdiff1d(np.arange(N_ITEMS), URM_ALL.indices[URM_ALL.indptr[u]:URM_ALL.indptr[u + 1]])
        cols.append(rng.choice(free, per_user, replace=False))
        rows.append(np.full(per_user, u))
    rows, cols = np.concatenate(rows), np.concatenate(cols)
    return sps.csr_matrix((np.ones(len(rows), np.float32), (rows, cols)), shape=URM_ALL.shape)


URM_NEGATIVE = _negatives()


def candidate_rows():
    """A fixed row of candidates for every user: 1 .. 40 items, the user without a profile and the item nobody has among them."""
    rng = np.random.default_rng(3)
    rows, cols = [], []
    for u in range(N_USERS):
        n = 1 + (u * 7) % 40
        cols.append(rng.choice(N_ITEMS, n, replace=False))
        rows.append(np.full(n, u))
    rows, cols = np.concatenate(rows + [[EMPTY_USER]]), np.concatenate(cols + [[UNSEEN_ITEM]])
    C = sps.csr_matrix((np.ones(len(rows), np.float32), (rows, cols)), shape=URM_ALL.shape)
    C.sum_duplicates()
    C.data[:] = 1
    return C


ALL_USERS = np.arange(N_USERS)
