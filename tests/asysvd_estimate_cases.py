"""The inputs of the AsySVD user-factor estimate tests (test_asysvd_estimate_*.py): the hand-off problem's URM_TRAIN and a small
adversarial CSR whose rows are stored in a shuffled, unsorted order, with a Y whose magnitudes spread over sixteen decades so that the
order of a row's additions and a fused multiply-add both reach the low bits of the result."""
from types import SimpleNamespace

import numpy as np
import scipy.sparse as sps

from recsys2019_deeplearning_evaluation_amd.matrix_factorization import _AsySVDLogic
from hand_off_cases import EMPTY_USER, URM_TRAIN

K_MAX = 256                                    # the most factors an ASY_SVD handle takes (csrc/mf_plan.h: ASY_KMAX)
K_LIST = (1, 3, 8, 63, 64, 65, K_MAX)          # one factor; an odd k below a lane group; one 16-byte pair per lane; 64 +- 1; two tiles

# ---- the adversarial CSR: 40 x 210 ------------------------------------------------------------------------------------------------------
ADV_ROWS, ADV_COLS = 40, 210
FULL_ROW, EMPTY_ROW, SINGLE_ROW = 3, 11, 20
# row -> cells: around the kernel's 64-cell chunk from both sides (50, 63, 64, 65, 200), around its 8 loads in flight (7, 8, 9) and
# every column at once; the rows not named here get 2 .. 30 cells
ADV_LENGTHS = {FULL_ROW: ADV_COLS, EMPTY_ROW: 0, SINGLE_ROW: 1, 0: 200, 1: 50, 2: 64, 4: 65, 5: 63, 6: 7, 7: 8, 8: 9, 39: 129}


def _adversarial():
    rng = np.random.default_rng(4711)
    indptr, indices, data = [0], [], []
    for r in range(ADV_ROWS):
        n = ADV_LENGTHS.get(r, int(rng.integers(2, 31)))
        cols = rng.permutation(ADV_COLS)[:n]                    # distinct columns in a shuffled order: NOT sorted
        indices.append(cols)
        data.append(rng.integers(1, 6, n))
        indptr.append(indptr[-1] + n)
    X = sps.csr_matrix((np.concatenate(data).astype(np.float32), np.concatenate(indices).astype(np.int32), np.array(indptr, np.int32)),
                       shape=(ADV_ROWS, ADV_COLS))
    assert not X.has_sorted_indices
    return X


URM_ADVERSARIAL = _adversarial()


def unsorted_copy(X, seed=99):
    """The same matrix with the cells of every row stored in a shuffled order (and the flag scipy keeps about it cleared)."""
    rng = np.random.default_rng(seed)
    indices, data = X.indices.copy(), X.data.copy()
    for r in range(X.shape[0]):
        s, e = X.indptr[r], X.indptr[r + 1]
        perm = rng.permutation(e - s)
        indices[s:e], data[s:e] = indices[s:e][perm], data[s:e][perm]
    out = sps.csr_matrix((data, indices, X.indptr.copy()), shape=X.shape)
    assert not out.has_sorted_indices
    return out


URM_TRAIN_UNSORTED = unsorted_copy(URM_TRAIN)
CASES = {"hand_off": URM_TRAIN, "hand_off_unsorted": URM_TRAIN_UNSORTED, "adversarial": URM_ADVERSARIAL}
EMPTY_ROWS = {"hand_off": EMPTY_USER, "hand_off_unsorted": EMPTY_USER, "adversarial": EMPTY_ROW}


def draw_Y(n_items, k, seed=0):
    """normal x 10^uniform(-8, 8), float64, both signs."""
    rng = np.random.default_rng(1000 * k + seed)
    return rng.standard_normal((n_items, k)) * 10.0 ** rng.uniform(-8, 8, (n_items, k))


def host_estimate(URM, Y):
    """The yardstick: _AsySVDLogic._estimate_user_factors itself (SciPy's URM.dot(Y), NumPy's row division) on a bare object."""
    return _AsySVDLogic._estimate_user_factors(SimpleNamespace(URM_train=URM), Y)


_REFERENCE = {}


def reference(case, k):
    """(Y, host estimate) of a case, computed once and shared: read-only arrays."""
    key = (case, k)
    if key not in _REFERENCE:
        X = CASES[case]
        Y = draw_Y(X.shape[1], k)
        want = host_estimate(X, Y)
        Y.setflags(write=False)
        want.setflags(write=False)
        _REFERENCE[key] = (Y, want)
    return _REFERENCE[key]
