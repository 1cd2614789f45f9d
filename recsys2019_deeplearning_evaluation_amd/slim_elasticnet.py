"""SLIM ElasticNet on MI355X: host front-end of the slimen_* entry points of libmi355rec.so.

Mirrors SLIMElasticNetRecommender (SLIM_ElasticNet/SLIMElasticNetRecommender.py:41-149), which fits one sklearn ElasticNet per
item on the CPU.  With fit_intercept=False sklearn's sparse coordinate descent is coordinate descent on the Gram matrix X^T X, one
matrix for all targets: the device builds it once, then solves every target in its own workgroup with the reference's random
coordinate sequence.  The per-target solver seeds come from NumPy's global RandomState exactly as the
reference draws them, so `np.random` is left where the reference's fit leaves it.
"""
import ctypes as C
import sys
import time
import warnings

import numpy as np
import scipy.sparse as sps

from . import _native as N
from .recommender_base import BaseItemSimilarityMatrixRecommender, check_matrix
from .scoring import GpuSimilarityScoringMixin

RAND_R_MAX = 2 ** 31 - 1          # sklearn/utils/_random.pxd: the bound of the per-fit seed draw (_cd_fast.pyx rng.randint(0, RAND_R_MAX))

try:
    from sklearn.exceptions import ConvergenceWarning
except ImportError:               # sklearn is not needed on the device side
    class ConvergenceWarning(UserWarning):
        """Stand-in for sklearn.exceptions.ConvergenceWarning."""


def _biggest_unit(seconds):
    value, unit = float(seconds), "sec"
    for factor, name in ((60, "min"), (60, "hour"), (24, "day"), (365, "year")):
        if value / factor < 1.0:
            break
        value, unit = value / factor, name
    return value, unit


class SLIMElasticNet_MI355X_Fit(N.Handle):
    """One Gram matrix on the device and fits of item ranges against it (multi-GPU sharding would hand each rank a range)."""
    _PREFIX = "mi355rec_slimen"

    def __init__(self, URM_train):
        X, arrays = N.both_layouts(URM_train)
        self.n_users, self.n_items = X.shape
        self._create(self.n_users, self.n_items, *[N.ptr(a) for a in arrays])

    def fit_range(self, start, end, seeds, alpha, l1_ratio, positive_only, topK, max_iter=100, tol=1e-4):
        """Fits targets [start, end); returns (rows, values, counts, n_iter, converged) with rows / values (end - start, slots).
        topK = -1 keeps every nonzero coefficient of each target instead of the reference's min(nnz - 1, topK)."""
        seeds = np.ascontiguousarray(seeds, dtype=np.uint32)
        assert len(seeds) == end - start
        self._call("fit", int(start), int(end), N.ptr(seeds), float(alpha), float(l1_ratio), int(bool(positive_only)), int(topK), int(max_iter),
                   float(tol))
        n = end - start
        slots = max(1, self.n_items - 1 if topK < 0 else min(int(topK), self.n_items - 1))
        counts, n_iter, conv = (np.zeros(n, np.int32) for _ in range(3))
        rows, values = np.zeros((n, slots), np.int32), np.zeros((n, slots), np.float32)
        self._call("get", N.ptr(counts), N.ptr(n_iter), N.ptr(conv), N.ptr(rows), N.ptr(values), slots)
        return rows, values, counts, n_iter, conv.astype(bool)

    def fit_info(self):
        v = [C.c_int64() for _ in range(4)]
        lds, gram_lds, gram_ms = C.c_int32(), C.c_int32(), C.c_double()
        self._call("fit_info", *[C.byref(x) for x in v], C.byref(lds), C.byref(gram_lds), C.byref(gram_ms))
        return {"changes": v[0].value, "sweeps": v[1].value, "steps": v[2].value, "gap_tests": v[3].value, "h_in_lds": bool(lds.value),
                "gram_in_lds": bool(gram_lds.value), "gram_ms": gram_ms.value}

    def gram_rows(self, row0, row1):
        """Rows [row0, row1) of the device's G = X^T X and diag[row0:row1] (tests: G is otherwise only read by the fits)."""
        rows, diag = np.zeros((row1 - row0, self.n_items), np.float32), np.zeros(row1 - row0, np.float32)
        self._call("get_gram", int(row0), int(row1), N.ptr(rows), N.ptr(diag))
        return rows, diag


def slots_to_csr(rows, values, counts, start, n_items):
    """Per-target (row, value) slots of targets start.. -> W_sparse float32 csr (n_items, n_items), W[row, target] = value."""
    keep = np.arange(rows.shape[1])[None, :] < counts[:, None]
    cols = np.broadcast_to(np.arange(start, start + len(counts))[:, None], rows.shape)[keep]
    W = sps.csr_matrix((values[keep], (rows[keep], cols)), shape=(n_items, n_items), dtype=np.float32)
    W.sort_indices()
    return W


class _SLIMElasticNetLogic:
    """Drop-in for SLIMElasticNetRecommender: same `fit` signature, same W_sparse (float32 csr, column j = the kept coefficients of
    target j), the reference's progress line, one ConvergenceWarning when targets stopped at max_iter without meeting the gap."""

    RECOMMENDER_NAME = "SLIMElasticNetRecommender"

    def __init__(self, URM_train, verbose=True):
        super(_SLIMElasticNetLogic, self).__init__(URM_train, verbose=verbose)

    def fit(self, l1_ratio=0.1, alpha=1.0, positive_only=True, topK=100):
        assert l1_ratio >= 0 and l1_ratio <= 1, \
            "{}: l1_ratio must be between 0 and 1, provided value was {}".format(self.RECOMMENDER_NAME, l1_ratio)
        self.l1_ratio = l1_ratio
        self.positive_only = positive_only
        self.topK = topK
        URM_train = check_matrix(self.URM_train, "csr", dtype=np.float32)
        n_items = URM_train.shape[1]
        start_time = time.time()
        # one seed per item, in item order, from the global RandomState (the reference's ElasticNet.fit draws them one by one)
        seeds = np.random.randint(0, RAND_R_MAX, size=n_items)
        solver = SLIMElasticNet_MI355X_Fit(URM_train)
        try:
            rows, values, counts, self.n_iter_, self.converged_ = solver.fit_range(0, n_items, seeds, alpha, l1_ratio, positive_only, topK)
            self.fit_stats = dict(solver.stats(), **solver.fit_info())
        finally:
            solver.close()
        self.W_sparse = slots_to_csr(rows, values, counts, 0, n_items)
        if not self.converged_.all():
            warnings.warn("Objective did not converge for {} of {} targets. You might want to increase the number of iterations, check the "
                          "scale of the features or consider increasing regularisation.".format(int((~self.converged_).sum()), n_items),
                          ConvergenceWarning)
        elapsed_time = time.time() - start_time
        new_time_value, new_time_unit = _biggest_unit(elapsed_time)
        self._print("Processed {} ( {:.2f}% ) in {:.2f} {}. Items per second: {:.2f}".format(
            n_items, 100.0, new_time_value, new_time_unit, float(n_items - 1) / max(elapsed_time, 1e-9)))
        sys.stdout.flush()
        sys.stderr.flush()


class SLIMElasticNetRecommender(_SLIMElasticNetLogic, GpuSimilarityScoringMixin, BaseItemSimilarityMatrixRecommender):
    pass
