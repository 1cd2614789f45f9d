"""EASE_R with its Gram step on MI355X.

The reference (EASE_R/EASE_R_Recommender.py:55-65) asks `Compute_Similarity(URM, shrink=0, topK=n_items, normalize=False,
similarity="cosine")` for X^T X and densifies it.  Here the same product comes straight from the similarity kernel's dense
(topK = 0) path.  What follows is the closed form of Steck's model, B = I - P diag(1 / diag P) with P = (X^T X + l2 I)^-1,
evaluated like the reference does it: one float32 `np.linalg.inv` on the host (a third-party LAPACK solve, outside the
hot path) and the division of every column by its own diagonal entry.

`EASE_R_MI355X_Recommender` keeps the whole closed form on the device (csrc/ease.hip): the Gram matrix goes
from the similarity handle straight into an `MI355XEase` handle, is inverted there in place by an unpivoted blocked elimination,
scaled, and reduced to its column-wise top-K; only W (or its top-K slabs) is downloaded.  That elimination is for positive-definite
matrices -- every binary or normalised URM -- and says so when the matrix is not (explicit ratings: the reference puts the
number of stored cells, not the sum of squares, on the diagonal); the fit then finishes with the host inverse of the class above
or, with `indefinite="device"`, with a pivoted float64 elimination on the device (csrc/ease_pivot.hip).
"""
import ctypes as C
import time

import numpy as np
import scipy.sparse as sps

from . import _native as N
from .recommender_base import BaseItemSimilarityMatrixRecommender, similarityMatrixTopK
from .scoring import GpuSimilarityScoringMixin, _ScoringMixin
from .similarity import Compute_Similarity_MI355X, slabs_to_csr


def _unit_l2(X, axis):
    """Scale the rows (axis=1) or columns (axis=0) of a sparse matrix to unit Euclidean length; empty ones stay empty."""
    M = (sps.csr_matrix if axis == 1 else sps.csc_matrix)(X, dtype=np.float32)
    length = np.sqrt(np.asarray(M.multiply(M).sum(axis=axis), dtype=np.float64)).ravel()
    length[length == 0.0] = 1.0
    M.data = (M.data / np.repeat(length, np.diff(M.indptr))).astype(np.float32)
    return M


class EASE_R_Recommender(BaseItemSimilarityMatrixRecommender):
    """Same surface as the reference class (EASE_R_Recommender.py:20): `fit(topK=None, l2_norm=1e3,
    normalize_matrix=False)`; `W_sparse` is the dense n_items x n_items weight matrix when topK is None, otherwise its
    column-wise top-K (`similarityMatrixTopK`) as a csr_matrix."""

    RECOMMENDER_NAME = "EASE_R_Recommender"

    def __init__(self, URM_train, verbose=True):
        super(EASE_R_Recommender, self).__init__(URM_train, verbose=verbose)

    def _gram_matrix(self):
        """X^T X with a zero diagonal, float32, from the device."""
        builder = Compute_Similarity_MI355X(self.URM_train, topK=0, shrink=0, normalize=False, similarity="cosine")
        try:
            gram = builder.compute_similarity()
            self.similarity_stats = builder.stats()
        finally:
            builder.close()
        return gram

    def fit(self, topK=None, l2_norm=1e3, normalize_matrix=False, verbose=True):
        self.verbose = verbose
        if normalize_matrix:                    # unit rows first, then unit columns of the result (:47-51)
            self.URM_train = sps.csr_matrix(_unit_l2(_unit_l2(self.URM_train, axis=1), axis=0))
        gram = self._gram_matrix()
        n_items = gram.shape[0]
        on_diagonal = slice(None, None, n_items + 1)             # stride of the diagonal in the flattened matrix
        # the diagonal of X^T X is taken as the number of stored cells of each item (:63), plus the ridge term
        gram.flat[on_diagonal] = np.diff(self.URM_train.tocsc().indptr) + l2_norm
        precision = np.linalg.inv(gram)
        weights = precision / -precision.diagonal()              # column j over -P[j, j]
        weights.flat[on_diagonal] = 0.0
        if topK is None:
            self.W_sparse = weights
        else:
            self.W_sparse = sps.csr_matrix(similarityMatrixTopK(weights, k=topK, verbose=False))

    def _compute_item_score(self, user_id_array, items_to_compute=None):
        """profiles . W for a dense or a sparse W; items outside `items_to_compute` get -inf."""
        scores = self.URM_train[user_id_array] @ self.W_sparse
        scores = scores.toarray() if sps.issparse(scores) else np.asarray(scores)
        if items_to_compute is None:
            return scores
        masked = np.full(scores.shape, -np.inf, dtype=np.float32)
        masked[:, items_to_compute] = scores[:, items_to_compute]
        return masked


class MI355XEase(N.Handle):
    """An n_items x n_items float32 matrix in HBM with the steps of the closed form: fill, invert in place (symmetric
    positive-definite input only: anything else raises FloatingPointError), weights, column-wise top-K."""
    _PREFIX = "mi355rec_ease"

    def __init__(self, n_items):
        self.n_items = int(n_items)
        self._create(self.n_items)

    def set_gram_from(self, similarity):
        """The matrix <- X^T X (zero diagonal) of a `Compute_Similarity_MI355X` built with topK=0, shrink=0, normalize=False; nothing
        crosses PCIe."""
        if not similarity._h:
            raise ValueError("the similarity handle is closed")
        self._call("set_gram_from_sim", similarity._h)

    def _square(self, G):
        G = N.as_f32(G)
        if G.shape != (self.n_items, self.n_items):
            raise ValueError("the matrix must be %d x %d, got %r" % (self.n_items, self.n_items, G.shape))
        return G

    def set_matrix(self, G):
        G = self._square(G)
        self._call("set_matrix", N.ptr(G), self.n_items)

    def get_matrix(self):
        G = np.empty((self.n_items, self.n_items), np.float32)
        self._call("get_matrix", N.ptr(G), self.n_items)
        return G

    def set_diagonal(self, diagonal):
        d = N.as_f32(diagonal)
        if d.shape != (self.n_items,):
            raise ValueError("the diagonal must have %d entries, got %r" % (self.n_items, d.shape))
        self._call("set_diagonal", N.ptr(d))

    def invert(self, pivoted=False):
        """The matrix <- its inverse.  pivoted=False: the unpivoted float32 elimination, positive-definite input only.  pivoted=True:
        partial pivoting in float64 (csrc/ease_pivot.hip) for any non-singular matrix; FloatingPointError when it is singular,
        NotImplementedError -- the matrix untouched -- when the float64 working copy does not fit the device."""
        self._call("invert_pivoted" if pivoted else "invert")

    def pivot_info(self):
        """Of the last invert(pivoted=True): swaps that moved a row, the smallest |pivot|, device milliseconds of pivot search + row
        swaps and of the update GEMM."""
        moved = C.c_int32()
        f = [C.c_double() for _ in range(3)]
        self._call("pivot_info", C.byref(moved), *[C.byref(x) for x in f])
        return {"moved_rows": moved.value, "min_pivot": f[0].value, "pivot_ms": f[1].value, "update_ms": f[2].value}

    def get_dense(self):
        """W = P / (-diag P) with a zero diagonal, float32 (n_items, n_items)."""
        W = np.empty((self.n_items, self.n_items), np.float32)
        self._call("get_dense", N.ptr(W), self.n_items)
        return W

    def get_topk(self, topK):
        """(idx int32, val float32) of shape (n_items, topK): per column of W its topK largest non-zero cells, value-descending,
        (-1, 0) padded.  NotImplementedError where the column or topK is beyond the in-LDS selection."""
        topK = int(topK)
        idx = np.empty((self.n_items, max(topK, 0)), np.int32)
        val = np.empty((self.n_items, max(topK, 0)), np.float32)
        self._call("get_topk", topK, N.ptr(idx), N.ptr(val))
        return idx, val

    def fit_info(self):
        i = [C.c_int32() for _ in range(3)]
        ms = [C.c_double() for _ in range(3)]
        launches = C.c_int64()
        self._call("fit_info", *[C.byref(x) for x in i + ms], C.byref(launches))
        return {"block": i[0].value, "steps": i[1].value, "failed_step": i[2].value, "invert_ms": ms[0].value, "gram_ms": ms[1].value,
                "topk_ms": ms[2].value, "launches": launches.value}


class _EASELogic:
    """Drop-in for the reference's EASE_R_Recommender (EASE_R_Recommender.py:20) with the same `fit(topK=None, l2_norm=1e3,
    normalize_matrix=False, verbose=True)` and the same `W_sparse` (float32 ndarray when topK is None, otherwise a csr_matrix).
    `fit_info` says where the inverse ran ("device", or "host" with the reason and the elimination step that refused) and where the
    model is scored ("scoring").  `dense_scoring` decides that for the dense W of topK=None: "host" (the default: the recommender
    base multiplies on the host) or "device" (MI355XDenseScorer, the same scores bit for bit).  A sparse W is
    scored by the device sparse scorer either way.  `indefinite` decides where a matrix the unpivoted elimination refuses (explicit
    ratings) is inverted: "host" (the default: float32 `np.linalg.inv`) or "device" (the pivoted float64 elimination of
    csrc/ease_pivot.hip; `fit_info["inverse"] == "device-pivoted"`, with `reason` the unpivoted refusal, `unpivoted_s` what that
    attempt cost and `pivot` the handle's pivot_info()).  A pivoted inverse that refuses -- singular, NaN, no memory for the float64
    copy -- ends on the host like the default, with `pivoted_reason` beside `reason`."""

    RECOMMENDER_NAME = "EASE_R_MI355X_Recommender"         # (saved models and logs tell the two classes apart)

    def __init__(self, URM_train, verbose=True, dense_scoring="host", indefinite="host"):
        if dense_scoring not in ("host", "device"):
            raise ValueError('dense_scoring must be "host" or "device", got {!r}'.format(dense_scoring))
        if indefinite not in ("host", "device"):
            raise ValueError('indefinite must be "host" or "device", got {!r}'.format(indefinite))
        self.indefinite = indefinite
        if dense_scoring == "device" and not isinstance(self, GpuSimilarityScoringMixin):
            raise ValueError('dense_scoring="device" needs the device-scoring mixin (reference_binding.bind(..., device_scoring=True))')
        super(_EASELogic, self).__init__(URM_train, verbose=verbose)
        self.dense_scoring = dense_scoring

    def _scoring_now(self):
        if isinstance(self, _ScoringMixin) and (self.device_scorable() or self.dense_device_scorable()):
            return "device"
        return "host"

    def fit(self, topK=None, l2_norm=1e3, normalize_matrix=False, verbose=True):
        self.verbose = verbose
        if normalize_matrix:                    # unit rows first, then unit columns of the result (:47-51)
            self.URM_train = sps.csr_matrix(_unit_l2(_unit_l2(self.URM_train, axis=1), axis=0))
        n_items = self.URM_train.shape[1]
        # the diagonal of X^T X is taken as the number of stored cells of each item (:63), plus the ridge term
        diagonal = (np.diff(self.URM_train.tocsc().indptr) + l2_norm).astype(np.float32)
        t_start = time.perf_counter()
        builder = Compute_Similarity_MI355X(self.URM_train, topK=0, shrink=0, normalize=False, similarity="cosine")
        ease = None
        try:
            ease = MI355XEase(n_items)
            ease.set_gram_from(builder)
            self.similarity_stats = builder.stats()
            ease.set_diagonal(diagonal)
            t_filled = time.perf_counter()
            weights = None
            try:
                ease.invert()
                info = dict(ease.fit_info(), inverse="device", reason="")
            except FloatingPointError as exc:
                # not positive definite.  The failed elimination has destroyed the matrix: the Gram matrix is built again (milliseconds)
                # instead of keeping a second n x n copy
                info = dict(ease.fit_info(), inverse="host", reason=str(exc))
                unpivoted_s = time.perf_counter() - t_filled
                ease.set_gram_from(builder)
                ease.set_diagonal(diagonal)
                if self.indefinite == "device":
                    info["unpivoted_s"] = unpivoted_s           # what the refused attempt cost
                    try:
                        ease.invert(pivoted=True)
                        info.update(ease.fit_info(), inverse="device-pivoted", unpivoted_failed_step=info["failed_step"], pivot=ease.pivot_info())
                    except (FloatingPointError, NotImplementedError) as pivoted_exc:       # singular, NaN, or no memory for the float64 copy
                        info["pivoted_reason"] = str(pivoted_exc)
                        ease.set_gram_from(builder)
                        ease.set_diagonal(diagonal)
            if info["inverse"] != "host":
                t_inverted = time.perf_counter()
                if topK is not None:
                    try:
                        idx, val = ease.get_topk(min(int(topK), n_items))
                        self.W_sparse = slabs_to_csr(idx, val, 0, n_items)
                    except NotImplementedError:         # a column or a topK beyond the in-LDS selection: rank the dense W on the host
                        weights = ease.get_dense()
                else:
                    self.W_sparse = ease.get_dense()         # (the attribute is the reference's: it is downloaded in either mode)
                    if self.dense_scoring == "device":       # the scorer takes the weights where they stand: no second trip over PCIe
                        self._get_dense_scorer(weights_from=ease)
                info["topk_ms"] = ease.fit_info()["topk_ms"]
            else:
                # the reference's pivoted float32 inverse finishes on the host
                gram = ease.get_matrix()
                precision = np.linalg.inv(gram)
                weights = precision / -precision.diagonal()              # column j over -P[j, j]
                weights.flat[::n_items + 1] = 0.0
                t_inverted = time.perf_counter()
                if topK is None:
                    self.W_sparse, weights = weights, None
            if weights is not None:
                self.W_sparse = sps.csr_matrix(similarityMatrixTopK(weights, k=topK, verbose=False))
        finally:
            if ease is not None:
                ease.close()
            builder.close()
        if isinstance(self, GpuSimilarityScoringMixin) and not self.dense_device_scorable():
            self.release_dense_scorer()             # (a sparse W after a dense one: n_items^2 floats of HBM go back)
        info.update(fill_s=t_filled - t_start, invert_s=t_inverted - t_filled, finish_s=time.perf_counter() - t_inverted,
                    scoring=self._scoring_now())
        self.fit_info = info

    def recommend(self, user_id_array, *args, **kwargs):
        """The device sparse scorer for a sparse W_sparse.  The dense array of topK=None goes to the device dense scorer with
        dense_scoring="device" (DESIGN section 16); otherwise it is scored by the recommender base on the host -- the device mixin,
        where the class has one, is stepped over."""
        if isinstance(self, _ScoringMixin) and not self.device_scorable() and not self.dense_device_scorable():
            return super(_ScoringMixin, self).recommend(user_id_array, *args, **kwargs)
        return super(_EASELogic, self).recommend(user_id_array, *args, **kwargs)

    _compute_item_score = EASE_R_Recommender._compute_item_score


class EASE_R_MI355X_Recommender(_EASELogic, GpuSimilarityScoringMixin, BaseItemSimilarityMatrixRecommender):
    pass
