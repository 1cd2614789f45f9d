"""Device scoring + ranking for factor models.

`MI355XScorer` keeps USER/ITEM factors (and biases) plus the "seen" CSR in HBM and answers the two questions the
reference's evaluation loop asks on every validation (Base/Evaluation/Evaluator.py:436):
  scores  = BaseMatrixFactorizationRecommender._compute_item_score   (BaseMatrixFactorizationRecommender.py:38-70)
  ranking = the filter + top-cutoff half of BaseRecommender.recommend (BaseRecommender.py:131-222)
`GpuScoringMixin` plugs it under `recommend()` of a BaseMatrixFactorizationRecommender without changing its signature;
`_compute_item_score` itself is left untouched (host NumPy), so either path can be checked against the other.
"""
import ctypes as C

import numpy as np
import scipy.sparse as sps

from . import _native as N


class _Scorer(N.Handle):
    """What the scorers share: recommend() over mi355rec_<kind>_recommend; n_items is the width of a score row.  Two class
    attributes tell the device evaluators (evaluation.py) how to drive a scorer."""
    EVAL_ADD = None             # its entry point of the evaluator: mi355rec_eval_<EVAL_ADD>, and <EVAL_ADD>_candidates
    EVAL_LARGE_BLOCKS = ()      # of "rows" / "candidates": the paths that keep no (users x n_items) score buffer, so that a launch
                                # takes the evaluator's FUSED_BLOCK users instead of the reference's block

    def recommend(self, user_id_array, cutoff, remove_seen=True, allowed_items=None, return_scores=False):
        """ranked: int32 (n, cutoff) with -1 padding; scores: float32 (n, n_items) with -inf for filtered items."""
        users = N.as_i32(np.atleast_1d(user_id_array))
        cutoff = int(min(cutoff, self.n_items))
        ranked = np.empty((len(users), cutoff), np.int32)
        scores = np.empty((len(users), self.n_items), np.float32) if return_scores else None
        mask = None if allowed_items is None else np.ascontiguousarray(allowed_items, dtype=np.uint8)
        self._call("recommend", N.ptr(users), len(users), cutoff, int(bool(remove_seen)), N.ptr(mask), N.ptr(ranked), N.ptr(scores))
        return ranked, scores

    def recommend_candidates(self, user_id_array, candidates_csr, cutoff, remove_seen=True, allowed_items=None):
        """Row r of `candidates_csr` (n x n_items; stored zeros dropped) holds the only items user_id_array[r] may be given: what
        recommend(..., items_to_compute=row) ranks (BaseRecommender.py:131-222), for a batch of users with a row each
        (EvaluatorNegativeItemSample, Evaluator.py:455-539).  int32 (n, cutoff), -1 padded; ties go to the lower item id."""
        users = N.as_i32(np.atleast_1d(user_id_array))
        rows = sps.csr_matrix(candidates_csr, copy=True)
        if rows.shape != (len(users), self.n_items):
            raise ValueError("candidates_csr is {}, expected {}".format(rows.shape, (len(users), self.n_items)))
        rows.eliminate_zeros()
        rows.sum_duplicates()
        rows.sort_indices()
        cutoff = int(min(cutoff, self.n_items))
        ranked = np.empty((len(users), cutoff), np.int32)
        mask = None if allowed_items is None else np.ascontiguousarray(allowed_items, dtype=np.uint8)
        indptr, indices = N.as_i32(rows.indptr), N.as_i32(rows.indices)
        self._call("recommend_candidates", N.ptr(users), len(users), N.ptr(indptr), N.ptr(indices), cutoff, int(bool(remove_seen)),
                   N.ptr(mask), N.ptr(ranked))
        return ranked


class MI355XScorer(_Scorer):
    _PREFIX = "mi355rec_scorer"
    EVAL_ADD = "add_scorer"
    EVAL_LARGE_BLOCKS = ("candidates",)

    def __init__(self, USER_factors, ITEM_factors, URM_seen, USER_bias=None, ITEM_bias=None, GLOBAL_bias=0.0):
        U, V = N.as_f32(USER_factors), N.as_f32(ITEM_factors)
        assert U.shape[1] == V.shape[1], "User and Item factors have inconsistent shape"
        self.n_users, self.n_items, self.n_factors = U.shape[0], V.shape[0], U.shape[1]
        self.use_bias = USER_bias is not None
        seen = URM_seen.tocsr()
        assert seen.shape == (self.n_users, self.n_items)
        indptr, indices = N.as_i32(seen.indptr), N.as_i32(seen.indices)
        bu = N.as_f32(USER_bias) if self.use_bias else None
        bi = N.as_f32(ITEM_bias) if self.use_bias else None
        self._create(self.n_users, self.n_items, self.n_factors, N.ptr(U), N.ptr(V), int(self.use_bias), N.ptr(bu), N.ptr(bi),
                     float(np.asarray(GLOBAL_bias)), N.ptr(indptr), N.ptr(indices))

    def update(self, USER_factors, ITEM_factors, USER_bias=None, ITEM_bias=None, GLOBAL_bias=0.0):
        U, V = N.as_f32(USER_factors), N.as_f32(ITEM_factors)
        assert U.shape == (self.n_users, self.n_factors) and V.shape == (self.n_items, self.n_factors)
        bu = N.as_f32(USER_bias) if self.use_bias else None
        bi = N.as_f32(ITEM_bias) if self.use_bias else None
        self._call("update", N.ptr(U), N.ptr(V), N.ptr(bu), N.ptr(bi), float(np.asarray(GLOBAL_bias)))

    def update_from(self, epoch_object):
        """The model a training handle holds in HBM -- a MatrixFactorization_MI355X_Epoch (BPR, FunkSVD) or an IALS_MI355X_Epoch -- into
        the scorer, device to device: the values `update(*np.float32(get_factors()), ...biases)` would upload, bit for bit, without
        the download, the host's float64 -> float32 pass and the upload.  ValueError when the shapes or the biases of the two differ
        or the handle is closed, NotImplementedError for an AsySVD handle; the scorer then keeps the model it had."""
        from .ials import IALS_MI355X_Epoch
        from .matrix_factorization import MatrixFactorization_MI355X_Epoch
        if isinstance(epoch_object, MatrixFactorization_MI355X_Epoch):
            entry = "update_from_mf"
        elif isinstance(epoch_object, IALS_MI355X_Epoch):
            entry = "update_from_ials"
        else:
            raise TypeError("update_from takes a MatrixFactorization_MI355X_Epoch or an IALS_MI355X_Epoch, got {}".format(
                type(epoch_object).__name__))
        if not epoch_object._h:
            raise ValueError("%s is closed" % type(epoch_object).__name__)
        self._call(entry, epoch_object._h)

    def score_capacity(self):
        """Cells of the device buffer for (users x n_items) score rows: 0 until a full-row recommend() has needed it; the candidate
        path never touches it."""
        cells = C.c_int64(0)
        self._call("score_capacity", C.byref(cells))
        return int(cells.value)


def _fingerprint(array):
    """Cheap content signature of a host array (256 strided elements + shape): an optimiser step moves practically every
    cell of a factor matrix, so in-place edits of an object the cache already holds are noticed without hashing it all."""
    a = np.asarray(array).ravel()
    if a.size == 0:
        return (0,)
    step = max(1, a.size // 256)
    return (np.asarray(array).shape, a[::step][:256].tobytes(), a[-1].tobytes())


def allowed_items(recommender, items_to_compute=None, remove_top_pop_flag=False, remove_custom_items_flag=False):
    """The item mask of recommend()'s filters (BaseRecommender.py:131-175: items outside `items_to_compute`, the top-popular and the
    custom ignored items are dropped) as uint8, 0 = excluded; None when no filter applies."""
    if items_to_compute is None and not remove_top_pop_flag and not remove_custom_items_flag:
        return None
    n_items = recommender.n_items
    allowed = np.zeros(n_items, np.uint8) if items_to_compute is not None else np.ones(n_items, np.uint8)
    if items_to_compute is not None:
        allowed[np.asarray(items_to_compute)] = 1
    if remove_top_pop_flag:
        allowed[recommender.filterTopPop_ItemsID] = 0
    if remove_custom_items_flag:
        allowed[recommender.items_to_ignore_ID] = 0
    return allowed


def ranked_lists(ranked):
    """(n, cutoff) ranked array -> n lists of item ids without the -1 that pads rows whose user has fewer than `cutoff` admissible
    items: rare -- one C-level tolist() otherwise, a tenth of the per-row masks' time on blocks of 1000 users."""
    return ranked.tolist() if ranked.size and int(ranked.min()) >= 0 else [row[row >= 0].tolist() for row in ranked]


class _ScoringMixin:
    """What the mixins below share: recommend() of BaseRecommender (same signature, same return values) over the ranked array of a
    device scorer, the cache of that scorer, and dropping it.  A subclass names its cache slots (`_SCORER_ATTRS`: pairs of the
    attribute that holds a scorer and the one that holds what it was built from), says which scorer serves the model now
    (`device_scorer()`) and describes each scorer to `_cached_scorer`.

    The cache rule: a slot holds STRONG references to the objects its scorer was built from and compares by identity (an id() of a
    freed object can be reused by its successor) plus a content `_fingerprint` (in-place edits).  A new scorer is built when
    URM_train is replaced or the layout changes; other values in the same layout are an `update` -- a new scorer where the scorer
    has none.  So the scorer follows early-stopping's _prepare_model_for_validation / best-model swaps and set_URM_train by itself."""
    _SCORER_ATTRS = ()
    _ASSERT_WARM_USERS = False      # the reference's cold-user assertion of the factor and non-personalized models

    def invalidate_scorer(self):
        """Forget the device copy of the model: the next recommend() uploads it again.  The caches notice REPLACED arrays (identity)
        and wholesale in-place changes (a strided 256-element fingerprint -- an optimiser step moves practically every cell); code
        that edits a few rows of a factor matrix in place (folding in cold users, say) must call this.  The package's own training
        loops call it from _prepare_model_for_validation."""
        for slot in self._SCORER_ATTRS:
            self._drop_scorer(slot)

    def _drop_scorer(self, slot):
        scorer_attr, src_attr = slot
        scorer = getattr(self, scorer_attr)
        setattr(self, scorer_attr, None)
        setattr(self, src_attr, None)
        if scorer is not None:
            scorer.close()

    def _cached_scorer(self, slot, sources, prints, build, update=None, new_layout=lambda scorer: False):
        """The scorer of `slot` for the current model.  sources: {name: object the scorer is made from}; prints: their fingerprints;
        build(): a new scorer; update(scorer): other values into the one there is (None: build again); new_layout(scorer): it
        cannot take them."""
        scorer_attr, src_attr = slot
        scorer, old = getattr(self, scorer_attr), getattr(self, src_attr)
        changed = old is None or old["print"] != prints or any(old.get(name) is not obj for name, obj in sources.items())
        if scorer is None or old is None or old["urm"] is not self.URM_train or new_layout(scorer) or (changed and update is None):
            self._drop_scorer(slot)
            scorer = build()
            setattr(self, scorer_attr, scorer)
        elif changed:
            update(scorer)
        setattr(self, src_attr, dict(sources, print=prints, urm=self.URM_train))
        return scorer

    def device_scorer(self):
        """The scorer that serves the model now -- under recommend() and under the device evaluators' fused path -- or None when the
        model has to go through the base class's recommend()."""
        raise NotImplementedError("{}: device_scorer".format(type(self).__name__))

    def _scorer_for(self, users):
        scorer = self.device_scorer()
        assert not self._ASSERT_WARM_USERS or scorer.n_users > np.max(users), \
            "{}: Cold users not allowed. Users in trained model are {}, requested prediction for users up to {}".format(
                self.RECOMMENDER_NAME, scorer.n_users, np.max(users))
        return scorer

    def recommend(self, user_id_array, cutoff=None, remove_seen_flag=True, items_to_compute=None, remove_top_pop_flag=False,
                  remove_custom_items_flag=False, return_scores=False):
        single_user = np.isscalar(user_id_array)
        users = np.atleast_1d(user_id_array)
        if cutoff is None:
            cutoff = self.URM_train.shape[1] - 1
        allowed = allowed_items(self, items_to_compute, remove_top_pop_flag, remove_custom_items_flag)
        ranked, scores = self._scorer_for(users).recommend(users, cutoff, remove_seen_flag, allowed, return_scores)
        ranking_list = ranked_lists(ranked)
        if single_user:
            ranking_list = ranking_list[0]
        return (ranking_list, scores) if return_scores else ranking_list


class GpuScoringMixin(_ScoringMixin):
    """recommend() of BaseRecommender (same signature, same return values) served by MI355XScorer, (re)built lazily from the host
    attributes USER_factors / ITEM_factors[/biases] and URM_train."""
    _scorer = None
    _scorer_src = None
    _SCORER_ATTRS = (("_scorer", "_scorer_src"),)
    _ASSERT_WARM_USERS = True

    def _get_scorer(self):
        sources, bias = {"USER_factors": self.USER_factors, "ITEM_factors": self.ITEM_factors}, {}
        if self.use_bias:
            bias = dict(USER_bias=self.USER_bias, ITEM_bias=self.ITEM_bias, GLOBAL_bias=self.GLOBAL_bias)
            sources.update(bias, GLOBAL_bias=np.asarray(self.GLOBAL_bias))
        return self._cached_scorer(
            self._SCORER_ATTRS[0], sources, [_fingerprint(a) for a in sources.values()],
            build=lambda: MI355XScorer(self.USER_factors, self.ITEM_factors, self.URM_train, **bias),    # uploads the seen CSR too
            update=lambda scorer: scorer.update(self.USER_factors, self.ITEM_factors, **bias),
            new_layout=lambda scorer: (scorer.use_bias != bool(self.use_bias)
                                       or scorer.n_factors != np.asarray(self.USER_factors).shape[1]))

    def device_scorer(self):
        return self._get_scorer()


class ValidationHandOff:
    """How an early-stopping fit hands the model to its validations: a mixin without bases for the logic classes of the recommenders
    whose training handle keeps the model in HBM (BPR-MF, FunkSVD, IALS; AsySVD carries the attribute and refuses "device").

    `validation_hand_off` (class or object attribute) is "host", the default -- every validation downloads the model into
    USER_factors / ITEM_factors[/biases] and the scorer uploads it again, as before -- or "device": the scorer is filled from the
    training handle device to device (`MI355XScorer.update_from`) and the host attributes are only marked stale.  While they are,
    `device_scorer()` returns that scorer as it is, without a fingerprint or an upload, whoever asks (recommend(), either device
    evaluator), and `_sync_host_model()` downloads the model for whatever reads the attributes on the host (_compute_item_score,
    save_model): the scorer's half, HandOffScoringMixin below, which device mode needs.  A new best model is downloaded from the
    training handle, which has not advanced since the validation.  At the end of fit the attributes are the best model, the flags
    are cleared and the scorer cache is back to its identity + fingerprint rule.

    A logic class provides `_download_model()`: the host attributes from `self.epoch_kernel`."""
    VALIDATION_HAND_OFF_MODES = ("host", "device")
    validation_hand_off = "host"
    _HAND_OFF_SUPPORTED = True      # (AsySVD: its user factors are estimated on the host from item-sized rows)
    _host_model_stale = False       # the host attributes are older than the model the scorer holds
    _scorer_current = False         # the scorer holds the training handle's model: device_scorer() returns it as it is

    def _hand_off_on_device(self):
        """True in device mode; ValueError for an unknown mode or a class that cannot hand off -- before the device is touched."""
        mode = self.validation_hand_off
        if mode not in self.VALIDATION_HAND_OFF_MODES:
            raise ValueError("{}: validation_hand_off must be one of {}, got {!r}".format(type(self).__name__,
                                                                                        self.VALIDATION_HAND_OFF_MODES, mode))
        if mode == "host":
            return False
        if not self._HAND_OFF_SUPPORTED:
            raise ValueError("{}: validation_hand_off = 'device' is not supported: the user factors of this model are estimated on "
                             "the host".format(type(self).__name__))
        if not getattr(self, "_HAND_OFF_SCORER", False):    # (set by the scorer's half: HandOffScoringMixin, HandOffSimilarityScoringMixin)
            raise ValueError("{}: validation_hand_off = 'device' needs the device scorer (HandOffScoringMixin)".format(type(self).__name__))
        return True

    def _begin_hand_off(self):
        """First thing in fit(): the mode is checked, and a device-mode fit starts without a scorer, as a host-mode one does."""
        self._end_hand_off()
        device = self._hand_off_on_device()
        if device:
            self.invalidate_scorer()
        return device

    def _end_hand_off(self):
        self._host_model_stale = False
        self._scorer_current = False

    def _download_model(self):
        raise NotImplementedError("{}: _download_model".format(type(self).__name__))


class HandOffScoringMixin(GpuScoringMixin):
    """GpuScoringMixin for the recommenders with a ValidationHandOff logic class: the scorer's half of device mode.  With the flags
    clear -- host mode, and device mode outside a fit -- every method is its parent's."""
    _HAND_OFF_SCORER = True         # what ValidationHandOff._hand_off_on_device looks for
    _host_model_stale = False
    _scorer_current = False

    def _hand_off_model(self):
        """_prepare_model_for_validation of device mode.  The first time in a fit the scorer is built from the host attributes as
        they stand (which uploads the seen CSR, too); from then on it is only filled from the training handle."""
        if not self._scorer_current:
            self._get_scorer()
        self._scorer.update_from(self.epoch_kernel)
        self._host_model_stale = True
        self._scorer_current = True

    def _sync_host_model(self):
        """The host attributes <- the model that is being validated, if they are stale; nothing is downloaded otherwise."""
        if self._host_model_stale:
            self._download_model()
            self._host_model_stale = False

    def device_scorer(self):
        if self._scorer_current:
            if self._scorer is not None and self._scorer_src["urm"] is self.URM_train:
                return self._scorer
            self._sync_host_model()             # (URM_train was replaced mid-fit: back to the cache rule, which builds a new scorer)
            self._scorer_current = False
        return super(HandOffScoringMixin, self).device_scorer()

    def invalidate_scorer(self):
        if self._host_model_stale and getattr(getattr(self, "epoch_kernel", None), "_h", None):
            self._sync_host_model()             # (the scorer held the only copy of the validated model outside the training handle)
        self._host_model_stale = False
        self._scorer_current = False
        super(HandOffScoringMixin, self).invalidate_scorer()

    def _compute_item_score(self, user_id_array, items_to_compute=None):
        self._sync_host_model()
        return super(HandOffScoringMixin, self)._compute_item_score(user_id_array, items_to_compute=items_to_compute)

    def save_model(self, folder_path, file_name=None):
        self._sync_host_model()
        return super(HandOffScoringMixin, self).save_model(folder_path, file_name=file_name)


class MI355XSparseScorer(_Scorer):
    """scores[u] = A[u, :] . B for sparse A, B (ItemKNN / SLIM: A = URM_train, B = W_sparse; UserKNN: A = W_sparse,
    B = URM_train), filtered and ranked on the device like MI355XScorer.

    By default the products of a score are summed by LDS float atomics, in an order that can differ between two calls.  With
    `exact=True` every score is bit for bit what SciPy's `A[users] @ B` gives for float32 operands: the stored cells of a row of A are
    walked in their storage order (A is used as `sps.csr_matrix(A)` holds it, never sorted), product rounded before the add; calls
    repeat bit for bit however a batch is cut into blocks.  B is uploaded with sorted indices (the order inside a row of B changes no
    score); a B that stores a column twice in one row is refused with ValueError."""
    _PREFIX = "mi355rec_spscorer"
    EVAL_ADD = "add_spscorer"

    def __init__(self, A, B, URM_seen, exact=False):
        A, B, seen = A.tocsr(), B.tocsr(), URM_seen.tocsr()
        assert A.shape[1] == B.shape[0] and seen.shape == (A.shape[0], B.shape[1])
        self.n_users, self.n_mid, self.n_items = A.shape[0], B.shape[0], B.shape[1]
        self.exact = bool(exact)
        if self.exact and not B.has_sorted_indices:
            B = B.sorted_indices()      # (a copy: the caller's matrix stays as it is)
        arrs = [N.as_i32(A.indptr), N.as_i32(A.indices), N.as_f32(A.data), N.as_i32(B.indptr), N.as_i32(B.indices),
                N.as_f32(B.data), N.as_i32(seen.indptr), N.as_i32(seen.indices)]
        self._create(A.shape[0], A.shape[1], B.shape[1], *[N.ptr(a) for a in arrs])
        if self.exact:
            try:
                self._call("set_exact", 1)
            except ValueError:
                self.close()
                raise

    def update_B(self, B):
        """Another B of the same shape, with any number of stored cells, in the place of the one the scorer holds; A and the seen CSR
        stay on the device.  B is treated as the constructor treats it (`tocsr()`, sorted indices in exact mode); afterwards the scorer
        answers as one built from (A, B) would.  ValueError naming the first offending row -- row pointers that do not start at 0 or
        decrease, a column id outside [0, n_items), in exact mode a column stored twice in a row -- and the scorer keeps the B it had."""
        B = B.tocsr()
        if B.shape != (self.n_mid, self.n_items):
            raise ValueError("B is {}, the scorer's is {}".format(B.shape, (self.n_mid, self.n_items)))
        if self.exact and not B.has_sorted_indices:
            B = B.sorted_indices()
        arrs = [N.as_i32(B.indptr), N.as_i32(B.indices), N.as_f32(B.data)]
        self._call("update_b", *[N.ptr(a) if len(a) else N.ptr(np.zeros(1, a.dtype)) for a in arrs])

    def weights(self):
        """B as the scorer holds it on the device, a csr_matrix (n_mid x n_items, float32): its arrays cell for cell."""
        indptr, nnz = np.empty(self.n_mid + 1, np.int32), C.c_int64(0)
        self._call("get_b", N.ptr(indptr), None, None, C.byref(nnz))
        indices, data = np.empty(max(1, nnz.value), np.int32), np.empty(max(1, nnz.value), np.float32)
        self._call("get_b", N.ptr(indptr), N.ptr(indices), N.ptr(data), C.byref(nnz))
        return sps.csr_matrix((data[:nnz.value], indices[:nnz.value], indptr), shape=(self.n_mid, self.n_items))

    def update_from(self, slim_epoch):
        """B <- similarityMatrixTopK(get_S(), topK) of a SLIM_BPR_MI355X_Epoch, the W its `get_S_and_W()` returns, array for array,
        built and copied on the device: no download, no SciPy matrix, no new scorer.  TypeError for any other object; ValueError for
        a closed handle, for one over other items than the scorer's B (a user-based scorer) and for a topK below 1;
        NotImplementedError for the sparse store (train_with_sparse_weights).  A refused call leaves the scorer as it was."""
        from .slim_bpr import SLIM_BPR_MI355X_Epoch
        if not isinstance(slim_epoch, SLIM_BPR_MI355X_Epoch):
            raise TypeError("update_from takes a SLIM_BPR_MI355X_Epoch, got {}".format(type(slim_epoch).__name__))
        if not slim_epoch._h:
            raise ValueError("%s is closed" % type(slim_epoch).__name__)
        self._call("update_from_slim", slim_epoch._h, int(slim_epoch.topK or 0))


class MI355XDenseScorer(_Scorer):
    """scores[u] = A[u, :] . B for a sparse A (CSR, n_users x n_mid) and a DENSE float32 B (n_mid x n_items): an item-similarity model
    whose W_sparse is an ndarray (A = URM_train, B = W_sparse; BaseSimilarityMatrixRecommender.py:73-92), filtered and ranked on the
    device like MI355XScorer.  Every score is bit for bit what SciPy's `A[users] @ B` gives: the stored cells of a row of A are summed
    in their storage order (A's indices are used as given, never sorted), product rounded before the add.  `B` is the array, or
    its shape `(n_mid, n_items)` for zero weights that `update` / `set_weights_from` fill later."""
    _PREFIX = "mi355rec_dscorer"
    EVAL_ADD = "add_dscorer"

    def __init__(self, A, B, URM_seen):
        if not sps.isspmatrix_csr(A):
            A = sps.csr_matrix(A)
        seen = URM_seen.tocsr()
        weights = None if isinstance(B, tuple) else self._weights(B, None)
        n_mid, n_items = B if weights is None else weights.shape
        assert A.shape[1] == n_mid and seen.shape == (A.shape[0], n_items)
        self.n_users, self.n_mid, self.n_items = A.shape[0], int(n_mid), int(n_items)
        arrs = [N.as_i32(A.indptr), N.as_i32(A.indices), N.as_f32(A.data), weights, N.as_i32(seen.indptr), N.as_i32(seen.indices)]
        self._create(self.n_users, self.n_mid, self.n_items, *[N.ptr(a) for a in arrs])

    @staticmethod
    def _weights(B, shape):
        B = N.as_f32(B)
        if B.ndim != 2 or (shape is not None and B.shape != shape):
            raise ValueError("the weights must be a 2-d array{}, got {!r}".format("" if shape is None else " of shape %r" % (shape,), B.shape))
        return B

    def update(self, B):
        """New weights of the same shape (a second fit); nothing is reallocated."""
        B = self._weights(B, (self.n_mid, self.n_items))
        self._call("update", N.ptr(B))

    def set_weights_from(self, ease):
        """B <- the weights of an `MI355XEase` handle after invert(), device to device: the values `ease.get_dense()` downloads."""
        if not ease._h:
            raise ValueError("the EASE handle is closed")
        self._call("set_from_ease", ease._h)


class GpuSimilarityScoringMixin(_ScoringMixin):
    """recommend() for BaseItemSimilarityMatrixRecommender / BaseUserSimilarityMatrixRecommender subclasses, served by
    MI355XSparseScorer.  `_SCORER_USER_BASED` selects the operand order.  Under this cache rule the scorer is rebuilt whenever
    W_sparse or URM_train is replaced (fit, early-stopping validation) or W_sparse changes in place; replacing its B in place
    (`MI355XSparseScorer.update_B` / `update_from`) is what HandOffSimilarityScoringMixin does during a device-mode fit.

    An item-based model whose W_sparse is a dense ndarray is served by MI355XDenseScorer when the class (or the object) sets
    `dense_scoring = "device"`; with the default "host" it is scored by the base class on the host, as before.  The dense scorer has a
    cache slot of its own: other weights of the same shape are an update.

    `sparse_scoring` (class or object attribute) chooses the sparse scorer's mode: "atomic", the default, sums a score's products
    with LDS float atomics -- near-tied scores can change places between two calls; "exact" gives SciPy's float32 scores bit for
    bit and lists by the tie rule alone (MI355XSparseScorer(exact=True)), at the price DESIGN section 17 measures.  The mode is part
    of the cached scorer's layout: changing it builds a new scorer on the next call."""
    _SCORER_USER_BASED = False
    SPARSE_SCORING_MODES = ("atomic", "exact")
    sparse_scoring = "atomic"
    _sp_scorer = None
    _sp_scorer_src = None
    dense_scoring = "host"
    _dense_scorer = None
    _dense_scorer_src = None
    _SCORER_ATTRS = (("_sp_scorer", "_sp_scorer_src"), ("_dense_scorer", "_dense_scorer_src"))

    def device_scorable(self):
        """False while W_sparse is a dense array (EASE_R with topK=None keeps the reference's ndarray): the sparse scorer takes a CSR, so
        such a model is scored by the base class on the host -- its own recommend() and the device evaluators' lists path -- unless
        `dense_device_scorable()`."""
        return not isinstance(getattr(self, "W_sparse", None), np.ndarray)

    def dense_device_scorable(self):
        """True when W_sparse is a dense array and `dense_scoring` is "device": recommend() and the device evaluators go through
        MI355XDenseScorer."""
        return self.dense_scoring == "device" and not self._SCORER_USER_BASED and isinstance(getattr(self, "W_sparse", None), np.ndarray)

    def _get_dense_scorer(self, weights_from=None):
        """The dense scorer for the current W_sparse and URM_train.  `weights_from`: an MI355XEase handle that holds W_sparse's values on
        the device -- they are copied from there instead of being uploaded from the host array."""
        W = self.W_sparse
        on_device = weights_from is not None
        scorer = self._cached_scorer(
            self._SCORER_ATTRS[1], {"W": W}, _fingerprint(W),
            build=lambda: MI355XDenseScorer(self.URM_train, W.shape if on_device else W, self.URM_train),
            update=lambda scorer: None if on_device else scorer.update(W),
            new_layout=lambda scorer: (scorer.n_mid, scorer.n_items) != W.shape)
        if on_device:
            scorer.set_weights_from(weights_from)
        return scorer

    def _get_sparse_scorer(self):
        # (SLIM's get_S_incremental_and_set_W assigns W_sparse twice per validation: the address of the first, freed matrix can be
        # handed to its successor, so an id() key would score with stale weights)
        W = self.W_sparse
        exact = self._sparse_scoring_exact()
        A, B = (W, self.URM_train) if self._SCORER_USER_BASED else (self.URM_train, W)
        prints = (W.shape, W.nnz, _fingerprint(W.data), _fingerprint(W.indices)) if hasattr(W, "nnz") else _fingerprint(W)
        return self._cached_scorer(self._SCORER_ATTRS[0], {"W": W}, prints, build=lambda: MI355XSparseScorer(A, B, self.URM_train, exact=exact),
                                   new_layout=lambda scorer: bool(getattr(scorer, "exact", False)) != exact)

    def _sparse_scoring_exact(self):
        if self.sparse_scoring not in self.SPARSE_SCORING_MODES:
            raise ValueError("{}: sparse_scoring must be one of {}, got {!r}".format(type(self).__name__, self.SPARSE_SCORING_MODES,
                                                                                   self.sparse_scoring))
        return self.sparse_scoring == "exact"

    def device_scorer(self):
        self._sparse_scoring_exact()        # (an unknown mode is refused before the device is touched, whichever scorer serves)
        if self.dense_device_scorable():
            return self._get_dense_scorer()
        return self._get_sparse_scorer() if self.device_scorable() else None

    def release_dense_scorer(self):
        """Give the dense scorer's n_items^2 floats of HBM back (a sparse W_sparse after a dense one)."""
        self._drop_scorer(self._SCORER_ATTRS[1])


class HandOffSimilarityScoringMixin(GpuSimilarityScoringMixin):
    """GpuSimilarityScoringMixin for a recommender with a ValidationHandOff logic class whose training handle can fill the sparse
    scorer (SLIM-BPR): the scorer's half of `validation_hand_off = "device"`, as HandOffScoringMixin is for the factor models.  With
    the flags clear -- host mode, and device mode outside a fit -- every method is its parent's.

    While `_host_model_stale` is set, W_sparse and S_incremental are the matrices of the last validation that was synced -- the
    first of the fit, or the last one before a `_sync_host_model()` -- not of the one being validated: code that reads `rec.W_sparse`
    directly in the middle of a device-mode fit sees that older matrix.  `_compute_item_score`, `save_model` and `invalidate_scorer`
    sync first."""
    _HAND_OFF_SCORER = True
    _host_model_stale = False
    _scorer_current = False

    def _hand_off_model(self):
        """_prepare_model_for_validation of device mode.  The first validation of a fit runs the host path as it stands -- which is
        also the one upload of URM_train and the seen CSR; from then on the scorer's B is replaced from the training handle."""
        if self._scorer_current and self._hand_off_scorer() is not None:
            self._sp_scorer.update_from(self.epoch_kernel)
            self._host_model_stale = True
            return
        self._download_model()
        self._host_model_stale = False
        self._get_sparse_scorer()
        self._scorer_current = True

    def _hand_off_scorer(self):
        """The sparse scorer while it can go on being filled from the training handle: same URM_train, same scoring mode."""
        scorer = self._sp_scorer
        if scorer is not None and self._sp_scorer_src["urm"] is self.URM_train and scorer.exact == self._sparse_scoring_exact():
            return scorer
        return None

    def _sync_host_model(self):
        """W_sparse and S_incremental <- the model that is being validated, if they are stale; nothing is downloaded otherwise."""
        if self._host_model_stale:
            self._download_model()
            self._host_model_stale = False

    def device_scorer(self):
        if self._scorer_current:
            scorer = self._hand_off_scorer()
            if scorer is not None:
                return scorer
            self._sync_host_model()             # (URM_train or sparse_scoring changed mid-fit: back to the cache rule, which builds a new scorer)
            self._scorer_current = False
        return super(HandOffSimilarityScoringMixin, self).device_scorer()

    def invalidate_scorer(self):
        if self._host_model_stale and getattr(getattr(self, "epoch_kernel", None), "_h", None):
            self._sync_host_model()             # (the scorer held the only copy of the validated W outside the training handle)
        self._host_model_stale = False
        self._scorer_current = False
        super(HandOffSimilarityScoringMixin, self).invalidate_scorer()

    def _compute_item_score(self, user_id_array, items_to_compute=None):
        self._sync_host_model()
        return super(HandOffSimilarityScoringMixin, self)._compute_item_score(user_id_array, items_to_compute=items_to_compute)

    def save_model(self, folder_path, file_name=None):
        self._sync_host_model()
        return super(HandOffSimilarityScoringMixin, self).save_model(folder_path, file_name=file_name)


class MI355XItemScorer(_Scorer):
    """One vector of item scores for every user (the reference's non-personalized models, Base/NonPersonalizedRecommender.py:30-43,
    119-132), filtered and ranked on the device like MI355XScorer.  The vector is sorted once per model; a user's list is the head of
    that order without the user's seen items -- work of cutoff + profile length per user instead of n_items.  A non-finite entry of
    the vector is never listed.  `URM_seen` is a host matrix or a `ResidentURM` (its structure is then copied device to device)."""
    _PREFIX = "mi355rec_itemscorer"
    EVAL_ADD = "add_itemscorer"
    EVAL_LARGE_BLOCKS = ("rows", "candidates")

    def __init__(self, item_scores, URM_seen):
        vec = N.as_f32(np.asarray(item_scores).ravel())
        self.n_users, self.n_items = URM_seen.shape
        assert len(vec) == self.n_items, "item_scores has {} entries for {} items".format(len(vec), self.n_items)
        if isinstance(URM_seen, N.ResidentURM):
            self._create(self.n_users, self.n_items, N.ptr(vec), URM_seen.indptr.ptr, URM_seen.indices.ptr, URM_seen.nnz,
                         entry="create_resident")
        else:
            seen = URM_seen.tocsr()
            indptr, indices = N.as_i32(seen.indptr), N.as_i32(seen.indices)
            self._create(self.n_users, self.n_items, N.ptr(vec), N.ptr(indptr), N.ptr(indices))

    def update(self, item_scores):
        vec = N.as_f32(np.asarray(item_scores).ravel())
        assert len(vec) == self.n_items
        self._call("update", N.ptr(vec))

    def window_bits(self):
        """W: positions of the sorted order one pass of the ranking kernel covers (2048: a wavefront per user, 8192: a workgroup)."""
        bits = C.c_int32(0)
        self._call("window_bits", C.byref(bits))
        return int(bits.value)

    def set_window_bits(self, bits):
        self._call("set_window_bits", int(bits))


class GpuItemScoreMixin(_ScoringMixin):
    """recommend() for recommenders whose scores are one vector shared by all users, served by MI355XItemScorer.  The vector is
    `_item_score_vector()`; a new vector of the same length is an update.  `_resident_urm`, when the recommender has one that holds
    URM_train, also serves as the scorer's seen CSR.  A model restored by load_model is scored without a fit."""
    _item_scorer = None
    _item_scorer_src = None
    _resident_urm = None
    _SCORER_ATTRS = (("_item_scorer", "_item_scorer_src"),)
    _ASSERT_WARM_USERS = True

    def _item_score_vector(self):
        raise NotImplementedError("{}: _item_score_vector".format(type(self).__name__))

    def _get_item_scorer(self):
        vector = self._item_score_vector()

        def build():
            resident = self._resident_urm
            return MI355XItemScorer(vector, resident if resident is not None and resident.matches(self.URM_train) else self.URM_train)

        return self._cached_scorer(self._SCORER_ATTRS[0], {"vector": vector}, _fingerprint(vector), build,
                                   update=lambda scorer: scorer.update(vector))

    def device_scorer(self):
        return self._get_item_scorer()
