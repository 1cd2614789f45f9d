"""The wrappers' shared lifecycle (`_native.Handle`) and the scoring mixins' shared recommend(), driven without a GPU: a fake
library object stands in for libmi355rec.so."""
import ctypes as C
import gc

import numpy as np
import pytest
import scipy.sparse as sps

from recsys2019_deeplearning_evaluation_amd import _native as N
from recsys2019_deeplearning_evaluation_amd import scoring


class FakeLibrary:
    """Records every call as (name, args); `rc` maps an entry point to the code it returns (0 otherwise)."""

    def __init__(self, rc=None):
        self.calls = []
        self.rc = dict(rc or {})

    def mi355rec_last_error(self):
        return b"message of the fake library"

    def __getattr__(self, name):
        if not name.startswith("mi355rec_thing_"):
            raise AttributeError(name)

        def entry(*args):
            self.calls.append((name, args))
            if name == "mi355rec_thing_create" and not self.rc.get(name):
                C.cast(args[0], C.POINTER(C.c_void_p))[0] = 0x1234      # what a create writes through its first argument
            if name == "mi355rec_thing_get_stats":
                C.cast(args[1], C.POINTER(N.Stats))[0].n_units = 7
            return self.rc.get(name, 0)
        return entry

    def names(self):
        return [name for name, _ in self.calls]


class Thing(N.Handle):
    _PREFIX = "mi355rec_thing"


@pytest.fixture
def fake(monkeypatch):
    lib = FakeLibrary()
    monkeypatch.setattr(N, "_lib", lib)        # what load() hands out once the library is open
    return lib


def test_create_passes_the_handle_by_reference_first(fake):
    t = Thing()
    assert t._h is None
    t._create(3, "x")
    (name, args), = fake.calls
    assert name == "mi355rec_thing_create" and args[1:] == (3, "x")
    assert C.cast(args[0], C.POINTER(C.c_void_p))[0] == 0x1234          # byref of the object's own handle
    assert isinstance(t._h, C.c_void_p) and t._h.value == 0x1234
    t._create(entry="create_again")
    assert fake.names()[-1] == "mi355rec_thing_create_again"


def test_call_prefixes_passes_the_handle_and_checks(fake):
    t = Thing()
    t._create()
    t._call("run", 5, None)
    name, args = fake.calls[-1]
    assert name == "mi355rec_thing_run" and args[0] is t._h and args[1:] == (5, None)
    assert t.stats()["n_units"] == 7 and fake.names()[-1] == "mi355rec_thing_get_stats"


@pytest.mark.parametrize("code,exc", [(N.E_INVALID, ValueError), (N.E_UNSUPPORTED, NotImplementedError),
                                      (N.E_NUMERIC, FloatingPointError), (N.E_HIP, N.NativeLibraryError),
                                      (N.E_NO_DEVICE, N.NativeLibraryError)])
def test_return_codes_map_to_the_exceptions_of_check(fake, code, exc):
    t = Thing()
    t._create()
    fake.rc["mi355rec_thing_run"] = code
    with pytest.raises(exc, match="message of the fake library") as info:
        t._call("run")
    assert type(info.value) is exc
    with pytest.raises(exc):
        N.check(code)


def test_close_destroys_exactly_once(fake):
    t = Thing()
    t._create()
    handle = t._h
    t.close()
    assert t._h is None
    t.close()
    t.__del__()
    del t
    gc.collect()
    destroys = [args for name, args in fake.calls if name == "mi355rec_thing_destroy"]
    assert len(destroys) == 1 and destroys[0] == (handle,)

    u = Thing()
    u._create()
    del u                                       # an object that was never closed is destroyed with its last reference
    gc.collect()
    assert fake.names().count("mi355rec_thing_destroy") == 2


def test_a_call_after_close_raises_and_reaches_nothing(fake):
    t = Thing()
    t._create()
    t.close()
    before = len(fake.calls)
    with pytest.raises(ValueError, match="Thing"):
        t._call("run", 1)
    with pytest.raises(ValueError, match="Thing"):
        t.stats()
    assert len(fake.calls) == before


def test_a_failed_create_leaves_nothing_to_destroy(fake):
    fake.rc["mi355rec_thing_create"] = N.E_INVALID
    t = Thing()
    with pytest.raises(ValueError):
        t._create(1)
    assert t._h is None
    t.close()
    t.__del__()
    with pytest.raises(ValueError, match="Thing"):
        t._call("run")
    del t
    gc.collect()
    assert fake.names() == ["mi355rec_thing_create"]


class StubScorer:
    """Ranks items 0, 1, 2, ... for every user; a user with an odd id has only `user % 3` admissible items (-1 padding)."""
    n_users = 10

    def recommend(self, users, cutoff, remove_seen, allowed, return_scores):
        self.seen_call = (np.asarray(users).tolist(), cutoff, remove_seen, allowed, return_scores)
        ranked = np.tile(np.arange(cutoff, dtype=np.int32), (len(users), 1))
        for row, u in zip(ranked, users):
            if u % 2:
                row[u % 3:] = -1
        return ranked, (np.zeros((len(users), 6), np.float32) if return_scores else None)


class FactorModel(scoring.GpuScoringMixin):
    RECOMMENDER_NAME = "FactorModel"
    n_items = 6
    URM_train = np.zeros((10, 6))

    def __init__(self):
        self.stub = StubScorer()

    def _get_scorer(self):
        return self.stub


class SimilarityModel(scoring.GpuSimilarityScoringMixin):
    n_items = 6
    URM_train = np.zeros((10, 6))

    def __init__(self):
        self.stub = StubScorer()

    def _get_sparse_scorer(self):
        return self.stub


@pytest.mark.parametrize("model_class", [FactorModel, SimilarityModel])
def test_mixins_share_one_recommend(model_class):
    rec = model_class()
    assert model_class.recommend is scoring._ScoringMixin.recommend
    # no padding anywhere: the lists are the rows
    assert rec.recommend(np.array([0, 2, 4]), cutoff=3) == [[0, 1, 2]] * 3
    assert rec.stub.seen_call == ([0, 2, 4], 3, True, None, False)
    # rows with padding lose it, rows without keep their length
    assert rec.recommend(np.array([0, 1, 5, 3]), cutoff=4, remove_seen_flag=False) == [[0, 1, 2, 3], [0], [0, 1], []]
    assert rec.stub.seen_call[2] is False
    # a scalar user id gives one list, not a list of lists; cutoff=None asks for n_items - 1
    assert rec.recommend(4) == [0, 1, 2, 3, 4]
    assert rec.recommend(5, cutoff=3) == [0, 1]
    # return_scores hands the scorer's score rows through, next to the lists
    lists, scores = rec.recommend(np.array([2, 5]), cutoff=3, return_scores=True)
    assert lists == [[0, 1, 2], [0, 1]] and scores.shape == (2, 6) and rec.stub.seen_call[4] is True
    lists, scores = rec.recommend(7, cutoff=2, return_scores=True)
    assert lists == [0] and scores.shape == (1, 6)
    # the item filters arrive as one uint8 mask
    rec.recommend(np.array([0]), cutoff=2, items_to_compute=[1, 3])
    np.testing.assert_array_equal(rec.stub.seen_call[3], [0, 1, 0, 1, 0, 0])


def test_factor_mixin_keeps_its_cold_user_assertion():
    rec = FactorModel()
    with pytest.raises(AssertionError, match="FactorModel: Cold users not allowed. Users in trained model are 10, "
                                             "requested prediction for users up to 12"):
        rec.recommend(np.array([1, 12]), cutoff=2)


def test_invalidate_scorer_closes_and_forgets():
    class Closable:
        closed = 0

        def close(self):
            self.closed += 1

    for model_class, attr, src in ((FactorModel, "_scorer", "_scorer_src"), (SimilarityModel, "_sp_scorer", "_sp_scorer_src")):
        rec, scorer = model_class(), Closable()
        setattr(rec, attr, scorer)
        setattr(rec, src, {"anything": 1})
        rec.invalidate_scorer()
        rec.invalidate_scorer()
        assert scorer.closed == 1 and getattr(rec, attr) is None and getattr(rec, src) is None


# ---- the cache rule of the scoring mixins (scoring._ScoringMixin._cached_scorer), one table over the four scorers -----------------
class CountingScorer:
    """Stands in for the MI355X*Scorer classes: remembers what it was built from and counts update / close / set_weights_from."""
    EVAL_ADD = "add_counting"
    EVAL_LARGE_BLOCKS = ()

    def __init__(self, *args, **kwargs):
        self.args, self.kwargs = args, kwargs
        self.updates = self.closed = 0
        self.filled_from = []
        self._h = object()
        self.log.append(self)

    def update(self, *args, **kwargs):
        self.updates += 1

    def close(self):
        self.closed += 1

    def set_weights_from(self, ease):
        self.filled_from.append((ease, self.updates))


class CountingFactorScorer(CountingScorer):
    def __init__(self, U, V, URM, **bias):
        super().__init__(U, V, URM, **bias)
        self.n_users, self.n_factors, self.use_bias = U.shape[0], U.shape[1], "USER_bias" in bias


class CountingDenseScorer(CountingScorer):
    def __init__(self, A, B, URM):
        super().__init__(A, B, URM)
        self.n_mid, self.n_items = B if isinstance(B, tuple) else B.shape


class CountingItemScorer(CountingScorer):
    n_users = 4


@pytest.fixture
def built(monkeypatch):
    """Every scorer the mixins build during a test, in order."""
    log = []
    monkeypatch.setattr(CountingScorer, "log", log, raising=False)
    monkeypatch.setattr(scoring, "MI355XScorer", CountingFactorScorer)
    monkeypatch.setattr(scoring, "MI355XSparseScorer", CountingScorer)
    monkeypatch.setattr(scoring, "MI355XDenseScorer", CountingDenseScorer)
    monkeypatch.setattr(scoring, "MI355XItemScorer", CountingItemScorer)
    return log


def _urm():
    return sps.csr_matrix(np.ones((4, 5), np.float32))


def _factor_model():
    rec = type("Factor", (scoring.GpuScoringMixin,), {"RECOMMENDER_NAME": "Factor"})()
    rec.URM_train, rec.use_bias = _urm(), False
    rec.USER_factors, rec.ITEM_factors = np.arange(12, dtype=np.float32).reshape(4, 3), np.arange(15, dtype=np.float32).reshape(5, 3)
    return rec


def _sparse_model():
    rec = type("Sparse", (scoring.GpuSimilarityScoringMixin,), {})()
    rec.URM_train, rec.W_sparse = _urm(), sps.csr_matrix(np.arange(1, 26, dtype=np.float32).reshape(5, 5))
    return rec


def _dense_model():
    rec = type("Dense", (scoring.GpuSimilarityScoringMixin,), {"dense_scoring": "device"})()
    rec.URM_train, rec.W_sparse = _urm(), np.arange(25, dtype=np.float32).reshape(5, 5)
    return rec


def _item_model():
    rec = type("Item", (scoring.GpuItemScoreMixin,), {"RECOMMENDER_NAME": "Item"})()
    rec.URM_train, rec.vector = _urm(), np.arange(5, dtype=np.float32)
    rec._item_score_vector = lambda: rec.vector
    return rec


# kind: (model, the mixin's getter, the attribute of its source array, the scorer has an update)
CACHE_KINDS = {"factor": (_factor_model, "_get_scorer", "ITEM_factors", True), "sparse": (_sparse_model, "_get_sparse_scorer", "W_sparse", False),
               "dense": (_dense_model, "_get_dense_scorer", "W_sparse", True), "item": (_item_model, "_get_item_scorer", "vector", True)}


def _replace_source(rec, attr):
    setattr(rec, attr, getattr(rec, attr).copy())


def _edit_source_in_place(rec, attr):
    source = getattr(rec, attr)
    (source.data if sps.issparse(source) else source)[...] *= 2


def _replace_urm(rec, attr):
    rec.URM_train = rec.URM_train.copy()


# change: (what happens to the model, rebuilds whatever the scorer can do)
CACHE_CHANGES = {"a replaced source array": (_replace_source, False), "an in-place edit": (_edit_source_in_place, False),
                 "URM_train replaced": (_replace_urm, True)}


@pytest.mark.parametrize("kind", CACHE_KINDS)
def test_cache_keeps_the_scorer_of_the_same_objects(built, kind):
    model, getter, _, _ = CACHE_KINDS[kind]
    rec = model()
    first = getattr(rec, getter)()
    assert getattr(rec, getter)() is first and rec.device_scorer() is first
    assert built == [first] and first.updates == 0 and first.closed == 0
    (_, src_attr), = [slot for slot in rec._SCORER_ATTRS if getattr(rec, slot[0]) is first]
    assert getattr(rec, src_attr)["urm"] is rec.URM_train


@pytest.mark.parametrize("change", CACHE_CHANGES)
@pytest.mark.parametrize("kind", CACHE_KINDS)
def test_cache_updates_where_it_can_and_rebuilds_where_it_must(built, kind, change):
    model, getter, attr, has_update = CACHE_KINDS[kind]
    apply, always_rebuilds = CACHE_CHANGES[change]
    rec = model()
    first = getattr(rec, getter)()
    apply(rec, attr)
    second = getattr(rec, getter)()
    if has_update and not always_rebuilds:
        assert second is first and built == [first] and (first.updates, first.closed) == (1, 0)
    else:
        assert second is not first and built == [first, second] and (first.updates, first.closed) == (0, 1)
        assert (second.updates, second.closed) == (0, 0)
    assert getattr(rec, getter)() is second and len(built) == (1 if second is first else 2) and second.updates == (second is first)


def test_cache_rebuilds_the_factor_scorer_for_another_layout(built):
    rec = _factor_model()
    first = rec._get_scorer()
    rec.use_bias, rec.USER_bias, rec.ITEM_bias, rec.GLOBAL_bias = True, np.ones(4, np.float32), np.ones(5, np.float32), np.float32(0.5)
    second = rec._get_scorer()
    assert second is not first and first.closed == 1 and second.use_bias and set(second.kwargs) == {"USER_bias", "ITEM_bias", "GLOBAL_bias"}
    rec.USER_factors, rec.ITEM_factors = np.ones((4, 7), np.float32), np.ones((5, 7), np.float32)
    third = rec._get_scorer()
    assert third is not second and second.closed == 1 and third.n_factors == 7 and built == [first, second, third]
    assert first.updates == 0 and second.updates == 0 and first.closed == 1


def test_cache_rebuilds_the_dense_scorer_for_another_shape(built):
    rec = _dense_model()
    first = rec._get_dense_scorer()
    assert first.args[1] is rec.W_sparse                # (a host build uploads the array)
    rec.URM_train, rec.W_sparse = sps.csr_matrix(np.ones((4, 6), np.float32)), np.ones((6, 6), np.float32)
    second = rec._get_dense_scorer()
    assert second is not first and (first.updates, first.closed) == (0, 1) and (second.n_mid, second.n_items) == (6, 6)


def test_cache_fills_the_dense_scorer_from_the_device(built):
    rec, ease = _dense_model(), object()
    first = rec._get_dense_scorer(weights_from=ease)
    assert first.args[1] == (5, 5) and first.filled_from == [(ease, 0)] and first.updates == 0      # built from the shape, then filled
    assert rec._dense_scorer_src["W"] is rec.W_sparse
    assert rec._get_dense_scorer() is first and first.updates == 0                                  # what the fill left is recognised
    rec.W_sparse = rec.W_sparse + 1                     # other weights of the same shape, again on the device: filled, not uploaded
    assert rec._get_dense_scorer(weights_from=ease) is first
    assert first.filled_from == [(ease, 0), (ease, 0)] and first.updates == 0 and built == [first]


def test_invalidate_scorer_closes_both_slots_of_the_similarity_mixin_once(built):
    rec = _sparse_model()
    sparse = rec._get_sparse_scorer()
    rec.W_sparse = rec.W_sparse.toarray()
    dense = rec._get_dense_scorer()
    assert rec._sp_scorer is sparse and rec._dense_scorer is dense
    rec.invalidate_scorer()
    rec.invalidate_scorer()
    assert (sparse.closed, dense.closed) == (1, 1)
    assert rec._sp_scorer is rec._sp_scorer_src is rec._dense_scorer is rec._dense_scorer_src is None


def test_the_cold_user_assertion_is_the_same_for_the_item_vector(built):
    rec = _item_model()
    with pytest.raises(AssertionError, match="Item: Cold users not allowed. Users in trained model are 4, requested prediction for users up to 9"):
        rec.recommend(np.array([1, 9]), cutoff=2)


# ---- the evaluators' dispatch: scorer -> entry point and block size -----------------------------------------------------------------
def _stub_scorer(scorer_class):
    scorer = object.__new__(scorer_class)      # (the class attributes are what the evaluators read; no library behind it)
    scorer._h = None
    return scorer


class _Evaluated(scoring._ScoringMixin):
    def __init__(self, scorer):
        self.scorer = scorer

    def device_scorer(self):
        return self.scorer


N_EVAL, N_ITEMS = 40000, 250000        # the reference's block: min(1000, 1e8 / n_items) = 400 users; FUSED_BLOCK = 16384
# scorer class: (entry point, its holdout block, its negative-sample block)
DISPATCH = {scoring.MI355XScorer: ("add_scorer", 400, 16384), scoring.MI355XSparseScorer: ("add_spscorer", 400, 400),
            scoring.MI355XDenseScorer: ("add_dscorer", 400, 400), scoring.MI355XItemScorer: ("add_itemscorer", 16384, 16384)}


def _stub_evaluator(evaluator_class, seen):
    ev = object.__new__(evaluator_class)
    ev.users_to_evaluate, ev.n_items, ev.candidates_on_device = np.arange(N_EVAL, dtype=np.int32), N_ITEMS, True
    ev._run_fused = lambda scorer, add, rec, block: seen.append(("fused", scorer, add, rec, block))
    ev._run_lists = lambda rec, block: seen.append(("lists", rec, block))
    return ev


@pytest.mark.parametrize("block_size", [None, 77])
@pytest.mark.parametrize("negative", [False, True])
@pytest.mark.parametrize("scorer_class", DISPATCH, ids=lambda c: c.__name__)
def test_evaluators_dispatch_on_the_scorer(scorer_class, negative, block_size):
    from recsys2019_deeplearning_evaluation_amd import evaluation
    add, holdout_block, negative_block = DISPATCH[scorer_class]
    seen = []
    ev = _stub_evaluator(evaluation.EvaluatorNegativeItemSample_MI355X if negative else evaluation.EvaluatorHoldout_MI355X, seen)
    assert ev.FUSED_BLOCK == 16384 and ev._block_size() == 400
    rec = _Evaluated(_stub_scorer(scorer_class))
    ev._run(rec, block_size)
    block = block_size or (negative_block if negative else holdout_block)
    assert seen == [("fused", rec.scorer, add + ("_candidates" if negative else ""), rec, block)]


@pytest.mark.parametrize("block_size", [None, 77])
@pytest.mark.parametrize("negative", [False, True])
def test_evaluators_fall_back_to_the_lists_path(negative, block_size):
    from recsys2019_deeplearning_evaluation_amd import evaluation
    evaluator_class = evaluation.EvaluatorNegativeItemSample_MI355X if negative else evaluation.EvaluatorHoldout_MI355X
    plain, no_scorer = object(), _Evaluated(None)       # not a scoring mixin; a mixin whose model must go through recommend()
    for rec in (plain, no_scorer):
        seen = []
        _stub_evaluator(evaluator_class, seen)._run(rec, block_size)
        assert seen == [("lists", rec, block_size or 400)]
    if negative:                                        # candidate rows the device cannot take: every recommender through recommend()
        seen, rec = [], _Evaluated(_stub_scorer(scoring.MI355XItemScorer))
        ev = _stub_evaluator(evaluator_class, seen)
        ev.candidates_on_device = False
        ev._run(rec, block_size)
        assert seen == [("lists", rec, block_size or 400)]
