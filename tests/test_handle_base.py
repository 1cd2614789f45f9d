"""The wrappers' shared lifecycle (`_native.Handle`) and the scoring mixins' shared recommend(), driven without a GPU: a fake
library object stands in for libmi355rec.so."""
import ctypes as C
import gc

import numpy as np
import pytest

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
