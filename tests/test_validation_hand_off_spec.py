"""What the validation hand-off promises without a device: the mode attribute and its refusals, and the two C-ABI entries -- declared
in include/mi355rec.h, exported by the library and bound with the declared argument types."""
import ctypes as C
import os
import re

import pytest

from recsys2019_deeplearning_evaluation_amd import (IALSRecommender, MI355XScorer, MatrixFactorization_AsySVD_MI355X,
                                                    MatrixFactorization_BPR_MI355X, MatrixFactorization_FunkSVD_MI355X, _native)
from recsys2019_deeplearning_evaluation_amd import recommender_base as RB
from recsys2019_deeplearning_evaluation_amd.reference_binding import bind
from hand_off_cases import URM_TRAIN

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ("mi355rec_scorer_update_from_mf", "mi355rec_scorer_update_from_ials")
HAND_OFF_CLASSES = (MatrixFactorization_BPR_MI355X, MatrixFactorization_FunkSVD_MI355X, IALSRecommender)


def _bound(**kwargs):
    return bind(RB.BaseMatrixFactorizationRecommender, RB.BaseItemSimilarityMatrixRecommender, RB.BaseUserSimilarityMatrixRecommender,
                RB.Incremental_Training_Early_Stopping, **kwargs)


def _bound_classes(R):
    return (R.MatrixFactorization_BPR_MI355X, R.MatrixFactorization_FunkSVD_MI355X, R.IALSRecommender)


@pytest.fixture
def no_library(monkeypatch):
    def load():
        raise AssertionError("the native library was loaded")
    monkeypatch.setattr(_native, "load", load)


def test_the_default_is_host_on_every_class_and_its_bound_counterpart():
    for cls in HAND_OFF_CLASSES + _bound_classes(_bound()) + _bound_classes(_bound(device_scoring=False)):
        assert cls.validation_hand_off == "host", cls
        assert cls.VALIDATION_HAND_OFF_MODES == ("host", "device"), cls
        rec = cls(URM_TRAIN, verbose=False)
        assert rec.validation_hand_off == "host" and not rec._host_model_stale and not rec._scorer_current


@pytest.mark.parametrize("cls", HAND_OFF_CLASSES + (MatrixFactorization_AsySVD_MI355X,))
def test_an_unknown_mode_is_a_value_error_before_the_library_is_loaded(no_library, cls):
    rec = cls(URM_TRAIN, verbose=False)
    rec.validation_hand_off = "hbm"
    with pytest.raises(ValueError, match="validation_hand_off must be one of"):
        rec.fit(epochs=1)
    if cls is not MatrixFactorization_AsySVD_MI355X:        # (AsySVD's own hook is host mode's: there is no other for it)
        with pytest.raises(ValueError, match="validation_hand_off must be one of"):
            rec._prepare_model_for_validation()


def test_device_mode_on_asysvd_is_a_value_error_at_fit(no_library):
    for cls in (MatrixFactorization_AsySVD_MI355X, _bound().MatrixFactorization_AsySVD_MI355X):
        rec = cls(URM_TRAIN, verbose=False)
        assert rec.validation_hand_off == "host"
        rec.validation_hand_off = "device"
        with pytest.raises(ValueError, match="not supported"):
            rec.fit(epochs=1, num_factors=4)


def test_device_mode_without_the_scoring_mixin_is_a_value_error_at_fit(no_library):
    for cls in _bound_classes(_bound(device_scoring=False)):
        rec = cls(URM_TRAIN, verbose=False)
        rec.validation_hand_off = "device"
        with pytest.raises(ValueError, match="needs the device scorer"):
            rec.fit(epochs=1)


def test_host_reads_of_a_model_that_is_not_stale_download_nothing(no_library, tmp_path):
    import numpy as np
    rec = MatrixFactorization_BPR_MI355X(URM_TRAIN, verbose=False)
    rng = np.random.default_rng(0)
    rec.USER_factors, rec.ITEM_factors = rng.normal(size=(URM_TRAIN.shape[0], 3)), rng.normal(size=(URM_TRAIN.shape[1], 3))
    np.testing.assert_array_equal(rec._compute_item_score(np.arange(5)), rec.USER_factors[:5] @ rec.ITEM_factors.T)
    rec.save_model(str(tmp_path) + os.sep, "model")
    rec.invalidate_scorer()


def _declarations():
    text = open(os.path.join(ROOT, "include", "mi355rec.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return {name: [a.strip() for a in args.split(",")]
            for name, args in re.findall(r"\bint\s+(mi355rec_scorer_update_from_[a-z]+)\s*\(([^)]*)\)\s*;", text)}


def test_the_header_declares_both_entries_in_the_scorer_group():
    decl = _declarations()
    assert sorted(decl) == sorted(ENTRIES)
    assert decl["mi355rec_scorer_update_from_mf"] == ["mi355rec_scorer_t scorer", "mi355rec_mf_t mf"]
    assert decl["mi355rec_scorer_update_from_ials"] == ["mi355rec_scorer_t scorer", "mi355rec_ials_t ials"]
    text = open(os.path.join(ROOT, "include", "mi355rec.h")).read()
    group = text[text.index("typedef struct mi355rec_scorer *mi355rec_scorer_t;"):text.index("typedef struct mi355rec_spscorer *mi355rec_spscorer_t;")]
    for name in ENTRIES:
        at = group.index("int %s(" % name)
        comment = group[group.rindex("/*", 0, at):at]
        assert "eplaces" in comment, "%s: the comment says what the entry replaces" % name


def test_native_binds_both_entries_with_the_declared_argument_types():
    for name in ENTRIES:
        restype, argtypes = _native.SIGNATURES[name]
        assert restype is C.c_int and argtypes == [C.c_void_p, C.c_void_p]      # two opaque handles
    lib = _native.load()
    for name in ENTRIES:
        fn = getattr(lib, name)
        assert fn.restype is C.c_int and list(fn.argtypes) == [C.c_void_p, C.c_void_p]
        assert fn(None, None) == _native.E_INVALID                              # refused before the device is touched
        assert lib.mi355rec_last_error().decode() == "NULL handle"
    assert callable(MI355XScorer.update_from)
