"""What the SLIM-BPR validation hand-off promises without a device: the mode attribute and its refusals at fit, the three C-ABI entries
of the sparse scorer -- declared in include/mi355rec.h, exported by the library and bound with matching argument counts -- and the
host arithmetic of csrc/spscorer_plan.h, through a shim and once more as a program of its own under the host sanitizers."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest
import scipy.sparse as sps

from recsys2019_deeplearning_evaluation_amd import MI355XSparseScorer, SLIM_BPR_MI355X, _native
from recsys2019_deeplearning_evaluation_amd import recommender_base as RB
from recsys2019_deeplearning_evaluation_amd.reference_binding import bind
from recsys2019_deeplearning_evaluation_amd.scoring import (GpuSimilarityScoringMixin, HandOffScoringMixin, HandOffSimilarityScoringMixin,
                                                            ValidationHandOff)
from hand_off_cases import URM_TRAIN

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
ENTRIES = {"mi355rec_spscorer_update_b": 4, "mi355rec_spscorer_get_b": 5, "mi355rec_spscorer_update_from_slim": 3}


def _bound(**kwargs):
    return bind(RB.BaseMatrixFactorizationRecommender, RB.BaseItemSimilarityMatrixRecommender, RB.BaseUserSimilarityMatrixRecommender,
                RB.Incremental_Training_Early_Stopping, **kwargs)


@pytest.fixture
def no_library(monkeypatch):
    def load():
        raise AssertionError("the native library was loaded")
    monkeypatch.setattr(_native, "load", load)


def test_the_default_is_host_on_the_class_and_both_bound_variants():
    for cls in (SLIM_BPR_MI355X, _bound().SLIM_BPR_MI355X, _bound(device_scoring=False).SLIM_BPR_MI355X):
        assert issubclass(cls, ValidationHandOff)
        assert cls.validation_hand_off == "host" and cls.VALIDATION_HAND_OFF_MODES == ("host", "device"), cls
        rec = cls(URM_TRAIN, verbose=False)
        assert rec.validation_hand_off == "host" and not rec._host_model_stale and not rec._scorer_current
    assert issubclass(SLIM_BPR_MI355X, HandOffSimilarityScoringMixin) and issubclass(_bound().SLIM_BPR_MI355X, HandOffSimilarityScoringMixin)
    assert not issubclass(_bound(device_scoring=False).SLIM_BPR_MI355X, GpuSimilarityScoringMixin)
    # one class attribute tells the logic class that the scorer's half is there, on either hand-off mixin
    assert HandOffScoringMixin._HAND_OFF_SCORER is True and HandOffSimilarityScoringMixin._HAND_OFF_SCORER is True
    assert not hasattr(GpuSimilarityScoringMixin, "_HAND_OFF_SCORER")


def test_with_the_flags_clear_the_mixin_reads_nothing_from_a_training_handle(no_library, tmp_path):
    rec = SLIM_BPR_MI355X(URM_TRAIN, verbose=False)
    rec.W_sparse = sps.identity(URM_TRAIN.shape[1], dtype=np.float32, format="csr")
    np.testing.assert_array_equal(rec._compute_item_score(np.arange(5)), URM_TRAIN[:5].toarray())
    rec.save_model(str(tmp_path) + os.sep, "model")
    rec.invalidate_scorer()
    rec._sync_host_model()


@pytest.mark.parametrize("cls", [SLIM_BPR_MI355X, _bound().SLIM_BPR_MI355X])
def test_the_refusals_of_fit_come_before_the_library_is_loaded(no_library, cls):
    rec = cls(URM_TRAIN, verbose=False)
    rec.validation_hand_off = "hbm"
    with pytest.raises(ValueError, match="validation_hand_off must be one of"):
        rec.fit(epochs=1)
    with pytest.raises(ValueError, match="validation_hand_off must be one of"):
        rec._prepare_model_for_validation()
    rec.validation_hand_off = "device"
    with pytest.raises(ValueError, match="train_with_sparse_weights"):
        rec.fit(epochs=1, train_with_sparse_weights=True)
    with pytest.raises(ValueError, match="topK"):
        rec.fit(epochs=1, topK=False)
    wide = cls(sps.csr_matrix(([1.0, 1.0], ([0, 1], [3, 69999])), shape=(4, 70000), dtype=np.float32), verbose=False)
    wide.validation_hand_off = "device"
    with pytest.raises(ValueError, match="65535 items.*70000"):
        wide.fit(epochs=1)
    assert not hasattr(rec, "epoch_kernel") and not hasattr(wide, "epoch_kernel")


def test_device_mode_without_the_scoring_mixin_is_a_value_error_at_fit(no_library):
    rec = _bound(device_scoring=False).SLIM_BPR_MI355X(URM_TRAIN, verbose=False)
    rec.validation_hand_off = "device"
    with pytest.raises(ValueError, match="needs the device scorer"):
        rec.fit(epochs=1)
    assert not hasattr(rec, "epoch_kernel")


def test_update_from_refuses_other_objects_before_the_library_is_asked(no_library):
    scorer = MI355XSparseScorer.__new__(MI355XSparseScorer)
    with pytest.raises(TypeError, match="SLIM_BPR_MI355X_Epoch"):
        scorer.update_from(object())


# ---- the C ABI --------------------------------------------------------------------------------------------------------------------

def _declarations():
    text = open(os.path.join(ROOT, "include", "mi355rec.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return {name: [a.strip() for a in args.split(",")] for name, args in re.findall(r"\bint\s+(mi355rec_spscorer_[a-z_]+)\s*\(([^)]*)\)\s*;", text)}


def test_the_header_declares_the_three_entries_in_the_sparse_scorer_group():
    decl = _declarations()
    for name, n_args in ENTRIES.items():
        assert len(decl[name]) == n_args, name
    assert decl["mi355rec_spscorer_update_b"] == ["mi355rec_spscorer_t h", "const int32_t *b_indptr", "const int32_t *b_indices", "const float *b_data"]
    assert decl["mi355rec_spscorer_get_b"] == ["mi355rec_spscorer_t h", "int32_t *indptr", "int32_t *indices", "float *data", "int64_t *nnz"]
    assert decl["mi355rec_spscorer_update_from_slim"] == ["mi355rec_spscorer_t h", "mi355rec_slim_t slim", "int32_t topK"]
    text = open(os.path.join(ROOT, "include", "mi355rec.h")).read()
    group = text[text.index("typedef struct mi355rec_spscorer *mi355rec_spscorer_t;"):text.index("typedef struct mi355rec_dscorer *mi355rec_dscorer_t;")]
    for name in ENTRIES:
        assert "int %s(" % name in group, name


def test_native_binds_the_three_entries_with_matching_argument_counts():
    decl = _declarations()
    for name, n_args in ENTRIES.items():
        restype, argtypes = _native.SIGNATURES[name]
        assert restype is C.c_int and len(argtypes) == n_args == len(decl[name]), name
    lib = _native.load()
    for name, n_args in ENTRIES.items():
        fn = getattr(lib, name)
        assert fn.restype is C.c_int and len(fn.argtypes) == n_args
    # refused before the device is touched
    assert lib.mi355rec_spscorer_update_b(None, None, None, None) == _native.E_INVALID
    assert lib.mi355rec_last_error().decode() == "NULL argument"
    assert lib.mi355rec_spscorer_get_b(None, None, None, None, None) == _native.E_INVALID
    assert lib.mi355rec_spscorer_update_from_slim(None, None, 5) == _native.E_INVALID
    assert lib.mi355rec_last_error().decode() == "NULL handle"
    for method in ("update_B", "weights", "update_from"):
        assert callable(getattr(MI355XSparseScorer, method))


# ---- csrc/spscorer_plan.h ---------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def build_dir(tmp_path_factory):
    return tmp_path_factory.mktemp("spscorer_plan")


@pytest.fixture(scope="module")
def shim(build_dir):
    so = os.path.join(str(build_dir), "spscorer_plan_shim.so")
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-shared", "-fPIC", os.path.join(HERE, "spscorer_plan_shim.cpp"), "-o", so], check=True)
    lib = C.CDLL(so)
    lib.sp_check_csr.argtypes = [C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p]
    lib.sp_spare_cells.argtypes, lib.sp_spare_cells.restype = [C.c_int64, C.c_int64], C.c_int64
    lib.sp_slim_w_cells_bound.argtypes, lib.sp_slim_w_cells_bound.restype = [C.c_int, C.c_int], C.c_int64
    lib.sp_bytes.argtypes = [C.c_int, C.c_int64, C.c_int64, C.c_double, C.c_void_p]
    return lib


def _finding(shim, n_cols, indptr, indices, ascending):
    indptr, indices = np.array(indptr, np.int32), np.array(indices, np.int32)
    out = np.zeros(3, np.int64)
    shim.sp_check_csr(len(indptr) - 1, n_cols, indptr.ctypes.data_as(C.c_void_p), indices.ctypes.data_as(C.c_void_p), int(ascending),
                      out.ctypes.data_as(C.c_void_p))
    return out.tolist()


OK, START, DECREASE, OUTSIDE, ORDER = range(5)
# name -> (n_cols, indptr, indices, ascending, [kind, row, value])
CSR_TABLE = {
    "no_cells": (5, [0, 0, 0], [], True, [OK, -1, 0]),
    "ok_sorted": (5, [0, 2, 2, 5], [0, 4, 1, 2, 3], True, [OK, -1, 0]),
    "ok_unsorted_atomic": (5, [0, 2, 2, 5], [4, 0, 3, 3, 1], False, [OK, -1, 0]),
    "first_indptr": (5, [1, 2, 3], [0, 1, 2], False, [START, -1, 1]),
    "indptr_decreases": (5, [0, 2, 1, 3], [0, 1, 2], False, [DECREASE, 1, 1]),
    "id_at_n_cols": (5, [0, 1, 3], [0, 1, 5], False, [OUTSIDE, 1, 5]),
    "id_negative": (5, [0, 1, 3], [-2, 1, 2], True, [OUTSIDE, 0, -2]),
    "unsorted_exact": (5, [0, 2, 2, 5], [4, 0, 1, 2, 3], True, [ORDER, 0, 0]),
    "column_twice_exact": (5, [0, 2, 2, 5], [0, 4, 1, 3, 3], True, [ORDER, 2, 3]),
    "pointers_before_ids": (5, [0, 3, 2], [9, 1, 2], True, [DECREASE, 1, 2]),
    "first_row_wins": (5, [0, 2, 4], [1, 0, 7, 2], True, [ORDER, 0, 0]),
}


def test_the_csr_check_names_the_first_bad_row(shim):
    seen = set()
    for name, (n_cols, indptr, indices, ascending, want) in CSR_TABLE.items():
        assert _finding(shim, n_cols, indptr, indices, ascending) == want, name
        seen.add(want[0])
    assert seen == {OK, START, DECREASE, OUTSIDE, ORDER}


def test_the_spare_buffers_grow_by_a_quarter_and_never_shrink(shim):
    assert [shim.sp_spare_cells(h, n) for h, n in ((0, 0), (0, 7), (100, 100), (100, 3), (100, 101), (100, 125), (100, 126), (100, 1000))] == \
        [0, 7, 100, 100, 125, 125, 126, 1000]
    assert shim.sp_slim_w_cells_bound(26744, 200) == 26744 * 200 and shim.sp_slim_w_cells_bound(200, 500) == 200 * 200
    assert shim.sp_slim_w_cells_bound(65535, 4096) < 2 ** 31


def test_the_byte_accounting_of_the_three_calls(shim):
    def figures(n_rows, nnz, cuts_cells, store_bytes):
        out = np.zeros(4, np.float64)
        shim.sp_bytes(n_rows, nnz, cuts_cells, store_bytes, out.ctypes.data_as(C.c_void_p))
        return out.tolist()

    csr = lambda n, nnz: 4.0 * (n + 1) + 8.0 * nnz
    exact = lambda n, nnz, cells: 2 * (4.0 * (n + 1) + 4.0 * nnz) + 4.0 * cells
    assert figures(200, 3000, 0, 160000.0) == [csr(200, 3000), 4.0 * 201, csr(200, 3000), 160000.0 + 2 * csr(200, 3000)]
    assert figures(200, 3000, 3400, 160000.0) == [csr(200, 3000) + exact(200, 3000, 3400), 4.0 * 201, csr(200, 3000),
                                                  160000.0 + 2 * csr(200, 3000) + exact(200, 3000, 3400)]
    assert figures(26744, 5348800, 0, 0.0)[3] == 2 * csr(26744, 5348800)


def test_plan_program_under_address_and_undefined_behaviour_sanitizers(build_dir):
    exe = build_dir / "spscorer_plan_main"
    # (the sanitizers' runtimes are linked into the program, so that it does not depend on the order the loader finds libraries in)
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer",
                    "-static-libasan", "-static-libubsan", os.path.join(HERE, "spscorer_plan_main.cpp"), "-o", str(exe)], check=True)
    done = subprocess.run([str(exe)], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert done.returncode == 0, done.stdout[-4000:]
    assert "spscorer_plan_main: OK" in done.stdout
