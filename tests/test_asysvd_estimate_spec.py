"""What AsySVD's device estimate of the user factors promises without a device.

The arithmetic: a NumPy model of the recurrence the kernel runs -- per cell, in storage order, product rounded before the add, one
division -- is `URM.dot(Y)` followed by the row division BIT FOR BIT on every case, which pins what "SciPy's arithmetic" means on the
machine the tests run on; and six planted faults (another order, a fused multiply-add, float32 sums, a reciprocal, a float32 divisor)
each differ from it bitwise on the same inputs, so that the equality the GPU tests assert means something.
The plan header csrc/asy_estimate_plan.h through a shim and once more as a program of its own under the host sanitizers.
The surface: both C-ABI entries declared, exported and bound; the `user_factor_estimate` attribute and its refusal."""
import ctypes as C
import os
import re
import subprocess
from fractions import Fraction

import numpy as np
import pytest

from recsys2019_deeplearning_evaluation_amd import MatrixFactorization_AsySVD_MI355X, MatrixFactorization_MI355X_Epoch, _native
from recsys2019_deeplearning_evaluation_amd import recommender_base as RB
from recsys2019_deeplearning_evaluation_amd.reference_binding import bind
from asysvd_estimate_cases import (ADV_COLS, ADV_LENGTHS, CASES, EMPTY_ROWS, FULL_ROW, K_LIST, K_MAX, SINGLE_ROW, URM_ADVERSARIAL, URM_TRAIN,
                                   draw_Y, host_estimate, reference)

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
ENTRIES = {"mi355rec_mf_asy_user_factors": 3, "mi355rec_asy_user_factors": 9}


def _bound(**kwargs):
    return bind(RB.BaseMatrixFactorizationRecommender, RB.BaseItemSimilarityMatrixRecommender, RB.BaseUserSimilarityMatrixRecommender,
                RB.Incremental_Training_Early_Stopping, **kwargs)


# ---- the recurrence ------------------------------------------------------------------------------------------------------------------

def model(URM, Y, order="storage", accumulate=np.float64, divide="divide", divisor_type=np.float64):
    """The kernel's recurrence in NumPy: a loop over the cells of a row (every factor of the row at once: the factors are independent
    chains), explicit float64 operations.  The keywords plant the faults."""
    out = np.zeros((URM.shape[0], Y.shape[1]), np.float64)
    length_sqrt = np.sqrt(np.ediff1d(URM.indptr))
    for u in range(URM.shape[0]):
        cells = np.arange(URM.indptr[u], URM.indptr[u + 1])
        if order == "reversed":
            cells = cells[::-1]
        elif order == "sorted":
            cells = cells[np.argsort(URM.indices[cells], kind="stable")]
        acc = np.zeros(Y.shape[1], accumulate)                                      # +0.0
        for t in cells:
            product = np.multiply(np.float64(URM.data[t]), Y[URM.indices[t]]).astype(accumulate)     # rounded on its own
            acc = np.add(acc, product)
        acc = acc.astype(np.float64)
        d = np.float64(divisor_type(length_sqrt[u]))
        if d > 0:
            acc = np.divide(acc, d) if divide == "divide" else np.multiply(acc, np.float64(1.0) / d)
        out[u] = acc
    return out


def model_fma(URM, Y):
    """The same with acc = fma(a, y, acc): ONE rounding of the exact a * y + acc, modelled with rationals."""
    out = np.zeros((URM.shape[0], Y.shape[1]), np.float64)
    length_sqrt = np.sqrt(np.ediff1d(URM.indptr))
    for u in range(URM.shape[0]):
        for f in range(Y.shape[1]):
            acc = 0.0
            for t in range(URM.indptr[u], URM.indptr[u + 1]):
                acc = float(Fraction(float(URM.data[t])) * Fraction(float(Y[URM.indices[t], f])) + Fraction(acc))
            out[u, f] = acc / length_sqrt[u] if length_sqrt[u] > 0 else acc
    return out


@pytest.mark.parametrize("case", sorted(CASES))
def test_the_recurrence_model_is_scipy_bit_for_bit(case):
    for k in K_LIST:
        Y, want = reference(case, k)
        got = model(CASES[case], Y)
        assert got.tobytes() == want.tobytes(), (case, k)
        empty = want[EMPTY_ROWS[case]]
        assert not empty.any() and not np.signbit(empty).any()                      # the empty profile: +0.0, never divided


def test_the_cases_are_what_the_kernel_can_get_wrong():
    X = URM_ADVERSARIAL
    lengths = np.ediff1d(X.indptr)
    assert not X.has_sorted_indices and not CASES["hand_off_unsorted"].has_sorted_indices and URM_TRAIN.has_sorted_indices
    assert lengths[FULL_ROW] == ADV_COLS and sorted(X.indices[X.indptr[FULL_ROW]:X.indptr[FULL_ROW + 1]]) == list(range(ADV_COLS))
    assert lengths[EMPTY_ROWS["adversarial"]] == 0 and lengths[SINGLE_ROW] == 1
    assert all(lengths[r] == n for r, n in ADV_LENGTHS.items())
    assert {200, 50, 63, 64, 65, 7, 8, 9} <= set(lengths.tolist())                 # a 64-cell chunk and 8 loads in flight, from both sides
    assert np.array_equal(CASES["hand_off_unsorted"].toarray(), URM_TRAIN.toarray())
    Y = draw_Y(ADV_COLS, 8)
    assert (Y > 0).any() and (Y < 0).any() and np.log10(np.abs(Y).max() / np.abs(Y).min()) > 12
    assert K_LIST[-1] == K_MAX == 256 and set(K_LIST) >= {1, 3, 8, 63, 64, 65}


FAULTS = {
    "reversed_order": dict(order="reversed"),
    "sorted_order_on_the_unsorted_case": dict(order="sorted"),
    "float32_accumulation": dict(accumulate=np.float32),
    "multiply_by_a_reciprocal": dict(divide="reciprocal"),
    "divisor_rounded_to_float32": dict(divisor_type=np.float32),
}


@pytest.mark.parametrize("fault", sorted(FAULTS))
def test_a_planted_fault_differs_from_scipy_bitwise(fault):
    for case in ("adversarial", "hand_off_unsorted"):
        Y, want = reference(case, 8)
        got = model(CASES[case], Y, **FAULTS[fault])
        assert got.shape == want.shape and got.tobytes() != want.tobytes(), (fault, case)
        if fault != "float32_accumulation":
            np.testing.assert_allclose(got, want, rtol=1e-6, atol=1e-7 * np.abs(want).max())     # the same numbers, other low bits


def test_a_fused_multiply_add_differs_from_scipy_bitwise():
    X = URM_ADVERSARIAL[:8]                 # 200, 50, 64, every column, 65, 63, 7 and 8 cells: about 650 exact cells x 3 factors
    Y = draw_Y(ADV_COLS, 3)
    want = host_estimate(X, Y)
    assert model(X, Y).tobytes() == want.tobytes()
    fused = model_fma(X, Y)
    assert fused.tobytes() != want.tobytes()
    np.testing.assert_allclose(fused, want, rtol=1e-6, atol=1e-7 * np.abs(want).max())


# ---- csrc/asy_estimate_plan.h ------------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def build_dir(tmp_path_factory):
    return tmp_path_factory.mktemp("asy_estimate_plan")


@pytest.fixture(scope="module")
def shim(build_dir):
    so = os.path.join(str(build_dir), "asy_estimate_plan_shim.so")
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-shared", "-fPIC", os.path.join(HERE, "asy_estimate_plan_shim.cpp"), "-o", so], check=True)
    lib = C.CDLL(so)
    lib.ae_layout.argtypes = [C.c_int64, C.c_int, C.c_void_p]
    lib.ae_constants.argtypes = [C.c_void_p]
    lib.ae_check_shape.argtypes, lib.ae_check_shape.restype = [C.c_int64, C.c_int64, C.c_int], C.c_int
    lib.ae_check_csr.argtypes = [C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]
    lib.ae_longest_first.argtypes = [C.c_int, C.c_void_p, C.c_void_p]
    lib.ae_bytes.argtypes, lib.ae_bytes.restype = [C.c_int64, C.c_int64, C.c_int], C.c_double
    return lib


def _layout(shim, n_rows, k):
    out = np.zeros(6, np.int64)
    shim.ae_layout(n_rows, k, out.ctypes.data_as(C.c_void_p))
    return out.tolist()


def test_plan_constants_and_the_lane_layout_of_the_k_list(shim):
    consts = np.zeros(4, np.int32)
    shim.ae_constants(consts.ctypes.data_as(C.c_void_p))
    assert consts.tolist() == [K_MAX, 256, 64, 8]
    # k -> factors per lane, lanes of a group, column tiles, items of a 256-lane workgroup; then items and grid for 300 rows
    want = {1: (1, 1, 1, 256), 3: (1, 4, 1, 64), 8: (2, 4, 1, 64), 63: (1, 64, 1, 4), 64: (2, 32, 1, 8), 65: (1, 64, 2, 4),
            128: (2, 64, 1, 4), 256: (2, 64, 2, 4)}
    assert set(K_LIST) <= set(want)
    for k, (vec, group, tiles, per_block) in want.items():
        items = 300 * tiles
        assert _layout(shim, 300, k) == [vec, group, tiles, per_block, items, -(-items // per_block)], k
    assert _layout(shim, 138493, 128)[4:] == [138493, 34624]


def test_plan_argument_checks(shim):
    OK, EMPTY, K_RANGE = range(3)
    table = [((300, 200, 1), OK), ((300, 200, K_MAX), OK), ((300, 200, K_MAX + 1), K_RANGE), ((300, 200, 0), K_RANGE),
             ((0, 200, 8), EMPTY), ((300, 0, 8), EMPTY), ((2 ** 31 - 1, 200, 255), OK)]
    for args, want in table:
        assert shim.ae_check_shape(*args) == want, args
    assert max(_layout(shim, 2 ** 31 - 1, k)[5] for k in range(1, K_MAX + 1)) == 2 ** 31 - 1      # never more workgroups than rows

    def finding(n_cols, indptr, indices):
        indptr, indices, out = np.array(indptr, np.int32), np.array(indices, np.int32), np.zeros(3, np.int64)
        shim.ae_check_csr(len(indptr) - 1, n_cols, indptr.ctypes.data_as(C.c_void_p), indices.ctypes.data_as(C.c_void_p), out.ctypes.data_as(C.c_void_p))
        return out.tolist()

    assert finding(5, [0, 3, 3, 5], [4, 0, 4, 2, 1]) == [0, -1, 0]                 # unsorted, a column twice: taken as stored
    assert finding(5, [0, 0, 0], []) == [0, -1, 0]
    assert finding(5, [1, 2, 3], [0, 1, 2]) == [1, -1, 1]
    assert finding(5, [0, 2, 1, 3], [0, 1, 2]) == [2, 1, 1]
    assert finding(5, [0, 1, 3], [0, 1, 5]) == [3, 1, 5]
    assert finding(5, [0, 1, 3], [-2, 1, 2]) == [3, 0, -2]


def test_plan_hands_the_rows_out_longest_first(shim):
    for X in CASES.values():
        indptr = np.ascontiguousarray(X.indptr, np.int32)
        order = np.full(X.shape[0], -1, np.int32)
        shim.ae_longest_first(X.shape[0], indptr.ctypes.data_as(C.c_void_p), order.ctypes.data_as(C.c_void_p))
        assert order.tolist() == np.argsort(-np.ediff1d(indptr), kind="stable").tolist()


def test_plan_bytes(shim):
    assert shim.ae_bytes(0, 3, 4) == 96.0
    for nnz, n_rows, k in ((2400, 300, 8), (20000263, 138493, 128), (20000263, 138493, 256)):
        assert shim.ae_bytes(nnz, n_rows, k) == nnz * (k * 8 + 8) + n_rows * k * 8


def test_plan_program_under_address_and_undefined_behaviour_sanitizers(build_dir):
    exe = build_dir / "asy_estimate_plan_main"
    # (the sanitizers' runtimes are linked into the program, so that it does not depend on the order the loader finds libraries in)
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer",
                    "-static-libasan", "-static-libubsan", os.path.join(HERE, "asy_estimate_plan_main.cpp"), "-o", str(exe)], check=True)
    done = subprocess.run([str(exe)], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert done.returncode == 0, done.stdout[-4000:]
    assert "asy_estimate_plan_main: OK" in done.stdout


# ---- the C ABI and the Python surface ------------------------------------------------------------------------------------------------------

def _declarations():
    text = open(os.path.join(ROOT, "include", "mi355rec.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return {name: [a.strip() for a in args.split(",")] for name, args in re.findall(r"\bint\s+(mi355rec_[a-z_]*asy_user_factors)\s*\(([^)]*)\)\s*;", text)}


def test_the_header_declares_both_entries():
    decl = _declarations()
    assert decl["mi355rec_mf_asy_user_factors"] == ["mi355rec_mf_t h", "const double *row_divisor", "double *out"]
    assert decl["mi355rec_asy_user_factors"] == ["int32_t n_rows", "int32_t n_items", "int32_t k", "const int32_t *indptr", "const int32_t *indices",
                                                 "const float *data", "const double *Y", "const double *row_divisor", "double *out"]


def test_native_binds_both_entries_and_they_refuse_null_before_the_device():
    decl = _declarations()
    for name, n_args in ENTRIES.items():
        restype, argtypes = _native.SIGNATURES[name]
        assert restype is C.c_int and len(argtypes) == n_args == len(decl[name]), name
    lib = _native.load()
    for name, n_args in ENTRIES.items():
        fn = getattr(lib, name)
        assert fn.restype is C.c_int and len(fn.argtypes) == n_args
    assert lib.mi355rec_mf_asy_user_factors(None, None, None) == _native.E_INVALID
    assert lib.mi355rec_last_error().decode() == "NULL argument"
    assert lib.mi355rec_asy_user_factors(3, 3, 2, None, None, None, None, None, None) == _native.E_INVALID
    assert lib.mi355rec_last_error().decode() == "NULL argument"


def _stateless(X, Y, out, n_items=None, k=None, indptr=None, indices=None):
    indptr = np.ascontiguousarray(X.indptr if indptr is None else indptr, np.int32)
    indices = np.ascontiguousarray(X.indices if indices is None else indices, np.int32)
    data, divisor = np.ascontiguousarray(X.data, np.float32), np.sqrt(np.ediff1d(X.indptr)).astype(np.float64)
    p = _native.ptr
    return _native.load().mi355rec_asy_user_factors(X.shape[0], X.shape[1] if n_items is None else n_items, Y.shape[1] if k is None else k, p(indptr),
                                                    p(indices), p(data), p(Y), p(divisor), p(out))


def test_the_stateless_entry_refuses_bad_arguments_before_the_device_and_leaves_the_output_alone():
    X, Y = URM_ADVERSARIAL, np.ascontiguousarray(draw_Y(ADV_COLS, 4))
    out = np.full((X.shape[0], 4), 7.25)
    error = lambda: _native.load().mi355rec_last_error().decode()
    late, back, ids = X.indptr.copy(), X.indptr.copy(), X.indices.copy()
    late[0], back[5], ids[-1] = 1, back[4] - 1, ADV_COLS
    assert _stateless(X, Y, out, indptr=late) == _native.E_INVALID and "start at 1" in error()
    assert _stateless(X, Y, out, indptr=back) == _native.E_INVALID and "decrease at row 4" in error()
    assert _stateless(X, Y, out, indices=ids) == _native.E_INVALID and "row 39 stores the column id 210, outside [0, 210)" in error()
    ids[-1], ids[0] = X.indices[-1], -1
    assert _stateless(X, Y, out, indices=ids) == _native.E_INVALID and "row 0 stores the column id -1" in error()
    assert _stateless(X, Y, out, n_items=0) == _native.E_INVALID and "empty URM" in error()
    assert _stateless(X, Y, out, k=0) == _native.E_INVALID and "n_factors must be >= 1" in error()
    assert _stateless(X, Y, out, k=K_MAX + 1) == _native.E_UNSUPPORTED and "exceeds 256" in error()
    assert (out == 7.25).all()


def test_the_estimate_mode_defaults_to_host_on_the_package_class_and_the_bound_class():
    for cls in (MatrixFactorization_AsySVD_MI355X, _bound().MatrixFactorization_AsySVD_MI355X, _bound(device_scoring=False).MatrixFactorization_AsySVD_MI355X):
        assert cls.user_factor_estimate == "host" and cls.USER_FACTOR_ESTIMATE_MODES == ("host", "device"), cls
        assert cls(URM_TRAIN, verbose=False).user_factor_estimate == "host"
    import recsys2019_deeplearning_evaluation_amd as pkg
    assert callable(pkg.asysvd_user_factors) and "asysvd_user_factors" in pkg.__all__
    assert callable(MatrixFactorization_MI355X_Epoch.estimate_user_factors)


@pytest.mark.parametrize("bound", [False, True])
def test_an_unknown_estimate_mode_is_a_value_error_before_the_library_is_loaded(monkeypatch, bound):
    def load():
        raise AssertionError("the native library was loaded")
    monkeypatch.setattr(_native, "load", load)
    cls = _bound().MatrixFactorization_AsySVD_MI355X if bound else MatrixFactorization_AsySVD_MI355X
    rec = cls(URM_TRAIN, verbose=False)
    rec.user_factor_estimate = "hbm"
    with pytest.raises(ValueError, match="user_factor_estimate must be one of"):
        rec.fit(epochs=1, num_factors=4)
    assert not hasattr(rec, "epoch_kernel")
    rec.ITEM_factors_Y_best = np.zeros((URM_TRAIN.shape[1], 4))
    with pytest.raises(ValueError, match="user_factor_estimate must be one of"):
        rec.set_URM_train(URM_TRAIN, estimate_item_similarity_for_cold_users=True)
