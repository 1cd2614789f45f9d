"""DIVERSITY_SIMILARITY without a GPU: the float64 restatement of tests/diversity_cases.py against the reference's values
(tests/golden/evaluator_diversity.npz, written by tests/golden/make_diversity_fixture.py from the reference's own evaluators and
Diversity_similarity), what `diversity_matrix_of` accepts and refuses, and the index arithmetic of csrc/eval_plan.h through a g++
shim (tests/eval_plan_shim.cpp) and once more as a program of its own under the address and undefined-behaviour sanitizers
(tests/eval_plan_main.cpp)."""
import ctypes as C
import itertools
import os
import subprocess

import numpy as np
import pytest
import scipy.sparse as sps

from diversity_cases import CASES, CUTOFFS, diversity_of_list, diversity_per_user, list_lengths, make_case
from recsys2019_deeplearning_evaluation_amd.evaluation import (DIVERSITY_MAX_WIDTH, METRICS, METRICS_WITH_DIVERSITY, diversity_matrix_of,
                                                               get_result_string)
from _util import GOLDEN

HERE = os.path.dirname(os.path.abspath(__file__))
FIXTURE = np.load(GOLDEN + "/evaluator_diversity.npz")
CUTOFF_LISTS = ([2, 3, 5], [10, 2, 65, 64, 130])


def reference_bounds(name):
    """Relative bound of a per-user value and of the metric against the reference's stored ones, [n_users][n_cutoffs] and a number per
    cutoff.  float64 matrix: both sides sum the same <= L^2 non-negative terms in float64, each sum within L^2 * 2^-53 of the exact
    one.  float32 matrix: under NEP 50 the reference accumulates a list in float32 (np.sum of a float32 row added to a Python float
    stays float32) and the users in float32 too."""
    L = list_lengths(FIXTURE[name + "_lists"], FIXTURE[name + "_cutoffs"]).astype(np.float64)
    if FIXTURE[name + "_D"].dtype == np.float64:
        return 2 * L ** 2 * 2.0 ** -53, 2 * L.max(axis=0) ** 2 * 2.0 ** -53 + len(L) * 2.0 ** -53
    return (L ** 2 + len(L)) * 2.0 ** -24, (L.max(axis=0) ** 2 + len(L)) * 2.0 ** -24


# ---- the restatement against the reference ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", CASES)
def test_restatement_matches_the_reference_per_user_and_per_cutoff(name):
    case = make_case(name)
    D, lists, cutoffs = FIXTURE[name + "_D"], FIXTURE[name + "_lists"], FIXTURE[name + "_cutoffs"].tolist()
    assert cutoffs == CUTOFFS[name] == case["cutoffs"] and np.array_equal(D, case["D"]) and D.dtype == case["D"].dtype
    if "lists" in case:
        assert np.array_equal(lists, case["lists"][FIXTURE[name + "_users"]])
    mine, ref = diversity_per_user(D, lists, cutoffs), FIXTURE[name + "_per_user"]
    per_user_bound, metric_bound = reference_bounds(name)
    assert np.all(np.abs(mine - ref) <= per_user_bound * np.abs(ref)), np.max(np.abs(mine - ref) / np.abs(ref) / per_user_bound)
    metric = mine.sum(axis=0) / len(mine)
    assert np.all(np.abs(metric - FIXTURE[name + "_metric"]) <= metric_bound * FIXTURE[name + "_metric"])


def test_the_fixture_cases_can_tell_the_quirks_apart():
    """A transposed index, an included diagonal and an included last row each move every case's metric by far more than its bound."""
    for name in CASES:
        D, lists, cutoffs = FIXTURE[name + "_D"].astype(np.float64), FIXTURE[name + "_lists"], FIXTURE[name + "_cutoffs"].tolist()
        right = diversity_per_user(D, lists, cutoffs).mean(axis=0)
        transposed = diversity_per_user(D.T, lists, cutoffs).mean(axis=0)
        no_diagonal = D.copy()
        np.fill_diagonal(no_diagonal, 0.0)

        def with_last_row(items):
            return sum(no_diagonal[i, items].sum() for i in items) / (len(items) * (len(items) - 1))

        def with_diagonal(items):
            return sum(D[i, items].sum() for i in items[:-1]) / (len(items) * (len(items) - 1))
        for variant in (with_last_row, with_diagonal):
            wrong = np.array([[variant(row[row >= 0][:c]) for c in cutoffs] for row in lists]).mean(axis=0)
            assert np.all(np.abs(wrong - right) > 1e-3 * right), (name, variant.__name__)
        assert np.all(np.abs(transposed - right) > 1e-6 * right), name
        lengths = (lists >= 0).sum(axis=1)
        assert lengths.min() == 2 and min(cutoffs) >= 2 and max(cutoffs) > lengths.min()
    assert FIXTURE["holdout_f32_D"].dtype == np.float32 and FIXTURE["holdout_f64_D"].dtype == np.float64
    assert os.path.getsize(GOLDEN + "/evaluator_diversity.npz") <= 512 * 1024


def test_short_lists_divide_by_zero_as_the_reference_does():
    D = np.full((4, 4), 0.5)
    for items in ([], [2]):
        with pytest.raises(ZeroDivisionError):
            diversity_of_list(D, items)
    assert diversity_of_list(D, [2, 1]) == 0.25             # one row (the last position gives none), one cell, over 2 * 1


# ---- diversity_matrix_of ------------------------------------------------------------------------------------------------------------
class _DiversityLike:
    def __init__(self, matrix):
        self.item_diversity_matrix = matrix


def test_diversity_matrix_of_accepts():
    rng = np.random.default_rng(5)
    D = rng.random((6, 6))
    for given in (D, _DiversityLike(D)):
        got = diversity_matrix_of(given, 6)
        assert got is D
    f32 = D.astype(np.float32)
    assert diversity_matrix_of(f32, 6) is f32
    fortran = np.asfortranarray(D)
    got = diversity_matrix_of(_DiversityLike(fortran), 6)
    assert got.flags["C_CONTIGUOUS"] and got.dtype == np.float64 and np.array_equal(got, D)
    ints = (rng.random((6, 6)) < 0.5).astype(np.int32)
    for given in (ints, ints.astype(bool), ints.astype(np.float16), ints.astype(np.uint8)):
        got = diversity_matrix_of(given, 6)
        assert got.dtype == np.float64 and got.flags["C_CONTIGUOUS"] and np.array_equal(got, ints)
    assert diversity_matrix_of(np.array([[1.5]]), 1, check_values=False)[0, 0] == 1.5      # (the evaluators check on the device)


@pytest.mark.parametrize("given", [object(), None, [[0.5]], "matrix", sps.csr_matrix(np.eye(3)), sps.coo_matrix(np.eye(3)),
                                   np.matrix(np.eye(3)), _DiversityLike(sps.csr_matrix(np.eye(3))), _DiversityLike(np.matrix(np.eye(3))),
                                   _DiversityLike(object()), np.eye(3, dtype=np.complex128), np.array([["a"] * 3] * 3)],
                         ids=lambda g: type(getattr(g, "item_diversity_matrix", g)).__name__)
def test_diversity_matrix_of_refuses_what_is_no_dense_matrix(given):
    with pytest.raises(NotImplementedError):
        diversity_matrix_of(given, 3)


@pytest.mark.parametrize("case", ["rows", "columns", "one_dimension", "three_dimensions", "above_one", "below_zero", "nan", "nan_float32"])
def test_diversity_matrix_of_raises_value_error(case):
    D = np.full((5, 5), 0.5)
    given = {"rows": D[:4], "columns": D[:, :4], "one_dimension": np.full(25, 0.5), "three_dimensions": D.reshape(5, 5, 1)}.get(case)
    if given is None:
        given = D.astype(np.float32) if case.endswith("float32") else D
        given[3, 1] = {"above_one": 1.5, "below_zero": -0.1}.get(case, np.nan)
    with pytest.raises(ValueError):
        diversity_matrix_of(given, 5)
    with pytest.raises(ValueError):
        diversity_matrix_of(_DiversityLike(given), 5)


def test_metric_lists_and_result_string():
    at = METRICS_WITH_DIVERSITY.index("DIVERSITY_SIMILARITY")
    assert METRICS_WITH_DIVERSITY[at - 1] == "AVERAGE_POPULARITY" and METRICS_WITH_DIVERSITY[at + 1] == "DIVERSITY_MEAN_INTER_LIST"
    assert [m for m in METRICS_WITH_DIVERSITY if m != "DIVERSITY_SIMILARITY"] == METRICS and len(METRICS) == 18
    text = get_result_string({5: {m: 0.25 for m in METRICS_WITH_DIVERSITY}})
    assert "AVERAGE_POPULARITY: 0.2500000, DIVERSITY_SIMILARITY: 0.2500000, DIVERSITY_MEAN_INTER_LIST: " in text


# ---- csrc/eval_plan.h -------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def build_dir(tmp_path_factory):
    return tmp_path_factory.mktemp("eval_plan")


@pytest.fixture(scope="module")
def shim(build_dir):
    so = os.path.join(str(build_dir), "eval_plan_shim.so")
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-shared", "-fPIC", os.path.join(HERE, "eval_plan_shim.cpp"), "-o", so], check=True)
    lib = C.CDLL(so)
    for name in ("ep_cell_offset", "ep_run_cell", "ep_matrix_cells", "ep_matrix_bytes", "ep_value_cells", "ep_upload_chunks"):
        getattr(lib, name).restype = C.c_uint64
    lib.ep_cell_offset.argtypes = [C.c_int] * 3
    lib.ep_run_cell.argtypes = [C.c_int, C.c_void_p, C.c_int, C.c_int]
    lib.ep_run.argtypes = [C.c_int, C.c_void_p]
    lib.ep_upload_chunks.argtypes = [C.c_uint64]
    lib.ep_range_blocks.argtypes = [C.c_uint64]
    lib.ep_denominator.restype = C.c_double
    lib.ep_list_values.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p]
    return lib


def ptr(a):
    return a.ctypes.data_as(C.c_void_p)


def test_plan_constants_and_sizes(shim):
    out = np.zeros(3, np.int64)
    shim.ep_constants(ptr(out))
    assert out.tolist() == [DIVERSITY_MAX_WIDTH, 64, 256 << 20] == [1024, 64, 268435456]
    assert [shim.ep_width_ok(w) for w in (0, 1, 64, 65, 1024, 1025)] == [0, 1, 1, 1, 1, 0]
    assert [shim.ep_threads(w) for w in (1, 64, 65, 1024)] == [64, 64, 256, 256]
    assert [shim.ep_elem_ok(b) for b in (0, 2, 4, 8, 16)] == [0, 0, 1, 1, 0]
    for n, elem in itertools.product((1, 300, 26744, 46341, 2000000), (4, 8)):
        assert shim.ep_matrix_cells(n) == n * n and shim.ep_matrix_bytes(n, elem) == n * n * elem
    assert shim.ep_matrix_bytes(26744, 8) == 5721932288             # the ML-20M shape: 5.7 GB
    assert shim.ep_value_cells(138493, 64) == 138493 * 64 and shim.ep_value_cells(2 ** 31 - 1, 64) == (2 ** 31 - 1) * 64
    for nbytes in (0, 1, (256 << 20) - 1, 256 << 20, (256 << 20) + 1, 5721932288):
        assert shim.ep_upload_chunks(nbytes) == -(-nbytes // (256 << 20))
    for cells in (0, 1, 2048, 2049, 300 * 300, 26744 ** 2, 2 ** 40):
        assert shim.ep_range_blocks(cells) == max(1, min(4096, -(-cells // 2048)))


@pytest.mark.parametrize("n_items", [46340, 46341, 2000000])
def test_cell_offset_is_64_bit(shim, n_items):
    """items[i] * n_items passes 2^31 from 46 341 items on."""
    for row, col in itertools.product((0, 1, n_items // 2, n_items - 1), repeat=2):
        assert shim.ep_cell_offset(row, col, n_items) == row * n_items + col
    assert (shim.ep_cell_offset(n_items - 1, n_items - 1, n_items) >= 2 ** 31) == (n_items >= 46341)


def cells_of_runs(shim, len_, n_shells):
    """(i, j) of every cell of the runs of shells 1 .. n_shells, through div_run_cell on the list 0, 1, 2, ...: offset i * n + j."""
    n = 1 << 12
    items = np.arange(max(len_, 1), dtype=np.int32)
    cells, run = [], np.zeros(4, np.int32)
    for w in range(2 * n_shells):
        shim.ep_run(w, ptr(run))
        shell, fixed, count, column = run.tolist()
        assert shell == w // 2 + 1 and count == (shell if column else shell - 1) and column == (w % 2 == 0)
        for q in range(count):
            i, j = divmod(shim.ep_run_cell(w, ptr(items), q, n), n)
            assert shim.ep_shell(i, j) == shell and (i, j) == ((q, fixed) if column else (fixed, q))
            cells.append((i, j))
    return cells


def test_shells_and_cutoffs_against_a_brute_force_enumeration(shim):
    """For every list length 0 .. 70 and both cutoff lists: the runs of the shells a cutoff sums are exactly the cells of the
    reference's loop over the list's first min(cutoff, length) entries, each once."""
    seen = set()
    for len_ in range(71):
        assert shim.ep_run_count(len_) == (2 * (len_ - 1) if len_ >= 2 else 0)
        for cutoff in sorted(set(sum(CUTOFF_LISTS, []))):
            L = min(cutoff, len_)
            shells = shim.ep_cutoff_shells(cutoff, len_)
            assert shim.ep_cutoff_length(cutoff, len_) == L
            seen.add(("short" if L < 2 else "whole_list" if cutoff >= len_ else "cut", "wide" if L > 64 else "one_wave"))
            if L < 2:
                assert shells == -1
                continue
            assert shells == L - 1 and 2 * shells <= shim.ep_run_count(len_) and shim.ep_denominator(cutoff, len_) == L * (L - 1)
            brute = [(i, j) for i in range(L - 1) for j in range(L) if j != i]
            got = cells_of_runs(shim, len_, shells)
            assert len(got) == len(set(got)) == (L - 1) ** 2 and set(got) == set(brute), (len_, cutoff)
    assert seen == {("short", "one_wave"), ("whole_list", "one_wave"), ("cut", "one_wave"), ("whole_list", "wide"), ("cut", "wide")}
    # a cell's shell is the smallest list length that holds it, less one
    for i, j in itertools.product(range(12), repeat=2):
        if i != j:
            assert shim.ep_shell(i, j) == min(L for L in range(2, 14) if i <= L - 2 and j <= L - 1) - 1


@pytest.mark.parametrize("name", CASES)
def test_the_kernels_order_of_summation_is_within_the_bound_of_the_restatement(shim, name):
    """ep_list_values walks a list as the kernel does (runs, shells, running sum): within 4 L^2 2^-53 of the row-by-row restatement."""
    D = np.ascontiguousarray(FIXTURE[name + "_D"], dtype=np.float64)
    cutoffs = FIXTURE[name + "_cutoffs"]
    lists = FIXTURE[name + "_lists"].astype(np.int32)
    want = diversity_per_user(D, lists, cutoffs.tolist())
    L = list_lengths(lists, cutoffs)
    for r, row in enumerate(lists):
        items = np.ascontiguousarray(row[row >= 0])
        out, runs = np.zeros(len(cutoffs)), np.zeros(max(1, 2 * (len(items) - 1)))
        shim.ep_list_values(ptr(D), len(D), ptr(items), len(items), ptr(cutoffs), len(cutoffs), ptr(runs), ptr(out))
        assert np.all(np.abs(out - want[r]) <= 4 * L[r] ** 2 * 2.0 ** -53 * want[r]), r
    single = np.zeros(2)
    shim.ep_list_values(ptr(D), len(D), ptr(np.array([3], np.int32)), 1, ptr(np.array([1, 5], np.int32)), 2, ptr(np.zeros(1)), ptr(single))
    assert np.isnan(single).all()


def test_plan_program_under_address_and_undefined_behaviour_sanitizers(build_dir):
    exe = build_dir / "eval_plan_main"
    # (the sanitizers' runtimes are linked into the program, so that it does not depend on the order the loader finds libraries in)
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer",
                    "-static-libasan", "-static-libubsan", os.path.join(HERE, "eval_plan_main.cpp"), "-o", str(exe)], check=True)
    done = subprocess.run([str(exe)], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert done.returncode == 0, done.stdout[-4000:]
    assert "eval_plan_main: OK" in done.stdout
