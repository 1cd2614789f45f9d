"""The host arithmetic under the PureSVD and NMF handles (csrc/blocks_plan.h) on the CPU.

A shim (tests/blocks_plan_shim.cpp) is compiled with g++ and called through ctypes on tables of inputs.  Every case
  * states the branch it must reach (named from the inputs alone), and each test asserts that the set of branches its table reached is
    complete, so that a case that stops reaching its branch fails,
  * is compared exactly with tests/golden/blocks_plan.npz -- recorded once by running the text of svd.hip and nmf.hip as it stood
    before this arithmetic became functions of its own (Side::build's loop and byte count, validate_layout, the two value scans of the
    create functions, GramPlan::make, spmm_enqueue's and lp_shift()'s width rule, enqueue_colsum, enqueue_dot, enqueue_sddmm, the sweep's
    launch numbers, the buffer sizes of the create functions, and every `launches +=` and finish_call of the step-wise calls, copied into
    a harness with a handle of plain numbers behind the same extern "C" interface as the shim) through record() below on these same
    tables; the fixture holds the tables, too, so a table that changes is noticed.
tests/blocks_plan_main.cpp goes through the header once more as a program of its own under the address and undefined-behaviour
sanitizers.
"""
import ctypes as C
import itertools
import os
import subprocess

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden", "blocks_plan.npz")

SPLIT, NT, GT, GR, RED_BLOCKS, CS_SLABS = 512, 256, 64, 16, 1024, 512
ROW_LIMIT = 128 * 65535
EPS32 = float(np.finfo(np.float32).eps)

# ---- the tables ---------------------------------------------------------------------------------------------------------------
ROW_LENGTHS = (0, 1, 511, 512, 513, 1023, 1024, 1025, 1537)
# both sides of each group width (16 | 32 | 64 lanes) and of each 64-wide Gram tile
WIDTHS = (1, 15, 16, 17, 31, 32, 33, 63, 64, 65, 128, 129, 4096)
WIDTH_TABLE = (0, -3) + WIDTHS + (4097,)
# 8388480 = 128 x 65535 rows is the most the block * matrix GEMM takes
ROWS = (1, 15, 16, 17, 63, 64, 65, 1000, 138493, ROW_LIMIT, ROW_LIMIT + 1)
GRAM_TABLE = list(itertools.product(ROWS, WIDTHS))
# the sweep's dynamic LDS is ceil(k / lanes) KiB: above 48 only with 64 lanes, from k = 3073 on
SWEEP_TABLE = list(itertools.product((1, 3, 4, 5, 8, 9, 16, 17, 1000, 138493), WIDTHS + (3072, 3073)))
DOT_TABLE = (0, 1, 1024, 1025, 2048, 1024 * 1024 - 1, 1024 * 1024, 1024 * 1024 + 1, 4096 * 4096, ROW_LIMIT * 4096)
PIECE_COUNTS = (0, 1, 3, 4, 5, 7, 8, 9, 15, 16, 17, 1000, 138493, 20000263 // 512 + 138493)
# n_users, n_items, pieces of the users' layout, of the items' layout
RED_SHAPES = [(1, 1, 1, 1), (5, 1100, 8, 1100), (1100, 5, 1100, 8), (3, 70000, 70000, 70000), (138493, 26744, 150000, 60000),
              (ROW_LIMIT, 1, ROW_LIMIT, ROW_LIMIT), (4, 4, 4100, 4), (10, 10, 5, 9000)]
# n_users, n_items, slots of either layout
SIZE_SHAPES = [(1, 1, 0, 0), (5, 1100, 8, 0), (1100, 5, 0, 8), (138493, 26744, 3, 70000), (ROW_LIMIT, 17, 0, 5)]
# n_users, n_items, nnz, long rows of either layout
ACCOUNT_SHAPES = [(5, 1100, 2051, 3, 0), (138493, 26744, 20000263, 2500, 4000), (7, 3, 0, 0, 0)]
ACCOUNT_WIDTHS = (1, 17, 210)


def ptr(a):
    return a.ctypes.data_as(C.c_void_p)


def ragged_layout(lengths):
    """row pointers and indices of a matrix whose row i holds its first lengths[i] columns, and of its transpose"""
    import scipy.sparse as sps
    n_cols = max(1, max(lengths, default=0))
    ptr_ = np.concatenate([[0], np.cumsum(lengths)]).astype(np.int32)
    idx = np.concatenate([np.arange(n, dtype=np.int32) for n in lengths] + [np.zeros(0, np.int32)])
    X = sps.csr_matrix((np.ones(len(idx), np.float32), idx, ptr_), shape=(len(lengths), n_cols))
    Xt = sps.csr_matrix(X.T)
    Xt.sort_indices()
    return (ptr_, idx), (Xt.indptr.astype(np.int32), Xt.indices.astype(np.int32))


(RAGGED, RAGGED_T), (EMPTY, EMPTY_T) = ragged_layout(ROW_LENGTHS), ragged_layout((0, 0, 0))
PIECE_LAYOUTS = {"ragged": RAGGED[0], "transpose": RAGGED_T[0], "empty": EMPTY[0], "empty_transpose": EMPTY_T[0]}


def i32(*v):
    return np.array(v, np.int32)


# name -> (n, n_other, row pointers, indices)
LAYOUT_TABLE = {
    "ok": (3, 4, i32(0, 2, 2, 3), i32(0, 3, 1)),
    "ok_no_cells": (2, 5, i32(0, 0, 0), i32()),
    "start_not_zero": (2, 4, i32(1, 2, 3), i32(0, 1, 2)),
    "decrease_first": (3, 4, i32(0, -1, 2, 3), i32(0, 1, 2)),
    "decrease_last": (3, 4, i32(0, 2, 3, 1), i32(0, 1, 2)),
    "index_negative": (2, 4, i32(0, 1, 3), i32(2, -7, 0)),
    "index_at_the_end": (2, 4, i32(0, 1, 3), i32(3, 0, 4)),
    # the first finding wins: pointers before indices, the earlier index before the later
    "decrease_and_index": (2, 4, i32(0, 3, 2), i32(9, 1, 2)),
    "two_indices": (2, 4, i32(0, 1, 3), i32(5, 6, 1)),
}


def f32(*v):
    return np.array(v, np.float32)


VALUE_TABLE = {
    "no_cells": f32(),
    "all_ones": f32(1, 1, 1, 1, 1),
    "one_above_one": f32(1, 1, 1.0000001, 1),
    "negative_first": f32(-1, 2, 3),
    "negative_last": f32(1, 1, 1, -0.5),
    "two_negatives": f32(2, -3, -4),
    "not_a_number": f32(1, np.nan, 2),
    "zeros": f32(0, 0, 1, 0),
    "at_eps": f32(EPS32, 1, EPS32),
    "above_eps": f32(np.nextafter(np.float32(EPS32), np.float32(1)), 1, 0.5),
    "sum_order": f32(1e8, 1, -0.0, 1e-8, 3, 1e8),
}
assert VALUE_TABLE["one_above_one"][2] != 1.0


# ---- running them -------------------------------------------------------------------------------------------------------------
def declare(lib):
    lib.bp_constants.argtypes = [C.c_void_p]
    lib.bp_width.argtypes = [C.c_int, C.c_void_p]
    lib.bp_rows_in_range.argtypes = [C.c_int, C.c_int]
    lib.bp_pieces.argtypes = [C.c_void_p, C.c_int, C.c_int] + [C.c_void_p] * 8
    lib.bp_upload_bytes.argtypes = [C.c_int64, C.c_int, C.c_int64, C.c_int64]
    lib.bp_upload_bytes.restype = C.c_int64
    lib.bp_layout.argtypes = [C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]
    lib.bp_values.argtypes = [C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p]
    lib.bp_gram.argtypes = [C.c_int, C.c_int, C.c_void_p]
    lib.bp_colsum.argtypes = [C.c_int, C.c_void_p]
    lib.bp_dot_blocks.argtypes = [C.c_int64]
    lib.bp_cell_grid.argtypes = [C.c_int64]
    lib.bp_sweep.argtypes = [C.c_int, C.c_int, C.c_void_p]
    lib.bp_piece_grids.argtypes = [C.c_int, C.c_int, C.c_void_p]
    lib.bp_red_part_cells.argtypes = [C.c_int] * 4
    lib.bp_red_part_cells.restype = C.c_int64
    lib.bp_sizes.argtypes = [C.c_int] * 5 + [C.c_void_p]
    lib.bp_accounting.argtypes = [C.c_int, C.c_int, C.c_int64, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]
    return lib


def call(fn, n_out, *args):
    out = np.zeros(n_out, np.int64)
    fn(*args, ptr(out))
    return out


def pieces_of(lib, row_ptr):
    """(row, begin, end, slot), (long_row, long_first, long_count), (pieces, long rows, slots, upload bytes)"""
    n = len(row_ptr) - 1
    room = n + int(row_ptr[-1]) // SPLIT + 1
    tables = [np.full(room, -9, np.int32) for _ in range(7)]
    counts = np.zeros(4, np.int64)
    assert lib.bp_pieces(ptr(row_ptr), n, room, *[ptr(t) for t in tables], ptr(counts)) == 1
    return [t[:counts[0]] for t in tables[:4]], [t[:counts[1]] for t in tables[4:]], counts


def values_of(lib, values):
    flags, sums = np.zeros(4, np.int64), np.zeros(3, np.float64)
    lib.bp_values(ptr(values), len(values), ptr(flags), ptr(sums))
    return flags, sums


ACCOUNT_COUNTS = (["set_block_bytes_0", "set_block_bytes_1", "gram_d2h_bytes", "apply_h2d_bytes", "permutation_bytes", "scalar_bytes",
                   "product_0", "product_1", "gram", "apply", "fill"]
                  + ["sweep_reuse%d_side%d" % rs for rs in itertools.product((0, 1), (0, 1))]
                  + ["mu_loss%d_reuse%d_side%d" % lrs for lrs in itertools.product((0, 1), (0, 1), (0, 1))]
                  + ["divergence_loss0", "divergence_loss1"])
ACCOUNT_FIGURES = ["product", "sweep_0", "sweep_1", "mu_frobenius_0", "mu_frobenius_1", "mu_kl", "fill_0", "fill_1", "divergence"]


def accounting_of(lib, n_users, n_items, nnz, r, long_users, long_items):
    """name -> launches or PCIe bytes, name -> (algorithmic bytes, flops)"""
    counts, figures = np.zeros(len(ACCOUNT_COUNTS), np.int64), np.zeros(2 * len(ACCOUNT_FIGURES), np.float64)
    lib.bp_accounting(n_users, n_items, nnz, r, ptr(i32(long_users, long_items)), ptr(counts), ptr(figures))
    return dict(zip(ACCOUNT_COUNTS, counts.tolist())), dict(zip(ACCOUNT_FIGURES, figures.reshape(-1, 2).tolist())), counts, figures


def record(lib):
    """name -> array, as the fixture holds them"""
    declare(lib)
    out = {}
    out["constants/result"] = call(lib.bp_constants, 11)
    out["width/table"], out["width/result"] = np.array(WIDTH_TABLE, np.int64), np.array([call(lib.bp_width, 5, r) for r in WIDTH_TABLE])
    for name, row_ptr in PIECE_LAYOUTS.items():
        pieces, long_rows, counts = pieces_of(lib, row_ptr)
        out["pieces/%s_row_ptr" % name] = row_ptr
        out["pieces/%s_pieces" % name], out["pieces/%s_long" % name], out["pieces/%s_counts" % name] = np.array(pieces), np.array(long_rows), counts
    out["pieces/upload_bytes"] = np.array([lib.bp_upload_bytes(nnz, ones, p, l) for nnz, ones, p, l in
                                           itertools.product((0, 2051, 20000263), (0, 1), (5, 150000), (0, 3))], np.int64)
    out["layout/table"] = np.array(list(LAYOUT_TABLE))
    for name, (n, n_other, p, idx) in LAYOUT_TABLE.items():
        out["layout/%s_in" % name] = np.concatenate([[n, n_other], p, idx]).astype(np.int64)
    out["layout/result"] = np.array([call(lib.bp_layout, 3, n, n_other, ptr(p), ptr(idx) if len(idx) else None) for n, n_other, p, idx in LAYOUT_TABLE.values()])
    out["values/table"] = np.array(list(VALUE_TABLE))
    for name, v in VALUE_TABLE.items():
        out["values/%s_in" % name] = v
    scans = [values_of(lib, v) for v in VALUE_TABLE.values()]
    out["values/flags"], out["values/sums"] = np.array([s[0] for s in scans]), np.array([s[1] for s in scans])
    out["gram/table"], out["gram/result"] = np.array(GRAM_TABLE, np.int64), np.array([call(lib.bp_gram, 3, n, r) for n, r in GRAM_TABLE])
    out["colsum/table"], out["colsum/result"] = np.array(ROWS, np.int64), np.array([call(lib.bp_colsum, 3, n) for n in ROWS])
    out["rows/in_range"] = np.array([lib.bp_rows_in_range(a, b) for a, b in itertools.product(ROWS, (1, ROW_LIMIT))], np.int64)
    out["dot/table"] = np.array(DOT_TABLE, np.int64)
    out["dot/result"] = np.array([[lib.bp_dot_blocks(n), lib.bp_cell_grid(min(n, 2 ** 31))] for n in DOT_TABLE], np.int64)
    out["sweep/table"], out["sweep/result"] = np.array(SWEEP_TABLE, np.int64), np.array([call(lib.bp_sweep, 5, n, k) for n, k in SWEEP_TABLE])
    grids = list(itertools.product(PIECE_COUNTS, WIDTHS))
    out["grids/table"], out["grids/result"] = np.array(grids, np.int64), np.array([call(lib.bp_piece_grids, 2, p, r) for p, r in grids])
    red = [(nu, ni, pu, pi, k) for (nu, ni, pu, pi), k in itertools.product(RED_SHAPES, WIDTHS)]
    out["red/table"] = np.array(red, np.int64)
    out["red/result"] = np.array([lib.bp_red_part_cells(pu, pi, max(nu, ni), k) for nu, ni, pu, pi, k in red], np.int64)
    sizes = [s + (r,) for s, r in itertools.product(SIZE_SHAPES, (1, 64, 65, 210))]
    out["sizes/table"] = np.array(sizes, np.int64)
    out["sizes/result"] = np.array([call(lib.bp_sizes, 6, nu, ni, r, su, si) for nu, ni, su, si, r in sizes])
    accounts = [s + (r,) for s, r in itertools.product(ACCOUNT_SHAPES, ACCOUNT_WIDTHS)]
    out["accounting/table"] = np.array(accounts, np.int64)
    done = [accounting_of(lib, nu, ni, nnz, r, lu, li) for nu, ni, nnz, lu, li, r in accounts]
    out["accounting/counts"], out["accounting/figures"] = np.array([d[2] for d in done]), np.array([d[3] for d in done])
    return out


FAMILIES = ("constants", "width", "pieces", "layout", "values", "gram", "colsum", "rows", "dot", "sweep", "grids", "red", "sizes", "accounting")


def build_shim(directory):
    so = os.path.join(str(directory), "blocks_plan_shim.so")
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-shared", "-fPIC", os.path.join(HERE, "blocks_plan_shim.cpp"), "-o", so], check=True)
    return declare(C.CDLL(so))


@pytest.fixture(scope="module")
def build_dir(tmp_path_factory):
    return tmp_path_factory.mktemp("blocks_plan")


@pytest.fixture(scope="module")
def shim(build_dir):
    return build_shim(build_dir)


@pytest.fixture(scope="module")
def golden():
    return np.load(GOLDEN)


@pytest.fixture(scope="module")
def recorded(shim):
    return record(shim)


# ---- against the recorded results ---------------------------------------------------------------------------------------------
def test_the_fixture_has_exactly_these_arrays(golden, recorded):
    assert sorted(golden.files) == sorted(recorded)
    assert {name.split("/")[0] for name in recorded} == set(FAMILIES)
    assert os.path.getsize(GOLDEN) <= 128 * 1024


@pytest.mark.parametrize("name", FAMILIES)
def test_results_equal_the_recorded_results(golden, recorded, name):
    for key in sorted(k for k in recorded if k.startswith(name + "/")):
        want, got = golden[key], recorded[key]
        assert got.shape == want.shape and got.dtype == want.dtype, key
        same = (got == want) | ((got != got) & (want != want)) if got.dtype.kind == "f" else got == want
        assert same.all(), (key, np.argwhere(~same)[:5].tolist())


def test_constants(recorded):
    # SPLIT, SPMM_THREADS, GT, GR, NT, RED_BLOCKS, CS_SLABS, the width range, the row limit of the block * matrix GEMM, the sweep's LDS threshold
    assert recorded["constants/result"].tolist() == [512, 256, 64, 16, 256, 1024, 512, 1, 4096, 8388480, 48 * 1024]


# ---- the lane group and the grids it fixes ----------------------------------------------------------------------------------------
def shift_branch(r):
    return 4 if r <= 16 else (5 if r <= 32 else 6)


def test_group_width_and_per_width_grids(recorded):
    seen = set()
    for r, (shift, in_range, tiles, reduce_grid, columns) in zip(WIDTH_TABLE, recorded["width/result"].tolist()):
        branch = "below" if r < 1 else ("above" if r > 4096 else "inside")
        seen.add((branch, shift_branch(r)))
        assert in_range == (branch == "inside") and shift == shift_branch(r), r
        if branch == "inside":
            assert tiles == -(-r // GT) and reduce_grid == -(-r * r // 256) and columns == -(-r // NT), r
    assert seen == {("below", 4), ("inside", 4), ("inside", 5), ("inside", 6), ("above", 6)}
    assert [shift_branch(r) for r in (16, 17, 32, 33)] == [4, 5, 5, 6]


def test_product_and_sddmm_grids(recorded):
    seen = set()
    for (pieces, r), (product, sddmm) in zip(recorded["grids/table"].tolist(), recorded["grids/result"].tolist()):
        per_block = NT >> shift_branch(r)                      # pieces of a workgroup: 16, 8 or 4
        seen.add((per_block, "whole" if pieces % per_block == 0 else "ragged"))
        assert product == sddmm == -(-pieces // per_block), (pieces, r)
    assert seen == {(p, w) for p in (16, 8, 4) for w in ("whole", "ragged")}


# ---- the piece plan -----------------------------------------------------------------------------------------------------------------
def length_branch(n):
    return "empty" if n == 0 else ("one_piece" if n <= SPLIT else ("whole_pieces" if n % SPLIT == 0 else "ragged_pieces"))


def test_piece_plan_from_its_definition(recorded):
    seen = set()
    for name, row_ptr in PIECE_LAYOUTS.items():
        (row, begin, end, slot), (long_row, long_first, long_count) = recorded["pieces/%s_pieces" % name], recorded["pieces/%s_long" % name]
        n_pieces, n_long, n_slots, upload = recorded["pieces/%s_counts" % name].tolist()
        lengths = np.diff(row_ptr)
        assert n_pieces == len(row) == sum(max(1, -(-int(n) // SPLIT)) for n in lengths) and n_long == len(long_row) == int((lengths > SPLIT).sum())
        assert upload == 4 * (2 * int(row_ptr[-1]) + 4 * n_pieces + 3 * n_long)
        assert (np.diff(row) >= 0).all() and set(row.tolist()) == set(range(len(lengths))), "every row, in order, has a piece"
        next_slot = 0
        for i, n in enumerate(lengths.tolist()):
            seen.add((name.startswith("empty") and "empty_matrix" or "matrix", length_branch(n)))
            mine = np.flatnonzero(row == i)
            # the pieces of a row tile it in order: each at most SPLIT cells, only the last one shorter
            assert begin[mine[0]] == row_ptr[i] and end[mine[-1]] == row_ptr[i + 1] and (begin[mine[1:]] == end[mine[:-1]]).all(), (name, i)
            assert ((end[mine] - begin[mine])[:-1] == SPLIT).all() and 0 <= end[mine[-1]] - begin[mine[-1]] <= SPLIT, (name, i)
            assert n == 0 or end[mine[-1]] > begin[mine[-1]], (name, i)
            # a slot is -1 exactly for one-piece rows; the slots of a long row are consecutive from `first`
            if len(mine) == 1:
                assert slot[mine[0]] == -1 and i not in long_row, (name, i)
            else:
                at = long_row.tolist().index(i)
                assert long_first[at] == next_slot and long_count[at] == len(mine) and slot[mine].tolist() == list(range(next_slot, next_slot + len(mine))), (name, i)
                next_slot += len(mine)
        assert n_slots == next_slot
    assert seen == {("matrix", b) for b in ("empty", "one_piece", "whole_pieces", "ragged_pieces")} | {("empty_matrix", "empty")}
    assert sorted(np.diff(PIECE_LAYOUTS["ragged"]).tolist()) == sorted(ROW_LENGTHS) and recorded["pieces/ragged_counts"].tolist()[:3] == [17, 5, 13]
    assert recorded["pieces/transpose_counts"].tolist()[:3] == [1537, 0, 0] and recorded["pieces/empty_counts"].tolist() == [3, 0, 0, 48]


# ---- what create looks at ---------------------------------------------------------------------------------------------------------
def test_layout_findings(recorded):
    found = dict(zip(LAYOUT_TABLE, recorded["layout/result"].tolist()))
    # kind (1 start, 2 decrease, 3 index), the row of a decrease, the index found outside
    assert found == {"ok": [0, 0, 0], "ok_no_cells": [0, 0, 0], "start_not_zero": [1, 0, 0], "decrease_first": [2, 0, 0], "decrease_last": [2, 2, 0],
                     "index_negative": [3, 0, -7], "index_at_the_end": [3, 0, 4], "decrease_and_index": [2, 1, 0], "two_indices": [3, 0, 5]}
    assert {f[0] for f in found.values()} == {0, 1, 2, 3}


def test_value_scans(recorded):
    flags = dict(zip(VALUE_TABLE, recorded["values/flags"].tolist()))
    sums = dict(zip(VALUE_TABLE, recorded["values/sums"].tolist()))
    seen = set()
    for name, v in VALUE_TABLE.items():
        svd_ones, ones, negative, at = flags[name]
        bad = np.flatnonzero(~(v >= 0))
        branch = "negative" if len(bad) else ("ones" if (v == 1).all() else "values")
        seen.add(branch)
        assert svd_ones == bool((v == 1).all()), name
        if branch == "negative":
            assert (ones, negative, at) == (0, 1, bad[0]) and (sums[name][0] == float(v[bad[0]]) or np.isnan(v[bad[0]])), name
            continue
        assert (ones, negative, at) == (int(branch == "ones"), 0, 0), name
        norm_x = sum_x = 0.0                               # float64 sums in storage order
        for x in v.tolist():
            norm_x += x * x
            sum_x += x if np.float32(x) > np.float32(EPS32) else 0.0
        assert sums[name][1:] == [norm_x, sum_x], name
    assert seen == {"negative", "ones", "values"}
    assert sums["at_eps"][2] == 1.0 and sums["above_eps"][2] > 1.5 + EPS32 and sums["zeros"][1:] == [1.0, 1.0]
    assert flags["one_above_one"][:2] == [0, 0] and flags["no_cells"][:2] == [1, 1]


# ---- Gram and column-sum slabs ------------------------------------------------------------------------------------------------------
def test_gram_plan_covers_the_rows(recorded):
    seen = set()
    for (n, r), (slabs, rows, cells) in zip(GRAM_TABLE, recorded["gram/result"].tolist()):
        pairs = -(-r // GT) * (-(-r // GT) + 1) // 2
        # as many slabs as there are rows for (64 each), while slabs x tile pairs stays within 1024 workgroups; never fewer than one
        seen.add(("one_slab_floor" if pairs > 1024 else ("rows_bound" if -(-n // (4 * GR)) <= 1024 // pairs else "tiles_bound"), pairs))
        assert slabs * rows >= n and rows % GR == 0 and (slabs - 1) * rows < n and slabs >= 1, (n, r)
        assert (slabs == 1 or slabs * pairs <= 1024) and cells == slabs * r * r, (n, r)
    assert {b for b, _ in seen} == {"one_slab_floor", "rows_bound", "tiles_bound"} and {p for _, p in seen} == {1, 3, 6, 2080}


def test_column_sum_slabs_cover_the_rows(recorded):
    seen = set()
    for n, (slabs, rows, used) in zip(ROWS, recorded["colsum/result"].tolist()):
        seen.add("few_rows" if n <= 64 * CS_SLABS else "all_slabs")
        assert 1 <= used <= slabs <= CS_SLABS and used * rows >= n and (used - 1) * rows < n, n
    assert seen == {"few_rows", "all_slabs"}
    limits = dict(zip(itertools.product(ROWS, (1, ROW_LIMIT)), recorded["rows/in_range"].tolist()))
    assert all(ok == (max(a, b) <= ROW_LIMIT) for (a, b), ok in limits.items()) and limits[(ROW_LIMIT, 1)] == 1 and limits[(ROW_LIMIT + 1, 1)] == 0


def test_dot_grid(recorded):
    seen = set()
    for n, (blocks, cells_grid) in zip(DOT_TABLE, recorded["dot/result"].tolist()):
        seen.add("one" if n <= 4 * NT else ("by_length" if n <= 4 * NT * RED_BLOCKS else "capped"))
        assert blocks == max(1, min(RED_BLOCKS, -(-n // (4 * NT)))) and cells_grid == -(-min(n, 2 ** 31) // NT), n
    assert seen == {"one", "by_length", "capped"}


# ---- the sweep --------------------------------------------------------------------------------------------------------------------
def test_sweep_plan(recorded):
    seen = set()
    for (n, k), (shift, rows_per_block, blocks, lds, raise_attribute) in zip(SWEEP_TABLE, recorded["sweep/result"].tolist()):
        lanes = 1 << shift_branch(k)
        seen.add((lanes, "raised" if lds > 48 * 1024 else "default", "whole" if n % (NT // lanes) == 0 else "ragged"))
        assert shift == shift_branch(k) and rows_per_block == NT // lanes and blocks == -(-n // rows_per_block), (n, k)
        assert lds == -(-k // lanes) * NT * 4 <= 64 * 1024 and raise_attribute == (lds > 48 * 1024), (n, k)
    # 16 and 32 lanes hold at most 32 columns: one float per thread, the threshold is out of their reach
    assert seen == {(l, "default", w) for l in (16, 32, 64) for w in ("whole", "ragged")} | {(64, "raised", w) for w in ("whole", "ragged")}
    by_k = {k: r[4] for (_, k), r in zip(SWEEP_TABLE, recorded["sweep/result"].tolist())}
    assert (by_k[3072], by_k[3073], by_k[4096]) == (0, 1, 1)


def test_red_part_covers_every_grid_that_writes_it(shim):
    """One cell per workgroup is written by the sweep on either side, the SDDMM on either side and both dot products."""
    seen = set()
    for (nu, ni, pu, pi), k in itertools.product(RED_SHAPES, WIDTHS + (3073,)):
        cells = shim.bp_red_part_cells(pu, pi, max(nu, ni), k)
        grids = {"sweep_users": call(shim.bp_sweep, 5, nu, k)[2], "sweep_items": call(shim.bp_sweep, 5, ni, k)[2],
                 "sddmm_users": call(shim.bp_piece_grids, 2, pu, k)[1], "sddmm_items": call(shim.bp_piece_grids, 2, pi, k)[1],
                 "dot_grams": shim.bp_dot_blocks(k * k), "dot_colsums": shim.bp_dot_blocks(k), "dot_blocks": shim.bp_dot_blocks(nu * k)}
        assert all(0 < g <= cells for g in grids.values()), (nu, ni, pu, pi, k, cells, grids)
        seen.add(max(grids, key=grids.get) if cells > RED_BLOCKS else "floor")
    assert seen >= {"floor", "sweep_users", "sweep_items", "sddmm_users", "sddmm_items"}


def test_create_sizes(recorded):
    seen = set()
    for (nu, ni, su, si, r), (n_max, cap, partial_rows, gram_cells, slabs_u, slabs_i) in zip(recorded["sizes/table"].tolist(), recorded["sizes/result"].tolist()):
        seen.add(("users_longer" if nu > ni else "items_longer" if ni > nu else "square", "no_slots" if su == si == 0 else "slots"))
        assert n_max == max(nu, ni) and cap == n_max * r and partial_rows == max(1, su, si), (nu, ni, r)
        assert gram_cells == max(slabs_u, slabs_i) * r * r >= 1, (nu, ni, r)
    assert seen == {("users_longer", "slots"), ("items_longer", "slots"), ("square", "no_slots")}


# ---- accounting -----------------------------------------------------------------------------------------------------------------------
def test_accounting(recorded):
    seen = set()
    for (nu, ni, nnz, lu, li, r), counts, figures in zip(recorded["accounting/table"].tolist(), recorded["accounting/counts"].tolist(),
                                                         recorded["accounting/figures"].tolist()):
        c, f = dict(zip(ACCOUNT_COUNTS, counts)), dict(zip(ACCOUNT_FIGURES, zip(figures[::2], figures[1::2])))
        seen.add(("long_users" if lu else "short_users", "long_items" if li else "short_items", "cells" if nnz else "no_cells"))
        product = [2 if lu else 1, 2 if li else 1]
        assert [c["set_block_bytes_0"], c["set_block_bytes_1"], c["gram_d2h_bytes"], c["apply_h2d_bytes"], c["permutation_bytes"], c["scalar_bytes"]] == \
            [4 * nu * r, 4 * ni * r, 8 * r * r, 4 * r * r, 4 * r, 8]
        assert [c["product_0"], c["product_1"], c["gram"], c["apply"], c["fill"]] == product + [2, 1, 1]
        for s in (0, 1):
            prepare = 3 + product[s]                     # Gram, its reduction, to_float, the product
            assert c["sweep_reuse0_side%d" % s] == prepare + 2 and c["sweep_reuse1_side%d" % s] == 2
            assert c["mu_loss0_reuse0_side%d" % s] == prepare + 2 and c["mu_loss0_reuse1_side%d" % s] == 2
            assert c["mu_loss1_reuse0_side%d" % s] == 4 + product[s] and c["mu_loss1_reuse1_side%d" % s] == 2 + product[s]
        assert c["divergence_loss0"] == 9 + product[0] and c["divergence_loss1"] == 9
        assert f["product"] == f["divergence"] == (nnz * (4.0 * r + 8.0), 2.0 * nnz * r) and f["mu_kl"] == (nnz * (4.0 * r + 12.0), 2.0 * nnz * r)
        for s, n in enumerate((nu, ni)):
            assert f["sweep_%d" % s] == (12.0 * n * r, 2.0 * n * r * r) and f["mu_frobenius_%d" % s] == (16.0 * n * r, 2.0 * n * r * r)
            assert f["fill_%d" % s] == (4.0 * n * r, 0.0)
    assert seen == {("long_users", "short_items", "cells"), ("long_users", "long_items", "cells"), ("short_users", "short_items", "no_cells")}


# ---- the same tables under the sanitizers -----------------------------------------------------------------------------------------
def test_plan_program_under_address_and_undefined_behaviour_sanitizers(build_dir):
    exe = build_dir / "blocks_plan_main"
    # (the sanitizers' runtimes are linked into the program, so that it does not depend on the order the loader finds libraries in)
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer",
                    "-static-libasan", "-static-libubsan", os.path.join(HERE, "blocks_plan_main.cpp"), "-o", str(exe)], check=True)
    done = subprocess.run([str(exe)], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert done.returncode == 0, done.stdout[-4000:]
    assert "blocks_plan_main: OK" in done.stdout
