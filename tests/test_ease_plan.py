"""The host arithmetic of the EASE_R closed form (csrc/ease_plan.h) on the CPU.

A shim (tests/ease_plan_shim.cpp) is compiled with g++ and called through ctypes on tables of inputs.  Every case
  * states the branch it must reach (named from the inputs alone), and each test asserts that the set of branches its table reached is
    complete, so that a case that stops reaching its branch fails,
  * is compared exactly with tests/golden/ease_plan.npz -- recorded once by running the text of ease.hip and ease_pivot.hip as it stood
    before this arithmetic became functions of its own (mi355rec_ease_create's block, npad, steps and fit, ease_bytes, pivot_bytes,
    ensure_work's cap and reserve, the LDS bytes and the grids of enqueue_elimination, the loop of enqueue_pivoted_elimination with
    every `launches +=`, the permutation and the stats of the two invert calls, copied into a harness with a handle of plain numbers
    behind the same extern "C" interface as the shim: tests/golden/ease_plan_parent_harness.cpp) through record() below on these same
    tables (tests/golden/make_ease_plan_fixture.py); the fixture holds the tables, too, so a table that changes is noticed.
tests/ease_plan_main.cpp goes through the header once more as a program of its own under the address and undefined-behaviour
sanitizers.
"""
import ctypes as C
import itertools
import os
import subprocess

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden", "ease_plan.npz")

TILE, PANEL_W, CHUNK = 128, 64, 64
MIB = 2 ** 20
EASE_RESERVE, PIVOT_RESERVE = 256 * MIB, 64 * MIB
LDS_BYTES = 160 * 1024
FITS, NO_ROOM, OVER_CAP = 0, 1, 2

# ---- the tables ---------------------------------------------------------------------------------------------------------------
# both sides of every multiple of 64 up to two tiles, a ragged 200, and the item counts of ML-1M, Netflix and ML-20M
N_TABLE = (1, 63, 64, 65, 127, 128, 129, 191, 192, 193, 200, 255, 256, 257, 3706, 17770, 26744)
BLOCKS = (64, 128)
SHAPES = list(itertools.product(N_TABLE, BLOCKS))
SMALL = [(n, b) for n, b in SHAPES if n <= 257]         # every step and every column is recorded
LARGE = [(n, b) for n, b in SHAPES if n > 257]          # sums over the steps only

BLOCK_ENV = "MI355REC_EASE_BLOCK"
CAP_ENV = "MI355REC_EASE_PIVOT_MAX_BYTES"
ENV_TABLE = {
    "unset": {},
    "block_64": {BLOCK_ENV: "64"}, "block_128": {BLOCK_ENV: "128"},
    "block_0": {BLOCK_ENV: "0"}, "block_32": {BLOCK_ENV: "32"}, "block_abc": {BLOCK_ENV: "abc"}, "block_empty": {BLOCK_ENV: ""},
    "block_tail": {BLOCK_ENV: "64k"}, "block_negative": {BLOCK_ENV: "-64"},
    "cap_1000": {CAP_ENV: "1000"}, "cap_empty": {CAP_ENV: ""}, "cap_abc": {CAP_ENV: "abc"}, "cap_tail": {CAP_ENV: "12abc"},
    "cap_negative": {CAP_ENV: "-1"}, "cap_beyond": {CAP_ENV: "99999999999999999999999"}, "cap_space": {CAP_ENV: "  42"},
    "both": {BLOCK_ENV: "64", CAP_ENV: "0"},
}

NEED = 1000 * MIB + 7
# need, free: both sides of need + reserve == free, and the extremes
EASE_FIT_TABLE = [(NEED, NEED + EASE_RESERVE + d) for d in (-1, 0, 1)] + [(NEED, 0), (0, EASE_RESERVE), (0, EASE_RESERVE - 1), (NEED, 2 ** 63)]
# need, free, cap (None: not set): both sides of the cap, of need + reserve == free, and the cap before the free memory
ROOM, TIGHT = NEED + PIVOT_RESERVE, NEED + PIVOT_RESERVE - 1
PIVOT_FIT_TABLE = ([(NEED, NEED + PIVOT_RESERVE + d, None) for d in (-1, 0, 1)] + [(NEED, ROOM, NEED + d) for d in (-1, 0, 1)]
                   + [(NEED, TIGHT, NEED + d) for d in (-1, 0, 1)] + [(NEED, 0, 0), (NEED, 2 ** 63, 0), (0, PIVOT_RESERVE, 0), (0, PIVOT_RESERVE - 1, 0),
                                                                     (NEED, ROOM, 2 ** 64 - 1)])


def swap_lists():
    """name -> (piv, n, npad): piv[g] >= g is the row swapped with row g (what the pick kernel writes), rows >= n keep piv[g] = g"""
    rng = np.random.RandomState(11)
    out = {}
    for n, npad in ((1, 128), (128, 128), (129, 256), (200, 256), (257, 384)):
        identity = np.arange(npad, dtype=np.int32)
        out["identity_%d" % n] = (identity, n, npad)
        if n > 1:
            one = identity.copy()
            one[0] = n - 1
            out["single_swap_%d" % n] = (one, n, npad)
            last = identity.copy()
            last[:n] = n - 1                                # row n - 1 is fetched, then sent down again, at every step
            out["always_the_last_row_%d" % n] = (last, n, npad)
            nxt = identity.copy()
            nxt[:n - 1] += 1                                # row 0 sinks to the bottom one row at a time
            out["always_the_next_row_%d" % n] = (nxt, n, npad)
            for seed in range(2):
                r = identity.copy()
                r[:n] = [rng.randint(g, n) for g in range(n)]
                out["random_%d_%d" % (n, seed)] = (r, n, npad)
    return out


SWAP_LISTS = swap_lists()
ACCOUNTING_TABLE = [(n, b, c) for (n, b), c in itertools.product(SHAPES, (4, 8))]


def ptr(a):
    return a.ctypes.data_as(C.c_void_p)


# ---- running them -------------------------------------------------------------------------------------------------------------
def declare(lib):
    lib.ep_constants.argtypes = [C.c_void_p]
    lib.ep_read_knobs.argtypes = [C.c_void_p, C.c_char_p, C.c_int]
    lib.ep_shape.argtypes = [C.c_int, C.c_int, C.c_void_p]
    lib.ep_ease_fit.argtypes = [C.c_uint64, C.c_uint64]
    lib.ep_pivot_fit.argtypes = [C.c_uint64, C.c_uint64, C.c_int, C.c_uint64]
    lib.ep_ease_step.argtypes = [C.c_int, C.c_int, C.c_int, C.c_void_p]
    lib.ep_ease_launches.argtypes = [C.c_int, C.c_int]
    lib.ep_ease_launches.restype = C.c_int64
    lib.ep_pivot_step.argtypes = [C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p]
    lib.ep_pivot_launches.argtypes = [C.c_int, C.c_int, C.c_int]
    lib.ep_pivot_launches.restype = C.c_int64
    lib.ep_inverse_permutation.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_void_p]
    lib.ep_accounting.argtypes = [C.c_int, C.c_int, C.c_int, C.c_void_p]
    return lib


def read_environment(lib, setting):
    """(block, valid, cap set, cap), the message create words -- as the library parses exactly `setting`"""
    saved = {name: os.environ.get(name) for name in (BLOCK_ENV, CAP_ENV)}
    try:
        for name in saved:
            os.environ.pop(name, None)
        os.environ.update(setting)
        k, message = np.zeros(4, np.uint64), C.create_string_buffer(128)
        lib.ep_read_knobs(ptr(k), message, 128)
        return k, message.value.decode()
    finally:
        for name, v in saved.items():
            os.environ.pop(name, None)
            if v is not None:
                os.environ[name] = v


def shape_of(lib, n, block):
    out = np.zeros(5, np.int64)
    assert lib.ep_shape(n, block, ptr(out)) == 1
    return out


def ease_steps(lib, n, block):
    steps = int(shape_of(lib, n, block)[1])
    out = np.zeros((steps, 5), np.int64)
    for step in range(steps):
        lib.ep_ease_step(n, block, step, ptr(out[step]))
    return out


def pivot_steps(lib, n, block):
    """[steps][10] as ep_pivot_step fills it, [steps][128] grids of the elimination launches (-1 beyond the step's columns)"""
    steps = int(shape_of(lib, n, block)[1])
    out, elim = np.zeros((steps, 10), np.int64), np.full((steps, 128), -1, np.int32)
    for step in range(steps):
        lib.ep_pivot_step(n, block, step, ptr(out[step]), ptr(elim[step]))
    return out, elim


def inverse_permutation(lib, piv, n, npad):
    out = np.full(npad, -1, np.int32)
    lib.ep_inverse_permutation(ptr(piv), n, npad, ptr(out))
    return out


def record(lib):
    """name -> array, as the fixture holds them"""
    declare(lib)
    out = {}
    c = np.zeros(7, np.int64)
    lib.ep_constants(ptr(c))
    out["constants/result"] = c
    env = [read_environment(lib, ENV_TABLE[name]) for name in ENV_TABLE]
    out["env/table"], out["env/knobs"], out["env/message"] = np.array(list(ENV_TABLE)), np.array([e[0] for e in env]), np.array([e[1] for e in env])
    out["shape/table"], out["shape/result"] = np.array(SHAPES, np.int64), np.array([shape_of(lib, n, b) for n, b in SHAPES])
    out["fit/ease_table"] = np.array(EASE_FIT_TABLE, np.uint64)
    out["fit/ease_result"] = np.array([lib.ep_ease_fit(need, free) for need, free in EASE_FIT_TABLE], np.int64)
    out["fit/pivot_table"] = np.array([(need, free, cap is not None, cap or 0) for need, free, cap in PIVOT_FIT_TABLE], np.uint64)
    out["fit/pivot_result"] = np.array([lib.ep_pivot_fit(need, free, cap is not None, cap or 0) for need, free, cap in PIVOT_FIT_TABLE], np.int64)
    out["steps/small_table"] = np.array([(n, b, s) for n, b in SMALL for s in range(len(ease_steps(lib, n, b)))], np.int64)
    out["steps/small_result"] = np.concatenate([ease_steps(lib, n, b) for n, b in SMALL])
    out["steps/large_sums"] = np.array([ease_steps(lib, n, b).sum(axis=0) for n, b in LARGE])
    out["steps/launches"] = np.array([lib.ep_ease_launches(n, b) for n, b in SHAPES], np.int64)
    small = [pivot_steps(lib, n, b) for n, b in SMALL]
    out["pivot/small_table"] = np.array([(n, b, s) for (n, b), (st, _) in zip(SMALL, small) for s in range(len(st))], np.int64)
    out["pivot/small_steps"], out["pivot/small_elims"] = np.concatenate([s[0] for s in small]), np.concatenate([s[1] for s in small])
    large = [pivot_steps(lib, n, b) for n, b in LARGE]
    # per shape: the sums of the ten columns, then of the elimination grids, the elimination launches and the steps with nothing to search
    out["pivot/large_sums"] = np.array([st.sum(axis=0).tolist() + [int(el[el > 0].sum()), int((el > 0).sum()), int((st[:, 1] <= 0).sum())]
                                        for st, el in large], np.int64)
    out["pivot/launches"] = np.array([[lib.ep_pivot_launches(n, b, g) for g in (0, 1)] for n, b in SHAPES], np.int64)
    out["perm/table"] = np.array(list(SWAP_LISTS))
    for name, (piv, n, npad) in SWAP_LISTS.items():
        out["perm/%s_in" % name] = np.concatenate([[n, npad], piv]).astype(np.int32)
        out["perm/%s_result" % name] = inverse_permutation(lib, piv, n, npad)
    acc = np.zeros((len(ACCOUNTING_TABLE), 3), np.float64)
    for row, (n, b, cell) in zip(acc, ACCOUNTING_TABLE):
        lib.ep_accounting(n, b, cell, ptr(row))
    out["accounting/table"], out["accounting/result"] = np.array(ACCOUNTING_TABLE, np.int64), acc
    return out


FAMILIES = ("constants", "env", "shape", "fit", "steps", "pivot", "perm", "accounting")


def build_shim(directory, source=os.path.join(HERE, "ease_plan_shim.cpp")):
    so = os.path.join(str(directory), "ease_plan_shim.so")
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-shared", "-fPIC", source, "-o", so], check=True)
    return declare(C.CDLL(so))


@pytest.fixture(scope="module")
def build_dir(tmp_path_factory):
    return tmp_path_factory.mktemp("ease_plan")


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
    assert os.path.getsize(GOLDEN) <= 64 * 1024


@pytest.mark.parametrize("name", FAMILIES)
def test_results_equal_the_recorded_results(golden, recorded, name):
    for key in sorted(k for k in recorded if k.startswith(name + "/")):
        want, got = golden[key], recorded[key]
        assert got.shape == want.shape and got.dtype == want.dtype, key
        where = np.argwhere(got != want)
        assert where.size == 0, (key, where[:5].tolist())


def test_constants(recorded):
    # EASE_TILE, TK, PANEL_W, CHUNK, GK, the reserve next to the handle, next to the pivoted workspace
    assert recorded["constants/result"].tolist() == [128, 32, 64, 64, 16, EASE_RESERVE, PIVOT_RESERVE]


# ---- shape and bytes ------------------------------------------------------------------------------------------------------------
def test_shape_bytes_and_lds(shim, recorded):
    seen = set()
    for (n, block), (npad, steps, ease_bytes, pivot_bytes, lds) in zip(SHAPES, recorded["shape/result"].tolist()):
        seen.add("npad == n" if npad == n else "npad != n")
        assert npad == -(-n // TILE) * TILE and steps * block == npad, (n, block)
        slab = n * n if npad != n else 0              # where the dense Gram columns are built before they take the matrix's pitch
        assert ease_bytes == 4 * (npad * npad + 3 * npad * block + block * block + slab), (n, block)
        assert pivot_bytes == 8 * (npad * npad + 4 * npad * block + 2 * block * block), (n, block)
        assert lds == 4 * (block * (block + 4) + block * PANEL_W + PANEL_W * (block + 4)) <= LDS_BYTES, (n, block)
    assert seen == {"npad == n", "npad != n"}
    # "too many items": the padded side must fit an int
    out = np.zeros(5, np.int64)
    assert shim.ep_shape(2 ** 31 - 128, 128, ptr(out)) == 1 and out[0] == 2 ** 31 - 128
    assert shim.ep_shape(2 ** 31 - 127, 128, ptr(out)) == 0 and shim.ep_shape(2 ** 31 - 1, 64, ptr(out)) == 0


def test_unpivoted_steps(recorded):
    at = 0
    for n, block in SMALL:
        npad = -(-n // TILE) * TILE
        steps = npad // block
        rows = recorded["steps/small_result"][at:at + steps].tolist()
        assert recorded["steps/small_table"][at:at + steps].tolist() == [[n, block, s] for s in range(steps)]
        at += steps
        assert rows == [[s * block, 1, npad // PANEL_W, npad // TILE, npad // PANEL_W] for s in range(steps)], (n, block)
    assert at == len(recorded["steps/small_result"])
    for (n, block), launches in zip(SHAPES, recorded["steps/launches"].tolist()):
        assert launches == 4 * (-(-n // TILE) * TILE // block), (n, block)


# ---- the pivoted route's steps ----------------------------------------------------------------------------------------------------
def pivoted_launches(n, block, gathered):
    """Written out independently of the loop: init and widen; six launches of the block step per step; per panel that holds rows of
    the matrix a load, a swap, a pick per column and an elimination after every column but the panel's last; the gather."""
    steps = -(-n // TILE) * TILE // block
    full, ragged = divmod(n, block)
    return 2 + 6 * steps + full * (2 * block + 1) + (2 * ragged + 1 if ragged else 0) + (1 if gathered else 0)


def test_pivoted_steps_reach_every_branch_and_stay_inside_the_panel(shim, recorded):
    seen = {}
    for (n, block), launches in zip(SHAPES, recorded["pivot/launches"].tolist()):
        npad = -(-n // TILE) * TILE
        steps, elims = pivot_steps(shim, n, block)
        assert len(steps) == npad // block
        total = 2
        for step, ((k0, cols, load, swap, transpose, long_side, short_side, tiles, writeback, count), elim) in enumerate(zip(steps.tolist(), elims.tolist())):
            case = (n, block, step)
            assert k0 == step * block and cols == min(block, n - k0), case
            assert (transpose, long_side, short_side, tiles, writeback) == (npad // 32, npad // 64, block // 64, npad // TILE, npad // PANEL_W), case
            assert min(transpose, long_side, short_side, tiles, writeback) >= 1, case
            if cols <= 0:
                seen.setdefault("cols <= 0", set()).add((n, block))
                assert (load, swap, count) == (0, 0, 6) and elim == [-1] * 128, case
                total += count
                continue
            seen.setdefault("0 < cols < NB" if cols < block else "cols == NB", set()).add((n, block))
            # the load kernel's workgroups are the chunks k0 / CHUNK .. (n - 1) / CHUNK: rows below npad, candidates below npad / CHUNK
            assert load >= 1 and swap == npad // 128 >= 1 and (k0 // CHUNK + load) * CHUNK <= npad and (k0 // CHUNK + load - 1) == (n - 1) // CHUNK, case
            assert elim[cols:] == [-1] * (128 - cols) and all(g >= 0 for g in elim[:cols]), case
            for j, grid in enumerate(elim[:cols]):
                g = k0 + j
                if grid == 0:
                    assert j == cols - 1, (case, j)             # only the last column searched goes without
                    seen.setdefault("no elimination: g + 1 == n" if g + 1 == n else "no elimination: j + 1 == NB", set()).add((n, block))
                    if g + 1 == n and j + 1 == block:
                        seen.setdefault("no elimination: both", set()).add((n, block))
                else:
                    first = (g + 1) // CHUNK
                    assert grid >= 1 and (first + grid) * CHUNK <= npad and first + grid - 1 == (n - 1) // CHUNK, (case, j)
            assert count == 6 + 2 + cols + sum(1 for grid in elim[:cols] if grid > 0), case
            total += count
        assert [total, total + 1] == launches == [pivoted_launches(n, block, g) for g in (False, True)], (n, block)
    assert {(1, 64), (129, 64)} <= seen["cols <= 0"]
    assert {(129, 128), (200, 64), (200, 128)} <= seen["0 < cols < NB"]
    assert seen["cols == NB"] and seen["no elimination: g + 1 == n"] and seen["no elimination: j + 1 == NB"] and seen["no elimination: both"]
    assert (129, 64) in seen["no elimination: g + 1 == n"] and (129, 64) in seen["no elimination: j + 1 == NB"]


def test_pivoted_steps_of_the_large_shapes_sum_to_the_recorded_sums(recorded):
    for (n, block), sums in zip(LARGE, recorded["pivot/large_sums"].tolist()):
        steps = -(-n // TILE) * TILE // block
        # columns searched: every row of the matrix once; an elimination after all of them but one per panel
        searched = sum(min(block, n - s * block) for s in range(steps) if n - s * block > 0)
        panels = sum(1 for s in range(steps) if n - s * block > 0)
        assert searched == n and sums[11] == n - panels and sums[12] == steps - panels, (n, block)
        assert sums[9] + 2 == pivoted_launches(n, block, False), (n, block)


# ---- fit verdicts -------------------------------------------------------------------------------------------------------------------
def test_fit_verdicts(recorded):
    seen = set()
    for (need, free), got in zip(EASE_FIT_TABLE, recorded["fit/ease_result"].tolist()):
        want = FITS if need + EASE_RESERVE <= free else NO_ROOM
        seen.add(("handle", want))
        assert got == want, (need, free)
    for (need, free, cap), got in zip(PIVOT_FIT_TABLE, recorded["fit/pivot_result"].tolist()):
        want = OVER_CAP if cap is not None and need > cap else (NO_ROOM if need + PIVOT_RESERVE > free else FITS)
        seen.add(("workspace", want, cap is not None))
        assert got == want, (need, free, cap)
    assert seen == {("handle", FITS), ("handle", NO_ROOM), ("workspace", FITS, False), ("workspace", NO_ROOM, False), ("workspace", FITS, True),
                    ("workspace", NO_ROOM, True), ("workspace", OVER_CAP, True)}
    by_case = dict(zip(PIVOT_FIT_TABLE, recorded["fit/pivot_result"].tolist()))
    # one byte either side of the cap, of the free memory -- and the cap is looked at first
    assert [by_case[(NEED, ROOM, NEED + d)] for d in (-1, 0, 1)] == [OVER_CAP, FITS, FITS]
    assert [by_case[(NEED, NEED + PIVOT_RESERVE + d, None)] for d in (-1, 0, 1)] == [NO_ROOM, FITS, FITS]
    assert [by_case[(NEED, TIGHT, NEED + d)] for d in (-1, 0, 1)] == [OVER_CAP, NO_ROOM, NO_ROOM]
    assert by_case[(NEED, 0, 0)] == OVER_CAP and by_case[(0, PIVOT_RESERVE, 0)] == FITS and by_case[(0, PIVOT_RESERVE - 1, 0)] == NO_ROOM
    by_case = dict(zip(EASE_FIT_TABLE, recorded["fit/ease_result"].tolist()))
    assert [by_case[(NEED, NEED + EASE_RESERVE + d)] for d in (-1, 0, 1)] == [NO_ROOM, FITS, FITS]


# ---- the environment ------------------------------------------------------------------------------------------------------------
def test_knob_parsing(recorded):
    knobs = dict(zip(ENV_TABLE, recorded["env/knobs"].astype(np.int64).tolist()))
    message = dict(zip(ENV_TABLE, recorded["env/message"].tolist()))
    assert knobs["unset"] == [128, 1, 0, 0]
    assert knobs["block_64"] == [64, 1, 0, 0] and knobs["block_128"] == [128, 1, 0, 0]
    for name, read in (("block_0", 0), ("block_32", 32), ("block_abc", 0), ("block_empty", 0), ("block_negative", -64)):
        assert knobs[name] == [read, 0, 0, 0] and message[name] == "MI355REC_EASE_BLOCK must be 64 or 128, got %d" % read, name
    assert knobs["block_tail"] == [64, 1, 0, 0]                                     # atoi stops at the first character that is no digit
    # the cap as strtoull reads it: nothing to read is 0 bytes, a sign wraps, too many digits saturate
    assert knobs["cap_1000"] == [128, 1, 1, 1000] and knobs["cap_empty"] == [128, 1, 1, 0] and knobs["cap_abc"] == [128, 1, 1, 0]
    assert knobs["cap_tail"] == [128, 1, 1, 12] and knobs["cap_space"] == [128, 1, 1, 42]
    caps = dict(zip(ENV_TABLE, recorded["env/knobs"][:, 3].tolist()))
    assert caps["cap_negative"] == 2 ** 64 - 1 and caps["cap_beyond"] == 2 ** 64 - 1
    assert knobs["both"] == [64, 1, 1, 0]


# ---- the permutation ------------------------------------------------------------------------------------------------------------
def test_the_permutation_undoes_the_row_swaps_on_the_columns(recorded):
    seen = set()
    rng = np.random.RandomState(3)
    for name, (piv, n, npad) in SWAP_LISTS.items():
        inv_perm = recorded["perm/%s_result" % name]
        P = np.eye(npad, dtype=np.int64)
        for g in range(n):                                 # the swaps, in order, on the rows of an identity
            P[[g, piv[g]]] = P[[piv[g], g]]
        M = rng.randint(-1000, 1000, size=(npad, npad)).astype(np.int64)
        assert np.array_equal(M[:, inv_perm], M @ P), name
        assert sorted(inv_perm.tolist()) == list(range(npad)) and inv_perm[n:].tolist() == list(range(n, npad)), name
        moved = int((piv[:n] != np.arange(n)).sum())
        seen.add(("identity" if moved == 0 else "one swap" if moved == 1 else "many swaps", "n < npad" if n < npad else "n == npad"))
        if name.startswith("always_the_next_row"):
            assert inv_perm[0] == n - 1                    # column 0 of the inverse stands where row 0 ended: at the bottom
    assert seen == {(m, p) for m in ("identity", "one swap", "many swaps") for p in ("n < npad", "n == npad")}


# ---- accounting -----------------------------------------------------------------------------------------------------------------
def test_accounting(recorded):
    for (n, block, cell), (flops, nbytes, units) in zip(ACCOUNTING_TABLE, recorded["accounting/result"].tolist()):
        steps = -(-n // TILE) * TILE // block
        assert flops == 2.0 * n ** 3 and nbytes == 2.0 * cell * float(n) * n * steps and units == steps, (n, block, cell)


# ---- the same tables under the sanitizers -----------------------------------------------------------------------------------------
def test_plan_program_under_address_and_undefined_behaviour_sanitizers(build_dir):
    exe = build_dir / "ease_plan_main"
    # (the sanitizers' runtimes are linked into the program, so that it does not depend on the order the loader finds libraries in)
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer",
                    "-static-libasan", "-static-libubsan", os.path.join(HERE, "ease_plan_main.cpp"), "-o", str(exe)], check=True)
    env = {k: v for k, v in os.environ.items() if k not in (BLOCK_ENV, CAP_ENV)}
    done = subprocess.run([str(exe)], env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert done.returncode == 0, done.stdout[-4000:]
    assert "ease_plan_main: OK" in done.stdout
