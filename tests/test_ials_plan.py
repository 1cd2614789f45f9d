"""The host arithmetic of an IALS half-step (csrc/ials_plan.h) on the CPU.

A shim (tests/ials_plan_shim.cpp) is compiled with g++ and called through ctypes on tables of inputs.  Every case
  * states the branch it must reach (the `*_branch` functions name it from the inputs alone), and each test asserts that the set of
    branches its table reached is complete, so that a case that stops reaching its branch fails,
  * is compared exactly with tests/golden/ials_plan.npz -- recorded once by running the text of ials.hip as it stood before this
    arithmetic became functions of its own (half_step, row_slots and launch_rows' switch, launch_solve's switch, rows_per_batch,
    ensure_systems' halving, the getenv sites and the kernel's part formula, copied into a harness with the knobs, the free bytes of
    the device and k as inputs, behind the same extern "C" interface as the shim) through record() below on these same tables; the
    fixture holds the tables, too, so a table that changes is noticed.
tests/ials_plan_main.cpp runs the tables through the header once more as a program of its own under the address and
undefined-behaviour sanitizers.
"""
import ctypes as C
import itertools
import os
import subprocess

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden", "ials_plan.npz")

CHUNK, GRAM_CHUNK, ROW_WAVES, TILE_WAVES, GRAM_WAVES, MAX_PARTS, MIN_BATCH_ROWS = 16, 32, 8, 7, 16, 64, 64
ROW_INSTANCES = (1, 2, 4, 6, 8, 10, 12, 13, 15, 17)
GRAM_INSTANCES = (1, 2, 3, 4, 5, 6, 7, 8)
SOLVE_INSTANCES = (1, 2, 4, 6, 8, 10, 11, 12, 13)
LDS_BYTES = 160 * 1024
UNKNOWN = 2 ** 64 - 1                      # free bytes nobody could tell
GIB = 2 ** 30

IALS = "MI355REC_IALS_"
ENV_NAMES = [IALS + s for s in ("TWO_STAGE", "SYSTEM_GIB", "PART_ROWS", "NO_SPLIT", "SAME_PANEL_WAVE", "PHASES")]
DEFAULT_KNOBS = [1, 0, 4096, 0, 0, 0]      # two_stage, system_gib set, part_rows, no_split, same_panel_wave, phases


def ptr(a):
    return a.ctypes.data_as(C.c_void_p)


def knobs(two_stage=1, gib=None, part_rows=4096, no_split=0):
    return np.array([two_stage, int(gib is not None), part_rows, no_split, 0, 0], np.int64), C.c_double(0.0 if gib is None else gib)


# ---- the tables ---------------------------------------------------------------------------------------------------------------
# both sides of every tile count (KT = 1 .. 16) and of the two-stage limit (207 | 208)
K_TABLE = sorted({1, 15, 16, 31, 47, 200, 207, 208, 224, 225, 239, 240, 255} | {16 * j - 1 for j in range(1, 17)} | {16 * j for j in range(1, 16)})
TILES_TABLE = list(itertools.product(K_TABLE, (1, 0)))                          # k, TWO_STAGE

PART_ROWS_ENV = (None, "32", "33", "1")                                         # unset: 4096; 33 rounds to 32; 1 floors to CHUNK
RANGES = ((0, 12), (2, 9), (5, 12))
ITEM_TABLE = list(itertools.product(PART_ROWS_ENV, (0, 1), RANGES, (16, 200)))  # PART_ROWS, NO_SPLIT, [r0, r1), k
ITEM_CAP, N_ROWS = 256, 12


def lengths(P):
    """profile lengths of the 12 rows for parts of P: cold rows, 1, both sides of the split limit 2 P and of the 64-part cap, ties"""
    return [1, 2 * P + 1, 0, 64 * P, 2 * P, 1, 64 * P + 1, 2 * P + 1, 0, 3 * P, 65 * P, 2 * P]


BATCH_ITEMS = ("32", 0, (0, 12), 200)                                           # the item list the batches are cut from
PART_BEG = 7
# free bytes, SYSTEM_GIB
GIB_TABLE = list(itertools.product((UNKNOWN, 64 * GIB, 16 * GIB, 2 ** 20), (None, 2.5, 0.0, 100.0)))
# system_gib, k, longest side
PER_BATCH_TABLE = list(itertools.product((8.0, 4.0, 0.001, 0.0001), (16, 200, 207), (10, 138493, 10 ** 7)))   # (0.0001: below the floor, not one slab)
# rows of the half-step, system_gib, k, longest side
HALVING_TABLE = ((138493, 8.0, 200, 138493), (26744, 8.0, 200, 138493), (100, 8.0, 200, 138493), (65, 8.0, 16, 1000), (64, 8.0, 200, 138493),
                 (5000, 0.001, 207, 5000))
HALVING_CAP = 40
# nnz of the rows, rows, rows of the other side, k
ACCOUNTING_TABLE = ((20000263.0, 138493, 26744, 200), (0.0, 0, 5, 1), (1000.0, 7, 9, 255))

ENV_TABLE = {
    "unset": {},
    "empty": {name: "" for name in ENV_NAMES},       # a number reads as 0 (two-stage off, floor of the buffer, parts of CHUNK); a switch is ON
    "numbers": {IALS + "TWO_STAGE": "1", IALS + "SYSTEM_GIB": "2.5", IALS + "PART_ROWS": "64"},
    "zeros": {name: "0" for name in ENV_NAMES},
    "tails": {IALS + "TWO_STAGE": " 7abc", IALS + "SYSTEM_GIB": "1e1x", IALS + "PART_ROWS": "33"},
    "not_numbers": {IALS + "TWO_STAGE": "yes", IALS + "SYSTEM_GIB": "much", IALS + "PART_ROWS": "abc"},
    "part_rows_1": {IALS + "PART_ROWS": "1"},
    "negative": {IALS + "TWO_STAGE": "-1", IALS + "SYSTEM_GIB": "-4", IALS + "PART_ROWS": "-100"},
}


# ---- running them -------------------------------------------------------------------------------------------------------------
def declare(lib):
    lib.ials_system_gib.argtypes = [C.c_uint64, C.c_void_p, C.c_double]
    lib.ials_system_gib.restype = C.c_double
    lib.ials_rows_per_batch.argtypes = [C.c_double, C.c_int, C.c_uint64]
    lib.ials_halving.argtypes = [C.c_int, C.c_double, C.c_int, C.c_uint64, C.c_void_p, C.c_void_p, C.c_int]
    lib.ials_accounting.argtypes = [C.c_double, C.c_int, C.c_int, C.c_int, C.c_void_p]
    return lib


def read_environment(lib, setting):
    """the knobs as the library parses them with exactly `setting` in the environment"""
    saved = {name: os.environ.get(name) for name in ENV_NAMES}
    try:
        for name in ENV_NAMES:
            os.environ.pop(name, None)
        os.environ.update(setting)
        k, gib = np.zeros(6, np.int64), C.c_double(0)
        lib.ials_read_knobs(ptr(k), C.byref(gib))
        return k, gib.value
    finally:
        for name, v in saved.items():
            os.environ.pop(name, None)
            if v is not None:
                os.environ[name] = v


def run_env(lib):
    got = [read_environment(lib, ENV_TABLE[name]) for name in ENV_TABLE]
    return np.array(list(ENV_TABLE)), np.array([g[0] for g in got]), np.array([g[1] for g in got])


def run_tiles(lib):
    out = []
    for k, two_stage in TILES_TABLE:
        r = np.zeros(12, np.int64)
        lib.ials_tiles(k, ptr(knobs(two_stage=two_stage)[0]), ptr(r))
        out.append(r)
    return np.array(TILES_TABLE, np.int64), np.array(out)


def work_items(lib, part_rows_env, no_split, r0, r1, k):
    """-> P, ptr, rows, items [n][4], (warm rows, items, split rows, part slots), nnz of the rows"""
    setting = {} if part_rows_env is None else {IALS + "PART_ROWS": part_rows_env}
    if no_split:
        setting[IALS + "NO_SPLIT"] = "1"
    kn, _ = read_environment(lib, setting)
    P = int(kn[2])
    indptr = np.concatenate([[0], np.cumsum(lengths(P))]).astype(np.int32)
    order = np.argsort(-np.diff(indptr), kind="stable").astype(np.int32)        # longest profile first, as the create call sorts
    rows, items = np.full(N_ROWS, -1, np.int32), np.full((ITEM_CAP, 4), -1, np.int32)
    counts, nnz = np.zeros(4, np.int64), C.c_double(0)
    assert lib.ials_work_items(ptr(indptr), ptr(order), N_ROWS, r0, r1, k, ptr(kn), ptr(rows), ptr(items), ITEM_CAP, ptr(counts), C.byref(nnz)) == 0
    return P, indptr, rows, items, counts, nnz.value


def run_items(lib):
    table, rows, items, counts, nnz = [], [], [], [], []
    for env, no_split, (r0, r1), k in ITEM_TABLE:
        P, _, r, it, c, z = work_items(lib, env, no_split, r0, r1, k)
        table.append([-1 if env is None else int(env), no_split, r0, r1, k, P])
        rows.append(r), items.append(it), counts.append(c), nnz.append(z)
    return np.array(table, np.int64), np.array(rows), np.array(items), np.array(counts), np.array(nnz)


def part_pairs(lib):
    """(L, n_parts) of every split row the item table produces, and a row whose trailing part is empty at CHUNK 32"""
    pairs = {(70, 5)}
    for env, no_split, (r0, r1), k in ITEM_TABLE:
        P, indptr, _, items, counts, _ = work_items(lib, env, no_split, r0, r1, k)
        pairs |= {(int(indptr[r + 1] - indptr[r]), int(n)) for r, _, n, _ in items[:counts[1]] if n > 1}
    return sorted(pairs)


def run_parts(lib):
    table, out = [], []
    for (L, n), chunk in itertools.product(part_pairs(lib), (CHUNK, GRAM_CHUNK)):
        got = np.full((MAX_PARTS, 2), -1, np.int32)
        for q in range(n):
            lib.ials_part_range(PART_BEG, PART_BEG + L, q, n, chunk, ptr(got[q]))
        table.append([L, n, chunk])
        out.append(got)
    return np.array(table, np.int64), np.array(out)


def batch_sizes(n_local):
    return (1, 2, n_local - 1, n_local, n_local + 5)


def run_batches(lib):
    _, _, rows, items, counts, _ = work_items(lib, BATCH_ITEMS[0], BATCH_ITEMS[1], *BATCH_ITEMS[2], BATCH_ITEMS[3])
    n_local, n_items = int(counts[0]), int(counts[1])
    cap = n_items + n_local
    table, all_items, slots, batches, sizes = [], [], [], [], []
    for per_batch in batch_sizes(n_local):
        a, s, b, c = np.full((cap, 4), -1, np.int32), np.full(cap, -1, np.int32), np.full((n_local, 4), -1, np.int32), np.zeros(2, np.int64)
        assert lib.ials_batches(ptr(rows), n_local, ptr(items), n_items, per_batch, N_ROWS, ptr(a), ptr(s), cap, ptr(b), n_local, ptr(c)) == 0
        table.append([per_batch, n_local, n_items])
        all_items.append(a), slots.append(s), batches.append(b), sizes.append(c)
    return np.array(table, np.int64), np.array(all_items), np.array(slots), np.array(batches), np.array(sizes)


def run_gib(lib):
    out = [lib.ials_system_gib(free, ptr(knobs(gib=g)[0]), knobs(gib=g)[1]) for free, g in GIB_TABLE]
    return np.array([[free, -1.0 if g is None else g] for free, g in GIB_TABLE], np.float64), np.array(out, np.float64)


def run_per_batch(lib):
    return np.array(PER_BATCH_TABLE, np.float64), np.array([lib.ials_rows_per_batch(g, k, n) for g, k, n in PER_BATCH_TABLE], np.int64)


def run_halving(lib):
    per_batch, gib, count = [], [], []
    for rows, g, k, longest in HALVING_TABLE:
        p, s = np.full(HALVING_CAP, -1, np.int64), np.full(HALVING_CAP, -1.0, np.float64)
        n = lib.ials_halving(rows, g, k, longest, ptr(p), ptr(s), HALVING_CAP)
        assert 0 < n <= HALVING_CAP
        per_batch.append(p), gib.append(s), count.append(n)
    return np.array(HALVING_TABLE, np.float64), np.array(per_batch), np.array(gib), np.array(count, np.int64)


def run_accounting(lib):
    out = []
    for row in ACCOUNTING_TABLE:
        r = np.zeros(2, np.float64)
        lib.ials_accounting(*row, ptr(r))
        out.append(r)
    return np.array(ACCOUNTING_TABLE, np.float64), np.array(out)


def record(lib):
    """name -> array, as the fixture holds them"""
    declare(lib)
    out = {}
    out["env/table"], out["env/knobs"], out["env/system_gib"] = run_env(lib)
    out["tiles/table"], out["tiles/result"] = run_tiles(lib)
    out["items/table"], out["items/rows"], out["items/items"], out["items/counts"], out["items/nnz"] = run_items(lib)
    out["parts/table"], out["parts/ranges"] = run_parts(lib)
    out["batches/table"], out["batches/items"], out["batches/sys_slot"], out["batches/batches"], out["batches/counts"] = run_batches(lib)
    out["gib/table"], out["gib/result"] = run_gib(lib)
    out["per_batch/table"], out["per_batch/result"] = run_per_batch(lib)
    out["halving/table"], out["halving/per_batch"], out["halving/gib"], out["halving/count"] = run_halving(lib)
    out["accounting/table"], out["accounting/result"] = run_accounting(lib)
    c = np.zeros(13, np.int64)
    lib.ials_constants(ptr(c))
    out["constants/result"] = c
    return out


FAMILIES = ("env", "tiles", "items", "parts", "batches", "gib", "per_batch", "halving", "accounting", "constants")


@pytest.fixture(scope="module")
def build_dir(tmp_path_factory):
    return tmp_path_factory.mktemp("ials_plan")


@pytest.fixture(scope="module")
def shim(build_dir):
    so = build_dir / "ials_plan_shim.so"
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-shared", "-fPIC", os.path.join(HERE, "ials_plan_shim.cpp"), "-o", str(so)], check=True)
    return declare(C.CDLL(str(so)))


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


@pytest.mark.parametrize("name", FAMILIES)
def test_results_equal_the_recorded_results(golden, recorded, name):
    for key in sorted(k for k in recorded if k.startswith(name + "/")):
        want, got = golden[key], recorded[key]
        assert got.shape == want.shape and got.dtype == want.dtype, key
        where = np.argwhere(got != want)
        assert where.size == 0, (key, where[:5].tolist())


def test_constants(recorded):
    # CHUNK, GRAM_CHUNK, ROW_THREADS, ROW_WAVES, TILE_WAVES, GRAM_THREADS, GRAM_WAVES, MAX_KT, MAX_NT, MAX_SOLVE_SLOTS, TP, part cap, slab stop
    assert recorded["constants/result"].tolist() == [16, 32, 512, 8, 7, 1024, 16, 16, 136, 13, 17, 64, 64]


# ---- tiles, instances, buffers ------------------------------------------------------------------------------------------------
def tiles_branch(k, two_stage):
    if not two_stage:
        return "two_stage_off"
    return "two_stage" if k <= 207 else "k_above_the_solve_stage"


def test_tile_arithmetic_and_buffer_sizes(shim, recorded):
    seen, rows_seen, gram_seen, solve_seen = set(), set(), set(), set()
    applies = {}
    for (k, two_stage), r in zip(TILES_TABLE, recorded["tiles/result"].tolist()):
        KT, NT, rows, gram, solve, solve_inst, two, lds0, lds1, lds2, slab_two, slab_one = r
        case = (k, two_stage)
        branch = tiles_branch(k, two_stage)
        seen.add(branch)
        applies[case] = two
        assert KT == -(-(k + 1) // 16) and 1 <= KT <= 16 and NT == KT * (KT + 1) // 2, case
        assert two == (branch == "two_stage"), case
        # the one-kernel epoch runs every k: its instance exists and holds all tiles, its LDS fits
        assert rows * ROW_WAVES >= NT and rows in ROW_INSTANCES and shim.ials_has_instance(0, rows), case
        assert slab_one == rows * 4 * 512 and 8 * lds0 <= LDS_BYTES, case
        rows_seen.add(rows)
        assert gram * GRAM_WAVES >= NT and slab_two == gram * 4 * 1024 and solve * TILE_WAVES >= NT and solve_inst <= 13, case
        if two:
            # what a two-stage epoch launches: instances exist and hold all tiles, both stages' LDS fits, ...
            assert gram in GRAM_INSTANCES and shim.ials_has_instance(1, gram), case
            assert solve_inst >= solve and solve_inst * TILE_WAVES >= NT and solve_inst in SOLVE_INSTANCES and shim.ials_has_instance(2, solve_inst), case
            assert 8 * lds1 <= LDS_BYTES and 8 * lds2 <= LDS_BYTES, case
            # ... and the parts of a split row, sized for the kernel that builds them, are at least what the other kernel would need
            assert slab_two >= slab_one, case
            gram_seen.add(gram), solve_seen.add(solve_inst)
    assert seen == {"two_stage", "two_stage_off", "k_above_the_solve_stage"}
    assert applies[(207, 1)] == 1 and applies[(208, 1)] == 0 and applies[(207, 0)] == 0 and applies[(1, 0)] == 0
    # Every instance a k <= 255 can reach is reached.  Compiled and out of reach: 13 slots of the one kernel (no KT has 97 .. 104
    # tiles), 7 and 8 of the Gramian stage and 11 of the solve stage (two-stage epochs stop at KT = 13: 91 tiles = 6 and 13 slots).
    assert rows_seen == set(ROW_INSTANCES) - {13}
    assert gram_seen == set(GRAM_INSTANCES) - {7, 8}
    assert solve_seen == set(SOLVE_INSTANCES) - {11}
    assert not shim.ials_has_instance(0, 3) and not shim.ials_has_instance(1, 9) and not shim.ials_has_instance(2, 3) and not shim.ials_has_instance(2, 14)


def test_the_gramian_stage_at_k_255_would_not_fit_and_is_never_launched(recorded):
    by_case = dict(zip(TILES_TABLE, recorded["tiles/result"].tolist()))
    for k in K_TABLE:
        lds1, two = by_case[(k, 1)][8], by_case[(k, 1)][6]
        assert two or k > 207
        if 8 * lds1 > LDS_BYTES:
            assert not two, k                                   # (stage 1 of such a k is not among the launches checked above)
    assert 8 * by_case[(255, 1)][8] > LDS_BYTES and not by_case[(255, 1)][6]
    assert 8 * by_case[(255, 1)][7] <= LDS_BYTES               # the one kernel, which does run k = 255, fits


# ---- work items ---------------------------------------------------------------------------------------------------------------
def row_branch(L, P, no_split, inside):
    if not inside:
        return "outside_the_range"
    if L == 0:
        return "cold"
    if L <= 2 * P:
        return "short"
    if no_split:
        return "long_but_no_split"
    return "split_capped" if -(-L // P) > MAX_PARTS else "split"


def test_work_items(recorded):
    seen, orders_seen, split_of = set(), set(), {}
    for (env, no_split, r0, r1, k, P), rows, items, counts, nnz in zip(recorded["items/table"].tolist(), recorded["items/rows"], recorded["items/items"],
                                                                       recorded["items/counts"].tolist(), recorded["items/nnz"].tolist()):
        case = (env, no_split, r0, r1, k)
        assert P == {-1: 4096, 32: 32, 33: 32, 1: CHUNK}[env], case
        n_rows, n_items, n_split, part_slots = counts
        L = lengths(P)
        rows, items = rows[:n_rows].tolist(), items[:n_items].tolist()
        branch = {r: row_branch(L[r], P, no_split, r0 <= r < r1) for r in range(N_ROWS)}
        seen |= set(branch.values())
        warm = [r for r in range(N_ROWS) if branch[r] not in ("outside_the_range", "cold")]
        # the warm rows of the range, longest first (ties: lower row first), and nothing else
        assert rows == sorted(warm, key=lambda r: (-L[r], r)) and nnz == sum(L[r] for r in warm), case
        assert {it[0] for it in items} == set(warm), case
        slots_taken, keys = 0, []
        for r in rows:                                               # (part slots are handed out in the order of `rows`)
            mine = [it for it in items if it[0] == r]
            if branch[r] in ("short", "long_but_no_split"):
                assert mine == [[r, 0, 1, 0]], (case, r)
                continue
            n = min(MAX_PARTS, -(-L[r] // P))
            assert (branch[r] == "split_capped") == (n < -(-L[r] // P)) and n > 1, (case, r)
            assert sorted(mine) == [[r, q, n, slots_taken] for q in range(n)], (case, r)
            slots_taken += n
            # the split depends on the row alone: the same in every range that holds the row
            assert split_of.setdefault((env, r), n) == n, (case, r)
        assert slots_taken == part_slots and n_split == sum(1 for r in warm if branch[r].startswith("split")), case
        for r, q, n, _ in items:                                     # most expensive first
            keys.append(L[r] / n + (k / 3.0 if q == 0 else 0.0))
        assert all(a >= b for a, b in zip(keys, keys[1:])), case
        orders_seen.add("cost_order" if n_split else "length_order")
        if not n_split:
            assert [it[0] for it in items] == rows, case
    assert seen == {"outside_the_range", "cold", "short", "long_but_no_split", "split", "split_capped"}
    assert orders_seen == {"cost_order", "length_order"}


# ---- parts of a split row -------------------------------------------------------------------------------------------------------
def test_part_ranges_tile_the_profile(recorded):
    seen = set()
    for (L, n, chunk), got in zip(recorded["parts/table"].tolist(), recorded["parts/ranges"].tolist()):
        case = (L, n, chunk)
        parts = got[:n]
        assert got[n:] == [[-1, -1]] * (MAX_PARTS - n), case
        assert parts[0][0] == PART_BEG and parts[-1][1] == PART_BEG + L, case
        assert all(b <= e for b, e in parts) and all(parts[q][1] == parts[q + 1][0] for q in range(n - 1)), case     # disjoint, ordered, no gap
        per = -(--(-L // n) // chunk) * chunk
        assert all(e - b == per for b, e in parts if e < PART_BEG + L), case                                         # whole chunks but the last
        seen.add("empty_trailing_part" if any(b == e for b, e in parts) else "every_part_takes_rows")
    assert seen == {"empty_trailing_part", "every_part_takes_rows"}
    assert [70, 5, GRAM_CHUNK] in recorded["parts/table"].tolist()


# ---- batches of a two-stage epoch -----------------------------------------------------------------------------------------------
def batch_branch(per_batch, n_local):
    if per_batch >= n_local:
        return "one_batch" if per_batch == n_local else "buffer_larger_than_the_half_step"
    if per_batch == 1:
        return "a_row_per_batch"
    return "ragged_last_batch" if n_local % per_batch else "even_batches"


def test_batches(shim, recorded):
    _, _, rows, items, counts, _ = work_items(shim, BATCH_ITEMS[0], BATCH_ITEMS[1], *BATCH_ITEMS[2], BATCH_ITEMS[3])
    rows, items = rows[:counts[0]].tolist(), items[:counts[1]].tolist()
    assert counts[2] > 0                                              # an item list with split rows
    pos = {r: i for i, r in enumerate(rows)}
    seen = set()
    for (per_batch, n_local, n_items), all_items, slots, batches, sizes in zip(recorded["batches/table"].tolist(), recorded["batches/items"].tolist(),
                                                                             recorded["batches/sys_slot"].tolist(), recorded["batches/batches"].tolist(),
                                                                             recorded["batches/counts"].tolist()):
        seen.add(batch_branch(per_batch, n_local))
        n_all, n_batches = sizes
        assert n_batches == -(-n_local // per_batch) and n_all == n_items + n_local, per_batch
        at = 0
        for b, (gram_off, gram_n, solve_off, solve_n) in enumerate(batches[:n_batches]):
            assert (gram_off, solve_off) == (at, at + gram_n), (per_batch, b)             # the offsets tile the list
            at += gram_n + solve_n
            gram, solve = all_items[gram_off:gram_off + gram_n], all_items[solve_off:solve_off + solve_n]
            mine = rows[b * per_batch:(b + 1) * per_batch]
            # stage 1: the global cost order, filtered to the rows of the batch
            assert gram == [it for it in items if pos[it[0]] // per_batch == b], (per_batch, b)
            # stage 2: one item per row of the batch
            assert solve == [[r, 0, 1, 0] for r in mine], (per_batch, b)
            slab = {}
            for it, s in zip(gram + solve, slots[gram_off:solve_off + solve_n]):
                assert 0 <= s < per_batch and slab.setdefault(it[0], s) == s, (per_batch, b)   # all parts and the solve item of a row: one slab
            assert len(set(slab.values())) == len(mine) and set(slab) == set(mine), (per_batch, b)   # distinct rows, distinct slabs
        assert at == n_all and all(v == [-1] * 4 for v in all_items[n_all:]), per_batch
    assert seen == {"a_row_per_batch", "even_batches", "ragged_last_batch", "one_batch", "buffer_larger_than_the_half_step"}


# ---- batch sizing ---------------------------------------------------------------------------------------------------------------
def gib_branch(free, knob):
    if knob is not None:
        return "knob_floored" if knob < 0.001 else "knob"
    if free == UNKNOWN or free / 4 / GIB >= 8:
        return "eight"
    return "quarter_of_free" if free / 4 / GIB >= 0.001 else "floor"


def test_system_gib(recorded):
    seen = set()
    for (free, knob), got in zip(GIB_TABLE, recorded["gib/result"].tolist()):
        branch = gib_branch(free, knob)
        seen.add(branch)
        assert got == {"knob": knob, "knob_floored": 0.001, "eight": 8.0, "quarter_of_free": free / 4 / GIB, "floor": 0.001}[branch], (free, knob)
    assert seen == {"knob", "knob_floored", "eight", "quarter_of_free", "floor"}


def test_rows_per_batch(recorded):
    slab_bytes = {k: int(r[10]) * 8 for (k, two_stage), r in zip(TILES_TABLE, recorded["tiles/result"]) if two_stage}
    seen = set()
    for (gib, k, longest), got in zip(PER_BATCH_TABLE, recorded["per_batch/result"].tolist()):
        fit = int(gib * GIB) // slab_bytes[k]
        branch = "not_even_one" if fit == 0 else ("longest_side" if fit >= longest else "buffer")
        seen.add(branch)
        assert got == {"not_even_one": 1, "longest_side": longest, "buffer": fit}[branch], (gib, k, longest)
    assert seen == {"not_even_one", "longest_side", "buffer"}


def test_halving_stops_at_64_slabs(recorded):
    slab_bytes = {k: int(r[10]) * 8 for (k, two_stage), r in zip(TILES_TABLE, recorded["tiles/result"]) if two_stage}
    seen = set()
    for (rows, gib, k, longest), per_batch, sizes, n in zip(HALVING_TABLE, recorded["halving/per_batch"].tolist(), recorded["halving/gib"].tolist(),
                                                           recorded["halving/count"].tolist()):
        per_batch, sizes = per_batch[:n], sizes[:n]
        seen.add("stops_at_once" if n == 1 else "halves")
        assert sizes[0] == gib and per_batch[0] <= rows and per_batch[-1] <= MIN_BATCH_ROWS, rows
        assert all(p > MIN_BATCH_ROWS for p in per_batch[:-1]), rows                       # stops at the first batch of at most 64 slabs
        for before, after, size in zip(per_batch, per_batch[1:], sizes[1:]):
            assert size == max(0.001, 0.5 * before * slab_bytes[k] / GIB) and before // 2 - 1 <= after <= (before + 1) // 2, (rows, before, after)
    assert seen == {"stops_at_once", "halves"}


def test_accounting(recorded):
    for (nnz, n_local, n_other, k), (flops, nbytes) in zip(ACCOUNTING_TABLE, recorded["accounting/result"].tolist()):
        k = float(k)
        assert flops == 2.0 * nnz * k * k + n_local * (k * k * k / 3.0 + 2.0 * k * k) + 2.0 * n_other * k * k
        assert nbytes == nnz * (8.0 * k + 8.0) + n_local * 8.0 * k


# ---- the environment ------------------------------------------------------------------------------------------------------------
def test_knob_parsing(recorded):
    knobs_of = dict(zip(ENV_TABLE, recorded["env/knobs"].tolist()))
    gib_of = dict(zip(ENV_TABLE, recorded["env/system_gib"].tolist()))
    assert knobs_of["unset"] == DEFAULT_KNOBS and gib_of["unset"] == 0.0
    # empty string: atoi / atof read 0 -- two-stage epochs off, a 0 GiB buffer (floored later), parts of CHUNK rows; a switch is on
    assert knobs_of["empty"] == [0, 1, CHUNK, 1, 1, 1] and gib_of["empty"] == 0.0
    assert knobs_of["numbers"] == [1, 1, 64, 0, 0, 0] and gib_of["numbers"] == 2.5
    assert knobs_of["zeros"] == [0, 1, CHUNK, 1, 1, 1] and gib_of["zeros"] == 0.0          # (NO_SPLIT=0 still means: no split)
    assert knobs_of["tails"] == [1, 1, 32, 0, 0, 0] and gib_of["tails"] == 10.0
    assert knobs_of["not_numbers"] == [0, 1, CHUNK, 0, 0, 0] and gib_of["not_numbers"] == 0.0
    assert knobs_of["part_rows_1"] == [1, 0, CHUNK, 0, 0, 0]
    assert knobs_of["negative"] == [1, 1, CHUNK, 0, 0, 0] and gib_of["negative"] == -4.0


# ---- the same tables under the sanitizers -----------------------------------------------------------------------------------------
def test_plan_program_under_address_and_undefined_behaviour_sanitizers(build_dir):
    exe = build_dir / "ials_plan_main"
    # (the sanitizers' runtimes are linked into the program, so that it does not depend on the order the loader finds libraries in)
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer",
                    "-static-libasan", "-static-libubsan", os.path.join(HERE, "ials_plan_main.cpp"), "-o", str(exe)], check=True)
    env = {k: v for k, v in os.environ.items() if not k.startswith(IALS)}
    done = subprocess.run([str(exe)], env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert done.returncode == 0, done.stdout[-4000:]
    assert "ials_plan_main: OK" in done.stdout
