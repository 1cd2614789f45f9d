"""The column schedule of a similarity build (csrc/sim_plan.h, plan_columns) on the CPU.

A shim (tests/sim_plan_shim.cpp) is compiled with g++ and called through ctypes on a table of synthetic inputs.  Every case
  * states the branch of the schedule it must reach (`reach`), so that a case that stops reaching it fails,
  * is compared exactly with tests/golden/sim_plan.npz -- recorded once by running the text of run_columns_lds as it stood before
    the schedule became a function of its own (copied into a harness with a stub handle) on this same table,
  * satisfies the schedule's invariants (test_invariants).
"""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden", "sim_plan.npz")

COSINE, TVERSKY, EUCLIDEAN = 0, 6, 7            # MI355REC_SIM_*
LDS_FIXED = 32 * 1024 + 96                      # selection scratch + the workgroup's shared scalars
LDS_PACKED_FIXED = 16 * 1024 + 96
SCALARS = ("threads", "max_grid", "lds", "lds_packed", "acc_words", "packed_words", "fast_topk", "n_packed", "n_legacy", "n_items",
           "part_slots", "n_split", "n_local", "cost_sum", "nnz_range", "start", "end", "has_out_slot")
IP = ("n_cols", "tile_w", "n_tiles", "acc_mode", "group_lanes", "topK", "dense", "similarity", "shrink", "cus", "lds_fixed",
      "lds_packed_fixed", "start", "end", "part", "n_parts", "slot_first", "slot_count",
      "one_wg_per_cu", "min_part_users", "fast_topk", "packed", "no_packed", "packed_heavy", "packed_demote", "phases")
DEFAULTS = dict(n_tiles=1, acc_mode=0, group_lanes=16, topK=10, dense=0, similarity=COSINE, shrink=0, cus=4, lds_fixed=LDS_FIXED,
                lds_packed_fixed=LDS_PACKED_FIXED, start=0, end=None, part=0, n_parts=0, slot_first=0, slot_count=0x7FFFFFFF,
                one_wg_per_cu=0, min_part_users=0, fast_topk=1, packed=-1, no_packed=0, packed_heavy=1, packed_demote=-1, phases=0,
                alpha=1.0, beta=1.0)


def columns(seed, n, lo, hi, special=()):
    """n columns with costs in [lo, hi); `special`: (column, cost, users, walk entries) of the columns a case is about."""
    rng = np.random.default_rng(seed)
    cost = rng.integers(lo, hi, size=n).astype(np.int64)
    users = np.maximum(1, cost // rng.integers(4, 12, size=n))
    walk = users + users // 16
    for c, k, u, w in special:
        cost[c], users[c], walk[c] = k, u, w
    ptr = lambda x: np.concatenate([[0], np.cumsum(x)]).astype(np.int32)
    order = np.argsort(-cost, kind="stable").astype(np.int32)          # most expensive first, ties by ascending column
    return dict(cost=cost, order=order, csc_ptr=ptr(users), walk_ptr=ptr(walk))


# ---- the inputs -------------------------------------------------------------------------------------------------------------
# tile_w 2 000: 40 880 B of LDS -> 512 threads, 3 workgroups per CU.  tile_w 12 000: 80 880 B -> 1024 threads, one per CU, and
# (all-ones data, topK 10, 16 lanes, mean cost below PACKED_MAX_PAIRS_PER_COLUMN) the packed-counts launch in front.
PLAIN = dict(cols=(11, 200, 100, 2000), tile_w=2000)
DOMINANT = dict(cols=(12, 150, 500, 1500, ((40, 1_000_000, 5000, 5000), (41, 300_000, 900, 900))), tile_w=2000, min_part_users=64)
WIDE = dict(tile_w=12000)
LIGHT = dict(WIDE, cols=(13, 120, 1000, 5000, ((7, 100, 20, 20),)))
MANY = dict(WIDE, cols=(14, 120, 190_000, 210_000, ((9, 300_000, 70_000, 100_000),)))
TOO_MANY = dict(WIDE, cols=(15, 120, 1000, 5000, ((9, 300_000, 70_000, 64 * 49152 + 1),)))
HEAVY = dict(WIDE, cols=(16, 200, 900, 1100, ((3, 600_000, 60_000, 60_000),)))
HEAVY_MINOR = dict(WIDE, cols=(17, 200, 9_000, 11_000, ((3, 600_000, 60_000, 60_000),)))
PACKED_SPLIT = dict(WIDE, cols=(18, 200, 2500, 3500, ((5, 200_000, 10_000, 10_000), (9, 300_000, 70_000, 64 * 49152 + 1))))
EXPENSIVE = dict(WIDE, cols=(19, 40, 1_900_000, 2_100_000))       # (40 columns: none is a quarter of a packed workgroup's share)
PARTS = dict(cols=(20, 50, 100, 2000), tile_w=2000)


def whole(r, c):
    """(index, item) of column c's unsplit item"""
    hits = [(i, it) for i, it in enumerate(r.items) if it[0] == c and it[3] >= 0 and (it[2] & 0xFFFF) == 1]
    assert len(hits) == 1, (c, hits)
    return hits[0]


def parts_of(r, c):
    return [(i, it) for i, it in enumerate(r.items) if it[0] == c and it[3] >= 0]


def merge_items(r):
    return [(i, it) for i, it in enumerate(r.items) if i >= r.n_packed and it[3] < 0]


def reach_dominant(r):
    # limit = 1 456 751 / 24 = 60 697: column 40 in 17 parts of 58 823, column 41 in 5 of 60 000 -- which the re-sort puts first
    a, b = parts_of(r, 40), parts_of(r, 41)
    assert r.threads == 512 and r.n_split == 2 and (len(a), len(b)) == (17, 5) and r.part_slots == 22
    assert [i for i, _ in b] == list(range(5)) and [i for i, _ in a] == list(range(5, 22))


def reach_few_entries(r):
    assert r.n_split == 1 and r.part_slots == 10 and len(parts_of(r, 40)) == 10           # 640 walk entries / MIN_PART_USERS


def reach_light(r):
    i, it = whole(r, 7)
    assert r.n_packed > 0 and r.threads == 1024 and i >= r.n_packed and it[3] == 1        # cost 100 < 16 * topK: the 32-bit list, .w == 1


def reach_many(r):
    p = parts_of(r, 9)
    n_c = 100_000
    assert r.n_packed > 0 and all(i < r.n_packed for i, _ in p) and len(p) == 3 and -(-n_c // len(p)) <= r.PACKED_PART_ENTRIES
    assert all(it[2] == (3 | 1 << 16) for _, it in p)
    (i, it), = merge_items(r)
    assert it[0] == 9 and it[3] == -(1 + p[0][1][3]) and tuple(r.ranges[i]) == (3, 3) and i == r.n_items - 1


def reach_too_many(r):
    p = parts_of(r, 9)
    assert r.n_packed > 0 and all(i >= r.n_packed for i, _ in p) and not merge_items(r)


def reach_heavy_out(r):
    assert r.n_packed > 0 and all(i >= r.n_packed for i, _ in parts_of(r, 9)) and not merge_items(r)


def reach_demoted(expected_parts):
    def check(r):
        p = parts_of(r, 3)
        # (the 32-bit limit from legacy_cost = 600 000: 8 parts of 75 000; from the call's cost_sum it would be fewer)
        assert r.n_packed > 0 and all(i >= r.n_packed for i, _ in p) and len(p) == expected_parts
    return check


def reach_not_demoted(r):
    p = parts_of(r, 3)
    assert r.n_packed > 0 and all(i < r.n_packed for i, _ in p)


def reach_packed_split(r):
    a, b = parts_of(r, 5), parts_of(r, 9)
    assert len(a) == 4 and all(i < r.n_packed and it[3] == 0 for i, it in a)            # 10 000 entries / (4 * 512), slots 0..3
    assert len(b) > 1 and all(i >= r.n_packed and it[3] == 4 for i, it in b)            # the 32-bit list's split goes on from slot 4
    assert r.n_split == 2 and r.part_slots == 4 + len(b)


def expect(**kw):
    def check(r):
        for k, v in kw.items():
            assert getattr(r, k) == v, (k, getattr(r, k), v)
    return check


def packed_on(r):
    assert r.n_packed > 0 and r.threads == 1024


def packed_off(r):
    assert r.n_packed == 0 and r.threads == 1024 and r.n_legacy == r.n_items


def reach_part(n_expected):
    def check(r):
        assert r.has_out_slot == 1 and r.n_local == n_expected and (r.out_slot >= 0).sum() == n_expected and (r.out_slot == -1).sum() == 50 - n_expected
        assert (r.start, r.end) == (0, 50)
    return check


CASES = {
    # 1. plain contiguous ranges
    "plain": (PLAIN, {}, expect(threads=512, max_grid=12, n_split=0, n_packed=0, n_local=200, fast_topk=1)),
    "plain_inner_range": (PLAIN, dict(start=37, end=151), expect(threads=512, n_split=0, n_local=114, start=37, end=151, has_out_slot=0)),
    "plain_one_wg_per_cu": (PLAIN, dict(one_wg_per_cu=1), expect(threads=1024, max_grid=4, n_split=0)),
    # 2. one dominant column
    "dominant": (DOMINANT, {}, reach_dominant),
    "dominant_few_entries": (dict(DOMINANT, cols=(12, 150, 500, 1500, ((40, 1_000_000, 640, 640),))), {},
                             reach_few_entries),
    "dominant_two_tiles": (DOMINANT, dict(n_tiles=2), expect(n_split=0, part_slots=0, n_items=150, fast_topk=0)),
    # 3. the packed-counts launch and what it leaves to the 32-bit one
    "packed_light": (LIGHT, {}, reach_light),
    "packed_many_users": (MANY, {}, reach_many),
    "packed_too_many_parts": (TOO_MANY, {}, reach_too_many),
    "packed_heavy_0": (MANY, dict(packed_heavy=0), reach_heavy_out),
    # 4. heavy demotion
    "demote_default": (HEAVY, {}, reach_demoted(8)),
    "demote_0": (HEAVY, dict(packed_demote=0), reach_not_demoted),
    "demote_minor_default": (HEAVY_MINOR, {}, reach_not_demoted),
    "demote_minor_1": (HEAVY_MINOR, dict(packed_demote=1), reach_demoted(8)),
    # 5. a split in the packed list, then one in the 32-bit list
    "packed_split": (PACKED_SPLIT, {}, reach_packed_split),
    # 6. the switches of the packed launch
    "packed_default": (LIGHT, {}, packed_on),
    "packed_0": (LIGHT, dict(packed=0), packed_off),
    "no_packed": (LIGHT, dict(no_packed=1), packed_off),
    "expensive_default": (EXPENSIVE, {}, packed_off),
    "expensive_packed_1": (EXPENSIVE, dict(packed=1), packed_on),
    "packed_dense": (LIGHT, dict(topK=0, dense=1), packed_off),
    "packed_32_lanes": (LIGHT, dict(group_lanes=32), packed_off),
    "packed_int32": (LIGHT, dict(acc_mode=1), packed_off),
    # 7. the threshold-first selection
    "fast_on": (PLAIN, {}, expect(fast_topk=1, threads=512)),
    "fast_0": (PLAIN, dict(fast_topk=0), expect(fast_topk=0)),
    "fast_euclidean": (PLAIN, dict(similarity=EUCLIDEAN), expect(fast_topk=0)),
    "fast_negative_shrink": (PLAIN, dict(shrink=-1), expect(fast_topk=0)),
    "fast_tversky_4": (PLAIN, dict(similarity=TVERSKY, alpha=4.0), expect(fast_topk=1)),
    "fast_tversky_4_5": (PLAIN, dict(similarity=TVERSKY, alpha=4.5), expect(fast_topk=0)),
    "fast_topk_128": (PLAIN, dict(topK=128), expect(fast_topk=1, threads=512)),
    "fast_topk_129": (PLAIN, dict(topK=129), expect(fast_topk=0, threads=512)),
    # 8. interleaved parts (50 columns = 16 groups of 3 and positions 48, 49 for parts 0 and 1: 17, 17, 16)
    "part_0_of_3": (PARTS, dict(part=0, n_parts=3), reach_part(17)),
    "part_1_of_3": (PARTS, dict(part=1, n_parts=3), reach_part(17)),
    "part_2_of_3": (PARTS, dict(part=2, n_parts=3), reach_part(16)),
    "part_0_of_1": (PARTS, dict(part=0, n_parts=1), reach_part(50)),
    "part_chunk": (PARTS, dict(part=1, n_parts=3, slot_first=2, slot_count=3), reach_part(3)),
    "part_chunk_past_end": (PARTS, dict(part=1, n_parts=3, slot_first=15, slot_count=10), reach_part(2)),
}


class Result:
    pass


def run_case(lib, name):
    """-> (the case's input arrays, its parameters, the plan the library at hand makes)"""
    setup, over, _ = CASES[name]
    par = dict(DEFAULTS, **{k: v for k, v in setup.items() if k != "cols"})
    par.update(over)
    col = columns(*setup["cols"])
    n = len(col["cost"])
    par["n_cols"] = n
    if par["end"] is None:
        par["end"] = n
    ip = np.array([par[k] for k in IP], dtype=np.int32)
    fp = np.array([par["alpha"], par["beta"]], dtype=np.float32)
    cap = 4 * n + 4096
    scalars = np.zeros(len(SCALARS), dtype=np.int64)
    items, ranges, out_slot = np.zeros((cap, 4), np.int32), np.zeros((cap, 2), np.int32), np.zeros(n, np.int32)
    ptr = lambda a: a.ctypes.data_as(C.c_void_p)
    lib.sim_plan_shim.restype = C.c_int
    n_items = lib.sim_plan_shim(ptr(col["cost"]), ptr(col["order"]), ptr(col["csc_ptr"]), ptr(col["walk_ptr"]), ptr(ip), ptr(fp), ptr(scalars),
                                ptr(items), ptr(ranges), ptr(out_slot), C.c_int(cap))
    assert n_items >= 0
    consts = np.zeros(5, dtype=np.int64)
    lib.sim_plan_constants(ptr(consts))
    r = Result()
    r.scalars, r.items, r.ranges, r.out_slot = scalars, items[:n_items].copy(), ranges[:n_items].copy(), out_slot
    for k, v in zip(SCALARS, scalars):
        setattr(r, k, int(v))
    r.PACKED_PART_ENTRIES = int(consts[0])
    assert tuple(consts[2:]) == (0, 1, 2)
    return col, par, r


@pytest.fixture(scope="module")
def shim(tmp_path_factory):
    so = tmp_path_factory.mktemp("sim_plan") / "sim_plan_shim.so"
    subprocess.run(["g++", "-std=c++17", "-O1", "-shared", "-fPIC", "-D__HIP_PLATFORM_AMD__", "-I/opt/rocm/include",
                    os.path.join(HERE, "sim_plan_shim.cpp"), "-o", str(so)], check=True)
    return C.CDLL(str(so))


@pytest.fixture(scope="module")
def golden():
    return np.load(GOLDEN)


@pytest.mark.parametrize("name", list(CASES))
def test_case_reaches_its_branch(shim, name):
    _, _, r = run_case(shim, name)
    CASES[name][2](r)


@pytest.mark.parametrize("name", list(CASES))
def test_plan_equals_the_recorded_plan(shim, golden, name):
    _, _, r = run_case(shim, name)
    for field in ("scalars", "items", "ranges", "out_slot"):
        want = golden[f"{name}/{field}"]
        got = getattr(r, field)
        assert got.shape == want.shape and np.array_equal(got, want), (name, field)


def test_the_fixture_has_exactly_these_cases(golden):
    assert sorted({k.split("/")[0] for k in golden.files}) == sorted(CASES)


def selection(par, order):
    """the columns of the call in output order, worked out independently of the library"""
    if par["n_parts"] == 0:
        return list(range(par["start"], par["end"]))
    mine = []
    for pos, c in enumerate(order):
        group, within = divmod(pos, par["n_parts"])
        if (par["n_parts"] - 1 - within if group % 2 else within) == par["part"]:
            mine.append(int(c))
    return mine[par["slot_first"]:par["slot_first"] + par["slot_count"]]


@pytest.mark.parametrize("name", list(CASES))
def test_invariants(shim, name):
    col, par, r = run_case(shim, name)
    cost, walk_ptr = col["cost"], col["walk_ptr"]
    chosen = selection(par, col["order"])
    assert r.n_local == len(chosen) and r.n_packed + r.n_legacy == r.n_items == len(r.items)
    assert r.cost_sum == int(cost[chosen].sum()) and r.nnz_range == int((col["csc_ptr"][1:] - col["csc_ptr"][:-1])[chosen].sum())
    if par["n_parts"] > 0:
        want_slot = np.full(par["n_cols"], -1, np.int32)
        want_slot[chosen] = np.arange(len(chosen))
        assert np.array_equal(r.out_slot, want_slot)
    else:
        assert r.has_out_slot == 0 and (r.out_slot == -1).all()
    merges = dict((int(it[0]), (i, it)) for i, it in merge_items(r))
    assert all(i >= r.n_items - len(merges) for i, _ in merges.values())           # the merge items close the 32-bit list
    seen, slots = {}, 0
    for i, it in enumerate(r.items):
        c, q, z, w = (int(v) for v in it)
        if w < 0 and i >= r.n_packed:
            continue
        seen.setdefault(c, []).append((i, q, z, w))
    assert sorted(seen) == sorted(chosen)               # every column of the selection, and no other
    for c, its in seen.items():
        packed_list = its[0][0] < r.n_packed
        assert all((i < r.n_packed) == packed_list for i, _, _, _ in its)          # in ONE of the two lists
        parts = its[0][2] & 0xFFFF
        many = bool(its[0][2] >> 16)
        assert all(z == its[0][2] for _, _, z, _ in its) and sorted(q for _, q, _, _ in its) == list(range(parts)) and len(its) == parts
        assert (c in merges) == many and (not many or packed_list)
        if parts > 1 or many:
            assert all(w == its[0][3] for _, _, _, w in its)                       # one first slot
            slots += parts
            if many:
                i, it = merges[c]
                assert it[3] == -(1 + its[0][3]) and tuple(r.ranges[i]) == (parts, parts)
        for i, _, _, _ in its:
            assert tuple(r.ranges[i]) == (walk_ptr[c], walk_ptr[c + 1])
    assert r.part_slots == slots
    item_cost = [int(cost[it[0]]) // (int(it[2]) & 0xFFFF) for it in r.items]
    for lo, hi in ((0, r.n_packed), (r.n_packed, r.n_items - len(merges))):
        assert all(item_cost[i] >= item_cost[i + 1] for i in range(lo, hi - 1)), (lo, hi)
