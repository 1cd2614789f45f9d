"""The host arithmetic of a SLIM-BPR launch (csrc/slim_plan.h) on the CPU.

A shim (tests/slim_plan_shim.cpp) is compiled with g++ and called through ctypes on tables of inputs.  Every case
  * states the branch it must reach (the `*_branch` functions name it from the inputs alone, `check_*` says what the result of that
    branch looks like), so that a case that stops reaching it fails,
  * is compared exactly with tests/golden/slim_plan.npz -- recorded once by running the text of slim.hip as it stood before this
    arithmetic became functions of its own (copied into a harness with the compute-unit count, the occupancy and the knobs as
    inputs) on these same tables; the fixture holds the tables, too, so a table that changes is noticed.
"""
import ctypes as C
import itertools
import os
import subprocess

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden", "slim_plan.npz")

KNOBS = ("nap", "no_presched", "prof", "inject_abort", "sym_spare_cus", "sym_wgs", "sym_long_wgs", "owners", "cus", "owner_min_steps",
         "no_owner_gate")
DEFAULTS = dict(nap=1, no_presched=0, prof=0, inject_abort=0, sym_spare_cus=64, sym_wgs=None, sym_long_wgs=None, owners=128, cus=None,
                owner_min_steps=24, no_owner_gate=0)
OPTIONAL = ("sym_wgs", "sym_long_wgs", "cus")          # knobs whose default depends on the launch: passed as (set, value)
MAX_OWNERS, FLOW_WAVES = 192, 16
BIG = 10 ** 6


def knobs(**kw):
    par = dict(DEFAULTS, **kw)
    out = []
    for name in KNOBS:
        v = par[name]
        out += [int(v is not None), 0 if v is None else v] if name in OPTIONAL else [v]
    return np.array(out, dtype=np.int64)


def ptr(a):
    return a.ctypes.data_as(C.c_void_p)


# ---- the tables ---------------------------------------------------------------------------------------------------------------
def sym_table():
    """cus, per_cu, ahead, n, n_short, SYM_SPARE_CUS, SYM_WGS, SYM_LONG_WGS (None: unset)"""
    return list(itertools.product((2, 8, 256), (1, 2), (0, 1), ((1, 1), (1, 0), (17, 16), (1000, 860), (1000, 0)),
                                  (None, 0, BIG), (None, 1, BIG), (None, 0, BIG)))


def dense_table():
    """n_items, sparse weights, OWNERS, CUS, slots, OWNER_MIN_STEPS; 256 compute units, 2 workgroups per compute unit without LDS"""
    return list(itertools.product((1, 12288, 12289, 39936, 39937), (0, 1), (None, 0, 128, 500), (None, 1, 64), (0, 32, 256), (None, 1)))


SEGMENT_TABLE = list(itertools.product((1, 4, 5, 6, 10, 299, 300, 303), (0, 1)))
BITS_TABLE = (0, 1, 2, 3, 2 ** 31, 2 ** 62 + 1)
# nnz, n, n_users, n_cells: the expected size wins (ML-20M shape) / the stream at hand wins / a tiny model (the 1024 floor)
ROOMY_TABLE = ((20_000_263, 138_494, 138_493, 40_000_000), (1000, 50, 100, 1_000_000), (10, 3, 2, 12))
# sparse weights, symmetric, n_items, NO_PRESCHED
MODES_TABLE = list(itertools.product((0, 1), (0, 1), (92681, 92682), (0, 1)))

SLIM = "MI355REC_SLIM_"
ENV_NAMES = [SLIM + s for s in ("NAP", "NO_PRESCHED", "PROF", "INJECT_ABORT", "SYM_SPARE_CUS", "SYM_WGS", "SYM_LONG_WGS", "OWNERS", "CUS",
                                "OWNER_MIN_STEPS", "NO_OWNER_GATE", "GATE_WAIT_S")] + ["MI355REC_LOCK_DIR", "XDG_RUNTIME_DIR"]
INTS = ("NAP", "SYM_SPARE_CUS", "SYM_WGS", "SYM_LONG_WGS", "OWNERS", "CUS", "OWNER_MIN_STEPS")
SWITCHES = ("NO_PRESCHED", "PROF", "INJECT_ABORT", "NO_OWNER_GATE")
ENV_TABLE = {
    "unset": {},
    "empty": {name: "" for name in ENV_NAMES},                       # an empty integer knob is an unset one; an empty switch is ON
    "numbers": dict({SLIM + s: str(7 + i) for i, s in enumerate(INTS)}, **{SLIM + "GATE_WAIT_S": "0.2"}),
    "zeros": dict({SLIM + s: "0" for s in INTS + SWITCHES}, **{SLIM + "GATE_WAIT_S": "0"}),
    "atoi_tails": {SLIM + "NAP": " 12abc", SLIM + "OWNERS": "-3", SLIM + "CUS": "abc", SLIM + "SYM_WGS": "+5.9", SLIM + "GATE_WAIT_S": "1e1x"},
    "wait_not_a_number": {SLIM + "GATE_WAIT_S": "soon"},
    "lock_dir": {"MI355REC_LOCK_DIR": "/somewhere/locks", "XDG_RUNTIME_DIR": "/run/user/1"},
    "xdg_only": {"MI355REC_LOCK_DIR": "", "XDG_RUNTIME_DIR": "/run/user/1"},
}


# ---- running them -------------------------------------------------------------------------------------------------------------
def none_as(v, stand_in=-1):
    return stand_in if v is None else v


def run_sym(lib):
    rows, out = [], []
    for cus, per_cu, ahead, (n, n_short), spare, wgs, long_wgs in sym_table():
        k = knobs(sym_spare_cus=64 if spare is None else spare, sym_wgs=wgs, sym_long_wgs=long_wgs)
        r = np.zeros(2, np.int64)
        lib.slim_sym_launch(cus, per_cu, ahead, n, n_short, ptr(k), ptr(r))
        rows.append([cus, per_cu, ahead, n, n_short, none_as(spare), none_as(wgs), none_as(long_wgs)])
        out.append(r)
    return np.array(rows, np.int64), np.array(out)


def run_dense(lib):
    rows, out = [], []
    for n_items, sparse, owners, cus_knob, slots, min_steps in dense_table():
        k = knobs(owners=128 if owners is None else owners, cus=cus_knob, owner_min_steps=24 if min_steps is None else min_steps)
        plan, grid = np.zeros(3, np.int64), np.zeros(6, np.int64)
        lib.slim_dense_plan(n_items, sparse, 256, ptr(k), ptr(plan))
        lib.slim_dense_grid(slots, 256, 2, C.c_int64(int(plan[2])), ptr(k), ptr(grid))
        rows.append([n_items, sparse, none_as(owners), none_as(cus_knob), slots, none_as(min_steps)])
        out.append(np.concatenate([plan, grid]))
    return np.array(rows, np.int64), np.array(out)


def run_segments(lib):
    rows, out = [], []
    for n, sparse in SEGMENT_TABLE:
        seg = np.zeros((16, 3), np.int64)
        count = lib.slim_segments(n, sparse, ptr(seg), 16)
        assert 0 < count <= 16
        seg[count:] = -1
        rows.append([n, sparse])
        out.append(seg)
    return np.array(rows, np.int64), np.array(out)


def run_bits(lib):
    lib.slim_bits_for.argtypes = [C.c_uint64]
    return np.array(BITS_TABLE, np.uint64), np.array([lib.slim_bits_for(v) for v in BITS_TABLE], np.int64)


def run_roomy(lib):
    lib.slim_roomy.argtypes = [C.c_uint64, C.c_int, C.c_int, C.c_int64]
    lib.slim_roomy.restype = C.c_uint64
    return np.array(ROOMY_TABLE, np.int64), np.array([lib.slim_roomy(*row) for row in ROOMY_TABLE], np.uint64)


def run_modes(lib):
    return np.array(MODES_TABLE, np.int64), np.array([lib.slim_flow_modes(sp, sym, n, ptr(knobs(no_presched=off))) for sp, sym, n, off in MODES_TABLE],
                                                      np.int64)


def read_environment(lib, setting):
    """the knobs as the library parses them with exactly `setting` in the environment"""
    saved = {name: os.environ.get(name) for name in ENV_NAMES}
    try:
        for name in ENV_NAMES:
            os.environ.pop(name, None)
        os.environ.update(setting)
        k, wait, where = np.zeros(14, np.int64), C.c_double(0), C.create_string_buffer(256)
        lib.slim_read_knobs(ptr(k), C.byref(wait), where, 256)
        return k, wait.value, where.value.decode()
    finally:
        for name, v in saved.items():
            os.environ.pop(name, None)
            if v is not None:
                os.environ[name] = v


def run_env(lib):
    got = [read_environment(lib, ENV_TABLE[name]) for name in ENV_TABLE]
    return np.array(list(ENV_TABLE)), (np.array([g[0] for g in got]), np.array([g[1] for g in got]), np.array([g[2] for g in got]))


FAMILIES = dict(sym=run_sym, dense=run_dense, segments=run_segments, bits=run_bits, roomy=run_roomy, modes=run_modes)


def record(lib):
    """name -> array, as the fixture holds them"""
    out = {}
    for name, run in FAMILIES.items():
        out[name + "/table"], out[name + "/result"] = run(lib)
    out["env/table"], (out["env/knobs"], out["env/wait_s"], out["env/lock_dir"]) = run_env(lib)
    return out


@pytest.fixture(scope="module")
def shim(tmp_path_factory):
    so = tmp_path_factory.mktemp("slim_plan") / "slim_plan_shim.so"
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-shared", "-fPIC", os.path.join(HERE, "slim_plan_shim.cpp"), "-o", str(so)],
                   check=True)
    return C.CDLL(str(so))


@pytest.fixture(scope="module")
def golden():
    return np.load(GOLDEN)


@pytest.fixture(scope="module")
def recorded(shim):
    return record(shim)


# ---- against the recorded results ---------------------------------------------------------------------------------------------
def test_the_fixture_has_exactly_these_arrays(golden, recorded):
    assert sorted(golden.files) == sorted(recorded)


@pytest.mark.parametrize("name", list(FAMILIES) + ["env"])
def test_results_equal_the_recorded_results(golden, recorded, name):
    for key in sorted(k for k in recorded if k.startswith(name + "/")):
        want, got = golden[key], recorded[key]
        assert got.shape == want.shape and got.dtype == want.dtype, key
        where = np.argwhere(got != want)
        assert where.size == 0, (key, where[:5].tolist())


def test_constants(shim):
    c = np.zeros(8, np.int64)
    shim.slim_constants(ptr(c))
    assert c.tolist() == [1024, 1024, 16, 4, 256, 192, 16, 8]


# ---- symmetric grid -----------------------------------------------------------------------------------------------------------
def sym_branch(n, n_short, wgs):
    if n == n_short:
        return "no_long_step"
    if n_short == 0:
        return "no_short_step"
    return "floor_of_two" if wgs == 1 else "both_queues"


def test_symmetric_grid_reaches_its_branches(recorded):
    seen = set()
    for (cus, per_cu, ahead, n, n_short, spare, wgs, long_knob), (long_wgs, grid) in zip(recorded["sym/table"], recorded["sym/result"]):
        case = (cus, per_cu, ahead, n, n_short, spare, wgs, long_knob)
        branch = sym_branch(n, n_short, wgs)
        seen.add(branch)
        spare_cus = 0 if not ahead else max(0, min(cus // 2, 64 if spare < 0 else spare))
        fit = (cus - spare_cus) * per_cu
        assert long_wgs <= n - n_short and grid - long_wgs <= max(1, -(-n_short // FLOW_WAVES)), case
        assert grid <= max(2, fit) and (wgs < 0 or grid <= max(2, wgs)), case       # never more than fits, nor than asked for
        if branch == "no_long_step":
            assert long_wgs == 0 and grid >= 1, case
        elif branch == "no_short_step":
            assert long_wgs >= 1 and grid == long_wgs + 1, case                     # (one workgroup finds the short queue empty)
        elif branch == "floor_of_two":
            assert (long_wgs, grid) == (1, 2), case
        else:
            assert long_wgs >= 1 and grid >= 2, case                                # never below 2 with both queues non-empty
            if long_knob == 0 or n - n_short == 1:
                assert long_wgs == 1, case
        if ahead and spare == BIG:
            assert grid <= max(2, (cus - cus // 2) * per_cu), case                  # at most half of the compute units are spared
    assert seen == {"no_long_step", "no_short_step", "floor_of_two", "both_queues"}


# ---- dense plan and grid ------------------------------------------------------------------------------------------------------
def dense_branch(n_items, sparse, owners, slots):
    if sparse:
        plan = "sparse_store"
    elif owners == 0:
        plan = "owners_off"
    elif n_items == 39937:
        plan = "row_too_large"                       # 159 760 + 4 096 bytes > 160 KiB; 39 936 items: exactly 160 KiB
    else:
        plan = "wanted"
    if slots == 0:
        return plan, "queue_only"
    return plan, "owners_big_lds" if n_items >= 12289 else "owners"          # 12 288 floats are the 48 KiB a kernel gets unasked


def test_dense_plan_and_grid_reach_their_branches(recorded):
    seen = set()
    for (n_items, sparse, owners, cus_knob, slots, min_steps), r in zip(recorded["dense/table"], recorded["dense/result"]):
        case = (n_items, sparse, owners, cus_knob, slots, min_steps)
        wanted, want_slots, row_bytes, has_owners, lds, grid, max_owners, steps, attribute = (int(v) for v in r)
        plan, launch = dense_branch(n_items, sparse, owners, slots)
        seen.add((plan, launch))
        assert row_bytes == (4 * n_items + 15) // 16 * 16, case
        assert wanted == (plan == "wanted"), case
        assert want_slots == {-1: 256, 1: 32, 64: 64}[cus_knob], case
        cap = min(MAX_OWNERS, 128 if owners < 0 else owners)
        assert steps == (24 if min_steps < 0 else 2), case
        if launch == "queue_only":
            assert (has_owners, lds, grid, attribute) == (0, 0, 512, 0) and max_owners == min(cap, 256), case
        else:
            assert (has_owners, lds, grid) == (1, row_bytes, slots) and attribute == (launch == "owners_big_lds"), case
            assert max_owners == min(cap, slots // 2) and (slots != 32 or max_owners <= 16), case
        if owners == 500 and slots == 0:
            assert max_owners == MAX_OWNERS, case
    assert {p for p, _ in seen} == {"sparse_store", "owners_off", "row_too_large", "wanted"}
    assert {q for _, q in seen} == {"queue_only", "owners", "owners_big_lds"}


# ---- segments -----------------------------------------------------------------------------------------------------------------
def test_segments_tile_the_epoch_and_prune_where_the_reference_does(recorded):
    seen = set()
    for (n, sparse), seg in zip(recorded["segments/table"], recorded["segments/result"]):
        seg = seg[seg[:, 0] >= 0]
        branch = "one_stream" if not sparse or n < 5 else "cut"
        seen.add(branch)
        assert seg[0, 0] == 0 and (seg[:, 1] > 0).all() and (seg[1:, 0] == seg[:-1, 0] + seg[:-1, 1]).all() and seg[-1, 0] + seg[-1, 1] == n, (n, sparse)
        if branch == "one_stream":
            assert seg.tolist() == [[0, n, 0]]
            continue
        # numCurrentBatch % (totalNumberOfBatch / 5) == 0 and numCurrentBatch != 0, after the step with that index
        every = n // 5
        last = seg[:, 0] + seg[:, 1] - 1
        assert (seg[:, 2] == ((last % every == 0) & (last != 0))).all(), (n, seg.tolist())
        assert sorted(last[seg[:, 2] == 1].tolist()) == [t for t in range(1, n) if t % every == 0], (n, seg.tolist())
    assert seen == {"one_stream", "cut"}


# ---- the small ones -----------------------------------------------------------------------------------------------------------
def test_bits_for(recorded):
    assert recorded["bits/result"].tolist() == [1, 1, 1, 2, 31, 63]


def test_roomy_capacity(recorded):
    for (nnz, n, n_users, n_cells), got in zip(ROOMY_TABLE, recorded["roomy/result"].tolist()):
        assert got == max(int(2.5 * nnz * n / n_users) + 1024, n_cells + n_cells // 4) and got >= n_cells
    expected_wins, stream_wins, floor = recorded["roomy/result"].tolist()
    assert expected_wins > 50_000_000 and stream_wins == 1_250_000 and floor == 1024 + 37


def test_flow_modes(recorded):
    for (sparse, sym, n_items, off), got in zip(MODES_TABLE, recorded["modes/result"].tolist()):
        supported = not (sym and n_items > 92681)
        assert got == int(supported) | 2 * int(supported and not sparse and not off)


def test_knob_parsing(recorded):
    knobs_of = dict(zip(ENV_TABLE, recorded["env/knobs"].tolist()))
    wait_of = dict(zip(ENV_TABLE, recorded["env/wait_s"].tolist()))
    dir_of = dict(zip(ENV_TABLE, recorded["env/lock_dir"].tolist()))
    default = knobs().tolist()
    assert knobs_of["unset"] == default and wait_of["unset"] == 600.0 and dir_of["unset"] == "/tmp"
    # empty string: an integer knob is unset, a switch is on, the wait is atof("") = 0, the directories fall through
    on = knobs(no_presched=1, prof=1, inject_abort=1, no_owner_gate=1).tolist()
    assert knobs_of["empty"] == on and wait_of["empty"] == 0.0 and dir_of["empty"] == "/tmp"
    assert knobs_of["numbers"] == knobs(nap=7, sym_spare_cus=8, sym_wgs=9, sym_long_wgs=10, owners=11, cus=12, owner_min_steps=13).tolist()
    assert wait_of["numbers"] == 0.2
    assert knobs_of["zeros"] == knobs(nap=0, sym_spare_cus=0, sym_wgs=0, sym_long_wgs=0, owners=0, cus=0, owner_min_steps=0, no_presched=1, prof=1,
                                      inject_abort=1, no_owner_gate=1).tolist() and wait_of["zeros"] == 0.0
    assert knobs_of["atoi_tails"] == knobs(nap=12, owners=-3, cus=0, sym_wgs=5).tolist() and wait_of["atoi_tails"] == 10.0
    assert wait_of["wait_not_a_number"] == 0.0
    assert dir_of["lock_dir"] == "/somewhere/locks" and dir_of["xdg_only"] == "/run/user/1"
