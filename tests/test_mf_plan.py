"""The host arithmetic of a BPR-MF / FunkSVD / AsySVD call (csrc/mf_plan.h) on the CPU.

A shim (tests/mf_plan_shim.cpp) is compiled with g++ and called through ctypes on tables of inputs.  Every case
  * states the branch it must reach (the `*_branch` functions name it from the inputs alone), and each test asserts that the set of
    branches its table reached is complete, so that a case that stops reaching its branch fails,
  * is compared exactly with tests/golden/mf_plan.npz -- recorded once by running the text of mf.hip as it stood before this
    arithmetic became functions of its own (launch_batch's ladder, kernel_class, launch_group_batch's switch, samples_in_flight,
    fast_schedule_fits, schedule_span, schedule_draws, fast_sched_params, enqueue_schedule, ensure_stream_capacity, enqueue_stream's
    loop, run_epochs_typed, ensure_epoch_graph, group_run_epochs_typed, mi355rec_mf_group_create's checks, the exact multi-GPU
    mode's numbers and the getenv sites, copied into a harness with a handle of plain numbers, behind the same extern "C" interface
    as the shim) through record() below on these same tables; the fixture holds the tables, too, so a table that changes is noticed.
tests/mf_plan_main.cpp goes through the header once more as a program of its own under the address and undefined-behaviour
sanitizers: smaller tables held in real arrays, and the cases of this file that sit at an integer limit.
"""
import ctypes as C
import itertools
import os
import subprocess

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden", "mf_plan.npz")

BPR, FUNK, ASY = 0, 1, 2
SCHED_THREADS, FAST_MAX_BATCHES, FAST_MAX_SLOTS, SCHED_STAMPS = 1024, 256, 8192, 8
ASY_CHUNK, GRAPH_SEGMENT, MAX_GRAPH_BATCHES = 1 << 16, 4096, 64 * 4096
# the compiled instances of the mini-batch kernel: (max chunks, LPR, KI, samples in flight)
ROW_WIDTHS = ((16, 16, 1, 4), (32, 32, 1, 2), (64, 64, 1, 1), (128, 64, 2, 1))

ENV_NAMES = ["MI355REC_MF_GENERAL_SCHEDULE", "MI355REC_MF_NO_FUSE", "MI355REC_MF_WHOLE_STREAM_SCHEDULE", "MI355REC_MF_TICKS",
             "MI355REC_MF_GROUP_PER_MEMBER_SCHEDULE", "MI355REC_MF_GROUP_NO_LOOKAHEAD", "MI355REC_NO_GRAPH"]
KNOB_NAMES = ["general", "no_fuse", "whole_stream", "ticks", "per_member", "no_lookahead", "no_graph"]


def ptr(a):
    return a.ctypes.data_as(C.c_void_p)


def shape(algorithm=BPR, n_users=1000, n_items=500, nnz=50000, k=64, f64=0, B=100, sharded=0, fast=1):
    return (algorithm, n_users, n_items, nnz, k, f64, B, sharded, fast)


def knobs(**on):
    assert set(on) <= set(KNOB_NAMES)
    return tuple(int(bool(on.get(name))) for name in KNOB_NAMES)


def arr(t):
    return np.array(t, np.int64)


def per_sample(s):
    return 3 if s[0] == BPR else 2


def tpb_of(s):
    return per_sample(s) * s[6]


def per_epoch_of(s):
    return (s[1] if s[0] == BPR else s[3]) // s[6] + 1


def with_batches(algorithm, nb, B=10, **kw):
    """a shape whose epoch has nb mini-batches"""
    if algorithm == BPR:
        return shape(BPR, n_users=(nb - 1) * B, B=B, **kw)
    return shape(algorithm, nnz=(nb - 1) * B, B=B, **kw)


def bits_for(n):
    b = 1
    while b < 63 and (1 << b) < n:
        b += 1
    return b


# ---- the tables ---------------------------------------------------------------------------------------------------------------
# both sides of every row of ROW_WIDTHS, rows that are no whole number of 16-byte chunks, rows wider than the last instance
WIDTH_TABLE = [(k, 0) for k in (1, 4, 10, 64, 68, 128, 132, 130, 256, 260, 512)] + [(k, 1) for k in (2, 5, 32, 34, 64, 66, 128, 130, 256, 258, 300, 512)]

FITS_TABLE = [(shape(), knobs(), 256), (shape(), knobs(), 257),
              (shape(BPR, B=2730), knobs(), 1), (shape(BPR, B=2731), knobs(), 1),                       # 8 190 | 8 193 header slots
              (shape(FUNK, B=4096), knobs(), 1), (shape(FUNK, B=4097), knobs(), 1),
              # 31 bits for (row, slot): 13 slot bits leave 18 for the rows, 10 leave 21
              (shape(FUNK, n_users=200000, n_items=62144, B=4096), knobs(), 1), (shape(FUNK, n_users=200000, n_items=62145, B=4096), knobs(), 1),
              (shape(BPR, n_users=2 ** 20, n_items=2 ** 20, B=100), knobs(), 1), (shape(BPR, n_users=2 ** 20, n_items=2 ** 20 + 1, B=100), knobs(), 1),
              (shape(k=10), knobs(), 1), (shape(k=516), knobs(), 1), (shape(k=131, f64=1), knobs(), 1), (shape(k=258, f64=1), knobs(), 1),
              (shape(), knobs(general=1), 1)]

SPAN_KINDS = {"bpr": dict(), "not_cached": dict(fast=0), "any_k": dict(k=10)}
SPAN_TABLE = [(with_batches(ASY if kind == "asy" else BPR, nb, B=1 if kind == "asy" else 10, sharded=sharded, **SPAN_KINDS.get(kind, {})),
               knobs(whole_stream=whole), nb)
              for nb, sharded, whole, kind in itertools.product((1, 139, 256, 257, 20001), (0, 1), (0, 1), ("bpr", "asy", "not_cached", "any_k"))]

NP_TPB = (1, 3, 1023, 1024, 1025, 2048, 2049, 4096, 4097, 8190, 8192)
NP_TABLE = [(tpb, 4 * (2 * max(1024, 1 << (tpb - 1).bit_length()) + 1) + d) for tpb in NP_TPB for d in (-4, 0, 4, 4096)]
FAST_TABLE = [(shape(BPR, B=1), knobs(), 100), (shape(BPR, B=341), knobs(), 20000), (shape(BPR, B=342), knobs(), 100), (shape(BPR, B=2730), knobs(), 70000),
              (shape(FUNK, B=512), knobs(), 100), (shape(FUNK, B=513), knobs(), 100000), (shape(FUNK, B=4096), knobs(), 100),
              (shape(BPR, sharded=1), knobs(), 100), (shape(BPR), knobs(no_fuse=1), 100), (shape(FUNK), knobs(no_fuse=1), 100),
              (shape(BPR, k=32, fast=0), knobs(), 100), (shape(BPR, k=128), knobs(general=1), 100), (with_batches(BPR, 257), knobs(), 100),
              (shape(BPR, n_users=2 ** 20, n_items=2 ** 20, B=100), knobs(), 100), (shape(FUNK, n_users=200000, n_items=62144, B=4096), knobs(), 100)]

BIG = 2 ** 31 - 1
GENERAL_TABLE = [(shape(BPR, n_users=BIG, n_items=BIG), 2 ** 32), (shape(BPR, n_users=BIG, n_items=BIG), 2 ** 32 + 1),
                 (shape(FUNK, B=4096), 5), (shape(BPR, B=2731), 5), (shape(FUNK, B=4096, sharded=1), 5), (shape(BPR, B=2731, sharded=1), 5),
                 (shape(), 1), (shape(), 20001)]


def buffer_shape(algorithm, fast1, nb):
    return with_batches(algorithm, nb, B=1 if algorithm == ASY else 10, k=64 if fast1 else 10)


# shape, knobs, samples, mini-batches, whole_stream
BUFFER_TABLE = [(buffer_shape(a, fast1, nb), knobs(), nb * (1 if a == ASY else 10), nb, whole)
                for fast1, whole, nb, a in itertools.product((1, 0), (0, 1), (1, 256, 257, 20001), (BPR, FUNK, ASY))]
BUFFER_TABLE += [(buffer_shape(BPR, 1, 257), knobs(whole_stream=1), 2570, 257, 0), (buffer_shape(BPR, 1, 257), knobs(general=1), 2570, 257, 0),
                 (shape(FUNK, k=10, B=1024), knobs(), 2 ** 30 - 1, 2 ** 20, 0), (shape(FUNK, k=10, B=1024), knobs(), 2 ** 30, 2 ** 20, 0)]   # 2^31 incidences

SEGMENTS = [(f, min(20001, f + GRAPH_SEGMENT)) for f in range(0, 20001, GRAPH_SEGMENT)]
FUNK_20001 = with_batches(FUNK, 20001, B=1000)
REPLAY = shape(BPR, B=4)
# shape, knobs, samples, mini-batches, draw, first, last
WALK_TABLE = [(with_batches(BPR, 10, B=64), knobs(), 640, 10, 1, 0, 10), (with_batches(BPR, 10, B=64), knobs(), 640, 10, 0, 0, 10),
              (with_batches(BPR, 256), knobs(), 2560, 256, 1, 0, 256), (shape(k=10), knobs(), 100 * 300, 300, 0, 0, 300)]
WALK_TABLE += [(FUNK_20001, knobs(), 20001 * 1000, 20001, 0, f, l) for f, l in SEGMENTS]
WALK_TABLE += [(FUNK_20001, knobs(whole_stream=1), 20001 * 1000, 20001, 0, f, l) for f, l in SEGMENTS]
WALK_TABLE += [(REPLAY, knobs(), 257 * 4 + 1, 258, 0, 0, 258), (REPLAY, knobs(), 257 * 4 + 1, 258, 0, 256, 258), (REPLAY, knobs(), 257 * 4 + 1, 258, 0, 7, 7),
               (REPLAY, knobs(), 3, 1, 0, 0, 1)]

EPOCH_PER = (10, GRAPH_SEGMENT, GRAPH_SEGMENT + 1, MAX_GRAPH_BATCHES, MAX_GRAPH_BATCHES + 1)
EPOCH_TABLE = [(with_batches(BPR, per, B=1), knobs(no_graph=ng), mt, ne)
               for per in EPOCH_PER for ng in (0, 1) for mt in (0, 1, per, per + 1) for ne in (0, 1, 2)]
EPOCH_TABLE += [(with_batches(ASY, nb, B=1), knobs(), mt, ne) for nb in (10, ASY_CHUNK, ASY_CHUNK + 1) for mt in (0, 1) for ne in (0, 1, 2)]
GROUP_KNOBS = (knobs(), knobs(no_graph=1), knobs(no_lookahead=1), knobs(no_graph=1, no_lookahead=1))
# knobs, all_fast, mini-batches per epoch, max_timed, epochs
GROUP_TABLE = [(kn, af, nb, mt, ne) for kn in GROUP_KNOBS for af in (0, 1) for nb in (10, GRAPH_SEGMENT, GRAPH_SEGMENT + 1)
               for mt in (0, 1, nb, nb + 1) for ne in (0, 1, 2)]
GROUP_WGS_TABLE = (1, 3, 4, 5, 12, 13, 192, 3000, 8190, 8192)
M0 = shape(BPR, k=64, B=100)
MISMATCH_TABLE = [(M0, M0), (M0, shape(BPR, k=8, B=100)), (M0, shape(BPR, k=68, B=100)), (M0, shape(FUNK, k=64, B=150, nnz=1000)),
                  (M0, shape(BPR, k=32, f64=1, B=100)), (M0, shape(BPR, k=64, B=50)), (M0, shape(BPR, k=64, B=100, n_users=1100)),
                  (M0, shape(BPR, k=64, B=100, n_users=1099, n_items=7))]

# header slots, k, float64, rank, world
SHARD_TABLE = [(tpb, k, f64, rank, world) for tpb in (1, 4, 5, 3000) for k, f64 in ((64, 0), (20, 1)) for world in (1, 2, 3, 8) for rank in range(world)]
BYTES_TABLE = [shape(BPR, k=128), shape(FUNK, k=1), shape(ASY, k=256, B=1), shape(BPR, k=10, f64=1)]

ENV_TABLE = {
    "unset": {},
    "empty": {name: "" for name in ENV_NAMES},        # on as soon as the variable exists
    "zeros": {name: "0" for name in ENV_NAMES},       # ... whatever it holds
    "ones": {name: "1" for name in ENV_NAMES},
    "two_of_them": {ENV_NAMES[2]: "", ENV_NAMES[6]: "0"},
}


# ---- running them -------------------------------------------------------------------------------------------------------------
def declare(lib):
    lib.mf_fast_numbers.argtypes = [C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p]
    lib.mf_sched_np.argtypes = [C.c_int, C.c_uint64, C.c_void_p]
    lib.mf_schedule.argtypes = [C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p]
    lib.mf_general.argtypes = [C.c_void_p, C.c_int64, C.c_void_p]
    lib.mf_buffers.argtypes = [C.c_void_p, C.c_void_p, C.c_uint64, C.c_int64, C.c_int, C.c_void_p]
    lib.mf_walk.argtypes = [C.c_void_p, C.c_void_p, C.c_int64, C.c_int64, C.c_int, C.c_int64, C.c_int64, C.c_void_p]
    lib.mf_epoch.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int64, C.c_void_p]
    lib.mf_group_epoch.argtypes = [C.c_void_p, C.c_int, C.c_int64, C.c_int, C.c_int64, C.c_void_p]
    lib.mf_group_mismatch.argtypes = [C.c_void_p, C.c_void_p]
    lib.mf_shard.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p]
    lib.mf_width.argtypes = [C.c_int, C.c_int, C.c_void_p]
    lib.mf_widest_k.argtypes = [C.c_int]
    lib.mf_bytes_per_sample.argtypes = [C.c_void_p]
    lib.mf_bytes_per_sample.restype = C.c_double
    return lib


def call(fn, n_out, *args):
    out = np.zeros(n_out, np.int64)
    fn(*[ptr(arr(a)) if isinstance(a, tuple) else a for a in args], ptr(out))
    return out


def read_environment(lib, setting):
    """the knobs as the library parses them with exactly `setting` in the environment"""
    saved = {name: os.environ.get(name) for name in ENV_NAMES}
    try:
        for name in ENV_NAMES:
            os.environ.pop(name, None)
        os.environ.update(setting)
        k = np.zeros(7, np.int64)
        lib.mf_read_knobs(ptr(k))
        return k
    finally:
        for name, v in saved.items():
            os.environ.pop(name, None)
            if v is not None:
                os.environ[name] = v


def flat(table):
    """a table of (tuple | number, ...) rows as one int64 matrix"""
    return np.array([[x for col in row for x in (col if isinstance(col, tuple) else (col,))] for row in table], np.int64)


def record(lib):
    """name -> array, as the fixture holds them"""
    declare(lib)
    out = {}
    out["env/table"] = np.array(list(ENV_TABLE))
    out["env/knobs"] = np.array([read_environment(lib, ENV_TABLE[name]) for name in ENV_TABLE])
    out["constants/result"] = call(lib.mf_constants, 15)
    out["width/table"], out["width/result"] = flat(WIDTH_TABLE), np.array([call(lib.mf_width, 6, k, f64) for k, f64 in WIDTH_TABLE])
    out["fits/table"], out["fits/result"] = flat(FITS_TABLE), np.array([call(lib.mf_schedule, 4, s, kn, nb) for s, kn, nb in FITS_TABLE])
    out["span/table"], out["span/result"] = flat(SPAN_TABLE), np.array([call(lib.mf_schedule, 4, s, kn, nb) for s, kn, nb in SPAN_TABLE])
    out["np/table"], out["np/result"] = flat(NP_TABLE), np.array([call(lib.mf_sched_np, 3, tpb, st) for tpb, st in NP_TABLE])
    out["fast/table"], out["fast/result"] = flat(FAST_TABLE), np.array([call(lib.mf_fast_numbers, 11, s, kn, st) for s, kn, st in FAST_TABLE])
    out["general/table"], out["general/result"] = flat(GENERAL_TABLE), np.array([call(lib.mf_general, 4, s, nb) for s, nb in GENERAL_TABLE])
    out["buffers/table"], out["buffers/result"] = flat(BUFFER_TABLE), np.array([call(lib.mf_buffers, 17, *row) for row in BUFFER_TABLE])
    out["walk/table"] = flat(WALK_TABLE)
    for i, (s, kn, n, nb, draw, first, last) in enumerate(WALK_TABLE):
        steps = np.full((last - first, 6), -1, np.int64)
        lib.mf_walk(ptr(arr(s)), ptr(arr(kn)), n, nb, draw, first, last, ptr(steps))
        out["walk/steps_%02d" % i] = steps
    out["epoch/table"], out["epoch/result"] = flat(EPOCH_TABLE), np.array([call(lib.mf_epoch, 7, *row) for row in EPOCH_TABLE])
    out["group/table"], out["group/result"] = flat(GROUP_TABLE), np.array([call(lib.mf_group_epoch, 3, *row) for row in GROUP_TABLE])
    out["group/wgs_table"], out["group/wgs"] = arr(GROUP_WGS_TABLE), arr([lib.mf_group_workgroups(t) for t in GROUP_WGS_TABLE])
    out["group/mismatch_table"] = flat(MISMATCH_TABLE)
    out["group/mismatch"] = arr([lib.mf_group_mismatch(ptr(arr(a)), ptr(arr(b))) for a, b in MISMATCH_TABLE])
    out["shard/table"] = flat(SHARD_TABLE)
    out["shard/result"] = np.array([call(lib.mf_shard, 4, shape(k=k, f64=f64), tpb, rank, world) for tpb, k, f64, rank, world in SHARD_TABLE])
    out["bytes/table"], out["bytes/result"] = flat(BYTES_TABLE), np.array([lib.mf_bytes_per_sample(ptr(arr(s))) for s in BYTES_TABLE], np.float64)
    return out


FAMILIES = ("env", "constants", "width", "fits", "span", "np", "fast", "general", "buffers", "walk", "epoch", "group", "shard", "bytes")


@pytest.fixture(scope="module")
def build_dir(tmp_path_factory):
    return tmp_path_factory.mktemp("mf_plan")


@pytest.fixture(scope="module")
def shim(build_dir):
    so = build_dir / "mf_plan_shim.so"
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-shared", "-fPIC", os.path.join(HERE, "mf_plan_shim.cpp"), "-o", str(so)], check=True)
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
    # SCHED_THREADS, FAST_MAX_BATCHES, FAST_MAX_SLOTS, QTASK_SLOT_MASK, QTASK_OFF_SHIFT, QTASK_OFF_MAX, QTASK_PAIR, SCHED_STAMPS, META_WIDE,
    # SLOT_ABSORBED, MU_SLOTS, ASY_KMAX, ASY_CHUNK, GRAPH_SEGMENT, MAX_GRAPH_BATCHES
    assert recorded["constants/result"].tolist() == [1024, 256, 8192, 8191, 13, 31, 1 << 29, 8, 1 << 30, 0x3fffffff, 64, 256, 65536, 4096, 262144]


# ---- row width -> kernel instance ---------------------------------------------------------------------------------------------
def width_branch(k, f64):
    vec = 2 if f64 else 4
    if k % vec:
        return "any_k_ragged"
    for n, row in enumerate(ROW_WIDTHS):
        if k // vec <= row[0]:
            return n
    return "any_k_wide"


def test_row_width_table(recorded):
    seen = set()
    for (k, f64), (lpr, ki, in_flight, klass, group_lpr, group_ki) in zip(WIDTH_TABLE, recorded["width/result"].tolist()):
        branch = width_branch(k, f64)
        seen.add((branch, f64))
        if isinstance(branch, int):
            # the class number IS the position of the chosen row; both launches and the schedule's wavefront shape read that row
            assert klass == branch and (lpr, ki, in_flight) == ROW_WIDTHS[branch][1:] and (group_lpr, group_ki) == (lpr, ki), (k, f64)
        else:
            assert klass == -1 and (lpr, ki, in_flight, group_lpr, group_ki) == (0, 0, 1, 0, 0), (k, f64)
    assert seen == {(b, f64) for b in (0, 1, 2, 3, "any_k_ragged", "any_k_wide") for f64 in (0, 1)} - {("any_k_wide", 0)}    # (k <= 512: 128 chunks of float32)
    assert width_branch(512, 0) == 3 and width_branch(258, 1) == "any_k_wide"


def test_widest_row_named_by_the_group_message(shim):
    # 128 chunks of 16 bytes: the limit the group's rejection of an any-k model prints, per precision
    assert (shim.mf_widest_k(0), shim.mf_widest_k(1)) == (512, 256)
    assert all(width_branch(k, f64) == 3 and width_branch(k + vec, f64) == "any_k_wide" for k, f64, vec in ((512, 0, 4), (256, 1, 2)))


# ---- which schedule -------------------------------------------------------------------------------------------------------------
def fits_branch(s, kn, nb):
    if kn[0]:
        return "general_schedule_set"
    if nb > FAST_MAX_BATCHES:
        return "too_many_batches"
    if tpb_of(s) > FAST_MAX_SLOTS:
        return "batch_too_large"
    if bits_for(s[1] + s[2]) + bits_for(max(tpb_of(s), SCHED_THREADS)) > 31:
        return "row_ids_too_wide"
    return "fits" if isinstance(width_branch(s[4], s[5]), int) else "any_k"


def test_fast_schedule_fits(recorded):
    seen = []
    for (s, kn, nb), (_, fits, _, _) in zip(FITS_TABLE, recorded["fits/result"].tolist()):
        seen.append(fits_branch(s, kn, nb))
        assert fits == (seen[-1] == "fits"), (s, kn, nb)
    assert seen == ["fits", "too_many_batches", "fits", "batch_too_large", "fits", "batch_too_large", "fits", "row_ids_too_wide", "fits", "row_ids_too_wide",
                    "any_k", "any_k", "any_k", "any_k", "general_schedule_set"]


def span_branch(s, kn, nb):
    if s[7]:
        return "whole_sharded"
    if nb <= FAST_MAX_BATCHES:
        return "whole_fits"
    if fits_branch(s, kn, 1) != "fits":
        return "whole_no_fast_schedule"
    return "whole_by_switch" if kn[2] else "parts"


def draws_branch(s, kn):
    if s[0] == ASY:
        return "asy"
    if s[7]:
        return "sharded"
    if not s[8]:
        return "not_cached"
    return "draws" if fits_branch(s, kn, per_epoch_of(s)) == "fits" else "does_not_fit"


def test_schedule_span_and_draws(recorded):
    spans, draws = set(), set()
    for (s, kn, nb), (per_epoch, _, span, draw) in zip(SPAN_TABLE, recorded["span/result"].tolist()):
        assert per_epoch == nb == per_epoch_of(s), (s, nb)
        sb, db = span_branch(s, kn, nb), draws_branch(s, kn)
        spans.add(sb), draws.add(db)
        assert span == (FAST_MAX_BATCHES if sb == "parts" else nb), (s, kn, nb)
        assert draw == (db == "draws"), (s, kn, nb)
        assert not draw or span == nb
    assert spans == {"whole_sharded", "whole_fits", "whole_no_fast_schedule", "whole_by_switch", "parts"}
    assert draws == {"asy", "sharded", "not_cached", "draws", "does_not_fit"}


# ---- the in-LDS schedule's numbers ----------------------------------------------------------------------------------------------
def test_sort_workgroup_sizes(recorded):
    seen = set()
    for (tpb, storage), (np_, mid, lds) in zip(NP_TABLE, recorded["np/result"].tolist()):
        assert np_ >= max(tpb, SCHED_THREADS) and np_ & (np_ - 1) == 0 and (np_ == SCHED_THREADS or np_ < 2 * tpb), tpb
        tables = 4 * (2 * np_ + 1)
        seen.add(("sort_scratch" if storage > tables else "run_starts_and_slots", np_))
        assert mid == -(-max(tables, storage) // 16) * 16 and lds == 4 * np_ + mid + np_ + 16, (tpb, storage)
    assert seen == {(arm, n) for arm in ("sort_scratch", "run_starts_and_slots") for n in (1024, 2048, 4096, 8192)}
    assert lds <= 160 * 1024


def fuse_branch(s, kn):
    if s[0] != BPR:
        return "not_bpr"
    if s[7]:
        return "sharded"
    return "no_fuse_set" if kn[1] else "fuse"


def test_fast_schedule_numbers(recorded):
    fuses, strides, used = set(), set(), set()
    for (s, kn, storage), (np_, slot_bits, entry_bits, mid, words, group, fuse, fill_all, lds, stride, reads_used) in zip(FAST_TABLE, recorded["fast/result"].tolist()):
        tpb = tpb_of(s)
        assert np_ == max(SCHED_THREADS, 1 << (tpb - 1).bit_length()) and slot_bits == bits_for(np_), s
        assert entry_bits == min(32 - slot_bits, bits_for(s[1] + s[2]) + 1) and words == FAST_MAX_BATCHES // 32 and fill_all == 1, s
        assert mid == -(-max(4 * (2 * np_ + 1), storage) // 16) * 16 and lds == 5 * np_ + mid + 16, s
        branch = width_branch(s[4], s[5])
        assert group == (ROW_WIDTHS[branch][3] if isinstance(branch, int) else 1), s
        fuses.add(fuse_branch(s, kn))
        assert fuse == (fuse_branch(s, kn) == "fuse"), (s, kn)
        # the cached flag sizes the stride; the fresh decision (this call's knobs, the epoch's length) decides about `used`
        assert stride == (3 * tpb if s[8] else 0), s
        ub = "not_cached" if not s[8] else ("reads_used" if fits_branch(s, kn, per_epoch_of(s)) == "fits" else fits_branch(s, kn, per_epoch_of(s)))
        used.add(ub), strides.add(bool(stride))
        assert reads_used == (ub == "reads_used"), (s, kn)
    assert fuses == {"fuse", "not_bpr", "sharded", "no_fuse_set"} and strides == {True, False}
    assert used == {"reads_used", "not_cached", "general_schedule_set", "too_many_batches"}


# ---- header slots of the in-LDS schedule --------------------------------------------------------------------------------------
# (mf_plan.npz stays as it is: these two functions are compared with the restatement below)
SLOT_GROUPS = (1, 2, 4)         # samples in flight of the instances in ROW_WIDTHS


def is_wide(length, group):
    """a run is split over the 4 wavefronts of a workgroup when it is longer than two rounds of one wavefront -- and than 3"""
    return length > max(2 * group, 3)


def slots_of(length, group):
    return 4 if is_wide(length, group) else 1


def parent_slots_of(length, group):
    """the rule the sort kernel had before list_is_wide(): `len > 2 * group` alone"""
    return 4 if length > 2 * group else 1


def partitions(m, largest=None):
    """every multiset of run lengths that adds up to m, largest run first"""
    largest = m if largest is None else largest
    if m == 0:
        yield ()
        return
    for first in range(min(m, largest), 0, -1):
        for rest in partitions(m - first, first):
            yield (first,) + rest


def declare_slots(lib):
    lib.mf_list_is_wide.argtypes = lib.mf_header_slots.argtypes = [C.c_int, C.c_int]
    return lib


@pytest.mark.parametrize("group", SLOT_GROUPS)
def test_a_run_takes_no_more_header_slots_than_it_has_incidences(shim, group):
    """A mini-batch has one header slot (and its launch one wavefront) per incidence, and the sort kernel hands slots out without a
    bound of its own: 4 * wide runs + the others.  So no run may take more slots than it has incidences.  `len > 2 * group` alone
    breaks this at (group 1, len 3): 4 slots for 3 incidences."""
    declare_slots(shim)
    over = [(group, n, shim.mf_header_slots(n, group)) for n in range(1, 8193) if shim.mf_header_slots(n, group) > n]
    assert over == [], over
    assert all(shim.mf_header_slots(n, group) == slots_of(n, group) and shim.mf_list_is_wide(n, group) == is_wide(n, group) for n in range(1, 8193))


@pytest.mark.parametrize("group", SLOT_GROUPS)
def test_the_runs_of_a_mini_batch_fit_its_header_slots(shim, group):
    """what the kernel relies on: however m incidences fall into runs, the runs' slots add up to at most m"""
    declare_slots(shim)
    seen = 0
    for m in range(1, 25):
        slots = {n: shim.mf_header_slots(n, group) for n in range(1, m + 1)}
        for runs in partitions(m):
            seen += 1
            used = sum(slots[n] for n in runs)
            assert used <= m, (group, m, runs, used)
    assert seen == 7337            # the partition numbers p(1) + .. + p(24)


def test_the_wide_threshold_of_the_wider_instances_is_unchanged(shim):
    """groups 2 and 4 (rows of up to 32 chunks: the headline k = 128 in float32 among them) keep `len > 2 * group` exactly, so their
    schedules stay what they were bit for bit; group 1 differs from it at len 3 alone"""
    declare_slots(shim)
    for group in (2, 4):
        assert all(shim.mf_list_is_wide(n, group) == (n > 2 * group) and shim.mf_header_slots(n, group) == parent_slots_of(n, group) for n in range(1, 8193))
    assert [n for n in range(1, 8193) if shim.mf_header_slots(n, 1) != parent_slots_of(n, 1)] == [3]


def test_the_parents_rule_overran_a_full_mini_batch():
    """the restated parent rule on the same two properties: it fails the per-run bound at (1, 3) only, and e.g. FunkSVD's mini-batch of 3
    samples with one item in all of them (runs 3, 1, 1, 1: 6 incidences) needs 7 slots"""
    assert [(g, n) for g in SLOT_GROUPS for n in range(1, 8193) if parent_slots_of(n, g) > n] == [(1, 3)]
    assert sum(parent_slots_of(n, 1) for n in (3, 1, 1, 1)) == 7 and sum(slots_of(n, 1) for n in (3, 1, 1, 1)) == 4


def test_general_schedule_numbers(recorded):
    seen = set()
    for (s, nb), (batch_bits, end_bit, fits, by_rank) in zip(GENERAL_TABLE, recorded["general/result"].tolist()):
        assert batch_bits == bits_for(nb) and end_bit == batch_bits + bits_for(s[1] + s[2]) and fits == (end_bit <= 64), (s, nb)
        branch = "sharded" if s[7] else ("batch_too_large" if tpb_of(s) > FAST_MAX_SLOTS else "by_counter")
        seen.add((branch, end_bit if end_bit >= 64 else "short"))
        assert by_rank == (branch != "by_counter"), (s, nb)
    assert seen == {("by_counter", 64), ("by_counter", 65), ("by_counter", "short"), ("batch_too_large", "short"), ("sharded", "short")}
    assert [r[2] for r in recorded["general/result"].tolist()[:2]] == [1, 0]


# ---- buffers --------------------------------------------------------------------------------------------------------------------
def buffer_branch(s, kn, nb, whole):
    if s[0] == ASY:
        return "asy"
    if fits_branch(s, kn, 1) != "fits":
        return "no_fast_schedule"
    if (whole or kn[2]) and fits_branch(s, kn, nb) != "fits":
        return "whole_stream_too_long"
    return "fast_in_parts" if nb > FAST_MAX_BATCHES else "fast"


def test_buffer_plan(recorded):
    seen, limits = set(), []
    for (s, kn, n, nb, whole), r in zip(BUFFER_TABLE, recorded["buffers/result"].tolist()):
        asy, fast1, general, incidences, inc_fit, table_batches, tasks, recs, batch_count, slot_recs, sorted_slot, qtask, used, touched, loss, ticks, sched_ticks = r
        case = (s, kn, n, nb, whole)
        branch = buffer_branch(s, kn, nb, whole)
        seen.add(branch)
        tpb = tpb_of(s)
        assert (loss, ticks, sched_ticks) == (4 * tpb, 8 * tpb, FAST_MAX_BATCHES * SCHED_STAMPS), case
        if branch == "asy":
            assert r[:14] == [1, 0, 0, 0, 1] + [0] * 9, case
            continue
        assert asy == 0 and fast1 == (branch != "no_fast_schedule") and general == (branch in ("no_fast_schedule", "whole_stream_too_long")), case
        assert (incidences, inc_fit) == ((n * per_sample(s), n * per_sample(s) < 2 ** 31) if general else (0, 1)), case
        if general and incidences >= 2 ** 31 - 2:
            limits.append(inc_fit)
        assert table_batches == (nb if general else min(nb, FAST_MAX_BATCHES)) == batch_count, case
        assert tasks == (table_batches + 1) * tpb and recs == table_batches * tpb, case
        assert slot_recs == 3 * tpb * (table_batches if fast1 else 1), case
        want = (table_batches * tpb, table_batches * tpb, table_batches, (s[1] + s[2]) * 8) if fast1 else (0, 0, 0, 0)
        assert (sorted_slot, qtask, used, touched) == want, case
    assert seen == {"asy", "no_fast_schedule", "whole_stream_too_long", "fast_in_parts", "fast"}
    assert limits == [1, 0]


# ---- the walk over a stream -------------------------------------------------------------------------------------------------------
def test_stream_walk(recorded):
    kinds, scheduled_in = set(), {}
    for i, (s, kn, n, nb, draw, first, last) in enumerate(WALK_TABLE):
        steps = recorded["walk/steps_%02d" % i].tolist()
        case = (i, s, kn, n, nb, draw, first, last)
        assert len(steps) == last - first, case
        B = s[6]
        span = FAST_MAX_BATCHES if span_branch(s, kn, nb) == "parts" else nb
        for b, (local, sched, offset, samples, batches, end) in zip(range(first, last), steps):
            part = b // span * span
            part_batches = min(span, nb - part)
            assert local == b - part and end == (part_batches if local + 1 == part_batches else 0), (case, b)
            if local:
                assert (sched, offset, samples, batches) == (0, 0, 0, 0), (case, b)
                continue
            kind = "draw" if draw else ("whole" if span == nb else "part")
            kinds.add(kind)
            scheduled_in.setdefault((s, kn, kind), []).append((first, last))
            assert sched == {"draw": 1, "whole": 2, "part": 3}[kind], (case, b)
            want = (part * B, min(n - part * B, part_batches * B), part_batches) if kind == "part" else (0, n, nb)
            assert (offset, samples, batches) == want, (case, b)
            assert offset + samples <= n and (batches - 1) * B < samples <= batches * B, (case, b)
    assert kinds == {"draw", "whole", "part"}
    # 20 001 mini-batches in graph segments: a schedule per 256 in every segment | one schedule, in the first segment only
    assert len(scheduled_in[(FUNK_20001, knobs(), "part")]) == -(-20001 // 256) and {r for r in scheduled_in[(FUNK_20001, knobs(), "part")]} == set(SEGMENTS)
    assert scheduled_in[(FUNK_20001, knobs(whole_stream=1), "whole")] == [SEGMENTS[0]]
    # the replayed stream's last part is short: 2 mini-batches, 5 samples
    assert recorded["walk/steps_%02d" % (len(WALK_TABLE) - 3)].tolist() == [[0, 3, 1024, 5, 2, 0], [1, 0, 0, 0, 0, 2]]
    assert recorded["walk/steps_%02d" % (len(WALK_TABLE) - 2)].shape == (0, 6)


# ---- epoch calls ------------------------------------------------------------------------------------------------------------------
def graph_branch(asy, no_graph, per, n_epochs, timed):
    if per > MAX_GRAPH_BATCHES:
        return "epoch_too_long"
    if n_epochs - timed <= 0:
        return "every_epoch_timed"
    if no_graph:
        return "no_graph_set"
    return "asy" if asy else "graph"


def test_epoch_decisions(recorded):
    seen, timed_seen = set(), set()
    for (s, kn, max_timed, n_epochs), (per, timed, graph, segments, seg_first, seg_last, launches) in zip(EPOCH_TABLE, recorded["epoch/result"].tolist()):
        case = (s, kn, max_timed, n_epochs)
        asy = s[0] == ASY
        assert per == per_epoch_of(s), case
        want_timed = min(n_epochs, -(-max_timed // per)) if max_timed > 0 else 0
        timed_seen.add(("none" if max_timed == 0 else ("one_epoch" if -(-max_timed // per) == 1 else "two_epochs"), want_timed))
        assert timed == want_timed, case
        branch = graph_branch(asy, kn[6], per, n_epochs, timed)
        seen.add(branch)
        assert graph == (branch == "graph"), case
        nb = 1 if asy else per
        assert segments == -(-nb // GRAPH_SEGMENT) and seg_first == (segments - 1) * GRAPH_SEGMENT and seg_last == nb, case
        assert launches == (n_epochs * -(-per // ASY_CHUNK) if asy else per * n_epochs), case
    assert seen == {"epoch_too_long", "every_epoch_timed", "no_graph_set", "asy", "graph"}
    assert timed_seen >= {("none", 0), ("one_epoch", 0), ("one_epoch", 1), ("two_epochs", 0), ("two_epochs", 1), ("two_epochs", 2)}


def test_group_decisions(recorded):
    seen = set()
    for (kn, all_fast, nb, max_timed, n_epochs), (timed, ahead, graph) in zip(GROUP_TABLE, recorded["group/result"].tolist()):
        case = (kn, all_fast, nb, max_timed, n_epochs)
        assert timed == (min(n_epochs, -(-max_timed // nb)) if max_timed > 0 else 0), case
        ab = "per_member" if not all_fast else ("one_epoch" if n_epochs <= 1 else ("no_lookahead_set" if kn[5] else "ahead"))
        gb = "ahead" if ab == "ahead" else ("epoch_too_long" if nb > GRAPH_SEGMENT else ("every_epoch_timed" if n_epochs - timed <= 0 else
                                                                                         ("no_graph_set" if kn[6] else "graph")))
        seen.add((ab, gb))
        assert ahead == (ab == "ahead") and graph == (gb == "graph"), case
    assert {a for a, _ in seen} == {"per_member", "one_epoch", "no_lookahead_set", "ahead"}
    assert {g for _, g in seen} == {"ahead", "epoch_too_long", "every_epoch_timed", "no_graph_set", "graph"}
    assert recorded["group/wgs"].tolist() == [-(--(-t // 4) // 3) for t in GROUP_WGS_TABLE]
    assert recorded["group/mismatch"].tolist() == [0, 0, 1, 1, 1, 2, 2, 0]


def test_shard_numbers(recorded):
    seen = set()
    total = {}
    for (tpb, k, f64, rank, world), (wgs, slots, mine, nbytes) in zip(SHARD_TABLE, recorded["shard/result"].tolist()):
        case = (tpb, k, f64, rank, world)
        assert wgs == -(-tpb // 4) and slots == -(-wgs // world) * 4 and nbytes == slots * k * (8 if f64 else 4), case
        seen.add("no_workgroup" if wgs <= rank else "workgroups")
        assert mine == len(range(rank, wgs, world)) and 4 * mine <= slots, case          # w % world == rank; its slots fit the slab
        total[(tpb, k, world)] = total.get((tpb, k, world), 0) + mine
    assert seen == {"no_workgroup", "workgroups"}
    assert all(n == -(-tpb // 4) for (tpb, _, _), n in total.items())


def test_accounting(recorded):
    assert recorded["bytes/result"].tolist() == [(3.0 if s[0] == BPR else 2.0) * 8.0 * s[4] for s in BYTES_TABLE]


# ---- the environment ------------------------------------------------------------------------------------------------------------
def test_knob_parsing(recorded):
    knobs_of = dict(zip(ENV_TABLE, recorded["env/knobs"].tolist()))
    assert knobs_of["unset"] == [0] * 7
    assert knobs_of["empty"] == knobs_of["zeros"] == knobs_of["ones"] == [1] * 7         # an empty string and "0" both read as ON
    assert knobs_of["two_of_them"] == [0, 0, 1, 0, 0, 0, 1]


# ---- the same tables under the sanitizers -----------------------------------------------------------------------------------------
def test_plan_program_under_address_and_undefined_behaviour_sanitizers(build_dir):
    exe = build_dir / "mf_plan_main"
    # (the sanitizers' runtimes are linked into the program, so that it does not depend on the order the loader finds libraries in)
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer",
                    "-static-libasan", "-static-libubsan", os.path.join(HERE, "mf_plan_main.cpp"), "-o", str(exe)], check=True)
    env = {k: v for k, v in os.environ.items() if k not in ENV_NAMES}
    done = subprocess.run([str(exe)], env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert done.returncode == 0, done.stdout[-4000:]
    assert "mf_plan_main: OK" in done.stdout
