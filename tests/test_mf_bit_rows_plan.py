"""The bit rows of the in-LDS MF schedule (csrc/mf_plan.h) on the CPU: the words of a mini-batch's bit row, whether the row fits the
sort kernel's LDS, the element count of the bit-row buffer, the switch MI355REC_MF_ROW_BITMAP, and the column pass that turns touch
bits into version parities -- the same functions the parity kernel runs, a wavefront per part of the stream's mini-batches.

A shim (tests/mf_bit_rows_shim.cpp) is compiled with g++ and called through ctypes.  The expected numbers are worked out here from the
layout alone: a row is ceil(n / 32) words rounded up to 4; the sort kernel's LDS is keys (4 np), the middle (the larger of 2 np + 1
words and the block sort's scratch, rounded up to 16), one flag byte per key, 16 spare bytes, the bit row; the parity in front of
mini-batch b is the start parity plus the number of earlier mini-batches that touch the row, modulo 2.
"""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
BPR, FUNK = 0, 1
FAST_MAX_BATCHES = 256
KNOB = "MI355REC_MF_ROW_BITMAP"


def ptr(a):
    return a.ctypes.data_as(C.c_void_p)


def shape(algorithm=BPR, n_users=1000, n_items=500, nnz=50000, k=64, f64=0, B=100, sharded=0, fast=1, bit_rows=1):
    return np.array((algorithm, n_users, n_items, nnz, k, f64, B, sharded, fast, bit_rows), np.int64)


@pytest.fixture(scope="module")
def lib(tmp_path_factory):
    so = tmp_path_factory.mktemp("mf_bit_rows") / "mf_bit_rows_shim.so"
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-shared", "-fPIC", os.path.join(HERE, "mf_bit_rows_shim.cpp"), "-o", str(so)], check=True)
    lib = C.CDLL(str(so))
    lib.br_row_words.restype = C.c_int
    lib.br_row_words.argtypes = [C.c_int64]
    lib.br_read_knob.restype = C.c_int
    lib.br_fast_fits.restype = C.c_int
    lib.br_fast_fits.argtypes = [C.c_void_p, C.c_int64]
    lib.br_fit.argtypes = [C.c_void_p, C.c_int, C.c_uint64, C.c_uint64, C.c_uint64, C.c_void_p]
    lib.br_numbers.argtypes = [C.c_void_p, C.c_uint64, C.c_void_p]
    lib.br_buffers.argtypes = [C.c_void_p, C.c_uint64, C.c_int64, C.c_int, C.c_void_p]
    lib.br_parity_constants.argtypes = [C.c_void_p]
    lib.br_parity_pass.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_int64]
    return lib


def row_words(n):
    return -(-(-(-n // 32)) // 4) * 4


@pytest.mark.parametrize("n_entries, want", [(1, 4), (31, 4), (32, 4), (33, 4), (127, 4), (128, 4), (129, 8), (165237, 5164), (497959, 15564)])
def test_row_words(lib, n_entries, want):
    assert row_words(n_entries) == want                         # (the model of this file and the figures agree)
    got = lib.br_row_words(n_entries)
    assert got == want
    assert got % 4 == 0 and 32 * got >= n_entries and 32 * (got - 4) < n_entries


def lds_model(np_keys, sort_storage, n_entries):
    middle = max(4 * (2 * np_keys + 1), sort_storage)
    middle = (middle + 15) // 16 * 16
    plain = 4 * np_keys + middle + np_keys + 16
    return plain, plain + 4 * row_words(n_entries)


# (B, algorithm) -> keys a workgroup sorts: 1 024 (3 x 100 slots), 4 096 (3 x 1 000: the ML-20M headline), 8 192 (2 x 4 096)
@pytest.mark.parametrize("algorithm, B, np_keys", [(BPR, 100, 1024), (BPR, 1000, 4096), (FUNK, 4096, 8192)])
@pytest.mark.parametrize("sort_storage", [0, 40000, 70000])          # below and above the 2 np + 1 words of every size but the last
@pytest.mark.parametrize("n_users, n_items", [(138493, 26744), (20, 13), (600000, 250001)])
def test_fit_at_the_limit(lib, algorithm, B, np_keys, sort_storage, n_users, n_items):
    s = shape(algorithm, n_users=n_users, n_items=n_items, B=B)
    static = 132
    plain, with_row = lds_model(np_keys, sort_storage, n_users + n_items)
    assert with_row % 16 == 0 and plain % 16 == 0
    for delta, want in ((-1, 0), (0, 1), (1, 1)):
        out = np.zeros(4, np.int64)
        lib.br_fit(ptr(s), 0, sort_storage, static, with_row + static + delta, ptr(out))
        assert out.tolist() == [np_keys, plain, with_row, want], (delta, out)
        lib.br_fit(ptr(s), 1, sort_storage, static, with_row + static + delta, ptr(out))        # the switch forces the per-row bitmap
        assert out.tolist() == [np_keys, plain, with_row, 0]


def test_fit_at_the_device_limit_of_160_kib(lib):
    """The headline shape fits with room to spare; at 4 096 keys about 850 k rows are the end, fewer at 8 192."""
    limit, static, out = 160 * 1024, 132, np.zeros(4, np.int64)

    def fits(algorithm, B, rows):
        lib.br_fit(ptr(shape(algorithm, n_users=rows - 10, n_items=10, B=B)), 0, 0, static, limit, ptr(out))
        return int(out[3])
    assert fits(BPR, 1000, 165237) == 1
    plain_4096, plain_8192 = lds_model(4096, 0, 1)[0], lds_model(8192, 0, 1)[0]
    last_4096 = (limit - static - plain_4096) // 16 * 128           # bits of the whole 16-byte groups that are left
    last_8192 = (limit - static - plain_8192) // 16 * 128
    assert 800000 < last_4096 < 900000 and last_8192 < last_4096
    assert fits(BPR, 1000, last_4096) == 1 and fits(BPR, 1000, last_4096 + 1) == 0
    assert fits(FUNK, 4096, last_8192) == 1 and fits(FUNK, 4096, last_8192 + 1) == 0
    # the fallback shapes of the device tests (tests/test_mf_bit_rows_gpu.py): the first has no bit row and, its keys needing 21 + 13
    # bits, no in-LDS schedule either; the second is on the in-LDS schedule with a row that does not fit beside 1 024 keys
    assert fits(BPR, 2000, 1200010) == 0
    assert lib.br_fast_fits(ptr(shape(BPR, n_users=1200000, n_items=10, B=2000)), 1) == 0
    assert fits(FUNK, 500, 1250010) == 0
    assert lib.br_fast_fits(ptr(shape(FUNK, n_users=1250000, n_items=10, B=500)), 41) == 1
    assert fits(FUNK, 500, 1200010) == 1                             # (1 024 keys leave room for 1.2 M rows)


def test_numbers_and_buffers(lib):
    for n_users, n_items in ((138493, 26744), (5, 3), (31, 33)):
        n = n_users + n_items
        for bit_rows in (0, 1):
            s = shape(BPR, n_users=n_users, n_items=n_items, B=1000, bit_rows=bit_rows)
            out = np.zeros(6, np.int64)
            lib.br_numbers(ptr(s), 0, ptr(out))
            assert out.tolist() == [8, row_words(n), bit_rows, 8, 0, 0]                          # (`words` keeps its value: 256 / 32)
            # whole epochs, a long stream in parts, the radix-sort schedule's whole stream (its short replays still run in LDS)
            for n_batches, whole, table in ((139, 0, 139), (1, 0, 1), (256, 0, 256), (20001, 0, 256), (20001, 1, 20001)):
                lib.br_buffers(ptr(s), n_batches * 1000, n_batches, whole, ptr(out))
                touched = n * (FAST_MAX_BATCHES // 32)
                want_rows = min(table, FAST_MAX_BATCHES) * row_words(n)
                assert out.tolist() == [1, table, 0 if bit_rows else touched, want_rows if bit_rows else 0, touched, 0], (n_batches, whole, out)
    # no in-LDS schedule for this handle: neither buffer
    s = shape(BPR, B=2731)
    out = np.zeros(6, np.int64)
    lib.br_buffers(ptr(s), 2731 * 5, 5, 0, ptr(out))
    assert out.tolist() == [0, 5, 0, 0, 0, 0]


def test_knob(lib):
    saved = os.environ.pop(KNOB, None)
    try:
        assert lib.br_read_knob() == 0
        os.environ[KNOB] = ""                                    # on as soon as it exists, like every MI355REC_MF_* switch
        assert lib.br_read_knob() == 1
        os.environ[KNOB] = "0"
        assert lib.br_read_knob() == 1
        del os.environ[KNOB]
        assert lib.br_read_knob() == 0
    finally:
        if saved is not None:
            os.environ[KNOB] = saved


def test_parts_cover_every_stream(lib):
    out = np.zeros(3, np.int64)
    lib.br_parity_constants(ptr(out))
    parts, part_max, max_batches = out.tolist()
    assert max_batches == FAST_MAX_BATCHES and parts * part_max >= max_batches


def pack_rows(T, words):
    """T[n_batches][n_entries] of 0 / 1 -> [n_batches][words] uint32, bit x & 31 of word x >> 5"""
    nb, n = T.shape
    padded = np.zeros((nb, words * 32), np.uint8)
    padded[:, :n] = T
    return np.ascontiguousarray(np.packbits(padded, axis=1, bitorder="little")).view("<u4").reshape(nb, words).copy()


@pytest.mark.parametrize("n_batches", [1, 2, 139, 256])
@pytest.mark.parametrize("n_entries", [1, 32, 70, 165, 1000])          # a partial last word (1, 70, 165, 1000), whole words (32), padding words (all)
@pytest.mark.parametrize("start", ["zeros", "ones", "random"])
def test_column_pass_is_a_cumulative_xor(lib, n_batches, n_entries, start):
    rng = np.random.default_rng(1000 * n_batches + n_entries)
    T = (rng.random((n_batches, n_entries)) < 0.3).astype(np.uint8)
    T[:, 0::7] = 0                                               # rows no mini-batch touches
    T[:, 3::7] = 1                                               # rows every mini-batch touches: the parity flips every time
    par = {"zeros": np.zeros(n_entries, np.uint8), "ones": np.ones(n_entries, np.uint8),
           "random": rng.integers(0, 2, n_entries).astype(np.uint8)}[start]
    words = row_words(n_entries)
    before = np.zeros((n_batches, n_entries), np.int64)           # touches in front of every mini-batch
    before[1:] = np.cumsum(T, axis=0, dtype=np.int64)[:-1]
    want_rows = pack_rows(((par[None, :] + before) & 1).astype(np.uint8), words)
    want_par = ((par + T.sum(axis=0, dtype=np.int64)) & 1).astype(np.uint8)

    rows = pack_rows(T, words)
    guard = np.full(n_entries + 64, 0xAB, np.uint8)                # par[] with a fence behind it: the partial word writes no further
    guard[:n_entries] = par
    lib.br_parity_pass(ptr(rows), words, n_batches, ptr(guard), n_entries)
    np.testing.assert_array_equal(rows, want_rows)
    np.testing.assert_array_equal(guard[:n_entries], want_par)
    assert (guard[n_entries:] == 0xAB).all()
    assert (rows[:, -(-n_entries // 32):] == 0).all()             # padding words stay empty
