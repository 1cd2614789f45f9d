"""The streams of tests/mf_stream_cases.py replayed on the device and through the CPU oracle: every kernel instance of the mini-batch
kernel at the row widths on both sides of its class boundary, both algorithms, the in-LDS and the radix-sort schedule, one task per
row (MI355REC_MF_NO_FUSE) for the streams that fill every header slot, the per-row bitmap (MI355REC_MF_ROW_BITMAP) for the stream of
300 mini-batches.  What each stream reaches is asserted on the CPU in tests/test_mf_stream_cases_spec.py.

Bar: test_mf_gpu.assert_factor_parity, element-wise |dev - ref| <= 1e-5 |ref| + 1e-6 max|ref|, on U, V and the biases.
"""
import functools

import numpy as np
import pytest
import scipy.sparse as sps

import mf_stream_cases as S
from oracle import oracle as O
from recsys2019_deeplearning_evaluation_amd import MatrixFactorization_MI355X_Epoch
from test_mf_gpu import assert_factor_parity
from test_mf_plan import ROW_WIDTHS

pytestmark = pytest.mark.gpu

# (sgd_mode, k): plain sgd keeps float32 state (16-byte chunks of 4 factors), adam float64 (chunks of 2).  Rows of up to 16 | 32 | 64 |
# 128 chunks are the four instances; a row that is no whole number of chunks runs on the any-k kernel.
INSTANCES = [("sgd", k) for k in (64, 68, 128, 132, 260, 6)] + [("adam", k) for k in (32, 34, 66, 130, 3)]
SCHEDULES = {"in_lds": None, "radix_sort": "MI355REC_MF_GENERAL_SCHEDULE"}


def group_of(mode, k):
    """samples a wavefront works on at a time: mf_plan.h's table (row_width), restated"""
    vec = 4 if mode == "sgd" else 2
    if k % vec:
        return 1
    return next((row[3] for row in ROW_WIDTHS if k // vec <= row[0]), 1)


def test_the_instances_sit_on_both_sides_of_every_class_boundary():
    assert [group_of(m, k) for m, k in INSTANCES] == [4, 2, 2, 1, 1, 1, 4, 2, 1, 1, 1]
    chunks = [k // (4 if m == "sgd" else 2) for m, k in INSTANCES]
    assert chunks == [16, 17, 32, 33, 65, 1, 16, 17, 33, 65, 1]


def urm(shape):
    X = sps.random(*shape, density=0.2, format="csr", random_state=3, dtype=np.float64)
    X.data[:] = 1.0 + np.floor(X.data * 5.0).clip(0, 4)
    return X


def settings(case, algorithm, mode, k, B):
    return dict(n_factors=k, algorithm_name=algorithm, batch_size=B, random_seed=9, sgd_mode=mode, learning_rate=0.05,
                user_reg=0.002, item_reg=0.003, positive_reg=0.003, negative_reg=0.004, bias_reg=0.005,
                use_bias=algorithm == "FUNK_SVD" and case in S.FUNK_WITH_BIAS)


@functools.lru_cache(maxsize=None)
def reference(case, algorithm, shape, mode, k):
    """the stream, the initial factors and where the oracle lands: computed once, shared by every schedule, read-only"""
    u, i, third, B = S.build(case, *shape, group_of(mode, k), algorithm)
    kw = settings(case, algorithm, mode, k, B)
    orc = O.OracleMF(urm(shape), **kw)
    U0, V0 = orc.initial_USER_factors.copy(), orc.initial_ITEM_factors.copy()
    orc.replay(u, i, j=third) if algorithm == "MF_BPR" else orc.replay(u, i, rating=third)
    out = dict(u=u, i=i, third=third, U0=U0, V0=V0, U=orc.get_USER_factors(), V=orc.get_ITEM_factors(), bu=orc.get_USER_bias(),
               bi=orc.get_ITEM_bias(), mu=np.array(float(orc.get_GLOBAL_bias())))
    for a in out.values():
        a.setflags(write=False)
    return kw, out


def replay_and_compare(case, algorithm, mode, k):
    for shape in S.SHAPES:
        kw, ref = reference(case, algorithm, shape, mode, k)
        dev = MatrixFactorization_MI355X_Epoch(urm(shape), initial_USER_factors=ref["U0"], initial_ITEM_factors=ref["V0"], **kw)
        try:
            if algorithm == "MF_BPR":
                dev.replay_samples(ref["u"], ref["i"], neg_item=ref["third"])
            else:
                dev.replay_samples(ref["u"], ref["i"], rating=ref["third"])
            what = "%s %s %dx%d " % (case, algorithm, *shape)
            assert_factor_parity(dev.get_USER_factors(), ref["U"], mode, what + "U")
            assert_factor_parity(dev.get_ITEM_factors(), ref["V"], mode, what + "V")
            if kw["use_bias"]:
                assert_factor_parity(dev.get_USER_bias(), ref["bu"], mode, what + "bu")
                assert_factor_parity(dev.get_ITEM_bias(), ref["bi"], mode, what + "bi")
                mu = float(ref["mu"])
                assert abs(float(dev.get_GLOBAL_bias()) - mu) < 1e-4 * max(1e-3, abs(mu)), what + "mu"
            assert dev.stats()["n_units"] == len(ref["u"])
        finally:
            dev.close()


CASES = [(algorithm, case) for algorithm in S.ALGORITHMS for case in S.cases_of(algorithm)]


@pytest.mark.parametrize("schedule", list(SCHEDULES))
@pytest.mark.parametrize("mode,k", INSTANCES)
@pytest.mark.parametrize("algorithm,case", CASES)
def test_stream_case_parity(gpu, monkeypatch, algorithm, case, mode, k, schedule):
    if SCHEDULES[schedule]:
        monkeypatch.setenv(SCHEDULES[schedule], "1")
    replay_and_compare(case, algorithm, mode, k)


@pytest.mark.parametrize("mode,k", INSTANCES)
@pytest.mark.parametrize("case", ["all_threes", "one_three_rest_single"])
def test_full_mini_batches_with_one_task_per_row(gpu, monkeypatch, case, mode, k):
    """without fused sample tasks BPR has no absorbed rows: every run takes a header of its own"""
    monkeypatch.setenv("MI355REC_MF_NO_FUSE", "1")
    replay_and_compare(case, "MF_BPR", mode, k)


@pytest.mark.parametrize("mode,k", INSTANCES)
@pytest.mark.parametrize("algorithm", S.ALGORITHMS)
def test_schedule_parts_on_the_per_row_bitmap(gpu, monkeypatch, algorithm, mode, k):
    monkeypatch.setenv("MI355REC_MF_ROW_BITMAP", "1")
    replay_and_compare("every_batch", algorithm, mode, k)


# ---- ids outside the model ------------------------------------------------------------------------------------------------------
def bad_id_cases(algorithm, n_users, n_items):
    arrays = [("user", n_users), ("item", n_items)] + ([("neg_item", n_items)] if algorithm == "MF_BPR" else [])
    return [(name, value) for name, limit in arrays for value in (-1, limit)]


@pytest.mark.parametrize("algorithm", ["MF_BPR", "FUNK_SVD", "ASY_SVD"])
def test_ids_outside_the_model_are_refused_and_the_handle_lives_on(gpu, algorithm):
    shape = S.SHAPES[0]
    n_users, n_items = shape
    asy = algorithm == "ASY_SVD"
    case, mode, k = "partial_tail", "sgd", 64
    if asy:
        kw = dict(n_factors=8, algorithm_name=algorithm, batch_size=1, random_seed=9, learning_rate=0.005)
        dev = MatrixFactorization_MI355X_Epoch(urm(shape), **kw)
        u, i, third = np.array([3, 5], np.int32), np.array([2, 7], np.int32), np.array([4.0, 0.0])
    else:
        kw, ref = reference(case, algorithm, shape, mode, k)
        dev = MatrixFactorization_MI355X_Epoch(urm(shape), initial_USER_factors=ref["U0"], initial_ITEM_factors=ref["V0"], **kw)
        u, i, third = ref["u"], ref["i"], ref["third"]
    try:
        before = dev.get_USER_factors().copy()
        for name, value in bad_id_cases(algorithm, n_users, n_items):
            for at in (0, len(u) - 1):
                args = dict(user=u.copy(), item=i.copy(), **({"neg_item": third.copy()} if algorithm == "MF_BPR" else {"rating": third.copy()}))
                args[name][at] = value
                with pytest.raises(ValueError, match="out of range"):
                    dev.replay_samples(**args)
        np.testing.assert_array_equal(dev.get_USER_factors(), before)        # nothing ran
        if asy:
            dev.replay_samples(u, i, rating=third)
            assert np.isfinite(dev.get_USER_factors()).all() and dev.stats()["n_units"] == 2
        else:
            dev.replay_samples(u, i, neg_item=third) if algorithm == "MF_BPR" else dev.replay_samples(u, i, rating=third)
            assert_factor_parity(dev.get_USER_factors(), ref["U"], mode, "U")
            assert_factor_parity(dev.get_ITEM_factors(), ref["V"], mode, "V")
            if kw["use_bias"]:
                assert_factor_parity(dev.get_USER_bias(), ref["bu"], mode, "bu")
                assert_factor_parity(dev.get_ITEM_bias(), ref["bi"], mode, "bi")
    finally:
        dev.close()
