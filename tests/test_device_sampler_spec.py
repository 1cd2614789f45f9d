"""What the device sample stream SHOULD be: the host model of it (oracle/device_sampler.py, a NumPy restatement of sampling.cuh and
mf_draw_sample) against the sampling RULE of sampleBPR_Cython / sampleMSE_Cython -- users uniform over those with a positive and a
negative item, the positive uniform over the profile, the negative uniform outside it, samples independent of each other, of the
epoch and of the seed.  test_device_sampler_gpu.py then pins the device to this model with exact equality.

Statistics (sampler_cases.sampler_statistics), N = 10^6 samples per seed on a 400 x 60 matrix whose smallest expected cell count
is 41.0: z = (chi2 - df) / sqrt(2 df) of the users, of the positive given the user and of the negative given the user, and
sqrt(N) * correlation of positive against negative quantile and of consecutive users.  Every figure is about standard normal
under the rule, the bound is 5 BOTH ways (a stream that is too regular is wrong as well; each fails with probability below 1e-6
under the rule) and the seeds are fixed, so the outcome is deterministic.  Measured with the committed model
(profiles/sampler_statistics.json): largest |z| 2.67 (z_neg, seed 2^31 - 1), largest |sqrt(N) corr| 2.24 (c_pos_neg, seed 2^32 + 5).
The two planted faults below are kept as tests that must FAIL the bounds: z_pos 5.3 .. 7.8 with 5 % of the last-entry picks
moved to the first entry, c_pos_neg 701 .. 702 with the negative's first attempt reusing the positive's draw.
"""
import json
import os

import numpy as np
import pytest

from oracle import device_sampler as DS
from oracle import oracle as O
import sampler_cases as SC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N = SC.N_STAT
_STREAMS = {}


def _stream(seed, first_sid=0):
    """(u, i, j, draws_used) of sample ids first_sid .. first_sid + N - 1 on the small matrix: drawn once, never modified."""
    key = (seed, first_sid)
    if key not in _STREAMS:
        out = DS.bpr_sample(SC.profiles(SC.small_urm()), seed, np.arange(first_sid, first_sid + N, dtype=np.uint64))
        for a in out:
            a.setflags(write=False)
        _STREAMS[key] = out
    return _STREAMS[key]


def _statistics(seed):
    key = ("statistics", seed)
    if key not in _STREAMS:
        _STREAMS[key] = SC.sampler_statistics(SC.small_urm(), *_stream(seed)[:3])
    return _STREAMS[key]


def _outside(figures):
    return {name: v for name, v in figures.items() if not abs(v) <= SC.BOUND}


# ---- anchors --------------------------------------------------------------------------------------------------------------------
def test_mix64_is_splitmix64():
    """The published first outputs of SplitMix64 from state 0 (Vigna's splitmix64.c; java.util.SplittableRandom): an anchor
    independent of this code base.  Output n + 1 is the mix of the state after n increments."""
    assert int(DS.mix64(0)[0]) == 0xE220A8397B1DCDAF
    assert int(DS.mix64(0x9E3779B97F4A7C15)[0]) == 0x6E789E6AA1B965F4
    assert int(DS.mix64(2 ** 64 - 1)[0]) == int(DS.mix64(-1)[0])                      # wrap-around, not overflow


def test_draw32_regression_anchor():
    """From a scratch restatement of sampling.cuh: these anchor ONLY against a regression of the model (the device is pinned to the
    model by the GPU tests; nothing outside this code base says what draw32 should be)."""
    assert [int(DS.draw32(77, sid, 0)[0]) for sid in (0, 1, 2)] == [3852512481, 2806225190, 2153658527]
    np.testing.assert_array_equal(DS.draw32(77, np.arange(3), 0), [3852512481, 2806225190, 2153658527])


def test_bounded_covers_the_range_and_no_more():
    r = np.array([0, 1, 2 ** 31, 2 ** 32 - 1], dtype=np.uint64)
    np.testing.assert_array_equal(DS.bounded(r, 60), [0, 0, 30, 59])
    np.testing.assert_array_equal(DS.bounded(r, 2 ** 31 - 1), [0, 0, 2 ** 30 - 1, 2 ** 31 - 2])
    np.testing.assert_array_equal(DS.bounded(r, 1), [0, 0, 0, 0])


# ---- the rule -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("seed", SC.SEEDS)
def test_stream_follows_the_reference_rule(seed):
    figures, smallest = _statistics(seed)
    print(seed, figures, smallest)
    assert smallest >= 30                                     # the chi-square approximation holds
    assert set(figures) == {"z_user", "z_pos", "z_neg", "c_pos_neg", "c_user_lag"}
    assert not _outside(figures), (seed, _outside(figures))
    u, i, j, used = _stream(seed)
    X = SC.small_urm()
    # the edges of a profile are reached: user 2's only negative, its first and last positive, user 3's only positive
    assert (j[u == 2] == 59).all() and {0, 58} <= set(i[u == 2].tolist()) and (i[u == 3] == 0).all() and (u == 3).any()
    assert used.min() == 3 and (used[u == 2] > 3).any()
    assert X.shape == (400, 60)


def test_recorded_statistics_are_those_of_the_committed_model():
    with open(os.path.join(ROOT, "profiles", "sampler_statistics.json")) as f:
        recorded = json.load(f)
    assert recorded["n_samples"] == N and recorded["bound"] == SC.BOUND
    assert sorted(int(s) for s in recorded["per_seed"]) == sorted(SC.SEEDS)
    for seed in SC.SEEDS:
        figures, smallest = _statistics(seed)
        for name, v in figures.items():
            assert recorded["per_seed"][str(seed)][name] == pytest.approx(v, abs=1e-6), (seed, name)
    assert recorded["largest_abs_z"] == pytest.approx(max(abs(_statistics(s)[0][k]) for s in SC.SEEDS for k in ("z_user", "z_pos", "z_neg")), abs=1e-6)
    assert recorded["largest_abs_corr"] == pytest.approx(max(abs(_statistics(s)[0][k]) for s in SC.SEEDS for k in ("c_pos_neg", "c_user_lag")), abs=1e-6)


@pytest.mark.parametrize("seed", SC.SEEDS)
def test_mutant_that_rarely_skips_the_last_entry_fails_the_bounds(seed):
    """Planted fault: 5 % of the picks of a profile's last entry go to its first entry instead."""
    u, i, j, _ = _stream(seed)
    P = SC.profiles(SC.small_urm())
    first, last = P.indices[P.indptr[:-1].clip(max=len(P.indices) - 1)], P.indices[(P.indptr[1:] - 1).clip(min=0)]
    moved = (P.lens[u] > 1) & (i == last[u]) & (np.random.RandomState(12345).random_sample(N) < 0.05)
    mutant = np.where(moved, first[u], i).astype(np.int32)
    figures, _ = SC.sampler_statistics(SC.small_urm(), u, mutant, j)
    print(seed, figures)
    assert "z_pos" in _outside(figures), figures
    assert _statistics(seed)[0]["z_pos"] + 3 < figures["z_pos"]


@pytest.mark.parametrize("seed", SC.SEEDS)
def test_mutant_that_reuses_the_positive_draw_for_the_negative_fails_the_bounds(seed):
    """Planted fault: the first attempt at the negative item takes the draw the positive item was made of."""
    P = SC.profiles(SC.small_urm())
    sid = np.arange(N, dtype=np.uint64)
    d = np.zeros(N, dtype=np.uint64)
    u = P.draw_user(seed, sid, d)
    np.testing.assert_array_equal(u, _stream(seed)[0])
    i = P.indices[P.indptr[u] + DS.bounded(DS.draw32(seed, sid, d), P.lens[u])]
    np.testing.assert_array_equal(i, _stream(seed)[1])
    reused = d.copy()
    d += np.uint64(1)
    j = P.draw_outside(seed, sid, d, u, first_draw=reused)
    figures, _ = SC.sampler_statistics(SC.small_urm(), u, i, j)
    print(seed, figures)
    assert "c_pos_neg" in _outside(figures) and figures["c_pos_neg"] > 100, figures


# ---- epochs, seeds, sample ids --------------------------------------------------------------------------------------------------
def _equal_user_rate_is_chance(a, b):
    p = 1.0 / 398.0
    rate = float((a == b).mean())
    print(rate, p, 5 * np.sqrt(p / N))
    assert abs(rate - p) <= 5 * np.sqrt(p / N), (rate, p)


@pytest.mark.parametrize("seed", [77, 2 ** 63 + 11])
def test_consecutive_epochs_are_disjoint_and_independent(seed):
    X = SC.small_urm()
    for algorithm, B in (("MF_BPR", 7), ("MF_BPR", 500), ("FUNK_SVD", 64), ("ASY_SVD", 1)):
        n = DS.mf_samples_per_epoch(X, algorithm, B)
        for e in (0, 1, 2 ** 40):
            a, b = DS._epoch_sids(e, n), DS._epoch_sids(e + 1, n)
            assert len(a) == n and int(a[-1]) + 1 == int(b[0]) and int(a[0]) == e * n                 # back to back, never shared
    n = X.shape[0] + 1
    assert int(DS._epoch_sids(3, n)[0]) == 3 * n
    # sample t of epoch e against sample t of epoch e + 1, at an epoch length of N: equal users at the rate of chance
    _equal_user_rate_is_chance(_stream(seed, 0)[0], _stream(seed, N)[0])


@pytest.mark.parametrize("seed", [0, 77, 2 ** 32 + 5])
def test_neighbouring_seeds_are_independent(seed):
    _equal_user_rate_is_chance(_stream(seed)[0], _stream(seed + 1)[0])


def test_every_bit_of_a_64_bit_seed_counts():
    sid = np.arange(4096, dtype=np.uint64)
    P = SC.profiles(SC.small_urm())
    for seed in (2 ** 32 + 5, 2 ** 63 + 11):
        for narrowed in (seed % 2 ** 32, seed % 2 ** 63):
            if narrowed != seed:
                assert (DS.bpr_sample(P, seed, sid)[0] == DS.bpr_sample(P, narrowed, sid)[0]).mean() < 0.02
    for bit in range(64):
        assert (DS.draw32(77 ^ (1 << bit), sid, 0) != DS.draw32(77, sid, 0)).mean() > 0.99, bit


def test_sample_ids_are_64_bit():
    """Nothing changes across 2^32, and nothing is taken modulo 2^32."""
    P = SC.profiles(SC.small_urm())
    sid = np.arange(2 ** 32 - 2048, 2 ** 32 + 2048, dtype=np.uint64)
    whole = DS.bpr_sample(P, 77, sid)
    low, high = slice(0, 2048), slice(2048, 4096)
    wrapped = DS.bpr_sample(P, 77, sid % np.uint64(2 ** 32))
    for a, b in zip(whole[:3], wrapped[:3]):
        np.testing.assert_array_equal(a[low], b[low])
    assert (whole[0][high] == wrapped[0][high]).mean() < 0.02
    for t in (0, 2047, 2048, 4095):                                # Python integers: no array arithmetic to wrap
        one = DS.bpr_sample(P, 77, [int(sid[0]) + t])
        assert [int(a[0]) for a in one[:3]] == [int(a[t]) for a in whole[:3]]
    # an epoch whose sample ids straddle 2^32 is one unbroken stream: samples_per_epoch is 500 at batch size 500
    e = 2 ** 32 // 500
    assert e * 500 < 2 ** 32 < (e + 1) * 500
    stream = DS.mf_epoch_stream(P, "MF_BPR", 500, 77, e)
    direct = DS.bpr_sample(P, 77, [e * 500 + t for t in range(500)])
    for a, b in zip(stream, direct[:3]):
        np.testing.assert_array_equal(a, b)
    stream = DS.slim_epoch_stream(P, 77, 2 ** 32 // 401)
    direct = DS.bpr_sample(P, 77, [2 ** 32 // 401 * 401 + t for t in range(401)])
    for a, b in zip(stream, direct[:3]):
        np.testing.assert_array_equal(a, b)


def test_samples_per_epoch():
    X = SC.small_urm()
    assert X.nnz == 5176
    assert [DS.mf_samples_per_epoch(X, "MF_BPR", B) for B in (1, 7, 400, 500)] == [401, 406, 800, 500]            # (n_users // B + 1) B
    assert [DS.mf_samples_per_epoch(X, "FUNK_SVD", B) for B in (1, 64, 5176, 6000)] == [5177, 5184, 10352, 6000]   # (nnz // B + 1) B
    assert DS.mf_samples_per_epoch(X, "ASY_SVD", 1) == 5177                                                        # nnz + 1 steps
    assert len(DS.slim_epoch_stream(X, 1, 0)[0]) == 401                                                            # n_users + 1 steps
    for algorithm, B in (("MF_BPR", 7), ("FUNK_SVD", 64), ("ASY_SVD", 1)):
        assert all(len(a) == DS.mf_samples_per_epoch(X, algorithm, B) for a in DS.mf_epoch_stream(X, algorithm, B, 5, 2, quota=0.3))


# ---- the MSE sampler ------------------------------------------------------------------------------------------------------------
def _mse_case():
    X = SC.small_urm("real")
    return X, SC.profiles(X), np.arange(200000, dtype=np.uint64)


def test_mse_without_quota_takes_every_sample_from_the_profile():
    X, P, sid = _mse_case()
    u, i, r = DS.mse_sample(P, 77, sid, 0.0)
    assert r.dtype == np.float32 and (r != 0).all()
    np.testing.assert_array_equal(np.asarray(X[u, i]).ravel().astype(np.float32).view(np.int32), r.view(np.int32))
    ub, ib, _, _ = DS.bpr_sample(P, 77, sid)
    np.testing.assert_array_equal(u, ub)                          # the same draws as the BPR sampler's user and positive item
    np.testing.assert_array_equal(i, ib)
    assert 0 not in set(u.tolist()) and 1 not in set(u.tolist())


def test_mse_quota_one_is_all_positive_with_one_more_draw_used():
    X, P, sid = _mse_case()
    u0, i0, _ = DS.mse_sample(P, 77, sid, 0.0)
    u, i, r = DS.mse_sample(P, 77, sid, 1.0)
    np.testing.assert_array_equal(u, u0)
    np.testing.assert_array_equal(np.asarray(X[u, i]).ravel().astype(np.float32).view(np.int32), r.view(np.int32))
    assert (r != 0).all()
    d = np.zeros(len(sid), dtype=np.uint64)
    np.testing.assert_array_equal(P.draw_user(77, sid, d), u)
    np.testing.assert_array_equal(P.indices[P.indptr[u] + DS.bounded(DS.draw32(77, sid, d), P.lens[u])], i0)
    np.testing.assert_array_equal(P.indices[P.indptr[u] + DS.bounded(DS.draw32(77, sid, d + np.uint64(1)), P.lens[u])], i)
    assert (i != i0).any()
    # the largest draw rounds to 2^32 in float32 and is still a positive at quota 1: r * 2^-32 <= 1
    assert np.float32(2 ** 32 - 1) * np.float32(2.0 ** -32) <= np.float32(1.0)


@pytest.mark.parametrize("seed", SC.SEEDS)
def test_mse_quota_is_the_fraction_of_positives(seed):
    """.pyx:898 draws a POSITIVE with probability `quota` (sic)."""
    X, P, sid = _mse_case()
    u, i, r = DS.mse_sample(P, seed, sid, 0.4)
    positive = r != 0
    sigma = np.sqrt(0.4 * 0.6 / len(sid))
    print(seed, positive.mean(), 5 * sigma)
    assert abs(positive.mean() - 0.4) <= 5 * sigma
    stored = np.asarray(X[u, i]).ravel().astype(np.float32)
    np.testing.assert_array_equal(stored.view(np.int32), r.view(np.int32))       # a negative carries 0 and lies outside the profile
    assert (r[~positive].view(np.int32) == 0).all()                              # (+0.0, not -0.0)
    # the compare is made in float32: a quota that float32 rounds UP takes the draws in between as positives
    assert float(np.float32(0.4)) > 0.4
    assert 0 not in set(u.tolist()) and 1 not in set(u.tolist())


def test_reference_rule_has_the_same_positive_fraction():
    """OracleMF draws from glibc's rand() by the reference's text (`rand() <= quota * RAND_MAX` selects a positive): the same
    fraction within the same bound, on the same matrix."""
    X = SC.small_urm("real")
    orc = O.OracleMF(X, n_factors=1, algorithm_name="FUNK_SVD", batch_size=64, negative_interactions_quota=0.4, random_seed=77,
                     learning_rate=1e-4)
    per_epoch = DS.mf_samples_per_epoch(X, "FUNK_SVD", 64)
    epochs = 20
    orc.record_samples(per_epoch * epochs)
    for _ in range(epochs):
        orc.epochIteration_Cython()
    u, i, _, r = orc.recorded()
    assert len(u) == per_epoch * epochs
    sigma = np.sqrt(0.4 * 0.6 / len(u))
    print((r != 0).mean(), 5 * sigma)
    assert abs((r != 0).mean() - 0.4) <= 5 * sigma
    np.testing.assert_array_equal(np.asarray(X[u, i]).ravel().astype(np.float64), r)
