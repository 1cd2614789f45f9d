"""The device sample stream against its host model (oracle/device_sampler.py), with exact equality everywhere: every path that
draws (the stand-alone MF sampler, the in-LDS schedule's workgroups, the radix-sort schedule, the group, the exact multi-GPU mode,
AsySVD, slim_sample_kernel behind all three stores and its schedule-ahead path), every seed width, and the epoch numbering:
a handle's first native epoch is epoch 0 of the model, and a replay_samples call between two native epochs moves no counter.
test_device_sampler_spec.py holds the model to the reference's sampling rule.  Ratings are compared as float32 bits.
"""
import ctypes as C

import numpy as np
import pytest

from oracle import device_sampler as DS
from recsys2019_deeplearning_evaluation_amd import (MatrixFactorization_MI355X_Epoch, MatrixFactorization_MI355X_Group,
                                                    SLIM_BPR_MI355X_Epoch, _native as N)
import sampler_cases as SC

pytestmark = pytest.mark.gpu

_URM = {"small": SC.small_urm, "large": SC.large_urm}
_MODEL = {}


def _model_mf(matrix, values, algorithm, batch_size, seed, epoch, quota=0.0):
    key = (matrix, values, algorithm, batch_size, seed, epoch, quota)
    if key not in _MODEL:
        out = DS.mf_epoch_stream(SC.profiles(_URM[matrix](values)), algorithm, batch_size, seed, epoch, quota)
        for a in out:
            a.setflags(write=False)
        _MODEL[key] = out
    return _MODEL[key]


def _model_slim(matrix, seed, epoch):
    key = (matrix, "slim", seed, epoch)
    if key not in _MODEL:
        out = DS.slim_epoch_stream(SC.profiles(_URM[matrix]("binary")), seed, epoch)
        for a in out:
            a.setflags(write=False)
        _MODEL[key] = out
    return _MODEL[key]


def _assert_stream(got, want, what):
    assert len(got) == len(want) == 3
    for name, g, w in zip(("user", "item", "third"), got, want):
        assert g.dtype == w.dtype and len(w) > 0, (what, name, g.dtype, w.dtype)
        if g.dtype == np.float32:
            g, w = g.view(np.int32), w.view(np.int32)
        np.testing.assert_array_equal(g, w, err_msg="%s: %s" % (what, name))


def _bpr(matrix, batch_size, seed, **more):
    return MatrixFactorization_MI355X_Epoch(_URM[matrix]("binary"), n_factors=8, algorithm_name="MF_BPR", batch_size=batch_size,
                                            random_seed=seed, sgd_mode="sgd", learning_rate=0.05, user_reg=0.01, positive_reg=0.01,
                                            negative_reg=0.02, **more)


def _set_schedule(monkeypatch, general):
    if general:
        monkeypatch.setenv("MI355REC_MF_GENERAL_SCHEDULE", "1")
    else:
        monkeypatch.delenv("MI355REC_MF_GENERAL_SCHEDULE", raising=False)


# ---- MF_BPR ---------------------------------------------------------------------------------------------------------------------
# large matrix: 1 and 7 are scheduled 256 mini-batches at a time behind the stand-alone sampler, 500 .. 2730 are drawn by the in-LDS
# schedule's workgroups (1025: more samples than threads; 2730: the last size whose 3 B incidences fit), 2731 is on the radix-sort
# schedule.  small matrix: 1 is two parts behind the stand-alone sampler, everything from 500 up is ONE mini-batch.
@pytest.mark.parametrize("general", [False, True], ids=["fast", "general"])
@pytest.mark.parametrize("batch_size", [1, 7, 500, 1025, 2730, 2731])
@pytest.mark.parametrize("matrix", ["small", "large"])
def test_bpr_stream_is_the_model(gpu, matrix, batch_size, general, monkeypatch):
    _set_schedule(monkeypatch, general)
    seed = 77
    dev = _bpr(matrix, batch_size, seed)
    for epoch in range(3):                                    # the first, second and third epoch of a handle: three calls
        dev.epochIteration_Cython()
        _assert_stream(dev.last_epoch_samples(), _model_mf(matrix, "binary", "MF_BPR", batch_size, seed, epoch), "call %d" % (epoch + 1))
    dev.close()
    dev = _bpr(matrix, batch_size, seed)
    dev.epochIteration_Cython(3)                              # ... and the third epoch of one call
    _assert_stream(dev.last_epoch_samples(), _model_mf(matrix, "binary", "MF_BPR", batch_size, seed, 2), "third epoch of one call")
    dev.close()


@pytest.mark.parametrize("seed", SC.SEEDS)
def test_bpr_stream_takes_all_64_seed_bits(gpu, seed, monkeypatch):
    _set_schedule(monkeypatch, False)
    for batch_size in (500, 7):                               # drawn by the schedule's workgroups | by the stand-alone sampler
        dev = _bpr("small", batch_size, seed)
        dev.epochIteration_Cython(2)
        _assert_stream(dev.last_epoch_samples(), _model_mf("small", "binary", "MF_BPR", batch_size, seed, 1), "batch size %d" % batch_size)
        dev.close()


# ---- FUNK_SVD, ASY_SVD ----------------------------------------------------------------------------------------------------------
def _funk(matrix, batch_size, seed, quota, use_bias, algorithm="FUNK_SVD"):
    return MatrixFactorization_MI355X_Epoch(_URM[matrix]("real"), n_factors=8, algorithm_name=algorithm, batch_size=batch_size,
                                            random_seed=seed, sgd_mode="sgd", learning_rate=0.01, user_reg=0.01, item_reg=0.1,
                                            bias_reg=0.01, use_bias=use_bias, negative_interactions_quota=quota)


# large matrix: 64 is 900-odd mini-batches behind the stand-alone sampler, 2000 and 4096 (the largest mini-batch of the in-LDS
# schedule) are drawn in the workgroups
@pytest.mark.parametrize("use_bias", [False, True], ids=["plain", "bias"])
@pytest.mark.parametrize("quota", [0.0, 0.4, 1.0])
@pytest.mark.parametrize("batch_size", [64, 2000, 4096])
@pytest.mark.parametrize("matrix", ["small", "large"])
def test_funk_stream_is_the_model(gpu, matrix, batch_size, quota, use_bias, monkeypatch):
    _set_schedule(monkeypatch, False)
    seed = 78
    dev = _funk(matrix, batch_size, seed, quota, use_bias)
    dev.epochIteration_Cython()
    got = dev.last_epoch_samples()
    _assert_stream(got, _model_mf(matrix, "real", "FUNK_SVD", batch_size, seed, 0, quota), "first epoch")
    assert (got[2] == 0).any() == (quota == 0.4)              # sampled negatives only then; (sic) quota 1 is all positives
    dev.epochIteration_Cython(2)
    _assert_stream(dev.last_epoch_samples(), _model_mf(matrix, "real", "FUNK_SVD", batch_size, seed, 2, quota), "third epoch")
    dev.close()


@pytest.mark.parametrize("seed", [2 ** 32 + 5, 2 ** 63 + 11])
def test_funk_stream_on_the_radix_sort_schedule_and_wide_seeds(gpu, seed, monkeypatch):
    _set_schedule(monkeypatch, True)
    dev = _funk("small", 2000, seed, 0.4, True)
    dev.epochIteration_Cython(2)
    _assert_stream(dev.last_epoch_samples(), _model_mf("small", "real", "FUNK_SVD", 2000, seed, 1, 0.4), "second epoch")
    dev.close()


def test_asy_svd_stream_is_the_model(gpu):
    X = SC.small_urm("real")
    dev = _funk("small", 1, 5, 0.4, True, algorithm="ASY_SVD")
    dev.epochIteration_Cython()
    got = dev.last_epoch_samples()
    assert len(got[0]) == X.nnz + 1                            # nnz / 1 + 1 single-sample steps
    _assert_stream(got, _model_mf("small", "real", "ASY_SVD", 1, 5, 0, 0.4), "first epoch")
    dev.close()


# ---- the seed a constructor draws -----------------------------------------------------------------------------------------------
def test_seed_drawn_by_the_mf_constructor(gpu):
    """random_seed=None: U then V from np.random.normal, then the seed from np.random.randint(0, 2^31 - 1)."""
    X = SC.small_urm()
    np.random.seed(1234)
    dev = MatrixFactorization_MI355X_Epoch(X, n_factors=8, algorithm_name="MF_BPR", batch_size=500, sgd_mode="sgd", learning_rate=0.05)
    rs = np.random.RandomState(1234)
    rs.normal(0.0, 0.1, (X.shape[0], 8)); rs.normal(0.0, 0.1, (X.shape[1], 8))
    seed = int(rs.randint(0, 2 ** 31 - 1))
    dev.epochIteration_Cython()
    _assert_stream(dev.last_epoch_samples(), DS.mf_epoch_stream(X, "MF_BPR", 500, seed, 0), "seed %d" % seed)
    dev.close()


def test_seed_drawn_by_the_slim_constructor(gpu):
    X = SC.small_urm()
    np.random.seed(4321)
    dev = SLIM_BPR_MI355X_Epoch(X, topK=False, symmetric=False, sgd_mode="sgd", learning_rate=0.02)
    seed = int(np.random.RandomState(4321).randint(0, 2 ** 31 - 1))
    dev.epochIteration_Cython()
    _assert_stream(dev.last_epoch_samples(), DS.slim_epoch_stream(X, seed, 0), "seed %d" % seed)
    dev.close()


# ---- the group ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("matrix,batch_size", [("small", 100), ("large", 500), ("large", 2731)])
def test_group_members_keep_their_own_64_bit_seed(gpu, matrix, batch_size, monkeypatch):
    """Seeds that collide if only 32 bits of them arrive."""
    _set_schedule(monkeypatch, False)
    seeds = [1, 2, 2 ** 32 + 1, 2 ** 32 + 2]
    members = [_bpr(matrix, batch_size, seed) for seed in seeds]
    group = MatrixFactorization_MI355X_Group(members)
    group.epochIteration_Cython(3)
    for seed, m in zip(seeds, members):
        _assert_stream(m.last_epoch_samples(), _model_mf(matrix, "binary", "MF_BPR", batch_size, seed, 2), "member with seed %d" % seed)
    assert (members[0].last_epoch_samples()[0] != members[2].last_epoch_samples()[0]).any()
    group.close()
    for m in members:
        m.close()


# ---- SLIM-BPR -------------------------------------------------------------------------------------------------------------------
_STORES = {"dense": dict(symmetric=False, topK=False), "symmetric": dict(symmetric=True, topK=False),
           "sparse": dict(train_with_sparse_weights=True, topK=10)}


def _slim(matrix, store, seed):
    return SLIM_BPR_MI355X_Epoch(_URM[matrix]("binary"), random_seed=seed, sgd_mode="sgd", learning_rate=0.02, li_reg=0.001, lj_reg=0.001,
                                 **_STORES[store])


# (the dense and the symmetric store draw and schedule epoch e + 1 behind epoch e, and keep it for the next call; the sparse store
# draws every epoch in front of its segments)
@pytest.mark.parametrize("matrix,seed", [("small", 77), ("small", 2 ** 32 + 5), ("small", 2 ** 63 + 11), ("large", 2 ** 63 + 11)])
@pytest.mark.parametrize("store", list(_STORES))
def test_slim_stream_is_the_model(gpu, store, matrix, seed):
    dev = _slim(matrix, store, seed)
    for epoch in range(3):
        dev.epochIteration_Cython()
        _assert_stream(dev.last_epoch_samples(), _model_slim(matrix, seed, epoch), "call %d" % (epoch + 1))
    dev.close()
    dev = _slim(matrix, store, seed)
    dev.epochIteration_Cython(3)
    _assert_stream(dev.last_epoch_samples(), _model_slim(matrix, seed, 2), "third epoch of one call")
    dev.epochIteration_Cython(2)                              # its first epoch was scheduled behind the last call
    _assert_stream(dev.last_epoch_samples(), _model_slim(matrix, seed, 4), "fifth epoch")
    dev.close()


# ---- a replay between two native epochs moves no counter ------------------------------------------------------------------------
@pytest.mark.parametrize("batch_size,general", [(500, False), (7, False), (500, True)])
def test_mf_replay_between_native_epochs(gpu, batch_size, general, monkeypatch):
    _set_schedule(monkeypatch, general)
    seed = 2 ** 32 + 5
    dev = _bpr("small", batch_size, seed)
    dev.epochIteration_Cython()
    _assert_stream(dev.last_epoch_samples(), _model_mf("small", "binary", "MF_BPR", batch_size, seed, 0), "first epoch")
    u, i, j = _model_mf("small", "binary", "MF_BPR", batch_size, 99, 6)          # some valid stream that is not this handle's
    dev.replay_samples(u, i, neg_item=j)
    assert len(dev.last_epoch_samples()[0]) == 0              # a replayed stream is not served as a drawn one
    dev.epochIteration_Cython()
    _assert_stream(dev.last_epoch_samples(), _model_mf("small", "binary", "MF_BPR", batch_size, seed, 1), "native epoch after a replay")
    dev.replay_samples(u[:37], i[:37], neg_item=j[:37])
    dev.epochIteration_Cython(2)
    _assert_stream(dev.last_epoch_samples(), _model_mf("small", "binary", "MF_BPR", batch_size, seed, 3), "fourth native epoch")
    dev.close()


def test_funk_replay_between_native_epochs(gpu, monkeypatch):
    _set_schedule(monkeypatch, False)
    dev = _funk("small", 2000, 78, 0.4, True)
    dev.epochIteration_Cython()
    u, i, r = _model_mf("small", "real", "FUNK_SVD", 2000, 99, 6, 0.4)
    dev.replay_samples(u, i, rating=r)
    dev.epochIteration_Cython()
    _assert_stream(dev.last_epoch_samples(), _model_mf("small", "real", "FUNK_SVD", 2000, 78, 1, 0.4), "native epoch after a replay")
    dev.close()


@pytest.mark.parametrize("store", list(_STORES))
def test_slim_replay_between_native_epochs(gpu, store):
    """The replayed stream takes the set that held the stream scheduled ahead for the next native epoch: that epoch is drawn again."""
    seed = 2 ** 63 + 11
    dev = _slim("small", store, seed)
    dev.epochIteration_Cython(2)
    _assert_stream(dev.last_epoch_samples(), _model_slim("small", seed, 1), "second epoch")
    u, i, j = _model_slim("small", 99, 6)
    dev.replay_samples(u, i, j)
    assert len(dev.last_epoch_samples()[0]) == 0
    dev.epochIteration_Cython()
    _assert_stream(dev.last_epoch_samples(), _model_slim("small", seed, 2), "native epoch after a replay")
    dev.replay_samples(u[:37], i[:37], j[:37])
    dev.replay_samples(u[37:90], i[37:90], j[37:90])
    dev.epochIteration_Cython(2)
    _assert_stream(dev.last_epoch_samples(), _model_slim("small", seed, 4), "fifth native epoch")
    dev.close()


# ---- the exact multi-GPU mode ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("world", [1, 3])
def test_sharded_epoch_draws_the_model_stream_on_every_rank(gpu, world):
    """`world` replicas in one process stand for the ranks (test_sharding_gpu.py); shard_begin_epoch draws with the stand-alone
    sampler, and the stream is served once shard_end_epoch has closed the epoch."""
    seed, batch_size = 2 ** 32 + 5, 100
    ranks = [_bpr("small", batch_size, seed) for _ in range(world)]
    lib = N.load()
    for epoch in range(2):
        slabs = [m.shard_begin_epoch(r, world) for r, m in enumerate(ranks)]
        n_batches, nbytes = slabs[0][3], slabs[0][2]
        assert n_batches == 400 // batch_size + 1
        for b in range(n_batches):
            for m in ranks:
                m.shard_batch(b)
            for dst in range(world):
                for src in range(world):
                    N.check(lib.mi355rec_device_memcpy(C.c_void_p(slabs[dst][1] + src * nbytes), C.c_void_p(slabs[src][0]), nbytes, 2))
            for m in ranks:
                m.shard_merge(b)
        for m in ranks:
            m.shard_end_epoch()
            _assert_stream(m.last_epoch_samples(), _model_mf("small", "binary", "MF_BPR", batch_size, seed, epoch), "sharded epoch %d" % (epoch + 1))
    ranks[-1].epochIteration_Cython()                         # a plain epoch continues the numbering
    _assert_stream(ranks[-1].last_epoch_samples(), _model_mf("small", "binary", "MF_BPR", batch_size, seed, 2), "plain epoch after two sharded ones")
    for m in ranks:
        m.close()
