"""The in-LDS MF schedule on BIT ROWS (the default: [mini-batch][row bit], built in LDS, turned into version parities by
mf_sched_parity_kernel) against the same schedule on the per-row bitmap it replaces (MI355REC_MF_ROW_BITMAP: global atomics, the
finish kernel, popcounts in the emit kernel) and against the oracle's replay of the device's own stream.

Both device paths are to write the same headers and records, so their factors are compared with np.array_equal; the oracle with the
suite's element-wise bar (test_mf_gpu.py).  Tiny shapes: k = 16, mini-batches of 4 samples unless a case says otherwise.
"""
import numpy as np
import pytest
import scipy.sparse as sps

from oracle import oracle as O
from recsys2019_deeplearning_evaluation_amd import MatrixFactorization_MI355X_Epoch, MatrixFactorization_MI355X_Group
from recsys2019_deeplearning_evaluation_amd.synthetic import synthetic_urm

pytestmark = pytest.mark.gpu

KNOB = "MI355REC_MF_ROW_BITMAP"
BPR = dict(n_factors=16, algorithm_name="MF_BPR", batch_size=4, random_seed=9, sgd_mode="sgd", learning_rate=0.05,
           user_reg=0.01, positive_reg=0.01, negative_reg=0.02)


def assert_factor_parity(dev, ref, what):
    """The suite's bar against the oracle (test_mf_gpu.py): element-wise |dev - ref| <= 1e-5 |ref| + 1e-6 max|ref|."""
    dev = np.asarray(dev, dtype=np.float64); ref = np.asarray(ref, dtype=np.float64)
    tol = 1e-5 * np.abs(ref) + 1e-6 * max(np.abs(ref).max(), 1e-30)
    excess = np.abs(dev - ref) - tol
    assert excess.max() <= 0, (what, "worst excess over the element-wise tolerance", excess.max())


def _set(monkeypatch, name, on):
    if on:
        monkeypatch.setenv(name, "1")
    else:
        monkeypatch.delenv(name, raising=False)


def _profiles(n_users, n_items, seed, always=()):
    """every user with 1 .. 5 items of its own (never all of them: BPR needs a negative), plus the items of `always`"""
    rng = np.random.default_rng(seed)
    rows, cols = [], []
    free = np.setdiff1d(np.arange(n_items), always)
    for u in range(n_users):
        own = rng.choice(free, size=int(rng.integers(1, min(5, len(free) - 1) + 1)), replace=False)
        own = np.union1d(own, always).astype(np.int64)
        rows += [u] * len(own); cols += own.tolist()
    X = sps.csr_matrix((np.ones(len(rows), np.float32), (rows, cols)), shape=(n_users, n_items))
    X.sort_indices()
    return X


def _samples_to_oracle(orc, kw, samples):
    if kw["algorithm_name"] == "MF_BPR":
        orc.replay(samples[0], samples[1], j=samples[2])
    else:
        orc.replay(samples[0], samples[1], rating=samples[2])


def _model(dev, kw):
    out = [dev.get_USER_factors(), dev.get_ITEM_factors()]
    if kw.get("use_bias"):
        out += [dev.get_USER_bias(), dev.get_ITEM_bias()]
    return out


def _three_ways(X, kw, monkeypatch, epochs=2):
    """`epochs` epochs on bit rows, on the per-row bitmap and replayed on the oracle: equal streams, equal factors, oracle parity."""
    orc = O.OracleMF(X, **kw)
    init = dict(initial_USER_factors=orc.initial_USER_factors, initial_ITEM_factors=orc.initial_ITEM_factors)
    out = []
    for bitmap in (False, True):
        _set(monkeypatch, KNOB, bitmap)
        dev = MatrixFactorization_MI355X_Epoch(X, **init, **kw)
        streams = []
        for _ in range(epochs):
            dev.epochIteration_Cython()
            streams.append(dev.last_epoch_samples())
            if not bitmap:
                _samples_to_oracle(orc, kw, streams[-1])
        out.append((_model(dev, kw), streams))
        dev.close()
    for sa, sb in zip(out[0][1], out[1][1]):
        assert len(sa[0]) == (( X.shape[0] if kw["algorithm_name"] == "MF_BPR" else X.nnz) // kw["batch_size"] + 1) * kw["batch_size"]
        for x, y in zip(sa, sb):
            np.testing.assert_array_equal(x, y)
    for a, b in zip(out[0][0], out[1][0]):
        np.testing.assert_array_equal(a, b)
    assert_factor_parity(out[0][0][0], orc.get_USER_factors(), "U")
    assert_factor_parity(out[0][0][1], orc.get_ITEM_factors(), "V")
    if kw.get("use_bias"):
        assert_factor_parity(out[0][0][2], orc.get_USER_bias(), "bu")
        assert_factor_parity(out[0][0][3], orc.get_ITEM_bias(), "bi")
    return out[0]


# one partial word; the user / item border inside a word (5, 31, 33, 100 users) and on a word border (32); more than four words: a row
# of two 16-byte groups (1 100 rows)
@pytest.mark.parametrize("n_users, n_items", [(5, 3), (31, 33), (32, 32), (33, 40), (100, 1000)])
def test_word_edges(gpu, n_users, n_items, monkeypatch):
    _three_ways(_profiles(n_users, n_items, seed=n_users), BPR, monkeypatch)


@pytest.mark.parametrize("n_batches", [1, 2, 255, 256])
def test_rows_touched_in_every_mini_batch(gpu, n_batches, monkeypatch):
    """Item 0 is in every profile (test_version_parity_across_bitmap_words): its row, and with 40 items most rows, is touched in nearly
    every mini-batch, so its column of the bit rows flips at every step of the column pass -- over 1, 2 and, at 255 / 256
    mini-batches, all 16 parts of the pass."""
    n_users = (n_batches - 1) * 4 + 2
    X = _profiles(n_users, 40, seed=n_batches, always=(0,))
    _, streams = _three_ways(X, BPR, monkeypatch)
    u, i, j = streams[-1]
    assert len(u) == 4 * n_batches
    assert (i == 0).any() or n_batches <= 2


def test_parities_carried_from_stream_to_stream(gpu, monkeypatch):
    """par[] after a stream is the start of the next: three epochs in one call (graph replays) against three calls, on both paths."""
    X = _profiles(61, 40, seed=3, always=(0,))
    orc = O.OracleMF(X, **BPR)
    init = dict(initial_USER_factors=orc.initial_USER_factors, initial_ITEM_factors=orc.initial_ITEM_factors)
    models = []
    for bitmap in (False, True):
        _set(monkeypatch, KNOB, bitmap)
        for calls in ((3,), (1, 1, 1)):
            dev = MatrixFactorization_MI355X_Epoch(X, **init, **BPR)
            for n in calls:
                dev.epochIteration_Cython(n)
                if not bitmap and n == 1:
                    u, i, j = dev.last_epoch_samples()
                    orc.replay(u, i, j=j)
            models.append((dev.get_USER_factors(), dev.get_ITEM_factors(), dev.last_epoch_samples()))
            dev.close()
    for other in models[1:]:
        np.testing.assert_array_equal(models[0][0], other[0])
        np.testing.assert_array_equal(models[0][1], other[1])
        for x, y in zip(models[0][2], other[2]):
            np.testing.assert_array_equal(x, y)
    assert_factor_parity(models[0][0], orc.get_USER_factors(), "U")
    assert_factor_parity(models[0][1], orc.get_ITEM_factors(), "V")


@pytest.mark.parametrize("use_bias", [False, True])
def test_parities_carried_from_part_to_part(gpu, use_bias, monkeypatch):
    """FunkSVD with about 600 mini-batches an epoch: three schedule parts of at most 256, each a stream of its own that starts from
    the par[] the part in front of it left."""
    X = synthetic_urm(200, 60, 2400, 1, 59, seed=4, values="real")
    n_batches = X.nnz // 4 + 1
    assert 2 * 256 < n_batches <= 3 * 256
    kw = dict(n_factors=16, algorithm_name="FUNK_SVD", batch_size=4, random_seed=21, sgd_mode="sgd", learning_rate=0.01,
              user_reg=0.01, item_reg=0.1, bias_reg=0.01, use_bias=use_bias, negative_interactions_quota=0.3)
    _three_ways(X, kw, monkeypatch)


def _train(X, kws, epochs, grouped):
    members = [MatrixFactorization_MI355X_Epoch(X, **kw) for kw in kws]
    if grouped:
        group = MatrixFactorization_MI355X_Group(members)
        group.epochIteration_Cython(1)
        group.epochIteration_Cython(epochs - 1)
        group.close()
    else:
        for m in members:
            m.epochIteration_Cython(epochs)
    out = [(m.get_USER_factors(), m.get_ITEM_factors(), m.last_epoch_samples()) for m in members]
    for m in members:
        m.close()
    return out


def _assert_same_models(a, b):
    for (Ua, Va, sa), (Ub, Vb, sb) in zip(a, b):
        np.testing.assert_array_equal(Ua, Ub)
        np.testing.assert_array_equal(Va, Vb)
        for x, y in zip(sa, sb):
            np.testing.assert_array_equal(x, y)


def test_group_of_two_against_training_alone(gpu, monkeypatch):
    X = _profiles(61, 40, seed=5, always=(0,))
    kws = [dict(BPR, random_seed=50 + n, learning_rate=0.02 * (n + 1)) for n in range(2)]
    _set(monkeypatch, KNOB, False)
    alone = _train(X, kws, 3, grouped=False)
    _assert_same_models(alone, _train(X, kws, 3, grouped=True))
    _set(monkeypatch, KNOB, True)
    _assert_same_models(alone, _train(X, kws, 3, grouped=False))
    _assert_same_models(alone, _train(X, kws, 3, grouped=True))


def test_group_whose_members_disagree_falls_back_as_a_whole(gpu, monkeypatch):
    """A handle decides once, with its first native call.  Member 0 made that call under MI355REC_MF_ROW_BITMAP, member 1 without: one
    launch cannot run the parity kernel for one and the finish kernel for the other, so the members schedule on their own streams --
    and end where they end alone."""
    X = _profiles(61, 40, seed=6, always=(0,))
    kws = [dict(BPR, random_seed=60 + n) for n in range(2)]
    out = []
    for grouped in (False, True):
        members = []
        for n, kw in enumerate(kws):
            _set(monkeypatch, KNOB, n == 0)
            members.append(MatrixFactorization_MI355X_Epoch(X, **kw))
            members[-1].epochIteration_Cython()
        _set(monkeypatch, KNOB, False)
        if grouped:
            group = MatrixFactorization_MI355X_Group(members)
            group.epochIteration_Cython(2)
            group.close()
        else:
            for m in members:
                m.epochIteration_Cython(2)
        out.append([(m.get_USER_factors(), m.get_ITEM_factors(), m.last_epoch_samples()) for m in members])
        for m in members:
            m.close()
    _assert_same_models(out[0], out[1])


def _paths_agree(X, kw, monkeypatch, epochs=2):
    """default, MI355REC_MF_ROW_BITMAP and the radix-sort schedule: equal streams; the first two bit-identical, the third within
    test_schedule_paths_agree's bar (its kernels share nothing with the in-LDS ones)"""
    out = []
    for bitmap, general in ((False, False), (True, False), (False, True)):
        _set(monkeypatch, KNOB, bitmap)
        _set(monkeypatch, "MI355REC_MF_GENERAL_SCHEDULE", general)
        dev = MatrixFactorization_MI355X_Epoch(X, **kw)
        dev.epochIteration_Cython(epochs)
        out.append((dev.get_USER_factors(), dev.get_ITEM_factors(), dev.last_epoch_samples()))
        dev.close()
    for other in out[1:]:
        for x, y in zip(out[0][2], other[2]):
            np.testing.assert_array_equal(x, y)
    np.testing.assert_array_equal(out[0][0], out[1][0])
    np.testing.assert_array_equal(out[0][1], out[1][1])
    for a, b in zip(out[0][:2], out[2][:2]):
        assert np.abs(a - b).max() <= 1e-6 * np.abs(b).max()


def test_fallback_by_size(gpu, monkeypatch):
    """1.2 M users x 10 items, k = 4, mini-batches of 2 000: a bit row of 150 KB does not fit beside 8 192 keys.  (With 21 bits of
    row id and 13 of slot the keys of this shape do not fit 31 bits either, so it is the radix-sort schedule that runs all three
    times; the next test is the shape that reaches the per-row bitmap by size.)"""
    n_users, n_items = 1200000, 10
    rng = np.random.default_rng(0)
    X = sps.csr_matrix((np.ones(n_users, np.float32), (np.arange(n_users), rng.integers(0, n_items, n_users))), shape=(n_users, n_items))
    kw = dict(n_factors=4, algorithm_name="MF_BPR", batch_size=2000, random_seed=3, sgd_mode="sgd", learning_rate=0.05, user_reg=0.01)
    _paths_agree(X, kw, monkeypatch)


def test_fallback_by_size_inside_the_lds_schedule(gpu, monkeypatch):
    """1.25 M users x 10 items, FunkSVD with mini-batches of 500: 1 000 header slots leave 21 bits for the rows, so the in-LDS schedule
    runs -- and the bit row, 156 KB, does not fit its workgroup (tests/test_mf_bit_rows_plan.py pins both): the per-row bitmap without
    the switch.  41 mini-batches an epoch."""
    n_users, n_items, nnz = 1250000, 10, 20000
    rng = np.random.default_rng(1)
    users = rng.choice(n_users, size=nnz, replace=False)
    X = sps.csr_matrix((rng.integers(1, 6, nnz).astype(np.float32), (users, rng.integers(0, n_items, nnz))), shape=(n_users, n_items))
    X.sort_indices()
    kw = dict(n_factors=4, algorithm_name="FUNK_SVD", batch_size=500, random_seed=8, sgd_mode="sgd", learning_rate=0.01, user_reg=0.01,
              item_reg=0.05, negative_interactions_quota=0.2)
    _paths_agree(X, kw, monkeypatch)
