"""The head of a native BPR-MF / FunkSVD epoch: the in-LDS schedule's workgroups draw their own mini-batch (no sampler launch), the
finish kernel advances the epoch counter, the emit kernel takes the version parities from whole bitmap rows and the position within
a run from the qtask word.

The partner inside one build is the radix-sort schedule (MI355REC_MF_GENERAL_SCHEDULE=1): it keeps the stand-alone sampler and builds
records and headers with kernels that share nothing with the in-LDS ones.  The second partner is the oracle's replay of the device's
own stream.  Headers and records have no getter, so they are not compared byte by byte here: what the mini-batch kernel makes of them
is (the factors), together with the bit-identity of the benchmark's outputs across builds (profiles/mf_epoch_head.txt).
"""
import numpy as np
import pytest
import scipy.sparse as sps

from oracle import oracle as O
from recsys2019_deeplearning_evaluation_amd import MatrixFactorization_MI355X_Epoch
from recsys2019_deeplearning_evaluation_amd.synthetic import synthetic_urm

pytestmark = pytest.mark.gpu


def assert_factor_parity(dev, ref, what):
    """The suite's bar against the oracle (test_mf_gpu.py): element-wise |dev - ref| <= 1e-5 |ref| + 1e-6 max|ref|."""
    dev = np.asarray(dev, dtype=np.float64); ref = np.asarray(ref, dtype=np.float64)
    tol = 1e-5 * np.abs(ref) + 1e-6 * max(np.abs(ref).max(), 1e-30)
    excess = np.abs(dev - ref) - tol
    assert excess.max() <= 0, (what, "worst excess over the element-wise tolerance", excess.max())


def _urm_with_a_full_and_an_empty_user(values):
    X = synthetic_urm(2000, 300, 60000, 1, 299, seed=3, values=values)
    X = X.tolil(); X[0, :] = 1.0; X[1, :] = 0.0; X = X.tocsr(); X.sort_indices()     # neither may ever be drawn (.pyx:950-958)
    X.eliminate_zeros()
    return X


_URMS = {}


def _urm(values):
    if values not in _URMS:
        _URMS[values] = _urm_with_a_full_and_an_empty_user(values)
    return _URMS[values]


def _three_epochs(X, kw, general, monkeypatch):
    if general:
        monkeypatch.setenv("MI355REC_MF_GENERAL_SCHEDULE", "1")
    else:
        monkeypatch.delenv("MI355REC_MF_GENERAL_SCHEDULE", raising=False)
    dev = MatrixFactorization_MI355X_Epoch(X, **kw)
    streams = []
    for _ in range(3):
        dev.epochIteration_Cython()
        streams.append(dev.last_epoch_samples())
    out = (dev.get_USER_factors(), dev.get_ITEM_factors(), streams)
    dev.close()
    return out


def _assert_paths_agree(X, kw, monkeypatch):
    fast = _three_epochs(X, kw, False, monkeypatch)
    general = _three_epochs(X, kw, True, monkeypatch)
    for epoch, (sa, sb) in enumerate(zip(fast[2], general[2])):
        assert len(sa[0]) > 0
        for x, y in zip(sa, sb):
            np.testing.assert_array_equal(x, y, err_msg="stream of epoch %d" % (epoch + 1))
    assert (fast[2][0][0] != fast[2][1][0]).any() and (fast[2][1][0] != fast[2][2][0]).any()      # three different epochs
    for a, b in zip(fast[:2], general[:2]):
        assert np.abs(a - b).max() <= 1e-6 * np.abs(b).max()                                     # (test_schedule_paths_agree's bar)
    return fast


# 1 and 7: more than 256 mini-batches per epoch, scheduled 256 at a time behind the stand-alone sampler; 500 .. 2730: drawn by the
# schedule's workgroups (1025 and up: more samples than threads; 2730: the last size whose 3 B incidences fit the 8 192 slots);
# 2731: back on the radix-sort schedule
@pytest.mark.parametrize("batch_size", [1, 7, 500, 1000, 1024, 1025, 2000, 2730, 2731])
def test_bpr_stream_drawn_in_the_schedule_workgroups(gpu, batch_size, monkeypatch):
    X = _urm("binary")
    kw = dict(n_factors=16, algorithm_name="MF_BPR", batch_size=batch_size, random_seed=77, sgd_mode="sgd", learning_rate=0.05,
              user_reg=0.01, positive_reg=0.01, negative_reg=0.02)
    U, V, streams = _assert_paths_agree(X, kw, monkeypatch)
    u, i, j = streams[-1]
    assert len(u) == (X.shape[0] // batch_size + 1) * batch_size                                 # .pyx:583
    assert 0 not in set(u.tolist()) and 1 not in set(u.tolist())
    assert (np.asarray(X[u, j]).ravel() == 0).all()                                              # the rejection loop did its work
    assert (np.asarray(X[u, i]).ravel() != 0).all()


# 2000 and 4096 (8 192 incidences: the largest mini-batch of the in-LDS schedule) are drawn in the workgroups; 64: 900-odd mini-batches,
# scheduled 256 at a time behind the stand-alone sampler, which must be what it was
@pytest.mark.parametrize("batch_size", [2000, 4096, 64])
def test_funk_stream_drawn_in_the_schedule_workgroups(gpu, batch_size, monkeypatch):
    X = _urm("real")
    kw = dict(n_factors=16, algorithm_name="FUNK_SVD", batch_size=batch_size, random_seed=78, sgd_mode="sgd", learning_rate=0.01,
              user_reg=0.01, item_reg=0.1, bias_reg=0.01, use_bias=True, negative_interactions_quota=0.4)
    if batch_size == 64:
        assert X.nnz // batch_size + 1 > 256
    U, V, streams = _assert_paths_agree(X, kw, monkeypatch)
    u, i, r = streams[-1]
    assert len(u) == (X.nnz // batch_size + 1) * batch_size                                      # .pyx:289
    assert 0 not in set(u.tolist()) and 1 not in set(u.tolist())
    assert (r == 0).any() and (r != 0).any()                                                     # sampled negatives and positives
    np.testing.assert_array_equal(np.asarray(X[u, i]).ravel().astype(np.float32), r)             # a negative is outside the profile


def test_epoch_counter_moves_once_per_epoch_whatever_the_launch_path(gpu):
    """The counter is advanced by the schedule's finish kernel, after every workgroup that read it has retired: three epochs in one
    call (graph replays), three calls of one epoch, and plain launches (profiling on) draw the same four streams."""
    X = _urm("binary")
    kw = dict(n_factors=16, algorithm_name="MF_BPR", batch_size=500, random_seed=5, sgd_mode="sgd", learning_rate=0.05, user_reg=0.01)
    out = []
    for variant in ("one call", "three calls", "plain launches"):
        dev = MatrixFactorization_MI355X_Epoch(X, **kw)
        if variant == "plain launches":
            dev.set_profiling(4096)
        if variant == "three calls":
            for _ in range(3):
                dev.epochIteration_Cython()
        else:
            dev.epochIteration_Cython(3)
        third = dev.last_epoch_samples()
        dev.epochIteration_Cython()
        out.append((third, dev.last_epoch_samples(), dev.get_USER_factors(), dev.get_ITEM_factors()))
        dev.close()
    for other in out[1:]:
        for x, y in zip(out[0][0] + out[0][1], other[0] + other[1]):
            np.testing.assert_array_equal(x, y)
        np.testing.assert_array_equal(out[0][2], other[2])
        np.testing.assert_array_equal(out[0][3], other[3])
    assert (out[0][0][0] != out[0][1][0]).any()                                                  # epoch 4 is not epoch 3 again


@pytest.mark.parametrize("n_batches", [31, 32, 33, 64, 65, 255, 256])
def test_version_parity_across_bitmap_words(gpu, n_batches, monkeypatch):
    """Item 0 is in every profile, so its row (and, with 40 items, most rows) is touched in nearly every mini-batch: the version a
    sample reads is the popcount over up to eight 32-bit words of the row's bitmap, with the word boundary at 32, 64, ... 256."""
    n_users, n_items = (n_batches - 1) * 4, 40
    rng = np.random.default_rng(n_batches)
    rows, cols = [], []
    for u in range(n_users):
        own = np.union1d([0], rng.choice(np.arange(1, n_items), size=int(rng.integers(1, 6)), replace=False))
        rows += [u] * len(own); cols += own.tolist()
    X = sps.csr_matrix((np.ones(len(rows), np.float32), (rows, cols)), shape=(n_users, n_items))
    X.sort_indices()
    kw = dict(n_factors=16, algorithm_name="MF_BPR", batch_size=4, random_seed=9, sgd_mode="sgd", learning_rate=0.05,
              user_reg=0.01, positive_reg=0.01, negative_reg=0.02)
    orc = O.OracleMF(X, **kw)
    init = dict(initial_USER_factors=orc.initial_USER_factors, initial_ITEM_factors=orc.initial_ITEM_factors)
    out = []
    for general in (False, True):
        if general:
            monkeypatch.setenv("MI355REC_MF_GENERAL_SCHEDULE", "1")
        dev = MatrixFactorization_MI355X_Epoch(X, **init, **kw)
        for _ in range(2):
            dev.epochIteration_Cython()
            u, i, j = dev.last_epoch_samples()
            assert len(u) == 4 * n_batches
            if not general:
                orc.replay(u, i, j=j)
        out.append((dev.get_USER_factors(), dev.get_ITEM_factors(), (u, i, j)))
        dev.close()
    for x, y in zip(out[0][2], out[1][2]):
        np.testing.assert_array_equal(x, y)
    for a, b in zip(out[0][:2], out[1][:2]):
        assert np.abs(a - b).max() <= 1e-6 * np.abs(b).max()
    assert_factor_parity(out[0][0], orc.get_USER_factors(), "U")
    assert_factor_parity(out[0][1], orc.get_ITEM_factors(), "V")
