"""Host model of the device sample stream -- TEST INFRASTRUCTURE ONLY.

A plain NumPy restatement of csrc/sampling.cuh (mix64, draw32, bounded, profile_lacks, sample_bpr) and of mf_draw_sample
(csrc/mf_core.cuh), written from the device text and never calling into the native library.  The stream is stateless: sample `sid`
is a pure function of (seed, sid, URM), all of it 64-bit unsigned integer arithmetic with wrap-around, apart from one float32
compare for the FunkSVD quota.  So this model reproduces the device bit for bit, and the device tests compare with exact equality
(tests/test_device_sampler_gpu.py); the statistics of the rule are tested on the CPU against this model
(tests/test_device_sampler_spec.py).

The stream
    draw32(seed, sid, d) = high 32 bits of mix64(seed ^ mix64(sid * 0xD1B54A32D192ED03 + d))         d = 0, 1, 2, ... per sample
    bounded(r, n)        = (r * n) >> 32
    user:     bounded(draw, n_users), drawn again while the profile is empty or full      (sampleBPR_Cython / sampleMSE_Cython)
    BPR:      i = row[bounded(draw, n_seen)];  j = bounded(draw, n_items), drawn again while j is in the profile
    MSE:      if quota != 0, one draw r decides: POSITIVE when float32(r) * 2^-32 <= float32(quota)  (the reference's "(sic)" reading)
              positive: i = row[bounded(draw, n_seen)], rating = the stored value;  negative: i by rejection, rating = 0

Epochs
    sid = epoch * samples_per_epoch + t, in 64 bits.  A handle's FIRST native epoch carries epoch number 0 (MfState::epoch and
    mi355rec_slim::epochs_done start at zero and move once per native epoch); a replay_samples call between two native epochs moves
    neither counter, for MF and for SLIM alike.
"""
import numpy as np
import scipy.sparse as sps

_U64 = np.uint64
_GOLDEN = _U64(0x9E3779B97F4A7C15)
_MUL_A = _U64(0xBF58476D1CE4E5B9)
_MUL_B = _U64(0x94D049BB133111EB)
_SID_MUL = _U64(0xD1B54A32D192ED03)
_S30, _S27, _S31, _S32 = _U64(30), _U64(27), _U64(31), _U64(32)


def _u64(x):
    """x (Python ints up to 2**64 - 1, or an integer array) as a uint64 ARRAY: array arithmetic wraps silently, scalars warn."""
    if isinstance(x, np.ndarray):
        return x.astype(np.uint64, copy=False)
    if isinstance(x, (int, np.integer)):
        return np.array([int(x) & 0xFFFFFFFFFFFFFFFF], dtype=np.uint64)
    return np.array([int(v) & 0xFFFFFFFFFFFFFFFF for v in x], dtype=np.uint64)


def mix64(x):
    """SplitMix64's output function of state x (the increment included), wrap-around uint64."""
    x = _u64(x) + _GOLDEN
    x = (x ^ (x >> _S30)) * _MUL_A
    x = (x ^ (x >> _S27)) * _MUL_B
    return x ^ (x >> _S31)


def draw32(seed, sid, d):
    """Draw number d of sample sid: a uint64 array of values below 2**32."""
    return mix64(_u64(seed) ^ mix64(_u64(sid) * _SID_MUL + _u64(d))) >> _S32


def bounded(r, n):
    """(r * n) >> 32 for r < 2**32 and 0 < n < 2**31: an int64 array of values in [0, n)."""
    return ((_u64(r) * _u64(n)) >> _S32).astype(np.int64)


class _Profiles:
    def __init__(self, X):
        X = sps.csr_matrix(X)
        if not X.has_sorted_indices:
            X = X.sorted_indices()
        self.n_users, self.n_items = X.shape
        self.indptr = np.asarray(X.indptr, dtype=np.int64)
        self.indices = np.asarray(X.indices, dtype=np.int64)
        self.data = np.asarray(X.data, dtype=np.float32)
        self.lens = np.diff(self.indptr)
        # (user, item) of every stored cell as one sorted key: profile_lacks is a binary search of it
        self.keys = np.repeat(np.arange(self.n_users, dtype=np.int64), self.lens) * self.n_items + self.indices
        assert (np.diff(self.keys) > 0).all(), "profiles must be sorted and free of duplicates"

    def lacks(self, u, item):
        key = u * self.n_items + item
        at = np.searchsorted(self.keys, key)
        return (at == len(self.keys)) | (self.keys[np.minimum(at, len(self.keys) - 1)] != key)

    def draw_user(self, seed, sid, d):
        """The user draw, repeated while the profile is empty or full.  Advances d in place."""
        u = np.empty(len(sid), dtype=np.int64)
        todo = np.arange(len(sid))
        while len(todo):
            cand = bounded(draw32(seed, sid[todo], d[todo]), self.n_users)
            d[todo] += _U64(1)
            u[todo] = cand
            n_seen = self.lens[cand]
            todo = todo[(n_seen == 0) | (n_seen == self.n_items)]
        return u

    def draw_outside(self, seed, sid, d, u, first_draw=None):
        """An item outside u's profile by rejection.  Advances d in place.  `first_draw` (tests only): the index of the draw the
        first attempt takes instead of a fresh one."""
        item = np.empty(len(sid), dtype=np.int64)
        todo = np.arange(len(sid))
        first = first_draw is not None
        while len(todo):
            if first:
                cand = bounded(draw32(seed, sid[todo], first_draw[todo]), self.n_items)
                first = False
            else:
                cand = bounded(draw32(seed, sid[todo], d[todo]), self.n_items)
                d[todo] += _U64(1)
            item[todo] = cand
            todo = todo[~self.lacks(u[todo], cand)]
        return item


def _profiles(X):
    return X if isinstance(X, _Profiles) else _Profiles(X)


def bpr_sample(X, seed, sid):
    """sample_bpr / the BPR branch of mf_draw_sample for every sample id in `sid`: (u, i, j, draws_used), int32 ids."""
    P = _profiles(X)
    sid = _u64(sid)
    d = np.zeros(len(sid), dtype=np.uint64)
    u = P.draw_user(seed, sid, d)
    i = P.indices[P.indptr[u] + bounded(draw32(seed, sid, d), P.lens[u])]
    d += _U64(1)
    j = P.draw_outside(seed, sid, d, u)
    return u.astype(np.int32), i.astype(np.int32), j.astype(np.int32), d.astype(np.int64)


def mse_sample(X, seed, sid, quota):
    """The FunkSVD / AsySVD branch of mf_draw_sample: (u, i, rating), rating float32 (0 for a sampled negative)."""
    P = _profiles(X)
    sid = _u64(sid)
    d = np.zeros(len(sid), dtype=np.uint64)
    u = P.draw_user(seed, sid, d)
    positive = np.ones(len(sid), dtype=bool)
    if quota != 0.0:           # (the draw is consumed only then)
        r = draw32(seed, sid, d).astype(np.float32)                          # exact below 2**24, round-to-nearest-even above
        positive = r * np.float32(2.0 ** -32) <= np.float32(quota)           # the compare in float32, as the kernel does it
        d += _U64(1)
    item = np.empty(len(sid), dtype=np.int64)
    rating = np.zeros(len(sid), dtype=np.float32)
    pos = np.flatnonzero(positive)
    at = P.indptr[u[pos]] + bounded(draw32(seed, sid[pos], d[pos]), P.lens[u[pos]])
    item[pos] = P.indices[at]
    rating[pos] = P.data[at]
    neg = np.flatnonzero(~positive)
    d_neg = d[neg]
    item[neg] = P.draw_outside(seed, sid[neg], d_neg, u[neg])
    return u.astype(np.int32), item.astype(np.int32), rating


def mf_samples_per_epoch(X, algorithm, batch_size):
    """batches_per_epoch (mf.hip) times the batch size: MF_BPR n_users // B + 1 mini-batches, FUNK_SVD nnz // B + 1, ASY_SVD
    nnz // 1 + 1 single-sample steps (its batch size is 1)."""
    P = _profiles(X)
    B = int(batch_size)
    if algorithm == "ASY_SVD":
        assert B == 1
    per_epoch = (P.n_users // B if algorithm == "MF_BPR" else int(P.indptr[-1]) // B) + 1
    return per_epoch * B


def _epoch_sids(epoch, n):
    return np.array([(int(epoch) * n) & 0xFFFFFFFFFFFFFFFF], dtype=np.uint64) + np.arange(n, dtype=np.uint64)


def mf_epoch_stream(X, algorithm, batch_size, seed, epoch, quota=0.0):
    """The stream of native epoch `epoch` (the first one of a handle is epoch 0) of a MatrixFactorization_MI355X_Epoch:
    (u, i, j) for MF_BPR, (u, i, rating) for FUNK_SVD and ASY_SVD."""
    assert algorithm in ("MF_BPR", "FUNK_SVD", "ASY_SVD")
    P = _profiles(X)
    sid = _epoch_sids(epoch, mf_samples_per_epoch(P, algorithm, batch_size))
    if algorithm == "MF_BPR":
        return bpr_sample(P, seed, sid)[:3]
    return mse_sample(P, seed, sid, quota)


def slim_epoch_stream(X, seed, epoch):
    """The stream of native epoch `epoch` (the first one is epoch 0) of a SLIM_BPR_MI355X_Epoch: n_users + 1 steps."""
    P = _profiles(X)
    return bpr_sample(P, seed, _epoch_sids(epoch, P.n_users + 1))[:3]
