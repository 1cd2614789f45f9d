"""The pivoted float64 inverse of EASE_R on the device (csrc/ease_pivot.hip): exact cases (scaled permutation, reversal, no swaps),
distance to the float64 closed form at both block sizes, fit(indefinite="device") on explicit ratings -- dense W, top-K slabs,
recommend() lists, the device dense scorer --, the untouched positive-definite route, refusals, repeats.  Cases and the method's
NumPy restatement: tests/ease_pivoted_cases.py."""
import numpy as np
import pytest
import scipy.sparse as sps

from recsys2019_deeplearning_evaluation_amd import EASE_R_MI355X_Recommender, EASE_R_Recommender, MI355XEase
from _util import check_topk_against_dense, csr_columns_as_slabs
import ease_cases as EC
import ease_pivoted_cases as PC

pytestmark = pytest.mark.gpu

BOUND = 1e-6            # of max |W64|: the float64 elimination (<= 1e-7) and three float32 roundings per cell (1.8e-7)
FIT_NAMES = sorted(PC.fit_cases())


@pytest.fixture(params=PC.BLOCKS)
def block(request, gpu, monkeypatch):
    """Every block size the handle offers (MI355REC_EASE_BLOCK is read when a handle is created)."""
    monkeypatch.setenv("MI355REC_EASE_BLOCK", str(request.param))
    ease = MI355XEase(3)
    try:
        assert ease.fit_info()["block"] == request.param
    finally:
        ease.close()
    return request.param


def dense(W):
    return W.toarray() if sps.issparse(W) else W


def pivoted(G, then=None):
    """(inverse float32, pivot_info, then(handle)) of one matrix on a handle of its own."""
    ease = MI355XEase(len(G))
    try:
        ease.set_matrix(G)
        ease.invert(pivoted=True)
        return ease.get_matrix(), ease.pivot_info(), then(ease) if then else None
    finally:
        ease.close()


def test_a_scaled_permutation_is_inverted_exactly(block):
    G = PC.scaled_permutation()
    P, info, _ = pivoted(G)
    assert np.array_equal(P, PC.exact_inverse_f32(G))
    assert info["moved_rows"] > 0 and info["min_pivot"] == np.abs(G[G != 0]).min()
    assert info["pivot_ms"] > 0 and info["update_ms"] > 0


def test_the_reversal_matrix_is_inverted_exactly(block):
    for n in (block + 1, 2 * block + 3):
        R = PC.reversal(n)
        P, info, _ = pivoted(R)
        assert np.array_equal(P, PC.exact_inverse_f32(R)), n
        assert info["moved_rows"] == n // 2 and info["min_pivot"] == 1.0, n


def test_a_diagonally_dominant_matrix_moves_no_row(block):
    G = PC.diagonally_dominant(2 * block + 3)
    P, info, _ = pivoted(G)
    assert info["moved_rows"] == 0
    assert np.array_equal(P, PC.exact_inverse_f32(G))


def test_inverse_against_float64(block):
    for name, G in PC.all_matrices(block):
        W64 = PC.weights_f64_of(name, block)
        _, info, W = pivoted(G, then=lambda ease: ease.get_dense())
        assert W.dtype == np.float32 and W.shape == W64.shape and (np.diag(W) == 0).all()
        if len(G) == 1:
            continue
        err = np.abs(W - W64).max() / np.abs(W64).max()
        print("block %3d  %-24s n %5d  device vs float64 %.2e  (%d rows moved, min |pivot| %.3g)" % (block, name, len(G), err, info["moved_rows"],
                                                                                                   info["min_pivot"]))
        assert err <= BOUND, (name, block, err)


_fits = {}


def fitted(name, topK, **kw):
    """One fit per (case, topK, constructor keywords), shared by the tests below (never modified)."""
    key = (name, topK) + tuple(sorted(kw.items()))
    if key not in _fits:
        X, fit_kw = PC.fit_cases()[name]
        rec = EASE_R_MI355X_Recommender(X.copy(), verbose=False, **kw)
        rec.fit(verbose=False, **dict(fit_kw, topK=topK))
        _fits[key] = rec
    return _fits[key]


def w64_of(name):
    return PC.weights_f64_of(name, PC.BLOCKS[-1])           # (the same matrix under either block size)


@pytest.mark.parametrize("name", FIT_NAMES)
def test_fit_takes_the_pivoted_device_inverse(gpu, name):
    rec = fitted(name, None, indefinite="device")
    info = rec.fit_info
    assert info["inverse"] == "device-pivoted" and "positive definite" in info["reason"]
    assert info["failed_step"] == -1 and info["unpivoted_failed_step"] >= 0 and info["unpivoted_s"] > 0
    assert set(info["pivot"]) == {"moved_rows", "min_pivot", "pivot_ms", "update_ms"} and info["pivot"]["min_pivot"] > 0
    assert info["block"] in PC.BLOCKS and info["invert_ms"] > 0 and info["scoring"] == "host"
    W, W64 = rec.W_sparse, w64_of(name)
    assert isinstance(W, np.ndarray) and W.dtype == np.float32 and W.shape == W64.shape and (np.diag(W) == 0).all()
    err = np.abs(W - W64).max() / np.abs(W64).max()
    print("%-24s n %5d  fit vs float64 %.2e  pivot %s" % (name, len(W), err, info["pivot"]))
    assert err <= BOUND, (name, err)


@pytest.mark.parametrize("name", FIT_NAMES)
def test_fit_top_50(gpu, name):
    rec = fitted(name, 50, indefinite="device")
    assert rec.fit_info["inverse"] == "device-pivoted"
    W, W64 = rec.W_sparse, w64_of(name)
    n = len(W64)
    topK = min(50, n)
    assert sps.isspmatrix_csr(W) and np.diff(W.tocsc().indptr).max() <= topK
    idx, val = csr_columns_as_slabs(W, topK)
    for c in range(n):
        check_topk_against_dense(idx[c], val[c], W64[:, c], topK, rtol=1e-4)
    got = W.toarray()
    kept = got != 0
    assert np.abs(got - W64)[kept].max() <= BOUND * np.abs(W64).max()


@pytest.mark.parametrize("name", FIT_NAMES)
def test_recommend_lists_equal_the_host_route_where_no_near_tie_crosses_the_cut(gpu, name):
    rec, host = fitted(name, 50, indefinite="device"), fitted(name, 50)
    assert host.fit_info["inverse"] == "host" and rec.device_scorable()
    X = sps.csr_matrix(rec.URM_train)
    users = np.arange(0, X.shape[0], 11 if X.shape[0] > 500 else 1)
    cutoff = 10 if X.shape[1] > 100 else 5
    lists = rec.recommend(users, cutoff=cutoff, remove_seen_flag=True)
    host_lists = host.recommend(users, cutoff=cutoff, remove_seen_flag=True)
    scores = (X[users] @ rec.W_sparse).toarray().astype(np.float64)
    host_scores = (X[users] @ host.W_sparse).toarray().astype(np.float64)
    compared = 0
    for u, items, host_items, row, host_row in zip(users, lists, host_lists, scores, host_scores):
        seen = X.indices[X.indptr[u]:X.indptr[u + 1]]
        assert len(items) == cutoff and not set(items) & set(seen)
        row[seen] = -np.inf
        host_row[seen] = -np.inf
        order = np.argsort(-row, kind="stable")
        ranked = row[order]
        gaps = np.abs(np.diff(ranked[:cutoff + 1]))
        # no near-tie down to the cut, and the two routes' scores -- two float32 W's, each within 1e-6 of W64 -- closer than the gaps
        head = order[:cutoff + 1]
        if gaps.min() > 1e-5 * max(abs(ranked[0]), 1e-30) and np.abs(row[head] - host_row[head]).max() < gaps.min() / 2:
            assert list(order[:cutoff]) == list(items) == list(host_items), u
            compared += 1
    assert compared > len(users) // 2


@pytest.mark.parametrize("name", FIT_NAMES)
def test_the_device_dense_scorer_takes_the_pivoted_weights(gpu, name):
    rec = fitted(name, None, indefinite="device", dense_scoring="device")
    assert rec.fit_info["inverse"] == "device-pivoted" and rec.fit_info["scoring"] == "device" and rec.dense_device_scorable()
    assert (rec.W_sparse == fitted(name, None, indefinite="device").W_sparse).all()
    host = EASE_R_Recommender(sps.csr_matrix(rec.URM_train).copy(), verbose=False)
    host.W_sparse = rec.W_sparse
    users = np.arange(0, rec.URM_train.shape[0], 7)
    for remove_seen in (True, False):
        assert rec.recommend(users, cutoff=8, remove_seen_flag=remove_seen) == host.recommend(users, cutoff=8, remove_seen_flag=remove_seen)


def test_positive_definite_input_keeps_the_unpivoted_route(gpu):
    X, kw = EC.fit_cases()["ml1m-0.1-l2=100-topK=None"]
    out = []
    for indefinite in ("device", "host"):
        rec = EASE_R_MI355X_Recommender(X.copy(), verbose=False, indefinite=indefinite)
        rec.fit(verbose=False, **kw)
        assert rec.fit_info["inverse"] == "device" and rec.fit_info["reason"] == "" and "pivot" not in rec.fit_info
        out.append(rec.W_sparse)
    assert out[0].dtype == np.float32 and np.array_equal(out[0], out[1])


def test_a_singular_pivoted_fit_ends_on_the_host(gpu):
    """An item nobody rated with l2 = 0: a zero row and column.  Both device eliminations refuse; the fit ends where the default ends
    (the host inverse raises for this matrix, as it does on the default route)."""
    X = sps.csr_matrix(EC.fixture()[0], dtype=np.float32).tolil()
    X[:, 3] = 0
    X = sps.csr_matrix(X)
    X.eliminate_zeros()
    for indefinite in ("device", "host"):
        rec = EASE_R_MI355X_Recommender(X.copy(), verbose=False, indefinite=indefinite)
        with pytest.raises(np.linalg.LinAlgError):
            rec.fit(topK=None, l2_norm=0.0, verbose=False)


@pytest.mark.parametrize("refusal", [FloatingPointError("stub: the matrix is singular"), NotImplementedError("stub: no device memory")])
def test_a_pivoted_inverse_that_refuses_ends_on_the_host_with_both_reasons(gpu, monkeypatch, refusal):
    """No test matrix is too large for the float64 copy, and a singular Gram matrix fails on the host too, so the refusal is stubbed."""
    real = MI355XEase.invert

    def invert(self, pivoted=False):
        if pivoted:
            raise refusal
        return real(self)

    monkeypatch.setattr(MI355XEase, "invert", invert)
    name = FIT_NAMES[0]
    X, kw = PC.fit_cases()[name]
    rec = EASE_R_MI355X_Recommender(X.copy(), verbose=False, indefinite="device")
    rec.fit(verbose=False, **kw)
    info = rec.fit_info
    assert info["inverse"] == "host" and info["failed_step"] >= 0 and "positive definite" in info["reason"]
    assert info["pivoted_reason"] == str(refusal) and "pivot" not in info and info["unpivoted_s"] > 0
    default = fitted(name, kw["topK"])
    assert default.fit_info["inverse"] == "host" and np.array_equal(dense(rec.W_sparse), dense(default.W_sparse))


def test_a_working_matrix_that_does_not_fit_is_refused_and_the_fit_ends_on_the_host(gpu, monkeypatch):
    """MI355REC_EASE_PIVOT_MAX_BYTES below the float64 working matrix: the refusal the library gives when the device has no room, on
    the library's own path."""
    monkeypatch.setenv("MI355REC_EASE_PIVOT_MAX_BYTES", "1000")
    G = PC.random_symmetric(131)
    ease = MI355XEase(len(G))
    try:
        ease.set_matrix(G)
        with pytest.raises(NotImplementedError, match="no device memory"):
            ease.invert(pivoted=True)
        assert np.array_equal(ease.get_matrix(), G)         # untouched, and still to be inverted
        with pytest.raises(ValueError):
            ease.pivot_info()
        monkeypatch.delenv("MI355REC_EASE_PIVOT_MAX_BYTES")
        ease.invert(pivoted=True)                           # the same handle, once there is room
        P64 = np.linalg.inv(G.astype(np.float64))
        assert np.abs(ease.get_matrix() - P64).max() <= BOUND * np.abs(P64).max()
    finally:
        ease.close()
    monkeypatch.setenv("MI355REC_EASE_PIVOT_MAX_BYTES", "1000")
    name = FIT_NAMES[1]
    X, kw = PC.fit_cases()[name]
    rec = EASE_R_MI355X_Recommender(X.copy(), verbose=False, indefinite="device")
    rec.fit(verbose=False, **kw)
    info = rec.fit_info
    assert info["inverse"] == "host" and info["failed_step"] >= 0 and "positive definite" in info["reason"]
    assert "no device memory" in info["pivoted_reason"] and "pivot" not in info
    W64 = w64_of(name)
    assert np.abs(dense(rec.W_sparse) - W64).max() <= BOUND * np.abs(W64).max()


def test_a_nan_is_refused_at_its_column_even_beside_an_infinity(block):
    n = block + 9
    G = PC.random_symmetric(n).copy()
    G[5, 2] = np.inf                                        # a lower row than the NaN's, in the same column of the first panel
    G[9, 2] = np.nan
    with pytest.raises(FloatingPointError):
        PC.pivoted_inverse_f64(G, block)
    ease = MI355XEase(n)
    try:
        ease.set_matrix(G)
        with pytest.raises(FloatingPointError, match="singular"):
            ease.invert(pivoted=True)
        assert ease.fit_info()["failed_step"] == 0
    finally:
        ease.close()


def test_refusals_return_and_the_handle_recovers(block):
    n = 2 * block + 37                      # the last block is ragged
    ease = MI355XEase(n)
    try:
        with pytest.raises(ValueError):
            ease.invert(pivoted=True)       # nothing has been set
        with pytest.raises(ValueError):
            ease.pivot_info()
        for at in (0, block + 5, n - 1):
            G = PC.random_symmetric(n).copy()
            G[:, at] = 0.0
            ease.set_matrix(G)
            with pytest.raises(FloatingPointError, match="singular") as exc:
                ease.invert(pivoted=True)
            step = ease.fit_info()["failed_step"]
            assert step == at // block and "step %d of" % step in str(exc.value)
            for call in (ease.get_dense, lambda: ease.invert(pivoted=True), ease.invert):
                with pytest.raises(ValueError):
                    call()
        G = PC.random_symmetric(n).copy()
        G[7, block + 9] = np.nan
        ease.set_matrix(G)
        with pytest.raises(FloatingPointError, match="singular"):
            ease.invert(pivoted=True)
        G = PC.random_symmetric(n)
        out = []
        for _ in range(2):
            ease.set_matrix(G)
            ease.invert(pivoted=True)
            out.append(ease.get_matrix())
            with pytest.raises(ValueError):
                ease.invert(pivoted=True)   # already inverted
        assert np.array_equal(out[0], out[1])
        P64 = np.linalg.inv(G.astype(np.float64))
        assert np.abs(out[0] - P64).max() <= BOUND * np.abs(P64).max()
        assert ease.pivot_info()["moved_rows"] > 0
        # the unpivoted route on the same handle is what it was
        S = EC.random_spd(n)
        ease.set_matrix(S)
        with pytest.raises(ValueError):
            ease.pivot_info()               # (of the matrix that is set: no pivoted inverse has run on it)
        ease.invert()
        P64 = np.linalg.inv(S.astype(np.float64))
        assert np.abs(ease.get_matrix() - P64).max() < EC.BAR * np.abs(P64).max()
    finally:
        ease.close()


def test_two_pivoted_fits_are_bitwise_equal(gpu):
    name = FIT_NAMES[-1]
    first = fitted(name, None, indefinite="device")
    X, kw = PC.fit_cases()[name]
    again = EASE_R_MI355X_Recommender(X.copy(), verbose=False, indefinite="device")
    again.fit(verbose=False, **dict(kw, topK=None))
    assert again.fit_info["inverse"] == "device-pivoted" and np.array_equal(first.W_sparse, again.W_sparse)
    assert again.fit_info["pivot"]["moved_rows"] == first.fit_info["pivot"]["moved_rows"]
    assert again.fit_info["pivot"]["min_pivot"] == first.fit_info["pivot"]["min_pivot"]
