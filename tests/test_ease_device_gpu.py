"""EASE_R_MI355X_Recommender and the MI355XEase handle on the device: accuracy against the float64 closed form, the top-K slabs, the
route (device inverse for positive-definite matrices, host inverse with the refusing step otherwise), numeric refusals at the
handle, repeatability, recommend(), and the device-resident dense output of the similarity build.  Cases: tests/ease_cases.py."""
import ctypes as C

import numpy as np
import pytest
import scipy.sparse as sps

from recsys2019_deeplearning_evaluation_amd import (Compute_Similarity_MI355X, EASE_R_MI355X_Recommender, EASE_R_Recommender,
                                                    EvaluatorHoldout_MI355X, EvaluatorNegativeItemSample_MI355X, MI355XEase, _native as N)
from recsys2019_deeplearning_evaluation_amd.recommender_base import similarityMatrixTopK
from _util import check_topk_against_dense, csr_columns_as_slabs
import ease_cases as EC

pytestmark = pytest.mark.gpu


def dense(W):
    return W.toarray() if sps.issparse(W) else W


@pytest.fixture(scope="module")
def block(gpu):
    ease = MI355XEase(3)
    try:
        return ease.fit_info()["block"]
    finally:
        ease.close()


_fits = {}


def fitted(name):
    """One fit per case, shared by the tests below (never modified)."""
    if name not in _fits:
        X, kw = dict(EC.fit_cases(), **EC.indefinite_cases())[name]
        rec = EASE_R_MI355X_Recommender(X.copy(), verbose=False)
        rec.fit(verbose=False, **kw)
        W64 = EC.weights_f64(EC.gram_f32(X, kw["l2_norm"], kw["normalize_matrix"]))
        _fits[name] = (rec, kw, W64)
    return _fits[name]


def check_fit(rec, kw, W64, name):
    n = W64.shape[0]
    W = rec.W_sparse
    got = dense(W)
    assert got.shape == (n, n) and got.dtype == np.float32 and (np.diag(got) == 0).all()
    scale = np.abs(W64).max()
    if kw["topK"] is None:
        assert isinstance(W, np.ndarray)
        err = np.abs(got - W64).max() / scale
        print("%-40s n %5d  device vs float64 %.2e (%s inverse)" % (name, n, err, rec.fit_info["inverse"]))
        assert err < EC.BAR, (name, err)
    else:
        assert sps.isspmatrix_csr(W)
        topK = min(kw["topK"], n)
        assert np.diff(W.tocsc().indptr).max() <= topK
        idx, val = csr_columns_as_slabs(W, topK)
        for c in range(n):
            check_topk_against_dense(idx[c], val[c], W64[:, c], topK, rtol=1e-4)
        kept = got != 0
        assert np.abs(got - W64)[kept].max() < EC.BAR * scale


@pytest.mark.parametrize("name", sorted(EC.fit_cases()))
def test_fit_matches_the_float64_closed_form_on_the_device_route(gpu, name):
    rec, kw, W64 = fitted(name)
    check_fit(rec, kw, W64, name)
    info = rec.fit_info
    assert info["inverse"] == "device" and info["failed_step"] == -1 and info["reason"] == ""
    assert info["block"] in (64, 128) and info["steps"] >= 1 and info["invert_ms"] > 0


def test_fixture_cases_match_the_reference(gpu):
    X, cases, stored = EC.fixture()
    for n, kw in enumerate(cases):
        rec, _, _ = fitted("fixture-%d" % n)
        got, want = dense(rec.W_sparse), stored[n]
        assert got.shape == want.shape
        if kw["topK"] is not None:
            assert ((got != 0) == (want != 0)).all(), kw
        assert np.abs(got - want).max() < EC.BAR * np.abs(want).max(), kw


@pytest.mark.parametrize("name", sorted(EC.indefinite_cases()))
def test_indefinite_matrices_take_the_host_inverse(gpu, name):
    rec, kw, W64 = fitted(name)
    info = rec.fit_info
    assert info["inverse"] == "host" and info["failed_step"] >= 0 and "positive definite" in info["reason"]
    check_fit(rec, kw, W64, name)


def test_column_slices(gpu, block):
    for n in EC.slice_sizes(block):
        X = EC.slice_urm(n)
        rec = EASE_R_MI355X_Recommender(X.copy(), verbose=False)
        rec.fit(topK=None, l2_norm=1.0, verbose=False)
        assert rec.fit_info["inverse"] == "device"
        W64 = EC.weights_f64(EC.gram_f32(X, 1.0))
        got = rec.W_sparse
        assert got.shape == (n, n) and got.dtype == np.float32 and (np.diag(got) == 0).all()
        err = np.abs(got - W64).max() / max(np.abs(W64).max(), 1e-300)
        print("slice %4d  device vs float64 %.2e" % (n, err))
        assert err < EC.BAR, (n, err)


def test_random_spd_uploads(gpu, block):
    for n in EC.random_spd_sizes(block):
        G = EC.random_spd(n)
        ease = MI355XEase(n)
        try:
            ease.set_matrix(G)
            assert (ease.get_matrix() == G).all()
            ease.invert()
            P = ease.get_matrix()
            P64 = np.linalg.inv(G.astype(np.float64))
            assert np.abs(P - P64).max() < EC.BAR * np.abs(P64).max(), n
            W, W64 = ease.get_dense(), EC.weights_from_precision(P64)
            assert (np.diag(W) == 0).all()
            if n > 1:
                err = np.abs(W - W64).max() / np.abs(W64).max()
                print("spd %4d  device vs float64 %.2e" % (n, err))
                assert err < EC.BAR, (n, err)
            info = ease.fit_info()
            assert info["steps"] == -(-n // 128) * 128 // block and info["failed_step"] == -1
        finally:
            ease.close()


def test_topk_slabs_and_host_ranking_describe_the_same_matrix(gpu):
    X = EC.urm("binary", 0.1)
    G = EC.gram_f32(X, 100.0)
    n = len(G)
    ease = MI355XEase(n)
    try:
        ease.set_matrix(G)
        ease.invert()
        W = ease.get_dense()
        for topK in (1, 50, n, n + 5):
            idx, val = ease.get_topk(topK)
            assert idx.shape == (n, topK)
            want_idx, want_val = csr_columns_as_slabs(similarityMatrixTopK(W, k=topK), topK)
            # the same values slot for slot; the rows may differ only between cells of equal value (the host's argpartition takes any
            # of the cells tied at the cut, the device the lowest rows)
            assert (val == want_val).all() and ((idx < 0) == (want_idx < 0)).all(), topK
            cols = np.broadcast_to(np.arange(n)[:, None], idx.shape)
            other = (idx != want_idx)
            assert (W[idx[other], cols[other]] == W[want_idx[other], cols[other]]).all(), topK
        with pytest.raises(NotImplementedError):
            ease.get_topk(4097)
        with pytest.raises(ValueError):
            ease.get_topk(0)
    finally:
        ease.close()


def _refused_step(ease):
    with pytest.raises(FloatingPointError) as exc:
        ease.invert()
    assert "step %d of" % ease.fit_info()["failed_step"] in str(exc.value)
    return ease.fit_info()["failed_step"]


def test_numeric_refusals_return_and_the_handle_recovers(gpu, block):
    n = 2 * 128 + 37                     # the last block is ragged
    ease = MI355XEase(n)
    try:
        for at in (5, n - 3):
            d = np.ones(n, np.float32)
            d[at] = -1.0
            ease.set_matrix(np.diag(d))
            assert _refused_step(ease) == at // block
            with pytest.raises(ValueError):
                ease.get_dense()
        G = EC.random_spd(n)
        G[7, 200] = np.nan
        ease.set_matrix(G)
        assert _refused_step(ease) >= 0
        G = EC.random_spd(n)
        ease.set_matrix(G)
        ease.invert()
        P64 = np.linalg.inv(G.astype(np.float64))
        assert np.abs(ease.get_matrix() - P64).max() < EC.BAR * np.abs(P64).max()
    finally:
        ease.close()
    ease = MI355XEase(2)
    try:
        ease.set_matrix(np.array([[0, 1], [1, 0]], np.float32))
        assert _refused_step(ease) == 0
    finally:
        ease.close()


def test_calls_out_of_order_raise_value_error(gpu):
    X = EC.urm("binary", 0.1)
    ease = MI355XEase(X.shape[1])
    sparse_builder = Compute_Similarity_MI355X(X, topK=10, shrink=0, normalize=False)
    narrow = Compute_Similarity_MI355X(sps.csr_matrix(X[:, :100]), topK=0, shrink=0, normalize=False)
    try:
        for call in (ease.get_dense, ease.invert, ease.get_matrix, lambda: ease.get_topk(5), lambda: ease.set_diagonal(np.ones(ease.n_items)),
                     lambda: ease.set_gram_from(sparse_builder), lambda: ease.set_gram_from(narrow),
                     lambda: ease.set_matrix(np.eye(3, dtype=np.float32))):
            with pytest.raises(ValueError):
                call()
        ease.set_matrix(np.eye(ease.n_items, dtype=np.float32))
        with pytest.raises(ValueError):
            ease.get_dense()
        ease.invert()
        with pytest.raises(ValueError):
            ease.invert()
        assert (ease.get_dense() == 0).all()
        lib = N.load()
        assert lib.mi355rec_ease_invert(None) == N.E_INVALID
        assert lib.mi355rec_ease_set_matrix(ease._h, None, 1) == N.E_INVALID
        assert lib.mi355rec_ease_create(None, 5) == N.E_INVALID
    finally:
        ease.close()
        sparse_builder.close()
        narrow.close()


def test_two_fits_are_bitwise_equal(gpu):
    X = EC.urm("binary", 0.3)
    out = []
    for _ in range(2):
        rec = EASE_R_MI355X_Recommender(X.copy(), verbose=False)
        rec.fit(topK=50, l2_norm=100.0, verbose=False)
        out.append(rec.W_sparse)
    a, b = out
    assert (a.indptr == b.indptr).all() and (a.indices == b.indices).all() and (a.data == b.data).all()


def test_recommend_sparse_matches_host_ranking(gpu):
    rec, kw, _ = fitted("ml1m-0.3-l2=1000-topK=50")
    X = sps.csr_matrix(rec.URM_train)
    users = np.arange(0, X.shape[0], 11)
    cutoff = 10
    lists = rec.recommend(users, cutoff=cutoff, remove_seen_flag=True)
    scores = (X[users] @ rec.W_sparse).toarray().astype(np.float64)
    compared = 0
    for u, items, row in zip(users, lists, scores):
        seen = X.indices[X.indptr[u]:X.indptr[u + 1]]
        assert len(items) == cutoff and not set(items) & set(seen)
        row[seen] = -np.inf
        order = np.argsort(-row, kind="stable")
        ranked = row[order]
        gaps = np.abs(np.diff(ranked[:cutoff + 1]))
        if gaps.min() > 1e-5 * max(abs(ranked[0]), 1e-30):           # no near-tie down to the cut
            assert list(order[:cutoff]) == list(items), u
            compared += 1
    assert compared > len(users) // 2


def test_recommend_dense_matches_the_host_class(gpu):
    rec, kw, _ = fitted("ml1m-0.1-l2=100-topK=None")
    host = EASE_R_Recommender(sps.csr_matrix(rec.URM_train).copy(), verbose=False)
    host.W_sparse = rec.W_sparse
    users = np.arange(0, rec.URM_train.shape[0], 7)
    for remove_seen in (True, False):
        assert rec.recommend(users, cutoff=8, remove_seen_flag=remove_seen) == host.recommend(users, cutoff=8, remove_seen_flag=remove_seen)
    assert rec.recommend(int(users[3]), cutoff=5) == host.recommend(int(users[3]), cutoff=5)


def test_device_evaluators_take_a_dense_w_through_the_lists_path(gpu):
    """topK=None leaves a dense W_sparse, which the sparse device scorer cannot take: both device evaluators must go through
    recommend() and give what they give for the host class holding the same W."""
    from negative_eval_cases import make_case
    case = make_case("sampled")
    train = sps.csr_matrix(case["train"], dtype=np.float32)
    rec = EASE_R_MI355X_Recommender(train.copy(), verbose=False)
    rec.fit(topK=None, l2_norm=20.0, verbose=False)
    assert isinstance(rec.W_sparse, np.ndarray) and not rec.device_scorable()
    host = EASE_R_Recommender(train.copy(), verbose=False)
    host.W_sparse = rec.W_sparse
    holdout = EvaluatorHoldout_MI355X(case["test"], case["cutoffs"], verbose=False)
    negative = EvaluatorNegativeItemSample_MI355X(case["test"], case["negative"], case["cutoffs"], verbose=False, **case["kwargs"])
    for ev in (holdout, negative):
        got, _ = ev.evaluateRecommender(rec)
        want, _ = ev.evaluateRecommender(host)
        assert got.keys() == want.keys()
        for cutoff in want:
            assert got[cutoff] == want[cutoff], (type(ev).__name__, cutoff)
        assert any(v > 0 for v in want[max(want)].values())
    # a sparse W of the same class takes the fused path again
    rec.fit(topK=30, l2_norm=20.0, verbose=False)
    assert rec.device_scorable()
    fused, _ = holdout.evaluateRecommender(rec)
    assert fused.keys() == want.keys() and any(v > 0 for v in fused[max(fused)].values())


def test_topk_beyond_the_device_selection_is_ranked_on_the_host(gpu, monkeypatch):
    """A column too long for the in-LDS selection (or topK > 4096) makes get_topk raise NotImplementedError: the fit then downloads
    the dense W and ranks it on the host.  No test matrix is that large, so the refusal is stubbed."""
    calls = []

    def refuse(self, topK):
        calls.append(topK)
        raise NotImplementedError("stub: beyond the in-LDS selection")

    monkeypatch.setattr(MI355XEase, "get_topk", refuse)
    name = "ml1m-0.1-l2=100-topK=50"
    X, kw = EC.fit_cases()[name]
    rec = EASE_R_MI355X_Recommender(X.copy(), verbose=False)
    rec.fit(verbose=False, **kw)
    assert calls == [50] and rec.fit_info["inverse"] == "device"
    check_fit(rec, kw, EC.weights_f64(EC.gram_f32(X, kw["l2_norm"])), name)


def test_create_refuses_a_matrix_that_does_not_fit(gpu):
    with pytest.raises(ValueError, match="do not fit"):
        MI355XEase(2000000)             # 16 TB: refused from the free-memory figure, nothing is allocated or launched
    with pytest.raises(ValueError):
        MI355XEase(0)


def test_dense_device_output_equals_the_downloaded_one(gpu):
    X = EC.urm("binary", 0.1)
    n = X.shape[1]
    builder = Compute_Similarity_MI355X(X, topK=0, shrink=0, normalize=False, similarity="cosine")
    try:
        want = builder.compute_similarity()                   # want[j, c] = similarity(j, c)
        for start, end, ld in ((0, n, n), (0, n, n + 24), (64, 200, n)):
            rows = end - start
            dev = N.DeviceArray(rows * ld)
            try:
                builder._call("compute_dense_device", start, end, dev.ptr, ld)
                got = dev.to_host().view(np.float32).reshape(rows, ld)
            finally:
                dev.close()
            assert (got[:, :n] == want[:, start:end].T).all(), (start, end, ld)
        with pytest.raises(ValueError):
            builder._call("compute_dense_device", 0, n, C.c_void_p(1), n - 1)
        with pytest.raises(ValueError):
            builder._call("compute_dense_device", 0, n, None, n)
    finally:
        builder.close()
