"""MI355XDenseScorer and EASE_R_MI355X_Recommender(dense_scoring="device") on the device: scores bit-equal to SciPy's csr @ ndarray,
lists exactly the ranking contract's (value descending, ties towards the lower item id, -1 padded), at the boundaries of the
kernel's column tile, on the in-LDS and the wide ranking route, for full rows and for candidate rows; then both device evaluators
through the fused dense path against their lists path.  No tolerance anywhere.  Models: tests/dense_score_cases.py."""
import numpy as np
import pytest
import scipy.sparse as sps

from recsys2019_deeplearning_evaluation_amd import (EASE_R_MI355X_Recommender, EASE_R_Recommender, EvaluatorHoldout_MI355X,
                                                    EvaluatorNegativeItemSample_MI355X, MI355XDenseScorer, MI355XEase)
from recsys2019_deeplearning_evaluation_amd import _native as N
from recsys2019_deeplearning_evaluation_amd import recommender_base as RB
from test_evaluation_gpu import _bitwise_equal
import dense_score_cases as DC
import ranking_cases as RC

pytestmark = pytest.mark.gpu
CUTOFF = 10
_built = {}


def built(name):
    """One scorer and one SciPy product per shape, shared by the tests below (never modified)."""
    if name not in _built:
        m = DC.model(name)
        product = np.asarray(m["X"][m["users"]] @ m["W"])
        _built[name] = (m, product, MI355XDenseScorer(m["X"], m["W"], m["seen"]))
    return _built[name]


def some_mask(n_out, seed):
    allowed = (np.random.default_rng(seed).random(n_out) < 0.7).astype(np.uint8)
    allowed[:2] = (0, 1)
    return allowed


@pytest.mark.parametrize("masked", [False, True])
@pytest.mark.parametrize("remove_seen", [True, False])
@pytest.mark.parametrize("name", sorted(DC.shapes()))
def test_scores_are_the_scipy_product_and_lists_are_exact(gpu, name, remove_seen, masked):
    m, product, scorer = built(name)
    n_out = product.shape[1]
    allowed = some_mask(n_out, 5) if masked else None
    cutoff = min(CUTOFF, n_out)
    ranked, scores = scorer.recommend(m["users"], cutoff, remove_seen, allowed, return_scores=True)
    want = RC.apply_filters(product, m["seen"], m["users"], remove_seen, allowed)
    assert scores.dtype == np.float32 and np.array_equal(scores, want)
    assert np.array_equal(ranked, RC.exact_rankings(want, cutoff))
    if not remove_seen and not masked:              # the empty profile: every score +0.0, the list is the lowest ids
        assert np.array_equal(ranked[DC.EMPTY_USER], np.arange(cutoff))
        assert not np.signbit(scores[DC.EMPTY_USER]).any()


@pytest.mark.parametrize("name", ["n5", "tile_plus_1", "wide"])
def test_a_cutoff_beyond_the_admissible_items_is_padded(gpu, name):
    m, product, scorer = built(name)
    n_out = product.shape[1]
    allowed = np.zeros(n_out, np.uint8)
    allowed[[0, n_out // 2, n_out - 1]] = 1
    cutoff = min(CUTOFF, n_out)
    ranked, _ = scorer.recommend(m["users"], cutoff, True, allowed)
    want = RC.exact_rankings(RC.apply_filters(product, m["seen"], m["users"], True, allowed), cutoff)
    assert np.array_equal(ranked, want) and (ranked[:, 3:] == -1).all()


@pytest.mark.parametrize("name", ["two_tiles_plus_3", "wide"])
def test_calls_repeat_bit_for_bit_and_blocks_can_be_split(gpu, name):
    m, product, scorer = built(name)
    users = m["users"]
    first = scorer.recommend(users, CUTOFF, True, None, return_scores=True)
    again = scorer.recommend(users, CUTOFF, True, None, return_scores=True)
    assert first[0].tobytes() == again[0].tobytes() and first[1].tobytes() == again[1].tobytes()
    parts = [scorer.recommend(users[a:b], CUTOFF, True, None, return_scores=True) for a, b in ((0, 1), (1, 8), (8, len(users)))]
    assert np.concatenate([p[0] for p in parts]).tobytes() == first[0].tobytes()
    assert np.concatenate([p[1] for p in parts]).tobytes() == first[1].tobytes()
    shuffled = users[::-1].copy()
    back = scorer.recommend(shuffled, CUTOFF, True, None, return_scores=True)
    assert back[0][::-1].tobytes() == first[0].tobytes() and back[1][::-1].tobytes() == first[1].tobytes()
    stats = scorer.stats()
    nnz = np.diff(m["X"].indptr)[users].sum()
    assert stats["n_units"] == len(users) and stats["algorithmic_bytes"] == 4.0 * nnz * product.shape[1]
    assert stats["kernel_ms"] > 0 and stats["call_ms"] > 0


@pytest.mark.parametrize("name", ["tile_plus_1", "wide"])
@pytest.mark.parametrize("remove_seen", [True, False])
def test_candidate_scores_are_the_cells_of_the_full_row(gpu, name, remove_seen):
    m, product, scorer = built(name)
    users, n_out = m["users"], product.shape[1]
    rng = np.random.default_rng(11)
    lengths = [1, 64, 65, 300] * 3
    rows = sps.lil_matrix((len(users), n_out), dtype=np.float32)
    for r in range(len(users)):
        picked = rng.choice(n_out, lengths[r], replace=False)
        if remove_seen and lengths[r] > 1:          # some seen items among the candidates
            seen = m["seen"].indices[m["seen"].indptr[users[r]]:m["seen"].indptr[users[r] + 1]]
            picked = np.union1d(picked[:lengths[r] - min(3, len(seen))], seen[:3])
        rows[r, picked] = 1
    rows = sps.csr_matrix(rows)
    assert remove_seen or {1, 64, 65, 300} == set(np.diff(rows.indptr).tolist())
    want = np.full(product.shape, -np.inf, np.float32)
    mask = rows.toarray() != 0
    want[mask] = RC.apply_filters(product, m["seen"], users, remove_seen)[mask]
    for cutoff in (5, 100):
        ranked = scorer.recommend_candidates(users, rows, cutoff, remove_seen)
        assert np.array_equal(ranked, RC.exact_rankings(want, cutoff)), cutoff
    allowed = some_mask(n_out, 6)
    ranked = scorer.recommend_candidates(users, rows, 20, remove_seen, allowed)
    want[:, allowed == 0] = -np.inf
    assert np.array_equal(ranked, RC.exact_rankings(want, 20))


def test_update_is_seen_by_the_next_call(gpu):
    m = DC.model("tile_minus_1")
    other = np.ascontiguousarray(-m["W"][::-1])
    scorer = MI355XDenseScorer(m["X"], m["W"], m["seen"])
    try:
        before = scorer.recommend(m["users"], CUTOFF, False, None, return_scores=True)[1]
        scorer.update(other)
        after = scorer.recommend(m["users"], CUTOFF, False, None, return_scores=True)[1]
        assert np.array_equal(before, np.asarray(m["X"] @ m["W"])) and np.array_equal(after, np.asarray(m["X"] @ other))
        assert not np.array_equal(before, after)
        with pytest.raises(ValueError):
            scorer.update(other[:, :-1])
        # zero weights until they are set
        empty = MI355XDenseScorer(m["X"], m["W"].shape, m["seen"])
        try:
            assert not empty.recommend(m["users"], CUTOFF, False, None, return_scores=True)[1].any()
            empty.update(other)
            assert np.array_equal(empty.recommend(m["users"], CUTOFF, False, None, return_scores=True)[1], after)
        finally:
            empty.close()
    finally:
        scorer.close()


def test_weights_taken_from_an_ease_handle_are_the_downloaded_ones(gpu):
    """130 items: the EASE handle's rows have a pitch of 256 cells, the scorer's of 132."""
    n = 130
    rng = np.random.default_rng(3)
    X = sps.random(60, n, 0.2, format="csr", dtype=np.float32, random_state=4)
    X.data[:] = rng.integers(1, 6, X.nnz)
    G = np.asarray((X.T @ X).todense(), dtype=np.float32) + 50 * np.eye(n, dtype=np.float32)
    users = np.arange(60, dtype=np.int32)
    ease = MI355XEase(n)
    try:
        ease.set_matrix(G)
        ease.invert()
        a = MI355XDenseScorer(X, (n, n), X)
        try:
            a.set_weights_from(ease)            # (before get_dense: the weights are scaled in place by whoever asks first)
            W = ease.get_dense()
            b = MI355XDenseScorer(X, W, X)
            try:
                got = a.recommend(users, CUTOFF, True, None, return_scores=True)
                want = b.recommend(users, CUTOFF, True, None, return_scores=True)
                assert got[1].tobytes() == want[1].tobytes() and got[0].tobytes() == want[0].tobytes()
                assert np.array_equal(got[1], RC.apply_filters(np.asarray(X @ W), X, users))
                assert (np.diag(W) == 0).all() and np.abs(W).max() > 0
            finally:
                b.close()
            wrong = MI355XDenseScorer(X[:, :n - 1], (n - 1, n - 1), X[:, :n - 1])
            try:
                with pytest.raises(ValueError, match="130 x 130"):
                    wrong.set_weights_from(ease)
            finally:
                wrong.close()
        finally:
            a.close()
    finally:
        ease.close()


def test_refusals_come_before_any_launch(gpu):
    m, product, scorer = built("n5")
    with pytest.raises(ValueError, match="user id 12 out of range"):
        scorer.recommend(np.array([1, 12]), 3)
    with pytest.raises(ValueError, match="user id -1 out of range"):
        scorer.recommend_candidates(np.array([-1]), sps.csr_matrix(np.ones((1, 5), np.float32)), 3)
    with pytest.raises(ValueError, match="cutoff"):
        scorer._call("recommend", N.ptr(m["users"]), 2, 6, 0, None, N.ptr(np.empty((2, 6), np.int32)), None)
    # 2^20 x 2^18 floats = 1.1 TB: refused from the free-memory figure
    n_mid, n_out = 1 << 20, 1 << 18
    A = sps.csr_matrix(([1.0], ([0], [n_mid - 1])), shape=(2, n_mid), dtype=np.float32)
    seen = sps.csr_matrix((2, n_out), dtype=np.float32)
    with pytest.raises(ValueError, match="do not fit"):
        MI355XDenseScorer(A, (n_mid, n_out), seen)
    # a column id is an address: checked on the host
    bad = sps.csr_matrix(([1.0], [7], [0, 1, 1]), shape=(2, 8), dtype=np.float32)
    bad.indices[0] = 8
    with pytest.raises(ValueError, match="profile column id 8"):
        MI355XDenseScorer(bad, (8, 16), sps.csr_matrix((2, 16), dtype=np.float32))


# ------------------------------------------------------------------------------------------------------------ end to end
class _ExactLists(RB.BaseRecommender):
    """The lists path fed with the ranking contract's lists of the HOST scores of a recommender."""

    def __init__(self, host):
        super().__init__(host.URM_train, verbose=False)
        self._host = host

    def recommend(self, user_id_array, cutoff=None, remove_seen_flag=True, items_to_compute=None, remove_top_pop_flag=False,
                  remove_custom_items_flag=False, return_scores=False):
        assert not remove_top_pop_flag and not remove_custom_items_flag and not return_scores
        users = np.atleast_1d(user_id_array)
        scores = np.asarray(self._host._compute_item_score(users, items_to_compute=items_to_compute), dtype=np.float32)
        X = sps.csr_matrix(self.URM_train)
        ranked = RC.exact_rankings(RC.apply_filters(scores, X, users, remove_seen_flag), min(cutoff, scores.shape[1]))
        return [row[row >= 0].tolist() for row in ranked]


@pytest.fixture(scope="module")
def fitted(gpu):
    from negative_eval_cases import make_case
    case = make_case("sampled")
    train = sps.csr_matrix(case["train"], dtype=np.float32)
    rec = EASE_R_MI355X_Recommender(train.copy(), verbose=False, dense_scoring="device")
    rec.fit(topK=None, l2_norm=20.0, verbose=False)
    return case, train, rec


def _host_of(rec, train):
    host = EASE_R_Recommender(train.copy(), verbose=False)
    host.W_sparse = rec.W_sparse
    return host


def _evaluators(case):
    return (EvaluatorHoldout_MI355X(case["test"], case["cutoffs"], verbose=False),
            EvaluatorNegativeItemSample_MI355X(case["test"], case["negative"], case["cutoffs"], verbose=False, **case["kwargs"]))


def _same_evaluation(ev, rec, other):
    got, got_text = ev.evaluateRecommender(rec)
    got_users = ev.per_user_values()
    want, want_text = ev.evaluateRecommender(other)
    want_users = ev.per_user_values()
    _bitwise_equal(got, want)
    assert got_text == want_text
    for cutoff in want_users:
        for metric, values in want_users[cutoff].items():
            assert np.array_equal(got_users[cutoff][metric], values), (cutoff, metric)
    assert any(v > 0 for v in want[max(want)].values())
    return got


def test_the_fitted_recommender_is_scored_on_the_device(fitted):
    case, train, rec = fitted
    assert rec.fit_info["scoring"] == "device" and rec.fit_info["inverse"] == "device"
    assert isinstance(rec.W_sparse, np.ndarray) and rec.dense_device_scorable() and not rec.device_scorable()
    assert rec._dense_scorer is not None and rec._dense_scorer_src["W"] is rec.W_sparse       # filled by fit, from the EASE handle
    scorer = rec._dense_scorer
    host = _host_of(rec, train)
    users = np.arange(0, train.shape[0], 7)
    for remove_seen in (True, False):
        lists, scores = rec.recommend(users, cutoff=8, remove_seen_flag=remove_seen, return_scores=True)
        want = RC.apply_filters(np.asarray(host._compute_item_score(users)), train, users, remove_seen)
        assert np.array_equal(scores, want)
        assert lists == [row[row >= 0].tolist() for row in RC.exact_rankings(want, 8)]
    assert rec._dense_scorer is scorer              # (no rebuild, no upload: the cache recognises what fit left)
    assert rec.recommend(int(users[3]), cutoff=5) == RC.exact_ranking(RC.apply_filters(
        np.asarray(host._compute_item_score(users[3:4])), train, users[3:4])[0], 5).tolist()


def test_both_evaluators_give_what_their_lists_path_gives(fitted):
    case, train, rec = fitted
    exact = _ExactLists(_host_of(rec, train))
    for ev in _evaluators(case):
        fused = _same_evaluation(ev, rec, exact)
        # whatever the block size
        again, _ = ev.evaluateRecommender(rec, block_size=37)
        _bitwise_equal(again, fused)


def test_a_second_fit_a_sparse_fit_and_the_default_class(gpu):
    from negative_eval_cases import make_case
    case = make_case("sampled")
    train = sps.csr_matrix(case["train"], dtype=np.float32)
    rec = EASE_R_MI355X_Recommender(train.copy(), verbose=False, dense_scoring="device")
    rec.fit(topK=None, l2_norm=20.0, verbose=False)
    holdout, negative = _evaluators(case)
    first, _ = holdout.evaluateRecommender(rec)
    scorer = rec._dense_scorer
    rec.fit(topK=None, l2_norm=300.0, verbose=False)
    assert rec._dense_scorer is scorer              # same shape, same URM_train: new weights in the same buffers
    second = _same_evaluation(holdout, rec, _ExactLists(_host_of(rec, train)))
    assert second != first
    # weights replaced behind the recommender's back are noticed by the cache (identity + fingerprint): uploaded from the host array
    rec.W_sparse = np.ascontiguousarray(rec.W_sparse.T)
    _same_evaluation(negative, rec, _ExactLists(_host_of(rec, train)))
    # a sparse W is the sparse scorer's again, and the dense buffers are given back
    rec.fit(topK=30, l2_norm=20.0, verbose=False)
    assert rec.device_scorable() and not rec.dense_device_scorable() and rec._dense_scorer is None
    assert rec.fit_info["scoring"] == "device"
    fused, _ = holdout.evaluateRecommender(rec)
    assert rec._sp_scorer is not None and any(v > 0 for v in fused[max(fused)].values())
    # the default-constructed class keeps the lists path
    default = EASE_R_MI355X_Recommender(train.copy(), verbose=False)
    default.fit(topK=None, l2_norm=20.0, verbose=False)
    assert default.fit_info["scoring"] == "host" and not default.dense_device_scorable() and not default.device_scorable()
    holdout.evaluateRecommender(default)
    default.recommend(np.arange(5), cutoff=5)
    assert default._dense_scorer is None and default._sp_scorer is None
    rec.invalidate_scorer()
    assert rec._sp_scorer is None and rec._dense_scorer is None
