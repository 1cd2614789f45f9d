"""MI355XSparseScorer(exact=True) and `sparse_scoring = "exact"` on the device: scores equal to SciPy's csr @ csr as
uint32 views, lists exactly the tie rule's (value descending, lower item id first, -1 padded), for rows inside one tile, at the first
width that leaves LDS and over three tiles, in both operand orders; calls repeat and blocks can be split without changing a bit;
candidate rows rank the cells of the full exact row; both device evaluators through the fused path against their lists path; the
mode is part of the scorer cache; a B with a column twice in a row is refused.  No tolerance anywhere.  Cases:
tests/sparse_exact_cases.py."""
import numpy as np
import pytest
import scipy.sparse as sps

from recsys2019_deeplearning_evaluation_amd import (EvaluatorHoldout_MI355X, EvaluatorNegativeItemSample_MI355X, ItemKNNCFRecommender,
                                                    MI355XSparseScorer, UserKNNCFRecommender)
from recsys2019_deeplearning_evaluation_amd import _native as N
from recsys2019_deeplearning_evaluation_amd import recommender_base as RB
from test_evaluation_gpu import _bitwise_equal
import ranking_cases as RC
import sparse_exact_cases as SC

pytestmark = pytest.mark.gpu
CUTOFF = 10
_built = {}


def built(name):
    """One exact scorer and one SciPy product per case, shared by the tests below (never modified)."""
    if name not in _built:
        c = SC.case(name)
        _built[name] = (c, SC.scipy_scores(c["A"], c["users"], c["B"]), MI355XSparseScorer(c["A"], c["B"], c["seen"], exact=True))
    return _built[name]


def same_bits(got, want):
    return got.dtype == np.float32 and got.shape == want.shape and np.array_equal(SC.bits(got), SC.bits(want))


@pytest.mark.parametrize("masked", [False, True])
@pytest.mark.parametrize("remove_seen", [True, False])
@pytest.mark.parametrize("name", sorted(SC.CASES))
def test_scores_are_scipy_bit_for_bit_and_lists_follow_the_tie_rule(gpu, name, remove_seen, masked):
    c, product, scorer = built(name)
    n_items = c["n_items"]
    allowed = SC.some_mask(n_items, 5) if masked else None
    cutoff = min(CUTOFF, n_items)
    ranked, scores = scorer.recommend(c["users"], cutoff, remove_seen, allowed, return_scores=True)
    want = RC.apply_filters(product, c["seen"], c["users"], remove_seen, allowed)
    assert same_bits(scores, want)                  # -inf exactly at the filtered cells, signed zeros as SciPy's
    assert np.array_equal(ranked, SC.exact_lists(want, cutoff))
    if not remove_seen and not masked:              # the empty profile: every score +0.0, the list is the lowest ids
        assert np.array_equal(ranked[SC.EMPTY_USER], np.arange(cutoff))
        assert not SC.bits(scores[SC.EMPTY_USER]).any()
    assert scorer.exact and scorer.stats()["kernel_ms"] > 0


@pytest.mark.parametrize("name", ["item_n65", "user_n1000", "item_first_wide", "user_three_tiles"])
def test_a_cutoff_beyond_the_admissible_items_is_padded(gpu, name):
    c, product, scorer = built(name)
    n_items = c["n_items"]
    allowed = np.zeros(n_items, np.uint8)
    allowed[[0, n_items // 2, n_items - 1]] = 1
    ranked, _ = scorer.recommend(c["users"], CUTOFF, False, allowed)
    want = SC.exact_lists(RC.apply_filters(product, c["seen"], c["users"], False, allowed), CUTOFF)
    assert np.array_equal(ranked, want) and (ranked[:, 3:] == -1).all() and (ranked[:, :3] >= 0).all()


@pytest.mark.parametrize("name", ["item_n1000", "user_n1000"])
def test_calls_repeat_bit_for_bit_and_a_batch_can_be_split_any_way(gpu, name):
    c, product, scorer = built(name)
    users = c["users"]
    assert len(users) == 40
    first = scorer.recommend(users, CUTOFF, True, None, return_scores=True)
    again = scorer.recommend(users, CUTOFF, True, None, return_scores=True)
    assert first[0].tobytes() == again[0].tobytes() and first[1].tobytes() == again[1].tobytes()
    for block in (1, 7, 32):
        parts = [scorer.recommend(users[a:a + block], CUTOFF, True, None, return_scores=True) for a in range(0, len(users), block)]
        assert np.concatenate([p[0] for p in parts]).tobytes() == first[0].tobytes(), block
        assert np.concatenate([p[1] for p in parts]).tobytes() == first[1].tobytes(), block
    back = scorer.recommend(users[::-1].copy(), CUTOFF, True, None, return_scores=True)
    assert back[0][::-1].tobytes() == first[0].tobytes() and back[1][::-1].tobytes() == first[1].tobytes()


def test_wide_rows_repeat_bit_for_bit(gpu):
    c, product, scorer = built("item_three_tiles")
    first = scorer.recommend(c["users"], CUTOFF, False, None, return_scores=True)
    again = scorer.recommend(c["users"], CUTOFF, False, None, return_scores=True)
    assert first[0].tobytes() == again[0].tobytes() and first[1].tobytes() == again[1].tobytes()
    parts = [scorer.recommend(c["users"][a:b], CUTOFF, False, None, return_scores=True) for a, b in ((0, 1), (1, 8))]
    assert np.concatenate([p[1] for p in parts]).tobytes() == first[1].tobytes()


@pytest.mark.parametrize("name", ["item_n1000", "user_n1000", "item_first_wide"])
@pytest.mark.parametrize("remove_seen", [True, False])
def test_candidates_are_ranked_by_the_cells_of_the_full_exact_row(gpu, name, remove_seen):
    c, product, scorer = built(name)
    users, n_items = c["users"], c["n_items"]
    rng = np.random.default_rng(11)
    lengths = [1, 64, 65, 300] * (len(users) // 4)
    rows = sps.lil_matrix((len(users), n_items), dtype=np.float32)
    for r in range(len(users)):
        picked = rng.choice(n_items, lengths[r], replace=False)
        seen = c["seen"].indices[c["seen"].indptr[users[r]]:c["seen"].indptr[users[r] + 1]]
        if remove_seen and lengths[r] > 1 and len(seen):        # some seen items among the candidates
            picked = np.union1d(picked[:lengths[r] - min(3, len(seen))], seen[:3])
        rows[r, picked] = 1
    rows = sps.csr_matrix(rows)
    want = np.full(product.shape, -np.inf, np.float32)
    mask = rows.toarray() != 0
    want[mask] = RC.apply_filters(product, c["seen"], users, remove_seen)[mask]
    for cutoff in (5, 100):
        ranked = scorer.recommend_candidates(users, rows, cutoff, remove_seen)
        assert np.array_equal(ranked, SC.exact_lists(want, cutoff)), cutoff
    assert scorer.stats()["kernel_ms"] > 0
    allowed = SC.some_mask(n_items, 6)
    ranked = scorer.recommend_candidates(users, rows, 20, remove_seen, allowed)
    want[:, allowed == 0] = -np.inf
    assert np.array_equal(ranked, SC.exact_lists(want, 20))


# ------------------------------------------------------------------------------------------------------------ end to end
def _operands(rec):
    """(A, B) as the scorer of a fitted recommender takes them: float32, A's cells in their stored order."""
    def f32(M):
        M = sps.csr_matrix(M)
        return sps.csr_matrix((M.data.astype(np.float32), M.indices, M.indptr), shape=M.shape)
    W, X = f32(rec.W_sparse), f32(rec.URM_train)
    return (W, X) if rec._SCORER_USER_BASED else (X, W)


class _ExactLists(RB.BaseRecommender):
    """The lists path fed with the tie rule's lists of the SciPy scores of a fitted similarity recommender."""

    def __init__(self, rec):
        super().__init__(rec.URM_train, verbose=False)
        self._A, self._B = _operands(rec)

    def recommend(self, user_id_array, cutoff=None, remove_seen_flag=True, items_to_compute=None, remove_top_pop_flag=False,
                  remove_custom_items_flag=False, return_scores=False):
        assert not remove_top_pop_flag and not remove_custom_items_flag and not return_scores
        users = np.atleast_1d(user_id_array)
        scores = SC.scipy_scores(self._A, users, self._B)
        allowed = None
        if items_to_compute is not None:
            allowed = np.zeros(scores.shape[1], np.uint8)
            allowed[np.asarray(items_to_compute)] = 1
        filtered = RC.apply_filters(scores, sps.csr_matrix(self.URM_train), users, remove_seen_flag, allowed)
        return [row[row >= 0].tolist() for row in SC.exact_lists(filtered, min(cutoff, scores.shape[1]))]


@pytest.fixture(scope="module")
def fitted(gpu):
    from negative_eval_cases import make_case
    case = make_case("sampled")
    train = sps.csr_matrix(case["train"], dtype=np.float32)
    item = ItemKNNCFRecommender(train.copy())
    item.fit(topK=20, shrink=5)
    user = UserKNNCFRecommender(train.copy())
    user.fit(topK=20, shrink=5)
    return case, {"item": item, "user": user}


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


@pytest.mark.parametrize("kind", ["item", "user"])
def test_both_evaluators_give_exactly_what_their_lists_path_gives(fitted, kind):
    case, recs = fitted
    rec = recs[kind]
    rec.sparse_scoring = "exact"
    try:
        stub = _ExactLists(rec)
        for ev in _evaluators(case):
            fused = _same_evaluation(ev, rec, stub)
            assert rec._sp_scorer is not None and rec._sp_scorer.exact
            again, _ = ev.evaluateRecommender(rec, block_size=37)       # whatever the block size
            _bitwise_equal(again, fused)
        # recommend() itself: the host's scores and the tie rule's lists
        users = np.arange(0, rec.URM_train.shape[0], 7)
        A, B = _operands(rec)
        lists, scores = rec.recommend(users, cutoff=8, remove_seen_flag=True, return_scores=True)
        want = RC.apply_filters(SC.scipy_scores(A, users, B), sps.csr_matrix(rec.URM_train), users, True)
        assert same_bits(scores, want)
        assert lists == [row[row >= 0].tolist() for row in SC.exact_lists(want, 8)]
    finally:
        del rec.sparse_scoring
        rec.invalidate_scorer()


def test_the_mode_is_part_of_the_scorer_cache(fitted):
    case, recs = fitted
    rec = recs["item"]
    rec.invalidate_scorer()
    users = np.arange(20)
    assert rec.sparse_scoring == "atomic"
    default = rec.device_scorer()
    assert isinstance(default, MI355XSparseScorer) and not default.exact          # today's behaviour, untouched
    rec.recommend(users, cutoff=5)
    assert rec.device_scorer() is default
    rec.sparse_scoring = "exact"
    try:
        exact = rec.device_scorer()
        assert exact is not default and exact.exact and default._h is None      # rebuilt; the old handle is closed
        A, B = _operands(rec)
        _, scores = rec.recommend(users, cutoff=5, remove_seen_flag=False, return_scores=True)
        assert same_bits(scores, SC.scipy_scores(A, users, B))
        assert rec.device_scorer() is exact
    finally:
        del rec.sparse_scoring
    back = rec.device_scorer()
    assert back is not exact and not back.exact and exact._h is None
    _, atomic_scores = rec.recommend(users, cutoff=5, remove_seen_flag=False, return_scores=True)
    assert np.allclose(atomic_scores, scores, rtol=1e-4, atol=1e-6)
    type(rec).sparse_scoring = "exact"              # on the class
    try:
        assert rec.device_scorer().exact
    finally:
        del type(rec).sparse_scoring
    assert rec.sparse_scoring == "atomic" and not rec.device_scorer().exact
    rec.invalidate_scorer()


def test_a_column_twice_in_a_row_of_b_is_refused_before_any_scoring_launch(gpu):
    rng = np.random.default_rng(3)
    A = sps.random(12, 9, 0.5, format="csr", dtype=np.float32, random_state=4)
    B = sps.random(9, 30, 0.3, format="csr", dtype=np.float32, random_state=5).sorted_indices()
    start = B.indptr[3]
    assert B.indptr[4] - start >= 2
    B.indices[start + 1] = B.indices[start]         # row 3 stores a column twice
    B.has_canonical_format = False
    seen = sps.csr_matrix((12, 30), dtype=np.float32)
    users = np.arange(12, dtype=np.int32)
    with pytest.raises(ValueError, match="row 3 of B"):
        MI355XSparseScorer(A, B, seen, exact=True)
    shuffled = B.copy()                             # the wrapper sorts B: the duplicate becomes adjacent and is still caught
    row = slice(shuffled.indptr[3], shuffled.indptr[4])
    order = rng.permutation(row.stop - row.start)
    shuffled.indices[row], shuffled.data[row] = shuffled.indices[row][order], shuffled.data[row][order]
    shuffled.has_sorted_indices = False
    with pytest.raises(ValueError, match="row 3 of B"):
        MI355XSparseScorer(A, shuffled, seen, exact=True)
    scorer = MI355XSparseScorer(A, B, seen)
    try:
        lib = N.load()
        assert lib.mi355rec_spscorer_set_exact(scorer._h, 1) == N.E_INVALID
        assert b"row 3 of B" in lib.mi355rec_last_error()
        assert scorer.stats()["n_launches"] == 0            # nothing was scored
        ranked, scores = scorer.recommend(users, 5, False, None, return_scores=True)    # the handle still scores, in atomic mode
        assert np.allclose(scores, (A @ B).toarray(), rtol=1e-5, atol=1e-6)
        assert lib.mi355rec_spscorer_set_exact(scorer._h, 0) == 0
        assert lib.mi355rec_spscorer_set_exact(None, 1) == N.E_INVALID
        assert lib.mi355rec_spscorer_set_exact(None, 0) == N.E_INVALID
    finally:
        scorer.close()
    # an unsorted row handed to the C ABI directly is refused as well: the kernel's ranges need ascending rows
    C = sps.random(9, 30, 0.3, format="csr", dtype=np.float32, random_state=5).sorted_indices()
    C.indices[C.indptr[5]:C.indptr[6]] = C.indices[C.indptr[5]:C.indptr[6]][::-1]
    assert C.indptr[6] - C.indptr[5] >= 2
    raw = MI355XSparseScorer(A, C, seen)
    try:
        assert N.load().mi355rec_spscorer_set_exact(raw._h, 1) == N.E_INVALID
        assert b"row 5 of B" in N.load().mi355rec_last_error()
    finally:
        raw.close()


def test_the_mode_can_be_switched_on_and_off_on_one_handle(gpu):
    c = SC.case("item_n1000")
    want = SC.scipy_scores(c["A"], c["users"], c["B"])
    scorer = MI355XSparseScorer(c["A"], c["B"].sorted_indices(), c["seen"])
    try:
        atomic = scorer.recommend(c["users"], CUTOFF, False, None, return_scores=True)[1]
        scorer._call("set_exact", 1)
        assert same_bits(scorer.recommend(c["users"], CUTOFF, False, None, return_scores=True)[1], want)
        scorer._call("set_exact", 0)
        scorer._call("set_exact", 1)
        assert same_bits(scorer.recommend(c["users"], CUTOFF, False, None, return_scores=True)[1], want)
        scorer._call("set_exact", 0)
        assert scorer.recommend(c["users"], CUTOFF, False, None, return_scores=True)[1].shape == atomic.shape
    finally:
        scorer.close()
