"""Replacing B of the sparse similarity scorer in place (mi355rec_spscorer_update_b / _get_b, MI355XSparseScorer.update_B / weights):
after every replacement the scorer answers as one freshly built with that B does -- bytes in both modes, since the weights of
slim_hand_off_cases are multiples of 1/64 and every score an exact float32 sum in any order -- and a refused B leaves it as it was."""
import numpy as np
import pytest
import scipy.sparse as sps

from recsys2019_deeplearning_evaluation_amd import MI355XSparseScorer
from recsys2019_deeplearning_evaluation_amd.evaluation import EvaluatorHoldout_MI355X
from recsys2019_deeplearning_evaluation_amd.recommender_base import BaseItemSimilarityMatrixRecommender
from recsys2019_deeplearning_evaluation_amd.scoring import GpuSimilarityScoringMixin
from hand_off_cases import N_ITEMS, N_USERS, URM_TEST, URM_TRAIN, candidate_rows
from slim_hand_off_cases import ALL_USERS, W1, W2, W3, W_EMPTY, weights

pytestmark = pytest.mark.gpu

CANDIDATES = candidate_rows()
assert sorted(set(URM_TRAIN.data.tolist())) == [1.0, 2.0, 3.0, 4.0, 5.0]


class _Serves(GpuSimilarityScoringMixin, BaseItemSimilarityMatrixRecommender):
    """A recommender that is nothing but a given scorer: what the device evaluator needs to drive it."""

    def __init__(self, URM, scorer):
        super(_Serves, self).__init__(URM, verbose=False)
        self._served = scorer

    def device_scorer(self):
        return self._served


def _answers(scorer, URM=URM_TRAIN):
    ranked, scores = scorer.recommend(ALL_USERS, N_ITEMS, return_scores=True)
    evaluator = EvaluatorHoldout_MI355X(URM_TEST, [5, 10], verbose=False)
    results, _ = evaluator.evaluateRecommender(_Serves(URM, scorer))
    evaluator.close()
    return ranked, scores, scorer.recommend_candidates(ALL_USERS, CANDIDATES, 25), results


def _assert_same_answers(got, want):
    assert got[1].tobytes() == want[1].tobytes()
    np.testing.assert_array_equal(got[0], want[0])
    np.testing.assert_array_equal(got[2], want[2])
    assert got[3] == want[3]


def _assert_same_weights(got, want):
    for name in ("indptr", "indices", "data"):
        a, b = getattr(got, name), getattr(want, name)
        assert a.dtype == b.dtype and a.shape == b.shape and (a == b).all(), name
    assert got.shape == want.shape


@pytest.mark.parametrize("exact", [False, True], ids=["atomic", "exact"])
def test_update_b_answers_as_a_fresh_scorer(gpu, exact):
    scorer = MI355XSparseScorer(URM_TRAIN, W1, URM_TRAIN, exact=exact)
    seen = []
    # growth, shrinking, no cell at all, growth from no cell
    for W in (W2, W3, W_EMPTY, W1):
        scorer.update_B(W)
        st = scorer.stats()
        assert st["call_ms"] > 0 and st["kernel_ms"] == st["call_ms"] and st["algorithmic_bytes"] >= 4.0 * (N_ITEMS + 1) + 8.0 * W.nnz
        fresh = MI355XSparseScorer(URM_TRAIN, W, URM_TRAIN, exact=exact)
        _assert_same_weights(scorer.weights(), fresh.weights())
        _assert_same_weights(scorer.weights(), W)
        want = _answers(fresh)
        assert W.nnz == 0 or np.abs(want[1][np.isfinite(want[1])]).max() > 0
        _assert_same_answers(_answers(scorer), want)
        fresh.close()
        seen.append(want[1].tobytes())
    assert len(set(seen)) == 4
    scorer.close()


@pytest.mark.parametrize("exact", [False, True], ids=["atomic", "exact"])
def test_update_b_of_a_user_based_scorer_replaces_the_urm_side(gpu, exact):
    W_users = weights(9, 0.03, n=N_USERS, long_row=2, empty_row=5)
    rng = np.random.default_rng(12)
    other = sps.csr_matrix(URM_TRAIN.multiply(rng.random(URM_TRAIN.shape) < 0.6), dtype=np.float32)     # fewer cells, same ratings
    other.eliminate_zeros()
    other.sort_indices()
    denser = sps.csr_matrix(URM_TRAIN + sps.random(N_USERS, N_ITEMS, 0.05, format="csr", dtype=np.float32, random_state=3).ceil(), dtype=np.float32)
    denser.sort_indices()
    assert other.nnz < URM_TRAIN.nnz < denser.nnz
    scorer = MI355XSparseScorer(W_users, URM_TRAIN, URM_TRAIN, exact=exact)
    for B in (denser, other):
        scorer.update_B(B)
        fresh = MI355XSparseScorer(W_users, B, URM_TRAIN, exact=exact)
        _assert_same_weights(scorer.weights(), fresh.weights())
        _assert_same_answers(_answers(scorer), _answers(fresh))
        fresh.close()
    scorer.close()


def _bad(kind):
    """(indptr, indices, data) of a 200 x 200 B with one defect, and the row the refusal must name"""
    W = W1.copy()
    row = 41
    s, e = W.indptr[row], W.indptr[row + 1]
    assert e - s >= 3
    if kind == "first_indptr":
        W.indptr[0], row = 1, 0
    elif kind == "decreasing_indptr":
        W.indptr[row + 1] = s - 1
    elif kind == "id_at_n_items":
        W.indices[e - 1] = N_ITEMS
    elif kind == "negative_id":
        W.indices[s] = -1
    elif kind == "unsorted":
        W.indices[s], W.indices[s + 1] = W.indices[s + 1], W.indices[s]
    elif kind == "column_twice":
        W.indices[s + 1] = W.indices[s]
    return W, row


class _Raw:
    """Arrays that go to update_B as they are: the wrapper's tocsr() / sorted_indices() see a csr that says it is sorted."""
    has_sorted_indices = True

    def __init__(self, W):
        self.indptr, self.indices, self.data, self.shape = W.indptr, W.indices, W.data, W.shape

    def tocsr(self):
        return self


@pytest.mark.parametrize("exact", [False, True], ids=["atomic", "exact"])
def test_every_refusal_of_update_b_leaves_the_scorer_as_it_was(gpu, exact):
    scorer = MI355XSparseScorer(URM_TRAIN, W2, URM_TRAIN, exact=exact)
    before = scorer.recommend(ALL_USERS, N_ITEMS, return_scores=True)
    kinds = ["first_indptr", "decreasing_indptr", "id_at_n_items", "negative_id"] + (["unsorted", "column_twice"] if exact else [])
    for kind in kinds:
        W, row = _bad(kind)
        with pytest.raises(ValueError, match=r"row %d\b" % row):
            scorer.update_B(_Raw(W))
        after = scorer.recommend(ALL_USERS, N_ITEMS, return_scores=True)
        assert after[1].tobytes() == before[1].tobytes(), kind
        np.testing.assert_array_equal(after[0], before[0])
        _assert_same_weights(scorer.weights(), W2)
    with pytest.raises(ValueError):
        scorer.update_B(W1[:, :N_ITEMS - 1])
    # a further valid update works
    scorer.update_B(W3)
    fresh = MI355XSparseScorer(URM_TRAIN, W3, URM_TRAIN, exact=exact)
    _assert_same_answers(_answers(scorer), _answers(fresh))
    fresh.close()
    scorer.close()


def test_the_atomic_mode_takes_an_unsorted_row(gpu):
    shuffled = weights(1, 0.05, long_row=3, empty_row=8, empty_column=5, shuffle_rows=True)
    assert not (np.diff(shuffled.indices[shuffled.indptr[3]:shuffled.indptr[4]]) > 0).all()
    scorer = MI355XSparseScorer(URM_TRAIN, W2, URM_TRAIN)
    scorer.update_B(_Raw(shuffled))
    _assert_same_weights(scorer.weights(), shuffled)
    fresh = MI355XSparseScorer(URM_TRAIN, shuffled, URM_TRAIN)
    _assert_same_answers(_answers(scorer), _answers(fresh))
    # the exact wrapper sorts a matrix that says it is unsorted, as the constructor does
    exact = MI355XSparseScorer(URM_TRAIN, W2, URM_TRAIN, exact=True)
    exact.update_B(shuffled)
    _assert_same_weights(exact.weights(), W1)
    assert _answers(exact)[1].tobytes() == _answers(fresh)[1].tobytes()
    for s in (scorer, fresh, exact):
        s.close()


def test_switching_modes_around_an_update_rebuilds_the_table(gpu):
    scorer = MI355XSparseScorer(URM_TRAIN, W1, URM_TRAIN)
    scorer._call("set_exact", 1)
    scorer.exact = True
    scorer.update_B(W2)
    scorer._call("set_exact", 0)
    scorer._call("set_exact", 1)
    fresh = MI355XSparseScorer(URM_TRAIN, W2, URM_TRAIN, exact=True)
    want = _answers(fresh)
    _assert_same_answers(_answers(scorer), want)
    # ... and a B replaced while the mode is off is the one the next switch-on serves
    scorer._call("set_exact", 0)
    scorer.exact = False
    scorer.update_B(W3)
    scorer._call("set_exact", 1)
    fresh3 = MI355XSparseScorer(URM_TRAIN, W3, URM_TRAIN, exact=True)
    want3 = _answers(fresh3)
    assert want3[1].tobytes() != want[1].tobytes()
    _assert_same_answers(_answers(scorer), want3)
    for s in (scorer, fresh, fresh3):
        s.close()
