"""What the four device scorers answer at the C boundary through their one interface (csrc/score.h: ScorerHandle under recommend,
recommend_candidates and the evaluator's add_from_scorer): each kind's own complaint about a user id, the growth of the buffers, the
stats of a call.  Every error here is a host-side check that returns before anything is launched.  All values are small integers, so
every sum is exact in float32 whatever its order (the sparse scorer adds with LDS atomics) and two calls give the same lists."""
import numpy as np
import pytest
import scipy.sparse as sps

from recsys2019_deeplearning_evaluation_amd import (EvaluatorHoldout_MI355X, EvaluatorNegativeItemSample_MI355X, MI355XScorer,
                                                    MI355XSparseScorer)
from recsys2019_deeplearning_evaluation_amd import _native as N
from recsys2019_deeplearning_evaluation_amd.evaluation import item_terms
from recsys2019_deeplearning_evaluation_amd.scoring import MI355XDenseScorer, MI355XItemScorer

pytestmark = pytest.mark.gpu

N_USERS, N_ITEMS, K, CUTOFF = 8, 40, 3, 5
KINDS = ["factor", "sparse", "dense", "item"]
COLD = "Cold users not allowed. Users in trained model are {0}, requested prediction for user {0}"
BAD_USER = {"factor": COLD.format(N_USERS), "item": COLD.format(N_USERS), "sparse": "user id 8 out of range", "dense": "user id 8 out of range"}


def _model():
    rng = np.random.default_rng(5)
    X = sps.csr_matrix((rng.random((N_USERS, N_ITEMS)) < 0.2).astype(np.float32))
    assert X.getnnz(axis=1).min() > 0
    U = rng.integers(-3, 4, (N_USERS, K)).astype(np.float32)
    V = rng.integers(-3, 4, (N_ITEMS, K)).astype(np.float32)
    return X, U, V


def _scorer(kind, n_users=N_USERS):
    X, U, V = _model()
    X, U = X[:n_users], U[:n_users]
    W = V @ V.T
    if kind == "factor":
        return MI355XScorer(U, V, X)
    if kind == "sparse":
        return MI355XSparseScorer(X, sps.csr_matrix(W), X)
    if kind == "dense":
        return MI355XDenseScorer(X, W, X)
    return MI355XItemScorer(V[:, 0], X)


def _candidates(n):
    rows = np.zeros((n, N_ITEMS), np.float32)
    rows[:, ::3] = 1
    return sps.csr_matrix(rows)


@pytest.mark.parametrize("kind", KINDS)
def test_a_user_id_out_of_range_gets_the_kinds_own_message(gpu, kind):
    sc = _scorer(kind)
    users = np.array([2, N_USERS])
    with pytest.raises(ValueError) as full:
        sc.recommend(users, CUTOFF)
    with pytest.raises(ValueError) as cand:
        sc.recommend_candidates(users, _candidates(2), CUTOFF)
    assert str(full.value) == BAD_USER[kind] and str(cand.value) == BAD_USER[kind]
    sc.close()


@pytest.mark.parametrize("negative", [False, True])
@pytest.mark.parametrize("kind", KINDS)
def test_the_evaluators_refuse_a_cold_user_in_the_same_words_for_every_kind(gpu, kind, negative):
    X, _, _ = _model()
    test = sps.csr_matrix(np.eye(N_USERS, N_ITEMS, dtype=np.float32))          # every user is evaluated, user 7 among them
    ev = (EvaluatorNegativeItemSample_MI355X(test, _candidates(N_USERS), [CUTOFF], verbose=False) if negative
          else EvaluatorHoldout_MI355X(test, [CUTOFF], verbose=False))
    sc = _scorer(kind, n_users=N_USERS - 1)
    novelty, popularity = item_terms(X)
    ev._call("begin", N.ptr(novelty), N.ptr(popularity), N.ptr(ev.users_to_evaluate), N_USERS)
    with pytest.raises(ValueError) as refused:
        ev._call(sc.EVAL_ADD + ("_candidates" if negative else ""), sc._h, 0, N_USERS, 1, None)
    assert str(refused.value) == COLD.format(N_USERS - 1)
    sc.close()
    ev.close()


@pytest.mark.parametrize("kind", KINDS)
def test_a_handle_that_has_grown_answers_as_a_fresh_one(gpu, kind):
    everyone = np.arange(N_USERS)
    grown, fresh = _scorer(kind), _scorer(kind)
    grown.recommend(everyone[:3], CUTOFF)
    ranked, scores = grown.recommend(everyone, CUTOFF, return_scores=True)
    want, want_scores = fresh.recommend(everyone, CUTOFF, return_scores=True)
    np.testing.assert_array_equal(ranked, want)
    np.testing.assert_array_equal(scores, want_scores)
    grown.recommend_candidates(everyone[:3], _candidates(3), CUTOFF)
    np.testing.assert_array_equal(grown.recommend_candidates(everyone, _candidates(N_USERS), CUTOFF),
                                  fresh.recommend_candidates(everyone, _candidates(N_USERS), CUTOFF))
    grown.close()
    fresh.close()


@pytest.mark.parametrize("kind", KINDS)
def test_stats_of_a_recommend(gpu, kind):
    X, _, _ = _model()
    sc = _scorer(kind)
    users = np.array([6, 1, 3])
    sc.recommend(users, CUTOFF)
    st = sc.stats()
    assert st["n_units"] == len(users) and st["n_launches"] == 1 and st["n_timed"] == 1 and st["kernel_ms"] > 0
    if kind == "factor":
        assert st["algorithmic_flops"] == 2 * len(users) * N_ITEMS * K
    elif kind == "dense":
        assert st["algorithmic_flops"] == 2 * int(X[users].nnz) * N_ITEMS
    else:
        assert st["call_ms"] == st["kernel_ms"]
    sc.close()


def test_candidates_alone_leave_the_factor_scorer_without_score_rows(gpu):
    sc = _scorer("factor")
    ranked = sc.recommend_candidates(np.arange(N_USERS), _candidates(N_USERS), CUTOFF)
    assert ranked.shape == (N_USERS, CUTOFF) and sc.score_capacity() == 0
    sc.close()
