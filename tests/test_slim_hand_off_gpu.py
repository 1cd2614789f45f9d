"""The device-to-device hand-off of a SLIM-BPR model to the sparse scorer (mi355rec_spscorer_update_from_slim,
MI355XSparseScorer.update_from) and the `validation_hand_off = "device"` mode of SLIM_BPR_MI355X built on it: the scorer's B ends as
the W of get_S_and_W() array for array, a device-mode fit is the host-mode fit, and the copies device mode exists to avoid are not
made."""
import os

import numpy as np
import pytest

from recsys2019_deeplearning_evaluation_amd import MI355XSparseScorer, SLIM_BPR_MI355X, SLIM_BPR_MI355X_Epoch
from recsys2019_deeplearning_evaluation_amd.evaluation import EvaluatorHoldout_MI355X, EvaluatorNegativeItemSample_MI355X
from _util import check_topk_against_dense
from hand_off_cases import N_ITEMS, N_USERS, URM_NEGATIVE, URM_TEST, URM_TRAIN
from slim_hand_off_cases import ALL_USERS, ITEM_COUNTS, PROBLEMS, W1, weights

pytestmark = pytest.mark.gpu

TOPKS = (1, 20, 150, 500)           # 500 is clamped to n_items, as the host call clamps it; 150: rows beyond one wavefront


def _epoch(n_items, symmetric, sgd_mode, topK=20, seed=5, **kwargs):
    return SLIM_BPR_MI355X_Epoch(PROBLEMS[n_items]["train"], topK=topK, symmetric=symmetric, sgd_mode=sgd_mode, learning_rate=0.05, li_reg=1e-3,
                                 lj_reg=1e-3, random_seed=seed, **kwargs)


def _assert_same_weights(got, want):
    assert got.shape == want.shape
    for name in ("indptr", "indices", "data"):
        a, b = getattr(got, name), getattr(want, name)
        assert a.dtype == b.dtype and a.shape == b.shape and (a == b).all(), name


def _answers(scorer, candidates):
    ranked, scores = scorer.recommend(ALL_USERS, scorer.n_items, return_scores=True)
    return ranked, scores, scorer.recommend_candidates(ALL_USERS, candidates, 25)


def _assert_lists_within_ties(atomic, exact_scorer, cutoff=10):
    """The lists of the atomic mode against the exact scores of the same model: check_topk_against_dense's rule -- everything strictly
    above the cutoff-th score is listed, nothing strictly below it, values in order -- at 1e-5 of the row's largest score, the bound
    of test_scoring_gpu.py for host-against-device scores.  That comparator is about similarity columns, where a zero is never emitted:
    it is applied to the users whose cutoff-th exact score is positive (zeros then lie below the cut); the others are counted."""
    ranked, scores = atomic.recommend(ALL_USERS, cutoff, remove_seen=False, return_scores=True)
    _, want = exact_scorer.recommend(ALL_USERS, cutoff, remove_seen=False, return_scores=True)
    compared = 0
    for u in ALL_USERS:
        if np.sort(want[u])[::-1][cutoff - 1] > 0:
            check_topk_against_dense(ranked[u], scores[u][ranked[u]], want[u].astype(np.float64), cutoff, rtol=1e-5)
            compared += 1
    return compared


@pytest.mark.parametrize("n_items", ITEM_COUNTS)
@pytest.mark.parametrize("symmetric,sgd_mode", [(True, "sgd"), (True, "adagrad"), (False, "sgd"), (False, "adagrad")])
def test_update_from_is_the_host_w(gpu, n_items, symmetric, sgd_mode):
    problem = PROBLEMS[n_items]
    URM, candidates = problem["train"], problem["candidates"]
    epoch = _epoch(n_items, symmetric, sgd_mode)
    assert epoch.precision == ("fp32" if sgd_mode == "sgd" else "fp64")
    start = weights(4, 0.05, n=n_items)
    atomic, exact = MI355XSparseScorer(URM, start, URM), MI355XSparseScorer(URM, start, URM, exact=True)
    sizes, compared = [], 0
    for epochs in (0, 1, 2):        # read out before any epoch, after 1 and after 3
        if epochs:
            epoch.epochIteration_Cython(epochs)
        for topK in TOPKS:
            epoch.topK = topK
            S_before = epoch.get_S_dense()
            _, W = epoch.get_S_and_W()
            for scorer in (atomic, exact):
                scorer.update_from(epoch)
                st = scorer.stats()
                assert st["call_ms"] > 0 and st["kernel_ms"] == st["call_ms"] and st["algorithmic_bytes"] >= 2 * (4.0 * (n_items + 1) + 8.0 * W.nnz)
                _assert_same_weights(scorer.weights(), W)
            assert (epoch.get_S_dense() == S_before).all()          # the epoch object is only read
            fresh = MI355XSparseScorer(URM, W, URM, exact=True)
            want, got = _answers(fresh, candidates), _answers(exact, candidates)
            assert got[1].tobytes() == want[1].tobytes()
            np.testing.assert_array_equal(got[0], want[0])
            np.testing.assert_array_equal(got[2], want[2])
            if W.nnz == 0:          # no cell: every score is an empty sum in either mode
                np.testing.assert_array_equal(atomic.recommend(ALL_USERS, 10)[0], fresh.recommend(ALL_USERS, 10)[0])
            else:
                compared += _assert_lists_within_ties(atomic, fresh)
            fresh.close()
            sizes.append(W.nnz)
            assert (epochs == 0) == (W.nnz == 0)
            assert W.nnz <= n_items * min(topK, n_items) and np.diff(W.indptr).max() <= min(topK, n_items)
    assert compared > 0
    steps = np.diff(sizes)
    assert (steps > 0).any() and (steps < 0).any()                 # nnz grew and shrank on the one scorer
    for h in (atomic, exact, epoch):
        h.close()


def test_rows_beyond_one_wavefront_were_handed_over(gpu):
    """topK = 150 after twenty epochs gives rows of W of more than 64 and of more than 128 cells on this problem (the lane stride of
    csr_adopt_kernel: two and three steps of a row's wavefront); topK = 1 and 20, above, give rows within one step."""
    epoch = _epoch(N_ITEMS, False, "sgd", topK=150)
    epoch.epochIteration_Cython(20)
    _, W = epoch.get_S_and_W()
    lengths = np.diff(W.indptr)
    assert lengths.max() > 128 and ((lengths > 64) & (lengths <= 128)).any()
    scorer = MI355XSparseScorer(URM_TRAIN, W1, URM_TRAIN)
    scorer.update_from(epoch)
    _assert_same_weights(scorer.weights(), W)
    scorer.close()
    epoch.close()


def test_every_refusal_leaves_the_scorer_as_it_was(gpu):
    epoch = _epoch(N_ITEMS, True, "sgd")
    epoch.epochIteration_Cython()
    cut = ITEM_COUNTS[1]

    def refused(scorer, handle, error, match, B):
        users = np.arange(scorer.n_users)
        before = scorer.recommend(users, scorer.n_items, return_scores=True)
        with pytest.raises(error, match=match):
            scorer.update_from(handle)
        after = scorer.recommend(users, scorer.n_items, return_scores=True)
        assert after[1].tobytes() == before[1].tobytes()
        np.testing.assert_array_equal(after[0], before[0])
        _assert_same_weights(scorer.weights(), B)
        scorer.close()

    item_based = lambda: MI355XSparseScorer(URM_TRAIN, W1, URM_TRAIN, exact=True)
    W_cut = weights(6, 0.05, n=cut)
    refused(MI355XSparseScorer(PROBLEMS[cut]["train"], W_cut, PROBLEMS[cut]["train"], exact=True), epoch, ValueError, "200 items", W_cut)
    refused(MI355XSparseScorer(weights(9, 0.03, n=N_USERS), URM_TRAIN, URM_TRAIN, exact=True), epoch, ValueError, "300 x 200", URM_TRAIN)
    epoch.topK = 0
    refused(item_based(), epoch, ValueError, "topK", W1)
    epoch.topK = 20
    refused(item_based(), object(), TypeError, "SLIM_BPR_MI355X_Epoch", W1)
    sparse_store = _epoch(N_ITEMS, False, "adagrad", train_with_sparse_weights=True)
    refused(item_based(), sparse_store, NotImplementedError, "train_with_sparse_weights", W1)
    sparse_store.close()
    epoch.close()
    refused(item_based(), epoch, ValueError, "closed", W1)
    closed = item_based()
    closed.close()
    with pytest.raises(ValueError, match="closed"):
        closed.update_from(_epoch(N_ITEMS, True, "sgd"))


# ---- a device-mode fit is the host-mode fit ---------------------------------------------------------------------------------------

FIT = dict(epochs=8, validation_every_n=2, stop_on_validation=True, lower_validations_allowed=8, validation_metric="MAP")
MODELS = {"sgd_symmetric": dict(sgd_mode="sgd", symmetric=True, topK=20, learning_rate=0.05, lambda_i=1e-3, lambda_j=1e-3, random_seed=31),
          "adagrad_dense": dict(sgd_mode="adagrad", symmetric=False, topK=20, learning_rate=0.05, lambda_i=1e-3, lambda_j=1e-3, random_seed=32)}


class _ListsEvaluator(EvaluatorHoldout_MI355X):
    """The holdout evaluator with every recommender asked through recommend()."""

    def _run(self, rec, block_size):
        self._dispatch(rec, block_size, None)


def _evaluator(kind):
    if kind == "negative":
        return EvaluatorNegativeItemSample_MI355X(URM_TEST, URM_NEGATIVE, [5, 10], verbose=False)
    return (_ListsEvaluator if kind == "lists" else EvaluatorHoldout_MI355X)(URM_TEST, [5, 10], verbose=False)


class _Recording:
    """A thin wrapper around an evaluator: every result dict of a fit, in order; `during` runs inside each validation."""

    def __init__(self, evaluator, during=None):
        self.evaluator, self.during, self.results = evaluator, during, []

    def evaluateRecommender(self, recommender):
        if self.during is not None:
            self.during(recommender, len(self.results))
        results, string = self.evaluator.evaluateRecommender(recommender)
        self.results.append(results)
        return results, string


def _fit(name, mode, evaluator_kind="holdout", during=None, sparse_scoring="exact"):
    rec = SLIM_BPR_MI355X(URM_TRAIN, verbose=False)
    rec.validation_hand_off = mode
    rec.sparse_scoring = sparse_scoring
    recording = _Recording(_evaluator(evaluator_kind), during)
    rec.fit(evaluator_object=recording, **FIT, **MODELS[name])
    recording.evaluator.close()
    return rec, recording.results


def _assert_same_matrix(a, b, name):
    assert type(a) is type(b) and a.format == b.format and a.shape == b.shape and a.dtype == b.dtype, name
    for part in ("indptr", "indices", "data"):
        x, y = getattr(a, part), getattr(b, part)
        assert x.dtype == y.dtype and x.shape == y.shape and x.tobytes() == y.tobytes(), (name, part)


def _assert_same_model(rec_a, rec_b):
    for name in ("W_sparse", "S_incremental", "S_best"):
        _assert_same_matrix(getattr(rec_a, name), getattr(rec_b, name), name)


def _assert_same_fit(a, b):
    (rec_a, results_a), (rec_b, results_b) = a, b
    assert len(results_a) == FIT["epochs"] // FIT["validation_every_n"] and results_a == results_b
    assert rec_a.epochs_best == rec_b.epochs_best and rec_a.best_validation_metric == rec_b.best_validation_metric
    _assert_same_model(rec_a, rec_b)


@pytest.mark.parametrize("name,evaluator_kind", [("sgd_symmetric", "holdout"), ("adagrad_dense", "holdout"), ("sgd_symmetric", "lists"),
                                                 ("adagrad_dense", "negative")])
def test_a_device_mode_fit_is_the_host_mode_fit(gpu, name, evaluator_kind):
    host = _fit(name, "host", evaluator_kind)
    _assert_same_fit(host, _fit(name, "host", evaluator_kind))      # the premise: two host-mode fits with one seed are byte-equal
    device = _fit(name, "device", evaluator_kind)
    _assert_same_fit(device, host)
    rec = device[0]
    assert not rec._host_model_stale and not rec._scorer_current
    assert rec.S_best.dtype == np.float64 and rec.W_sparse.dtype == np.float32
    # after fit the scorer follows the host attributes again: recommend() serves the final model in both modes
    lists_d, scores_d = rec.recommend(ALL_USERS, cutoff=10, return_scores=True)
    lists_h, scores_h = host[0].recommend(ALL_USERS, cutoff=10, return_scores=True)
    assert scores_d.tobytes() == scores_h.tobytes() and lists_d == lists_h


def test_a_device_mode_fit_in_the_atomic_mode_leaves_the_host_mode_model(gpu):
    """In the default atomic mode the metric values depend on the order of LDS atomics in either mode: the models are compared."""
    (host, results_h), (device, results_d) = _fit("sgd_symmetric", "host", sparse_scoring="atomic"), _fit("sgd_symmetric", "device", sparse_scoring="atomic")
    assert len(results_h) == len(results_d) and host.epochs_best == device.epochs_best
    _assert_same_matrix(device.W_sparse, host.W_sparse, "W_sparse")
    _assert_same_matrix(device.S_best, host.S_best, "S_best")


# ---- the copies are really gone ---------------------------------------------------------------------------------------------------

def _count(monkeypatch, owner, method, counts, key):
    original = getattr(owner, method)

    def counted(self, *args, **kwargs):
        counts[key] = counts.get(key, 0) + 1
        return original(self, *args, **kwargs)

    monkeypatch.setattr(owner, method, counted)


def _counting(monkeypatch):
    counts = {}
    _count(monkeypatch, MI355XSparseScorer, "__init__", counts, "scorer")
    _count(monkeypatch, MI355XSparseScorer, "update_from", counts, "update_from")
    _count(monkeypatch, SLIM_BPR_MI355X_Epoch, "get_S_and_W", counts, "get_S_and_W")
    _count(monkeypatch, SLIM_BPR_MI355X_Epoch, "get_S", counts, "get_S")
    return counts


def _new_bests_after_the_first(results):
    best, n = results[0][5]["MAP"], 0
    for r in results[1:]:
        if r[5]["MAP"] > best:
            best, n = r[5]["MAP"], n + 1
    return n


@pytest.mark.parametrize("name", sorted(MODELS))
def test_device_mode_builds_one_scorer_and_reads_s_for_new_bests_only(gpu, monkeypatch, name):
    counts = _counting(monkeypatch)
    rec, results = _fit(name, "device")
    n = len(results)
    assert n == 4
    assert counts["scorer"] == 1                                    # host mode: one per validation (below)
    assert counts["update_from"] == n - 1
    assert counts["get_S_and_W"] == 2                               # the first validation and the final model; nothing synced
    assert counts["get_S"] == 1 + _new_bests_after_the_first(results)      # fit's initial S, then one per new best
    counts.clear()
    _, results_host = _fit(name, "host")
    assert results_host == results
    assert counts["scorer"] == n and counts["get_S_and_W"] == n + 1 and counts["get_S"] == 1 and counts.get("update_from", 0) == 0


# ---- stale host attributes --------------------------------------------------------------------------------------------------------

def test_host_reads_in_the_middle_of_a_device_mode_fit_see_the_model_under_validation(gpu, monkeypatch, tmp_path):
    counts = _counting(monkeypatch)
    users = ALL_USERS[::3]
    folder = str(tmp_path) + os.sep

    def during(rec, validation):
        scorer = rec.device_scorer()
        assert rec._scorer_current and rec._host_model_stale == (validation > 0)
        if validation == 0:
            return
        stale_W = rec.W_sparse
        synced = counts["get_S_and_W"]
        if validation == 2:
            rec.save_model(folder, "mid_fit")
            loaded = SLIM_BPR_MI355X(URM_TRAIN, verbose=False)
            loaded.load_model(folder, "mid_fit")
            _assert_same_weights(loaded.W_sparse, scorer.weights())
        host = rec._compute_item_score(users)
        assert counts["get_S_and_W"] == synced + 1 and not rec._host_model_stale and rec.W_sparse is not stale_W
        rec._compute_item_score(users)
        assert counts["get_S_and_W"] == synced + 1                  # a second read downloads nothing
        _assert_same_weights(rec.W_sparse, scorer.weights())
        _, device = scorer.recommend(users, N_ITEMS, remove_seen=False, return_scores=True)
        assert host.dtype == np.float32 and host.tobytes() == device.tobytes()
        assert rec.device_scorer() is scorer and counts["scorer"] == 1      # the sync built no scorer

    rec, results = _fit("sgd_symmetric", "device", during=during)
    assert counts["get_S_and_W"] == 2 + 3 and counts["scorer"] == 1
    # reading the attributes mid-fit changes nothing of the fit: a new best after a sync still records the right S_best
    _assert_same_fit((rec, results), _fit("sgd_symmetric", "host"))


def test_set_urm_train_in_the_middle_of_a_device_mode_fit_falls_back_to_a_rebuilt_scorer(gpu, monkeypatch):
    counts = _counting(monkeypatch)

    def during(rec, validation):
        if validation != 1:
            return
        old = rec.device_scorer()
        assert rec._host_model_stale and old is rec._sp_scorer
        want = old.recommend(ALL_USERS, N_ITEMS, return_scores=True)[1]
        rec.set_URM_train(URM_TRAIN.copy())
        new = rec.device_scorer()
        assert new is not old and not old._h and counts["scorer"] == 2 and not rec._host_model_stale and not rec._scorer_current
        _assert_same_weights(new.weights(), rec.W_sparse)
        assert new.recommend(ALL_USERS, N_ITEMS, return_scores=True)[1].tobytes() == want.tobytes()

    rec, results = _fit("sgd_symmetric", "device", during=during)
    # the first validation builds a scorer, the second fills it and then falls back to a rebuilt one, the third runs the host path again
    # (one more), the fourth is filled on the device
    assert counts["scorer"] == 3 and counts["update_from"] == 2
    _assert_same_fit((rec, results), _fit("sgd_symmetric", "host"))
