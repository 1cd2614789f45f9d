"""EvaluatorNegativeItemSample_MI355X and the scorers' recommend_candidates on the device against the reference's
EvaluatorNegativeItemSample (tests/golden/evaluator_negative.npz, written by tests/golden/make_negative_evaluator_fixture.py from the
reference's own evaluator, metric functions and recommenders) and against a NumPy ranking oracle."""
import math

import numpy as np
import pytest
import scipy.sparse as sps

from negative_eval_cases import CASES, MODELS, ROW_LIMIT, make_case, set_model
from recsys2019_deeplearning_evaluation_amd import (EvaluatorHoldout_MI355X, EvaluatorNegativeItemSample_MI355X, MatrixFactorization_BPR_MI355X,
                                                    MI355XScorer, MI355XSparseScorer)
from recsys2019_deeplearning_evaluation_amd import _native as N
from recsys2019_deeplearning_evaluation_amd.evaluation import METRICS, PER_USER
# the helpers and the tolerances of the holdout evaluator's tests: n_users * 2^-24 relative for the float32-accumulated metrics, 1e-9 elsewhere
from test_evaluation_gpu import (CLASSES, FLOAT32_VALUES, POPULATION, _FixtureLists, _ListsOnly, _bitwise_equal,
                                 _check_against_reference_dict)
from _util import GOLDEN

FIXTURE = np.load(GOLDEN + "/evaluator_negative.npz")
LISTS_CASES = [("sampled", "mf"), ("sampled_graded", "mf_bias"), ("sampled_graded", "item")]
FUSED_CASES = [(name, model) for name in CASES for model in MODELS[name]]


def _evaluator(case, **kwargs):
    return EvaluatorNegativeItemSample_MI355X(case["test"], case["negative"], case["cutoffs"], verbose=False, **case["kwargs"], **kwargs)


def _build(name, model):
    case = make_case(name)
    return case, set_model(CLASSES[model](case["train"], verbose=False), case["models"][model])


@pytest.fixture(scope="module")
def replayed(gpu):
    """The reference's stored lists through the lists path, once per replayed (case, model): evaluator, results, text."""
    out = {}
    for name, model in LISTS_CASES:
        case = make_case(name)
        tag = "%s_%s" % (name, model)
        rec = _FixtureLists(case["train"], FIXTURE[name + "_users"], FIXTURE[tag + "_lists"])
        ev = _evaluator(case)
        out[name, model] = (ev,) + ev.evaluateRecommender(rec)
    return out


@pytest.mark.gpu
@pytest.mark.parametrize("name,model", LISTS_CASES)
def test_lists_path_per_user_values_match_the_reference(replayed, name, model):
    case = make_case(name)
    ev = replayed[name, model][0]
    assert np.array_equal(ev.users_to_evaluate, FIXTURE[name + "_users"])
    per_user = ev.per_user_values()
    ref = FIXTURE["%s_%s_per_user" % (name, model)]
    for c, cutoff in enumerate(case["cutoffs"]):
        for v, metric in enumerate(PER_USER):
            got, want = per_user[cutoff][metric], ref[:, c, v]
            if metric == "HIT_RATE":
                assert np.array_equal(got, want), (cutoff, metric)
            else:
                np.testing.assert_allclose(got, want, rtol=1e-6 if metric in FLOAT32_VALUES else 1e-12, atol=0, err_msg="%s@%d" % (metric, cutoff))
                if metric in FLOAT32_VALUES:
                    assert np.array_equal(got, got.astype(np.float32)), "float32 metrics keep their float32 value"


@pytest.mark.gpu
@pytest.mark.parametrize("name,model", LISTS_CASES)
def test_lists_path_result_dict_matches_the_reference(replayed, name, model):
    case = make_case(name)
    tag = "%s_%s" % (name, model)
    _, results, text = replayed[name, model]
    ref_pu, ref_dict = FIXTURE[tag + "_per_user"], FIXTURE[tag + "_dict"]
    n = len(FIXTURE[name + "_users"])
    for c, cutoff in enumerate(case["cutoffs"]):
        assert list(results[cutoff]) == METRICS
        for v, metric in enumerate(PER_USER):
            want = math.fsum(ref_pu[:, c, v]) / n
            rtol = 1e-6 if metric in FLOAT32_VALUES else 1e-12
            assert results[cutoff][metric] == pytest.approx(want, rel=rtol, abs=1e-300), (cutoff, metric)
        for metric in POPULATION:
            assert results[cutoff][metric] == pytest.approx(ref_dict[c, METRICS.index(metric)], rel=1e-12), (cutoff, metric)
    _check_against_reference_dict(results, ref_dict, n, case["cutoffs"])
    assert text.startswith("CUTOFF: 1 - ROC_AUC: ")


@pytest.mark.gpu
@pytest.mark.parametrize("name,model", LISTS_CASES)
def test_lists_path_item_counters_match_the_reference(replayed, name, model):
    case = make_case(name)
    ev = replayed[name, model][0]
    for c, cutoff in enumerate(case["cutoffs"]):
        assert np.array_equal(ev.item_counts[cutoff], FIXTURE["%s_%s_counts" % (name, model)][c]), cutoff


@pytest.mark.gpu
@pytest.mark.parametrize("name,model", FUSED_CASES)
def test_fused_path_matches_reference_and_lists_path(gpu, name, model, capsys):
    case, rec = _build(name, model)
    ev = EvaluatorNegativeItemSample_MI355X(case["test"], case["negative"], case["cutoffs"], verbose=True, **case["kwargs"])
    said = capsys.readouterr().out
    # a row past the limit sends the whole evaluation through recommend(), and the evaluator says so once, when it is built
    assert ev.candidates_on_device == (name != "long_rows_over")
    assert said.count("goes through recommend()") == (name == "long_rows_over")
    assert np.array_equal(ev.URM_items_to_rank.indptr, FIXTURE[name + "_rank_indptr"])
    assert np.array_equal(ev.URM_items_to_rank.indices, FIXTURE[name + "_rank_indices"])
    fused, _ = ev.evaluateRecommender(rec)
    _check_against_reference_dict(fused, FIXTURE["%s_%s_dict" % (name, model)], len(ev.users_to_evaluate), case["cutoffs"])
    again, _ = ev.evaluateRecommender(rec)
    _bitwise_equal(fused, again)
    other_blocks, _ = ev.evaluateRecommender(rec, block_size=37)
    _bitwise_equal(fused, other_blocks)
    lists, _ = ev.evaluateRecommender(_ListsOnly(rec))
    _bitwise_equal(fused, lists)
    assert not rec.items_to_ignore_flag
    assert "goes through recommend()" not in capsys.readouterr().out


@pytest.mark.gpu
def test_fused_path_counts_match_the_reference_counters(gpu):
    case, rec = _build("sampled_graded", "mf_bias")
    ev = _evaluator(case)
    ev.evaluateRecommender(rec)
    per_user = ev.per_user_values()
    ref = FIXTURE["sampled_graded_mf_bias_per_user"]
    for c, cutoff in enumerate(case["cutoffs"]):
        assert np.array_equal(per_user[cutoff]["HIT_RATE"], ref[:, c, PER_USER.index("HIT_RATE")])
        assert np.array_equal(ev.item_counts[cutoff], FIXTURE["sampled_graded_mf_bias_counts"][c])


@pytest.mark.gpu
def test_users_without_an_admissible_candidate_get_an_empty_list(gpu):
    case, rec = _build("sampled", "mf")
    ev = _evaluator(case)
    ev.evaluateRecommender(rec)
    at = {int(u): p for p, u in enumerate(ev.users_to_evaluate)}
    covered = sum(ev.item_counts[200])
    assert covered == sum(min(200, n) for n in _admissible_counts(case, ev))
    ranked = rec._get_scorer().recommend_candidates(np.arange(16), ev.URM_items_to_rank[:16], 200)
    assert np.all(ranked[:4] == -1) and all(u in at for u in range(4))
    assert list((ranked >= 0).sum(axis=1)[4:]) == [1, 1, 1, 1, 5, 5, 10, 10, 64, 64, 65, 65]


def _admissible_counts(case, ev):
    rows, train = ev.URM_items_to_rank, sps.csr_matrix(case["train"])
    return [len(np.setdiff1d(rows.indices[rows.indptr[u]:rows.indptr[u + 1]], train.indices[train.indptr[u]:train.indptr[u + 1]]))
            for u in ev.users_to_evaluate]


# ---- candidate ranking, exactly -----------------------------------------------------------------------------------------------

def _oracle(scores, users, rows, cutoff, seen, mask):
    """np.lexsort((item, -score)) over each user's filtered candidates, -1 padded."""
    out = np.full((len(users), cutoff), -1, np.int32)
    for r, u in enumerate(users):
        items = rows.indices[rows.indptr[r]:rows.indptr[r + 1]]
        if seen is not None:
            items = np.setdiff1d(items, seen.indices[seen.indptr[u]:seen.indptr[u + 1]])
        if mask is not None:
            items = items[mask[items] != 0]
        order = np.lexsort((items, -scores[u, items]))[:cutoff]
        out[r, :len(order)] = items[order]
    return out


def _rows(rng, lengths, n_items):
    indptr = np.concatenate([[0], np.cumsum(lengths)])
    indices = np.concatenate([np.sort(rng.choice(n_items, n, replace=False)) for n in lengths] + [np.zeros(0, np.int64)])
    return sps.csr_matrix((np.ones(len(indices), np.float32), indices, indptr), shape=(len(lengths), n_items))


def _draw_sparse(rng, n_rows, n_cols, per_row, values):
    """per_row uniformly drawn cells in every row (repeats add up), values(n) their contents."""
    rows = np.repeat(np.arange(n_rows), per_row)
    m = sps.csr_matrix(sps.coo_matrix((values(len(rows)), (rows, rng.integers(0, n_cols, len(rows)))), shape=(n_rows, n_cols)))
    m.sum_duplicates()
    return m


N_USERS, N_ITEMS = 24, 500
LENGTHS = [0, 1, 5, 9, 10, 11, 63, 64, 65, 100, 199, 200, 201, 300, 500]


def _check_scorer(scorer, scores, seen, rng, n_items=N_ITEMS, lengths=LENGTHS, cutoffs=(10, 100)):
    users = np.concatenate([rng.permutation(N_USERS)[:len(lengths) - 3], [3, 3, 3]])         # a user three times, with a row each
    rows = _rows(rng, lengths, n_items)
    mask = (rng.random(n_items) < 0.8).astype(np.uint8)
    emptied = mask.copy()
    emptied[rows.indices[rows.indptr[9]:rows.indptr[10]]] = 0                                 # the mask leaves nothing of row 9
    for cutoff in cutoffs:
        for remove_seen in (True, False):
            for allowed in (None, mask, emptied):
                got = scorer.recommend_candidates(users, rows, cutoff, remove_seen, allowed)
                want = _oracle(scores, users, rows, cutoff, seen if remove_seen else None, allowed)
                assert got.dtype == np.int32 and np.array_equal(got, want), (cutoff, remove_seen, allowed is not None)
                assert allowed is not emptied or np.all(got[9] == -1)
    one = scorer.recommend_candidates(5, rows[13], 100)                                       # a batch of one
    assert np.array_equal(one, _oracle(scores, [5], rows[13], 100, seen, None))


@pytest.mark.gpu
@pytest.mark.parametrize("bias", [False, True])
@pytest.mark.parametrize("k", [1, 3, 16, 63, 64, 65, 128, 200])
def test_factor_candidates_rank_exactly_with_masses_of_ties(gpu, k, bias):
    rng = np.random.default_rng(1000 * k + bias)
    U = rng.integers(-1, 2, (N_USERS, k)).astype(np.float32)                # scores are small integers: dozens of items per value
    V = rng.integers(-1, 2, (N_ITEMS, k)).astype(np.float32)
    seen = sps.random(N_USERS, N_ITEMS, 0.2, format="csr", dtype=np.float32, random_state=k)
    scores = U.astype(np.int64) @ V.astype(np.int64).T
    kwargs = {}
    if bias:
        bu, bi = rng.integers(-2, 3, N_USERS), rng.integers(-2, 3, N_ITEMS)
        scores = scores + bu[:, None] + bi[None, :] + 1
        kwargs = dict(USER_bias=bu.astype(np.float32), ITEM_bias=bi.astype(np.float32), GLOBAL_bias=1.0)
    scorer = MI355XScorer(U, V, seen, **kwargs)
    assert len(np.unique(scores)) * 20 < scores.size
    _check_scorer(scorer, scores, seen, rng)
    assert scorer.score_capacity() == 0


@pytest.mark.gpu
def test_factor_candidates_with_512_factors(gpu):
    rng = np.random.default_rng(512)
    U = rng.integers(-1, 2, (N_USERS, 512)).astype(np.float32)
    V = rng.integers(-1, 2, (N_ITEMS, 512)).astype(np.float32)
    seen = sps.random(N_USERS, N_ITEMS, 0.2, format="csr", dtype=np.float32, random_state=512)
    _check_scorer(MI355XScorer(U, V, seen), U.astype(np.int64) @ V.astype(np.int64).T, seen, rng, cutoffs=(100,))


@pytest.mark.gpu
@pytest.mark.parametrize("n_items", [N_ITEMS, 40000])                       # the score row in LDS, and in HBM
def test_similarity_candidates_rank_exactly_with_masses_of_ties(gpu, n_items):
    rng = np.random.default_rng(n_items)
    A = _draw_sparse(rng, N_USERS, n_items, 20, lambda n: np.ones(n, np.float32))
    B = _draw_sparse(rng, n_items, n_items, 40, lambda n: rng.integers(1, 4, n).astype(np.float32))
    scores = np.asarray((A @ B).todense()).astype(np.int64)                 # small integers and many zeros
    scorer = MI355XSparseScorer(A, B, A)
    lengths = LENGTHS[:-1] + [min(n_items, 1500)]
    _check_scorer(scorer, scores, A, rng, n_items, lengths)


@pytest.mark.gpu
def test_long_candidate_rows_and_the_limits(gpu):
    rng = np.random.default_rng(4096)
    n_items = 6000
    U = rng.integers(-2, 3, (N_USERS, 8)).astype(np.float32)
    V = rng.integers(-2, 3, (n_items, 8)).astype(np.float32)
    seen = sps.random(N_USERS, n_items, 0.05, format="csr", dtype=np.float32, random_state=3)
    scores = U.astype(np.int64) @ V.astype(np.int64).T
    scorer = MI355XScorer(U, V, seen)
    sparse = MI355XSparseScorer(sps.csr_matrix(U != 0, dtype=np.float32), sps.csr_matrix(np.abs(V.T)), seen)
    sparse_scores = (U != 0).astype(np.int64) @ np.abs(V.T).astype(np.int64)
    lengths = [1024, 1025, 2048, 2049, ROW_LIMIT, 0, 100]                   # both sides of the counting-rank | bitonic-sort switch, the limit
    users = np.arange(len(lengths))
    rows = _rows(rng, lengths, n_items)
    for cutoff in (50, ROW_LIMIT):
        for remove_seen in (True, False):
            got = scorer.recommend_candidates(users, rows, cutoff, remove_seen)
            assert np.array_equal(got, _oracle(scores, users, rows, cutoff, seen if remove_seen else None, None)), (cutoff, remove_seen)
        got = sparse.recommend_candidates(users, rows, cutoff)
        assert np.array_equal(got, _oracle(sparse_scores, users, rows, cutoff, seen, None)), cutoff
    too_long = _rows(rng, [ROW_LIMIT + 1], n_items)
    for s in (scorer, sparse):
        with pytest.raises(NotImplementedError):
            s.recommend_candidates([0], too_long, 10)
        with pytest.raises(NotImplementedError):
            s.recommend_candidates([0], rows[:1], ROW_LIMIT + 1)
        with pytest.raises(ValueError):
            s.recommend_candidates([0, 1], rows[:1], 10)                    # a row per user
        with pytest.raises(ValueError):
            s.recommend_candidates([N_USERS], rows[:1], 10)                 # cold user
        # the C function checks what the wrapper would have put right: ids in range, strictly ascending
        ranked = np.empty((1, 10), np.int32)
        user = np.zeros(1, np.int32)
        for indptr, indices in (([0, 3], [5, 4, 7]), ([0, 3], [4, 4, 7]), ([0, 2], [5, n_items]), ([0, 2], [-1, 3]), ([1, 2], [1, 2])):
            indptr, indices = np.array(indptr, np.int32), np.array(indices, np.int32)
            with pytest.raises(ValueError):
                s._call("recommend_candidates", N.ptr(user), 1, N.ptr(indptr), N.ptr(indices), 10, 1, None, N.ptr(ranked))


@pytest.mark.gpu
def test_the_evaluator_checks_its_candidate_rows(gpu):
    case = make_case("sampled")
    ev = _evaluator(case)
    n_users = case["test"].shape[0]
    indptr = np.zeros(n_users + 1, np.int32)
    indptr[1:] = 2
    with pytest.raises(ValueError):
        ev._call("set_candidates", N.ptr(indptr), N.ptr(np.array([7, 3], np.int32)))
    with pytest.raises(ValueError):
        ev._call("set_candidates", N.ptr(indptr), N.ptr(np.array([7, 320], np.int32)))
    wide_lists = EvaluatorNegativeItemSample_MI355X(make_case("long_rows")["test"], make_case("long_rows")["negative"], [ROW_LIMIT + 1],
                                                    verbose=False)
    assert not wide_lists.candidates_on_device                              # lists wider than the ranking's limit


# ---- what the fused path does not do ---------------------------------------------------------------------------------------

@pytest.mark.gpu
def test_a_fused_factor_evaluation_does_no_full_row_work(gpu):
    case, rec = _build("sampled", "mf")
    scorer = rec._get_scorer()
    assert scorer.score_capacity() == 0
    ev = _evaluator(case)
    ev.evaluateRecommender(rec)
    assert rec._get_scorer() is scorer and scorer.score_capacity() == 0     # no (users x n_items) score buffer
    holdout = EvaluatorHoldout_MI355X(case["test"], case["cutoffs"], verbose=False)
    holdout.evaluateRecommender(rec)
    grown = scorer.score_capacity()
    assert grown >= 320                                                     # (the full-catalogue path is what allocates it)
    ev.evaluateRecommender(rec)
    assert scorer.score_capacity() == grown


class _FullCatalogue(EvaluatorNegativeItemSample_MI355X):
    """An evaluator with candidate rows uploaded that runs the parent's full-catalogue paths: mi355rec_eval_add_scorer / add_spscorer on
    a handle that mi355rec_eval_set_candidates has been called on."""
    _run = EvaluatorHoldout_MI355X._run
    _run_lists = EvaluatorHoldout_MI355X._run_lists


@pytest.mark.gpu
@pytest.mark.parametrize("model", ["mf", "item"])
def test_the_candidate_rows_do_not_change_the_full_catalogue_calls(gpu, model):
    case, rec = _build("sampled", model)
    ev = _FullCatalogue(case["test"], case["negative"], case["cutoffs"], verbose=False)
    assert ev.candidates_on_device
    holdout = EvaluatorHoldout_MI355X(case["test"], case["cutoffs"], verbose=False)
    _bitwise_equal(ev.evaluateRecommender(rec)[0], holdout.evaluateRecommender(rec)[0])


@pytest.mark.gpu
def test_early_stopping_takes_the_negative_sample_evaluator(gpu):
    case = make_case("sampled")
    ev = EvaluatorNegativeItemSample_MI355X(case["test"], case["negative"], [10], verbose=False)
    seen = []

    class Recording:
        def evaluateRecommender(self, rec):
            results, text = ev.evaluateRecommender(rec)
            seen.append(results[10]["MAP"])
            return results, text

    rec = MatrixFactorization_BPR_MI355X(case["train"], verbose=False)
    rec.fit(epochs=6, num_factors=16, batch_size=64, learning_rate=0.05, random_seed=7, validation_every_n=2,
            evaluator_object=Recording(), validation_metric="MAP")
    assert len(seen) == 3
    assert rec.best_validation_metric == max(seen)
    direct = MatrixFactorization_BPR_MI355X(case["train"], verbose=False)
    direct.fit(epochs=2, num_factors=16, batch_size=64, learning_rate=0.05, random_seed=7, validation_every_n=1, evaluator_object=ev,
               validation_metric="MAP")
    assert direct.best_validation_metric is not None
