"""EvaluatorHoldout_MI355X on the device against the reference's EvaluatorHoldout (tests/golden/evaluator.npz, written by
tests/golden/make_evaluator_fixture.py from the reference's own evaluator, metric functions and recommenders)."""
import math

import numpy as np
import pytest

from eval_cases import CASES, MODELS, make_case, set_model
from recsys2019_deeplearning_evaluation_amd import EvaluatorHoldout_MI355X, MatrixFactorization_BPR_MI355X
from recsys2019_deeplearning_evaluation_amd import recommender_base as RB
from recsys2019_deeplearning_evaluation_amd.evaluation import METRICS, PER_USER
from recsys2019_deeplearning_evaluation_amd.scoring import GpuScoringMixin, GpuSimilarityScoringMixin
from _util import GOLDEN

FIXTURE = np.load(GOLDEN + "/evaluator.npz")
FLOAT32_VALUES = {"ROC_AUC", "PRECISION", "PRECISION_RECALL_MIN_DEN", "RECALL", "NDCG"}
FLOAT32_ACCUMULATED = FLOAT32_VALUES | {"F1"}
POPULATION = {"DIVERSITY_MEAN_INTER_LIST", "DIVERSITY_HERFINDAHL", "COVERAGE_ITEM", "COVERAGE_USER", "DIVERSITY_GINI", "SHANNON_ENTROPY"}


class _MF(GpuScoringMixin, RB.BaseMatrixFactorizationRecommender):
    RECOMMENDER_NAME = "MF_test"


class _ItemSim(GpuSimilarityScoringMixin, RB.BaseItemSimilarityMatrixRecommender):
    RECOMMENDER_NAME = "ItemSim_test"


class _UserSim(GpuSimilarityScoringMixin, RB.BaseUserSimilarityMatrixRecommender):
    RECOMMENDER_NAME = "UserSim_test"
    _SCORER_USER_BASED = True


CLASSES = {"mf": _MF, "mf_bias": _MF, "item": _ItemSim, "user": _UserSim}


class _ListsOnly:
    """Hides the device scorer of a recommender: the evaluator takes the lists path through its recommend()."""

    def __init__(self, rec):
        self._rec = rec

    def __getattr__(self, name):
        return getattr(self._rec, name)


class _FixtureLists(RB.BaseRecommender):
    """A host recommender that answers with the reference's stored lists."""

    def __init__(self, train, users, table):
        super().__init__(train, verbose=False)
        self._rows = {int(u): [int(i) for i in row if i >= 0] for u, row in zip(users, table)}

    def recommend(self, user_id_array, cutoff=None, remove_seen_flag=True, items_to_compute=None, remove_top_pop_flag=False,
                  remove_custom_items_flag=False, return_scores=False):
        lists = [self._rows[int(u)][:cutoff] for u in user_id_array]
        return (lists, None) if return_scores else lists


def _build(name, model):
    case = make_case(name)
    return case, set_model(CLASSES[model](case["train"], verbose=False), case["models"][model])


def _check_against_reference_dict(results, ref_dict, n_users, cutoffs):
    for c, cutoff in enumerate(cutoffs):
        for m, metric in enumerate(METRICS):
            got, want = results[cutoff][metric], ref_dict[c, m]
            rtol = n_users * 2.0 ** -24 if metric in FLOAT32_ACCUMULATED else 1e-9
            assert got == pytest.approx(want, rel=rtol, abs=1e-300), (cutoff, metric, got, want)


def _bitwise_equal(a, b):
    for cutoff in a:
        for metric in METRICS:
            x, y = a[cutoff][metric], b[cutoff][metric]
            assert x == y or (math.isnan(x) and math.isnan(y)), (cutoff, metric, x, y)
    assert list(a) == list(b) and all(list(a[c]) == list(b[c]) for c in a)


LISTS_CASES = [("binary", "mf"), ("graded", "mf_bias"), ("graded", "item")]


@pytest.mark.gpu
@pytest.mark.parametrize("name,model", LISTS_CASES)
def test_lists_path_per_user_values_match_the_reference(gpu, name, model):
    case = make_case(name)
    tag = "%s_%s" % (name, model)
    users = FIXTURE[name + "_users"]
    rec = _FixtureLists(case["train"], users, FIXTURE[tag + "_lists"])
    ev = EvaluatorHoldout_MI355X(case["test"], case["cutoffs"], verbose=False, **case["kwargs"])
    assert np.array_equal(ev.users_to_evaluate, users)
    ev.evaluateRecommender(rec)
    per_user = ev.per_user_values()
    ref = FIXTURE[tag + "_per_user"]
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
def test_lists_path_result_dict_matches_the_reference(gpu, name, model):
    case = make_case(name)
    tag = "%s_%s" % (name, model)
    users = FIXTURE[name + "_users"]
    rec = _FixtureLists(case["train"], users, FIXTURE[tag + "_lists"])
    ev = EvaluatorHoldout_MI355X(case["test"], case["cutoffs"], verbose=False, **case["kwargs"])
    results, text = ev.evaluateRecommender(rec)
    ref_pu, ref_dict = FIXTURE[tag + "_per_user"], FIXTURE[tag + "_dict"]
    n = len(users)
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
def test_lists_path_item_counters_match_the_reference(gpu, name, model):
    case = make_case(name)
    tag = "%s_%s" % (name, model)
    rec = _FixtureLists(case["train"], FIXTURE[name + "_users"], FIXTURE[tag + "_lists"])
    ev = EvaluatorHoldout_MI355X(case["test"], case["cutoffs"], verbose=False, **case["kwargs"])
    ev.evaluateRecommender(rec)
    for c, cutoff in enumerate(case["cutoffs"]):
        assert np.array_equal(ev.item_counts[cutoff], FIXTURE[tag + "_counts"][c]), cutoff


FUSED_CASES = [(name, model) for name in CASES for model in MODELS[name]]


@pytest.mark.gpu
@pytest.mark.parametrize("name,model", FUSED_CASES)
def test_fused_path_matches_reference_and_lists_path(gpu, name, model):
    case, rec = _build(name, model)
    ev = EvaluatorHoldout_MI355X(case["test"], case["cutoffs"], verbose=False, **case["kwargs"])
    fused, _ = ev.evaluateRecommender(rec)
    _check_against_reference_dict(fused, FIXTURE["%s_%s_dict" % (name, model)], len(ev.users_to_evaluate), case["cutoffs"])
    again, _ = ev.evaluateRecommender(rec)
    _bitwise_equal(fused, again)
    other_blocks, _ = ev.evaluateRecommender(rec, block_size=37)
    _bitwise_equal(fused, other_blocks)
    lists, _ = ev.evaluateRecommender(_ListsOnly(rec))
    _bitwise_equal(fused, lists)
    assert not rec.items_to_ignore_flag


@pytest.mark.gpu
def test_fused_path_counts_match_the_reference_counters(gpu):
    case, rec = _build("graded", "mf_bias")
    ev = EvaluatorHoldout_MI355X(case["test"], case["cutoffs"], verbose=False, **case["kwargs"])
    ev.evaluateRecommender(rec)
    per_user = ev.per_user_values()
    ref = FIXTURE["graded_mf_bias_per_user"]
    for c, cutoff in enumerate(case["cutoffs"]):
        assert np.array_equal(per_user[cutoff]["HIT_RATE"], ref[:, c, PER_USER.index("HIT_RATE")])
        assert np.array_equal(ev.item_counts[cutoff], FIXTURE["graded_mf_bias_counts"][c])


@pytest.mark.gpu
def test_early_stopping_takes_the_device_evaluator(gpu):
    case = make_case("binary")
    ev = EvaluatorHoldout_MI355X(case["test"], [10], verbose=False)
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
