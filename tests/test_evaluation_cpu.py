"""Host parts of EvaluatorHoldout_MI355X: the O(n_items) finalisation against the reference's values (tests/golden/evaluator.npz), the
result string, argument errors, and no host path without a device."""
import numpy as np
import pytest
import scipy.sparse as sps

from eval_cases import make_case
from recsys2019_deeplearning_evaluation_amd import EvaluatorHoldout_MI355X, _native
from recsys2019_deeplearning_evaluation_amd.evaluation import METRICS, f1_score, get_result_string, population_metrics
from _util import GOLDEN

FIXTURE = np.load(GOLDEN + "/evaluator.npz")
POPULATION = ["DIVERSITY_MEAN_INTER_LIST", "DIVERSITY_HERFINDAHL", "COVERAGE_ITEM", "COVERAGE_USER", "DIVERSITY_GINI", "SHANNON_ENTROPY"]


@pytest.mark.parametrize("name,model", [("binary", "mf"), ("graded", "mf_bias"), ("graded", "item")])
def test_population_metrics_from_the_reference_counters(name, model):
    case = make_case(name)
    tag = "%s_%s" % (name, model)
    counts, ref = FIXTURE[tag + "_counts"], FIXTURE[tag + "_dict"]
    n_eval = len(FIXTURE[name + "_users"])
    n_users = case["test"].shape[0]
    n_ignore_users = len(case["kwargs"].get("ignore_users", []))
    covered = (FIXTURE[tag + "_lists"] >= 0).any(axis=1)        # (no list is empty at cutoff 1 unless it is empty)
    for c, cutoff in enumerate(case["cutoffs"]):
        got = population_metrics(counts[c], n_eval, cutoff, case["kwargs"].get("ignore_items", []), n_users, n_ignore_users,
                                 int(covered.sum()))
        for metric in POPULATION:
            assert got[metric] == pytest.approx(ref[c, METRICS.index(metric)], rel=1e-12), (cutoff, metric)


def test_f1_from_the_reference_precision_and_recall():
    for tag in ("binary_mf", "graded_user", "wide_mf"):
        ref = FIXTURE[tag + "_dict"]
        for row in ref:
            p, r = row[METRICS.index("PRECISION")], row[METRICS.index("RECALL")]
            assert f1_score(float(p), float(r)) == pytest.approx(row[METRICS.index("F1")], rel=1e-6)
    assert f1_score(0.0, 0.0) == 0.0


def test_result_string_has_the_reference_format():
    results = {5: {"ROC_AUC": 0.5, "PRECISION": 1 / 3}, 10: {"ROC_AUC": 1.0, "PRECISION": 0.25}}
    assert get_result_string(results) == ("CUTOFF: 5 - ROC_AUC: 0.5000000, PRECISION: 0.3333333, \n"
                                          "CUTOFF: 10 - ROC_AUC: 1.0000000, PRECISION: 0.2500000, \n")


def test_argument_errors_come_before_the_device():
    X = sps.random(20, 10, 0.3, format="csr", dtype=np.float32, random_state=0)
    with pytest.raises(ValueError):
        EvaluatorHoldout_MI355X([X], [5])
    with pytest.raises(NotImplementedError):
        EvaluatorHoldout_MI355X(X, [5], diversity_object=object())


def test_no_host_path_without_a_device():
    if _native.device_count() > 0:
        pytest.skip("a device is present")
    X = sps.random(20, 10, 0.3, format="csr", dtype=np.float32, random_state=0)
    with pytest.raises(_native.NativeLibraryError):
        EvaluatorHoldout_MI355X(X, [5], verbose=False)
