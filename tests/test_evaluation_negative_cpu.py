"""Host parts of EvaluatorNegativeItemSample_MI355X against the reference's EvaluatorNegativeItemSample
(tests/golden/evaluator_negative.npz, written by tests/golden/make_negative_evaluator_fixture.py): the candidate rows, the evaluated
users and the argument errors."""
import contextlib
import io

import numpy as np
import pytest
import scipy.sparse as sps

from negative_eval_cases import CASES, ROW_LIMIT, candidate_mask, make_case
from recsys2019_deeplearning_evaluation_amd import EvaluatorNegativeItemSample_MI355X, _native
from recsys2019_deeplearning_evaluation_amd.evaluation import items_to_rank, users_to_evaluate
from oracle import ref_loader
from _util import GOLDEN

FIXTURE = np.load(GOLDEN + "/evaluator_negative.npz")


@pytest.mark.parametrize("name", CASES)
def test_items_to_rank_equals_the_reference_rows(name):
    case = make_case(name)
    rows = items_to_rank(case["test"], case["negative"])
    assert rows.shape == case["test"].shape and rows.has_sorted_indices
    assert np.array_equal(rows.indptr, FIXTURE[name + "_rank_indptr"])
    assert np.array_equal(rows.indices, FIXTURE[name + "_rank_indices"])
    assert np.all(rows.data == 1)
    assert np.array_equal(rows.toarray() != 0, candidate_mask(case["test"], case["negative"]))


def test_the_cases_hold_what_they_are_meant_to_reach():
    sampled = make_case("sampled")
    stored = sps.csr_matrix(sampled["negative"])
    assert (stored.data == 0).sum() > 0                                             # explicit zeros among the negatives
    assert sps.csr_matrix(sampled["test"]).multiply(stored).nnz > 0                 # an item in both matrices
    assert stored.multiply(sampled["train"]).nnz > 0                                # train items among the negatives
    lengths = {name: np.diff(FIXTURE[name + "_rank_indptr"]) for name in CASES}
    assert list(lengths["long_rows"][:3]) == [1024, 1025, ROW_LIMIT] and lengths["long_rows"].max() == ROW_LIMIT
    assert lengths["long_rows_over"][3] == ROW_LIMIT + 1
    assert np.all(lengths["wide"] == 200)
    graded = make_case("sampled_graded")
    assert candidate_mask(graded["test"], graded["negative"])[:, graded["kwargs"]["ignore_items"]].any()
    assert len(np.unique(graded["test"].data)) > 1


@pytest.mark.parametrize("name", CASES)
def test_items_to_rank_equals_the_live_reference_class(name):
    reference = ref_loader.load_python_reference("Base.Evaluation.Evaluator", "EvaluatorNegativeItemSample")
    if reference is None:
        pytest.skip("the reference tree is not present")
    case = make_case(name)
    with contextlib.redirect_stdout(io.StringIO()):
        theirs = reference(case["test"], case["negative"], case["cutoffs"], **case["kwargs"]).URM_items_to_rank
    ours = items_to_rank(case["test"], case["negative"])
    theirs.sort_indices()
    assert np.array_equal(ours.indptr, theirs.indptr) and np.array_equal(ours.indices, theirs.indices)


def test_items_to_rank_on_a_hand_made_example():
    test = sps.csr_matrix((np.array([5.0, 0.0, 2.0]), np.array([3, 1, 0]), np.array([0, 2, 2, 3])), shape=(3, 5))
    negative = sps.csr_matrix((np.array([1.0, 1.0, 0.0, 1.0, 1.0]), np.array([4, 3, 2, 0, 2]), np.array([0, 3, 4, 5])), shape=(3, 5))
    rows = items_to_rank(test, negative)
    assert rows.indptr.tolist() == [0, 2, 3, 5]
    assert rows.indices.tolist() == [3, 4, 0, 0, 2]         # item 3 once, the stored zeros (1 in test, 2 in negative) dropped, ascending
    with pytest.raises(ValueError):
        items_to_rank(test, sps.csr_matrix((3, 6)))


@pytest.mark.parametrize("name", CASES)
def test_users_to_evaluate_equal_the_fixture(name):
    case = make_case(name)
    kw = case["kwargs"]
    users, _ = users_to_evaluate(case["test"], kw.get("min_ratings_per_user", 1), kw.get("ignore_items"), kw.get("ignore_users"))
    assert users.dtype == np.int32 and np.array_equal(users, FIXTURE[name + "_users"])


def test_argument_errors_come_before_the_device():
    X = sps.random(20, 10, 0.3, format="csr", dtype=np.float32, random_state=0)
    negative = sps.random(20, 10, 0.3, format="csr", dtype=np.float32, random_state=1)
    with pytest.raises(ValueError):
        EvaluatorNegativeItemSample_MI355X([X], negative, [5])
    with pytest.raises(ValueError):
        EvaluatorNegativeItemSample_MI355X(X, sps.csr_matrix((20, 11)), [5])
    with pytest.raises(ValueError):
        EvaluatorNegativeItemSample_MI355X(X, sps.csr_matrix((19, 10)), [5])
    with pytest.raises(NotImplementedError):
        EvaluatorNegativeItemSample_MI355X(X, negative, [5], diversity_object=object())
    with pytest.raises(ValueError):
        EvaluatorNegativeItemSample_MI355X(X, negative, [5, 5])


def test_no_host_path_without_a_device():
    if _native.device_count() > 0:
        pytest.skip("a device is present")
    X = sps.random(20, 10, 0.3, format="csr", dtype=np.float32, random_state=0)
    with pytest.raises(_native.NativeLibraryError):
        EvaluatorNegativeItemSample_MI355X(X, X, [5], verbose=False)
