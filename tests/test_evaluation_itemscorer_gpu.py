"""EvaluatorHoldout_MI355X and EvaluatorNegativeItemSample_MI355X with TopPop and GlobalEffects: the fused path through the shared-vector
scorer against the lists path of the same device lists, and against the fused path of the factor scorer with one factor (U = ones,
V = the vector) -- all three must agree bit for bit, whatever the block size."""
import numpy as np
import pytest
import scipy.sparse as sps

from non_personalized_cases import CUTOFFS, case_urm
from recsys2019_deeplearning_evaluation_amd import (EvaluatorHoldout_MI355X, EvaluatorNegativeItemSample_MI355X, GlobalEffects, TopPop)
from test_evaluation_gpu import _ListsOnly, _MF, _bitwise_equal

MODELS = {"toppop": (TopPop, "item_pop", {}), "global_effects": (GlobalEffects, "item_bias", dict(lambda_user=10, lambda_item=25))}


@pytest.fixture(scope="module")
def split(gpu):
    """The `ratings` URM of the fixture split 80 / 20 by cell, sampled negatives for every user, the two fitted models and their
    one-factor stand-ins."""
    rng = np.random.default_rng(5)
    URM = sps.csr_matrix(case_urm("ratings"))
    to_test = rng.random(URM.nnz) < 0.2
    coo = URM.tocoo()
    train = sps.csr_matrix((coo.data[~to_test], (coo.row[~to_test], coo.col[~to_test])), shape=URM.shape)
    test = sps.csr_matrix((coo.data[to_test], (coo.row[to_test], coo.col[to_test])), shape=URM.shape)
    dense = URM.toarray() != 0
    negative = sps.csr_matrix(((rng.random(URM.shape) < 0.15) & ~dense).astype(np.float32))
    out = dict(train=train, test=test, negative=negative, models={})
    for name, (cls, vector, kw) in MODELS.items():
        rec = cls(train, verbose=False)
        rec.fit(**kw)
        stand_in = _MF(train, verbose=False)
        stand_in.USER_factors = np.ones((train.shape[0], 1), np.float32)
        stand_in.ITEM_factors = np.ascontiguousarray(np.asarray(getattr(rec, vector), dtype=np.float32)[:, None])
        out["models"][name] = (rec, stand_in)
    return out


def _evaluators(split, **kwargs):
    return {"holdout": EvaluatorHoldout_MI355X(split["test"], CUTOFFS, verbose=False, **kwargs),
            "negative": EvaluatorNegativeItemSample_MI355X(split["test"], split["negative"], CUTOFFS, verbose=False, **kwargs)}


@pytest.mark.gpu
@pytest.mark.parametrize("evaluator", ["holdout", "negative"])
@pytest.mark.parametrize("model", list(MODELS))
def test_fused_path_equals_lists_path_and_one_factor_route(split, model, evaluator, monkeypatch):
    rec, stand_in = split["models"][model]
    ev = _evaluators(split)[evaluator]
    calls = []
    real = ev._run_fused
    monkeypatch.setattr(ev, "_run_fused", lambda scorer, add, *a: (calls.append(add), real(scorer, add, *a))[1])
    fused, _ = ev.evaluateRecommender(rec)
    assert calls == ["add_itemscorer" if evaluator == "holdout" else "add_itemscorer_candidates"]
    assert fused[CUTOFFS[0]]["PRECISION"] > 0 and fused[CUTOFFS[-1]]["COVERAGE_USER"] > 0.9
    for block in (7, 1000):
        _bitwise_equal(fused, ev.evaluateRecommender(rec, block_size=block)[0])
        _bitwise_equal(fused, ev.evaluateRecommender(_ListsOnly(rec), block_size=block)[0])
    _bitwise_equal(fused, ev.evaluateRecommender(stand_in)[0])
    assert calls[-1] == ("add_scorer" if evaluator == "holdout" else "add_scorer_candidates")


@pytest.mark.gpu
@pytest.mark.parametrize("evaluator", ["holdout", "negative"])
def test_ignored_items_and_seen_items_go_through_the_mask(split, evaluator):
    rec, stand_in = split["models"]["toppop"]
    ignore = np.argsort(-rec.item_pop)[:30]
    ev = _evaluators(split, ignore_items=ignore, exclude_seen=False)[evaluator]
    fused, _ = ev.evaluateRecommender(rec)
    _bitwise_equal(fused, ev.evaluateRecommender(_ListsOnly(rec))[0])
    _bitwise_equal(fused, ev.evaluateRecommender(stand_in)[0])
    assert not rec.items_to_ignore_flag


@pytest.mark.gpu
@pytest.mark.parametrize("evaluator", ["holdout", "negative"])
def test_cold_user_request_raises_the_reference_message(split, evaluator):
    few = split["train"][:split["train"].shape[0] - 5]
    rec = TopPop(few, verbose=False)
    rec.fit()
    ev = _evaluators(split)[evaluator]
    with pytest.raises(ValueError, match="Cold users not allowed. Users in trained model are %d" % few.shape[0]):
        ev.evaluateRecommender(rec)
