"""Reference-generated fixture for the device holdout evaluator: the REFERENCE's own EvaluatorHoldout (Base/Evaluation/Evaluator.py:382),
metric functions (Base/Evaluation/metrics.py) and recommenders (Base/BaseMatrixFactorizationRecommender.py,
Base/BaseSimilarityMatrixRecommender.py), imported from the reference tree, on the seeded cases of tests/eval_cases.py.  For every
(case, model): the reference's EvaluatorHoldout result dict; for the ones the lists-path tests replay, also the reference's ranked lists,
the per-user value of every metric at every cutoff (the reference's functions, called as Evaluator.py:323-348 calls them) and the
item counters of its Coverage_Item objects.  Writes tests/golden/evaluator.npz.
Run where the reference tree exists:  python tests/golden/make_evaluator_fixture.py"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from oracle import ref_loader                                                   # noqa: E402
from eval_cases import CASES, MODELS, make_case, set_model                      # noqa: E402

MF = ref_loader.load_python_reference("Base.BaseMatrixFactorizationRecommender", "BaseMatrixFactorizationRecommender")
assert MF is not None, "needs the reference tree"
from Base.BaseSimilarityMatrixRecommender import BaseItemSimilarityMatrixRecommender, BaseUserSimilarityMatrixRecommender  # noqa: E402
from Base.Evaluation.Evaluator import EvaluatorHoldout, EvaluatorMetrics, _remove_item_interactions                      # noqa: E402
from Base.Evaluation import metrics as M                                                                                 # noqa: E402

METRICS = [m.value for m in EvaluatorMetrics if m != EvaluatorMetrics.DIVERSITY_SIMILARITY]
PER_USER = ["ROC_AUC", "PRECISION", "PRECISION_RECALL_MIN_DEN", "RECALL", "MAP", "MRR", "NDCG", "HIT_RATE", "ARHR", "NOVELTY",
            "AVERAGE_POPULARITY"]
KEEP_LISTS = {("binary", "mf"), ("graded", "mf_bias"), ("graded", "item")}
BASES = {"mf": MF, "mf_bias": MF, "item": BaseItemSimilarityMatrixRecommender, "user": BaseUserSimilarityMatrixRecommender}


def evaluated_users(case):
    kw = case["kwargs"]
    pruned = _remove_item_interactions(case["test"], np.array(kw.get("ignore_items", [])))
    users = np.flatnonzero(np.ediff1d(pruned.indptr) >= kw.get("min_ratings_per_user", 1))
    return np.setdiff1d(users, kw.get("ignore_users", []))


def reference_lists(rec, case, users):
    """recommend() of the reference on the sorted users, one block, as EvaluatorHoldout calls it (Evaluator.py:436-442); asserts that
    no list reaches a tied score (ties make the order of equal items arbitrary in the reference)."""
    kw = case["kwargs"]
    cutoff = max(case["cutoffs"])
    if "ignore_items" in kw:
        rec.set_items_to_ignore(np.array(kw["ignore_items"]))
    lists, scores = rec.recommend(users, remove_seen_flag=kw.get("exclude_seen", True), cutoff=cutoff, remove_top_pop_flag=False,
                                  remove_custom_items_flag="ignore_items" in kw, return_scores=True)
    if "ignore_items" in kw:
        rec.reset_items_to_ignore()
    for r, row in enumerate(scores):
        finite = np.sort(row[np.isfinite(row)])[::-1][:cutoff + 1]
        assert np.all(np.diff(finite) < 0), "tied scores in the list of user %d" % users[r]
    table = np.full((len(users), min(cutoff, case["test"].shape[1])), -1, np.int32)
    for r, items in enumerate(lists):
        table[r, :len(items)] = items
    return lists, table


def reference_per_user(case, users, lists, URM_train):
    """Evaluator.py:306-348 per user, with the reference's metric functions; returns [n_users][n_cutoffs][11] and the counters."""
    test = case["test"].tocsr()
    kw = case["kwargs"]
    ignore = np.array(kw.get("ignore_items", []))
    out = np.zeros((len(users), len(case["cutoffs"]), len(PER_USER)))
    coverage = [M.Coverage_Item(test.shape[1], ignore) for _ in case["cutoffs"]]
    for p, (u, items) in enumerate(zip(users, lists)):
        relevant = test.indices[test.indptr[u]:test.indptr[u + 1]]
        ratings = test.data[test.indptr[u]:test.indptr[u + 1]]
        items = np.array(items)
        is_relevant = np.in1d(items, relevant, assume_unique=True)
        for c, cutoff in enumerate(case["cutoffs"]):
            rel_c, items_c = is_relevant[:cutoff], items[:cutoff]
            ap, rr, nov, pop = M.MAP(), M.MRR(), M.Novelty(URM_train), M.AveragePopularity(URM_train)
            ap.add_recommendations(rel_c, relevant)
            rr.add_recommendations(rel_c)
            nov.add_recommendations(items_c)
            pop.add_recommendations(items_c)
            out[p, c] = [M.roc_auc(rel_c), M.precision(rel_c), M.precision_recall_min_denominator(rel_c, len(relevant)),
                         M.recall(rel_c, relevant), ap.cumulative_AP, rr.cumulative_RR,
                         M.ndcg(items_c, relevant, relevance=ratings, at=cutoff), rel_c.sum(), M.arhr(rel_c), nov.novelty,
                         pop.cumulative_popularity]
            coverage[c].add_recommendations(items_c)
    return out, np.array([cov.recommended_counter for cov in coverage]).astype(np.int32)


def main():
    out = {}
    for name in CASES:
        case = make_case(name)
        users = evaluated_users(case)
        out[name + "_users"] = users.astype(np.int32)
        for model in MODELS[name]:
            rec = set_model(BASES[model](case["train"], verbose=False), case["models"][model])
            lists, table = reference_lists(rec, case, users)
            evaluator = EvaluatorHoldout(case["test"], case["cutoffs"], verbose=False, **case["kwargs"])
            results, _ = evaluator.evaluateRecommender(rec)
            tag = "%s_%s" % (name, model)
            out[tag + "_dict"] = np.array([[float(results[c][m]) for m in METRICS] for c in case["cutoffs"]])
            if (name, model) in KEEP_LISTS:
                per_user, counts = reference_per_user(case, users, lists, rec.get_URM_train())
                out[tag + "_lists"] = table.astype(np.int16)
                out[tag + "_per_user"] = per_user
                out[tag + "_counts"] = counts
            print(tag, "users", len(users), "MAP@10 %.5f" % results[10]["MAP"])
    path = os.path.join(ROOT, "tests", "golden", "evaluator.npz")
    np.savez_compressed(path, **out)
    print("written", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
