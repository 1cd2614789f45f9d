"""Reference-generated fixture for the device negative-sample evaluator: the REFERENCE's own EvaluatorNegativeItemSample
(Base/Evaluation/Evaluator.py:455-539), metric functions (Base/Evaluation/metrics.py) and recommenders, imported from the reference
tree through oracle.ref_loader (its NumPy-2 aliases are what let the class run: np.bool at Evaluator.py:183, 484), on the seeded
cases of tests/negative_eval_cases.py.  For every (case, model): the reference's result dict; for the cases the lists-path tests
replay, also the reference's ranked lists, the per-user value of every metric at every cutoff and the item counters of its
Coverage_Item objects (as make_evaluator_fixture.py stores them); for every case the evaluated users and the reference's
URM_items_to_rank.  Asserts that no two admissible candidates of an evaluated user share a score.
Writes tests/golden/evaluator_negative.npz.  Run where the reference tree exists:
    python tests/golden/make_negative_evaluator_fixture.py"""
import contextlib
import io
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
from make_evaluator_fixture import BASES, METRICS, evaluated_users, reference_per_user      # noqa: E402  (needs the reference tree)
from negative_eval_cases import CASES, MODELS, make_case, set_model                          # noqa: E402
from Base.Evaluation.Evaluator import EvaluatorNegativeItemSample                            # noqa: E402

KEEP_LISTS = {("sampled", "mf"), ("sampled_graded", "mf_bias"), ("sampled_graded", "item")}


def reference_lists(rec, evaluator, case, users):
    """recommend() of the reference per user, as EvaluatorNegativeItemSample calls it (Evaluator.py:519-530); asserts that the
    admissible candidates of every user have distinct scores (the reference's order of equal scores is arbitrary)."""
    kw = case["kwargs"]
    cutoff = max(case["cutoffs"])
    if "ignore_items" in kw:
        rec.set_items_to_ignore(np.array(kw["ignore_items"]))
    lists = []
    for u in users:
        items, scores = rec.recommend(np.atleast_1d(u), remove_seen_flag=kw.get("exclude_seen", True), cutoff=cutoff,
                                      remove_top_pop_flag=False, items_to_compute=evaluator._get_user_specific_items_to_compute(u),
                                      remove_custom_items_flag="ignore_items" in kw, return_scores=True)
        finite = scores[0][np.isfinite(scores[0])]
        assert len(np.unique(finite)) == len(finite), "tied scores among the candidates of user %d" % u
        assert len(items[0]) == min(cutoff, len(finite))
        lists.append(items[0])
    if "ignore_items" in kw:
        rec.reset_items_to_ignore()
    table = np.full((len(users), min(cutoff, case["test"].shape[1])), -1, np.int32)
    for r, items in enumerate(lists):
        table[r, :len(items)] = items
    return lists, table


def main():
    out = {}
    for name in CASES:
        case = make_case(name)
        users = evaluated_users(case)
        out[name + "_users"] = users.astype(np.int32)
        for model in MODELS[name]:
            rec = set_model(BASES[model](case["train"], verbose=False), case["models"][model])
            with contextlib.redirect_stdout(io.StringIO()):             # (the reference class has no `verbose`)
                evaluator = EvaluatorNegativeItemSample(case["test"], case["negative"], case["cutoffs"], **case["kwargs"])
                results, _ = evaluator.evaluateRecommender(rec)
            lists, table = reference_lists(rec, evaluator, case, users)
            rank = evaluator.URM_items_to_rank
            assert rank.has_sorted_indices and np.all(rank.data == 1)
            out[name + "_rank_indptr"] = rank.indptr.astype(np.int32)
            out[name + "_rank_indices"] = rank.indices.astype(np.int32)
            tag = "%s_%s" % (name, model)
            out[tag + "_dict"] = np.array([[float(results[c][m]) for m in METRICS] for c in case["cutoffs"]])
            if (name, model) in KEEP_LISTS:
                per_user, counts = reference_per_user(case, users, lists, rec.get_URM_train())
                out[tag + "_lists"] = table.astype(np.int16)
                out[tag + "_per_user"] = per_user
                out[tag + "_counts"] = counts
            print(tag, "users", len(users), "longest row", int(np.diff(rank.indptr).max()), "MAP@10 %.5f" % results[10]["MAP"])
    path = os.path.join(ROOT, "tests", "golden", "evaluator_negative.npz")
    np.savez_compressed(path, **out)
    print("written", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
