"""Reference-generated fixture for DIVERSITY_SIMILARITY on the device evaluators: the REFERENCE's own EvaluatorHoldout and
EvaluatorNegativeItemSample (Base/Evaluation/Evaluator.py) with diversity_object=Diversity_similarity(D) (Base/Evaluation/metrics.py:641-694),
imported from the reference tree, on the seeded cases of tests/diversity_cases.py.  The holdout cases are evaluated through a host
recommender that answers with fixed lists, the negative-sample case through the reference's matrix-factorization recommender.
Per case: D, the evaluated users, their lists, the cutoffs, the reference's metric per cutoff and the per-user values (a fresh
Diversity_similarity per user and cutoff, add_recommendations on the list's first `cutoff` entries); for the negative-sample case also
the other metrics of the reference's result dict.  Asserts what the reference needs in order not to raise: every cutoff >= 2, every
evaluated user has at least two items at every cutoff.
Writes tests/golden/evaluator_diversity.npz (arrays only).  Run where the reference tree exists:
    python tests/golden/make_diversity_fixture.py"""
import contextlib
import io
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
from make_evaluator_fixture import MF, METRICS, evaluated_users                             # noqa: E402  (needs the reference tree)
from make_negative_evaluator_fixture import reference_lists                                # noqa: E402
from diversity_cases import CASES, make_case                                                # noqa: E402
from eval_cases import set_model                                                            # noqa: E402
from Base.BaseRecommender import BaseRecommender                                            # noqa: E402
from Base.Evaluation.Evaluator import EvaluatorHoldout, EvaluatorNegativeItemSample         # noqa: E402
from Base.Evaluation.metrics import Diversity_similarity                                    # noqa: E402


class FixedLists(BaseRecommender):
    """Answers with stored lists (and a score matrix of the shape the reference's evaluator asserts)."""
    RECOMMENDER_NAME = "FixedLists"

    def __init__(self, URM_train, table):
        super().__init__(URM_train, verbose=False)
        self.table = table

    def recommend(self, user_id_array, cutoff=None, remove_seen_flag=True, items_to_compute=None, remove_top_pop_flag=False,
                  remove_custom_items_flag=False, return_scores=False):
        lists = [[int(i) for i in self.table[int(u)] if i >= 0][:cutoff] for u in user_id_array]
        return (lists, np.zeros((len(lists), self.n_items), np.float32)) if return_scores else lists


def reference_per_user(D, lists, cutoffs):
    out = np.zeros((len(lists), len(cutoffs)))
    for r, items in enumerate(lists):
        for c, cutoff in enumerate(cutoffs):
            metric = Diversity_similarity(D)
            metric.add_recommendations(list(items[:cutoff]))
            out[r, c] = metric.diversity                    # (np.float32 for a float32 matrix under NEP 50: stored exactly)
    return out


def main():
    out = {}
    for name in CASES:
        case = make_case(name)
        cutoffs, D = case["cutoffs"], case["D"]
        assert min(cutoffs) >= 2
        users = evaluated_users(case)
        if "negative" in case:
            rec = set_model(MF(case["train"], verbose=False), case["model"])
            with contextlib.redirect_stdout(io.StringIO()):             # (the reference class has no `verbose`)
                evaluator = EvaluatorNegativeItemSample(case["test"], case["negative"], cutoffs, diversity_object=Diversity_similarity(D))
                results, _ = evaluator.evaluateRecommender(rec)
            lists, table = reference_lists(rec, evaluator, case, users)
            out[name + "_dict"] = np.array([[float(results[c][m]) for m in METRICS] for c in cutoffs])
        else:
            rec = FixedLists(case["train"], case["lists"])
            evaluator = EvaluatorHoldout(case["test"], cutoffs, verbose=False, diversity_object=Diversity_similarity(D))
            results, _ = evaluator.evaluateRecommender(rec)
            table = case["lists"][users]
            lists = [row[row >= 0] for row in table]
        lengths = np.array([len(items) for items in lists])
        assert lengths.min() >= 2, "the reference divides by zero on a list of fewer than two items"
        assert any(cutoff > lengths.min() for cutoff in cutoffs), "no cutoff above a user's list"
        for cutoff in cutoffs:
            assert list(results[cutoff]).index("DIVERSITY_SIMILARITY") == list(results[cutoff]).index("AVERAGE_POPULARITY") + 1
        out[name + "_D"] = D
        out[name + "_users"] = users.astype(np.int32)
        out[name + "_lists"] = table.astype(np.int16)
        out[name + "_cutoffs"] = np.array(cutoffs, np.int32)
        out[name + "_metric"] = np.array([float(results[c]["DIVERSITY_SIMILARITY"]) for c in cutoffs])
        out[name + "_per_user"] = reference_per_user(D, lists, cutoffs)
        print(name, "users", len(users), "lists of", lengths.min(), "to", lengths.max(), "items", out[name + "_metric"])
    path = os.path.join(ROOT, "tests", "golden", "evaluator_diversity.npz")
    np.savez_compressed(path, **out)
    print("written", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
