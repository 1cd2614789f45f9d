"""Wall time of one EvaluatorHoldout_MI355X.evaluateRecommender at the ML-20M shape (named_urm("ml20m"), leave-one-out split as
bench.py's holdout_split: 138 493 test users), cutoffs [10] and [5, 10, 20, 50], for BPR-shaped k = 128 factors and an ItemKNN
W_sparse (topK 100): the fused path (device scorer -> metric kernel), the lists path (recommend() lists uploaded) and bench.py's
3-metric host evaluator (PRECISION / RECALL / MAP) in the same process, and the host-side share of every evaluation that
the per-item NOVELTY / AVERAGE_POPULARITY terms take (get_URM_train() + column counts).  Each time is the best of 3 after one warm-up and ends
in a device synchronise.

    python scripts/eval_time.py --out profiles/eval_time.json
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from bench import HoldoutEvaluator, holdout_split                                                 # noqa: E402
from recsys2019_deeplearning_evaluation_amd import EvaluatorHoldout_MI355X, ItemKNNCFRecommender, _native   # noqa: E402
from recsys2019_deeplearning_evaluation_amd import recommender_base as RB                         # noqa: E402
from recsys2019_deeplearning_evaluation_amd.evaluation import item_terms                           # noqa: E402
from recsys2019_deeplearning_evaluation_amd.scoring import GpuScoringMixin                         # noqa: E402
from recsys2019_deeplearning_evaluation_amd.synthetic import named_urm                             # noqa: E402


class FactorModel(GpuScoringMixin, RB.BaseMatrixFactorizationRecommender):
    RECOMMENDER_NAME = "FactorModel"


class ListsOnly:
    """The same recommender without its device scorer in sight: the evaluator takes the lists path."""

    def __init__(self, rec):
        self._rec = rec

    def __getattr__(self, name):
        return getattr(self._rec, name)


def best_of(fn, repeats=3):
    fn()
    times = []
    for _ in range(repeats):
        t0 = time.perf_counter()
        fn()
        _native.load().mi355rec_device_synchronize()
        times.append(time.perf_counter() - t0)
    return min(times)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "eval_time.json"))
    args = ap.parse_args()
    urm = named_urm("ml20m")
    train, test = holdout_split(urm)
    rng = np.random.default_rng(11)
    mf = FactorModel(train, verbose=False)
    mf.USER_factors = rng.normal(0, 0.1, (train.shape[0], 128)).astype(np.float32)
    mf.ITEM_factors = rng.normal(0, 0.1, (train.shape[1], 128)).astype(np.float32)
    knn = ItemKNNCFRecommender(train, verbose=False)
    knn.fit(topK=100, shrink=0)
    record = {"device": _native.device_name(), "shape": "ml20m", "n_users": train.shape[0],
              "n_items": train.shape[1], "train_nnz": int(train.nnz), "test_users": int((np.diff(test.indptr) > 0).sum()),
              "timing": "best of 3 after one warm-up, seconds, ending in a device synchronise", "rows": []}
    for name, rec in (("bpr_k128", mf), ("itemknn_topk100", knn)):
        for cutoffs in ([10], [5, 10, 20, 50]):
            ev = EvaluatorHoldout_MI355X(test, cutoffs, verbose=False)
            row = {"model": name, "cutoffs": cutoffs, "metrics": 18, "users": len(ev.users_to_evaluate)}
            row["fused_s"] = best_of(lambda: ev.evaluateRecommender(rec))
            row["host_item_terms_s"] = best_of(lambda: item_terms(rec.get_URM_train()))    # (part of every evaluation, both paths)
            fused, _ = ev.evaluateRecommender(rec)
            row["lists_s"] = best_of(lambda: ev.evaluateRecommender(ListsOnly(rec)))
            lists, _ = ev.evaluateRecommender(ListsOnly(rec))
            row["fused_equals_lists"] = fused == lists
            row["MAP@10"] = fused[10]["MAP"]
            if cutoffs == [10]:
                host = HoldoutEvaluator(test, cutoff=10)
                row["host_3_metrics_s"] = best_of(lambda: host.evaluateRecommender(rec))
                row["host_MAP@10"] = host.evaluateRecommender(rec)[0][10]["MAP"]
            ev.close()
            print(json.dumps(row), flush=True)
            record["rows"].append(row)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(record, f, indent=1)
    print("written", args.out)


if __name__ == "__main__":
    main()
