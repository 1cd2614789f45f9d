"""Wall time of one EvaluatorNegativeItemSample_MI355X.evaluateRecommender at the ML-20M shape (named_urm("ml20m"), leave-one-out
split as bench.py's holdout_split: 138 493 test users, 1 test item + 99 sampled negatives each), cutoff [10], for BPR-shaped k = 128
factors and an ItemKNN W_sparse (topK 100) -- the two models of scripts/eval_time.py:
  negative_fused_s   the fused path: candidates scored, ranked and measured on the device;
  holdout_fused_s    the fused full-catalogue EvaluatorHoldout_MI355X on the same users in the same run: the yardstick.  The factor
                     model's negative evaluation does strictly less device work (no GEMM, a 100-wide ranking) and must not be slower;
                     ItemKNN does the same accumulation and a smaller ranking: not slower, with a 10 % allowance;
  lists_2000_s       the per-user lists path (one recommend() per user, what a recommender without a device scorer -- or the
                     reference's evaluator over this package's recommenders -- gets) on the first 2 000 users;
                     lists_all_users_extrapolated_s scales it to all users: an extrapolation, not a measurement.
  item_terms_s       evaluation.item_terms(URM_train), the host work every evaluateRecommender of either class starts with.
Every run ends in a device synchronise and follows one warm-up.  negative_fused_s and holdout_fused_s are the best of 6: two sets of 3
per evaluator, interleaved (negative, holdout, negative, holdout), so that neither has the better moment of the run; the other times
are the best of 3.  All runs are kept.

    python scripts/eval_negative_time.py --out profiles/eval_negative_time.json
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import scipy.sparse as sps

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from bench import holdout_split                                                                   # noqa: E402
from recsys2019_deeplearning_evaluation_amd import (EvaluatorHoldout_MI355X, EvaluatorNegativeItemSample_MI355X,      # noqa: E402
                                                    ItemKNNCFRecommender, _native)
from recsys2019_deeplearning_evaluation_amd import recommender_base as RB                         # noqa: E402
from recsys2019_deeplearning_evaluation_amd.evaluation import item_terms                           # noqa: E402
from recsys2019_deeplearning_evaluation_amd.scoring import GpuScoringMixin                         # noqa: E402
from recsys2019_deeplearning_evaluation_amd.synthetic import named_urm                             # noqa: E402

N_NEGATIVES, LISTS_USERS = 99, 2000


class FactorModel(GpuScoringMixin, RB.BaseMatrixFactorizationRecommender):
    RECOMMENDER_NAME = "FactorModel"


class ListsOnly:
    """The same recommender without its device scorer in sight: the evaluator takes the lists path."""

    def __init__(self, rec):
        self._rec = rec

    def __getattr__(self, name):
        return getattr(self._rec, name)


def sample_negatives(rng, train, test, per_user, draws=128):
    """Up to `per_user` distinct items per user outside train | test: the first admissible ones of `draws` uniform draws."""
    n_users, n_items = train.shape
    users = np.repeat(np.arange(n_users, dtype=np.int64), draws)
    keys = users * n_items + rng.integers(0, n_items, n_users * draws)
    taken = sps.csr_matrix(train) + sps.csr_matrix(test)
    taken_keys = np.repeat(np.arange(n_users, dtype=np.int64), np.diff(taken.indptr)) * n_items + taken.indices
    keys = keys[~np.isin(keys, taken_keys)]
    _, first = np.unique(keys, return_index=True)
    keys = keys[np.sort(first)]                          # distinct, still in draw order inside every user
    users = keys // n_items
    rank = np.arange(len(keys)) - np.searchsorted(users, users, side="left")
    keep = rank < per_user
    return sps.csr_matrix((np.ones(int(keep.sum()), np.float32), (users[keep], keys[keep] % n_items)), shape=train.shape)


def runs_of(fn, repeats=3):
    fn()
    times = []
    for _ in range(repeats):
        t0 = time.perf_counter()
        fn()
        _native.load().mi355rec_device_synchronize()
        times.append(time.perf_counter() - t0)
    return times


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "eval_negative_time.json"))
    ap.add_argument("--skip-lists", action="store_true", help="fused paths only (for a kernel trace)")
    args = ap.parse_args()
    urm = named_urm("ml20m")
    train, test = holdout_split(urm)
    rng = np.random.default_rng(11)
    negative = sample_negatives(rng, train, test, N_NEGATIVES)
    head = sps.csr_matrix(sps.vstack([test[:LISTS_USERS], sps.csr_matrix((test.shape[0] - LISTS_USERS, test.shape[1]), dtype=test.dtype)]))
    mf = FactorModel(train, verbose=False)
    mf.USER_factors = rng.normal(0, 0.1, (train.shape[0], 128)).astype(np.float32)
    mf.ITEM_factors = rng.normal(0, 0.1, (train.shape[1], 128)).astype(np.float32)
    knn = ItemKNNCFRecommender(train, verbose=False)
    knn.fit(topK=100, shrink=0)
    cutoffs = [10]
    negative_ev = EvaluatorNegativeItemSample_MI355X(test, negative, cutoffs, verbose=False)
    holdout_ev = EvaluatorHoldout_MI355X(test, cutoffs, verbose=False)
    head_ev = EvaluatorNegativeItemSample_MI355X(head, negative, cutoffs, verbose=False)
    lengths = np.diff(negative_ev.URM_items_to_rank.indptr)
    record = {"device": _native.device_name(), "shape": "ml20m", "n_users": train.shape[0], "n_items": train.shape[1],
              "train_nnz": int(train.nnz), "test_users": len(negative_ev.users_to_evaluate), "cutoffs": cutoffs,
              "candidates_per_user": {"min": int(lengths.min()), "median": float(np.median(lengths)), "max": int(lengths.max())},
              "timing": "seconds; every run follows one warm-up and ends in a device synchronise; negative_fused_s and holdout_fused_s: "
                        "best of 6, two interleaved sets of 3 each (*_runs_s and *_again_runs_s); every other *_s: best of 3 (*_runs_s)",
              "rows": []}
    record["item_terms_runs_s"] = runs_of(lambda: item_terms(train))
    record["item_terms_s"] = min(record["item_terms_runs_s"])
    for name, rec, allowance in (("bpr_k128", mf, 1.0), ("itemknn_topk100", knn, 1.1)):
        row = {"model": name, "users": len(negative_ev.users_to_evaluate)}
        for key, ev in (("negative_fused", negative_ev), ("holdout_fused", holdout_ev), ("negative_fused_again", negative_ev),
                        ("holdout_fused_again", holdout_ev)):
            row[key + "_runs_s"] = runs_of(lambda: ev.evaluateRecommender(rec))
        row["negative_fused_s"] = min(row["negative_fused_runs_s"] + row["negative_fused_again_runs_s"])
        row["holdout_fused_s"] = min(row["holdout_fused_runs_s"] + row["holdout_fused_again_runs_s"])
        row["negative_over_holdout"] = row["negative_fused_s"] / row["holdout_fused_s"]
        row["allowance"] = allowance
        row["not_slower_than_holdout"] = row["negative_fused_s"] <= allowance * row["holdout_fused_s"]
        row["MAP@10_negative"] = negative_ev.evaluateRecommender(rec)[0][10]["MAP"]
        row["MAP@10_holdout"] = holdout_ev.evaluateRecommender(rec)[0][10]["MAP"]
        if not args.skip_lists:
            row["lists_users"] = len(head_ev.users_to_evaluate)
            row["lists_2000_runs_s"] = runs_of(lambda: head_ev.evaluateRecommender(ListsOnly(rec)))
            row["lists_2000_s"] = min(row["lists_2000_runs_s"])
            row["fused_2000_s"] = min(runs_of(lambda: head_ev.evaluateRecommender(rec)))
            row["lists_all_users_extrapolated_s"] = row["lists_2000_s"] * row["users"] / row["lists_users"]
            row["lists_extrapolation"] = "lists_2000_s x users / 2000: an extrapolation, not a measurement"
            row["lists_equals_fused_2000"] = head_ev.evaluateRecommender(ListsOnly(rec))[0] == head_ev.evaluateRecommender(rec)[0]
        print(json.dumps(row), flush=True)
        record["rows"].append(row)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(record, f, indent=1)
    print("written", args.out)


if __name__ == "__main__":
    main()
