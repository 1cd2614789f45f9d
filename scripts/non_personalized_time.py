"""Times of the non-personalized recommenders at the ML-20M shape (named_urm("ml20m"), leave-one-out split as bench.py's
holdout_split), every figure the median of 7 runs after one warm-up, every run ending in a device synchronise; all runs are kept.
  fit            TopPop.fit and GlobalEffects.fit from the host CSR and from a ResidentURM, against the reference classes' fit on the
                 same machine -- or, where the reference tree is not on the machine, against a host NumPy / SciPy statement of the same
                 steps (`host_fit_source` says which).
  holdout        one EvaluatorHoldout_MI355X evaluation of TopPop at cut-off 10:
                   item_scorer      fused, through MI355XItemScorer (the default kernel shape);
                   one_factor       fused, through MI355XScorer with k = 1 (U = ones, V = item_pop): the only device route before;
                   host_2000        BaseRecommender.recommend on the host for the first 2 000 users, through the lists path;
                                    host_all_users_extrapolated_s scales it to all users: an extrapolation, not a measurement.
                 evaluate_s is the whole evaluateRecommender (item_terms on the host, begin, the blocks, finish); blocks_s is the blocks
                 alone -- scoring, ranking and metric kernels -- which is where the routes differ.
  kernel_shapes  the ranking kernel with a wavefront per user (W = 2048) and with a 256-lane workgroup per user (W = 8192), alternating:
                 blocks_s as above, and rank_ms, the event-timed kernel over all users in launches of 16 384.

    python scripts/non_personalized_time.py --out profiles/non_personalized_time.json
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import scipy.sparse as sps

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from bench import holdout_split                                                                   # noqa: E402
from oracle import ref_loader                                                                     # noqa: E402
from recsys2019_deeplearning_evaluation_amd import (EvaluatorHoldout_MI355X, GlobalEffects, ResidentURM, TopPop, _native)   # noqa: E402
from recsys2019_deeplearning_evaluation_amd import recommender_base as RB                         # noqa: E402
from recsys2019_deeplearning_evaluation_amd.scoring import GpuScoringMixin                         # noqa: E402
from recsys2019_deeplearning_evaluation_amd.synthetic import named_urm                             # noqa: E402

REPEATS, LISTS_USERS, RANK_BLOCK = 7, 2000, 16384


class FactorModel(GpuScoringMixin, RB.BaseMatrixFactorizationRecommender):
    RECOMMENDER_NAME = "FactorModel"


class HostLists:
    """The recommender scored by BaseRecommender.recommend on the host: the evaluator takes the lists path."""

    def __init__(self, rec):
        self._rec = rec

    def __getattr__(self, name):
        return getattr(self._rec, name)

    def recommend(self, *args, **kwargs):
        return RB.BaseRecommender.recommend(self._rec, *args, **kwargs)


def sync():
    _native.load().mi355rec_device_synchronize()


def runs_of(fn, repeats=REPEATS):
    fn()
    sync()
    times = []
    for _ in range(repeats):
        t0 = time.perf_counter()
        fn()
        sync()
        times.append(time.perf_counter() - t0)
    return times


def host_top_pop(URM):
    return np.ediff1d(sps.csc_matrix(URM).indptr)


def host_global_effects(URM, lambda_user=10, lambda_item=25):
    """The steps of GlobalEffects.fit with NumPy / SciPy on the host: CSC copy, float32 mean, column sums, CSR copy, row sums."""
    csc = sps.csc_matrix(URM, dtype=np.float32)
    mu = csc.data.sum(dtype=np.float32) / csc.data.shape[0]
    col_nnz = np.diff(csc.indptr)
    centred = csc.copy()
    centred.data -= mu
    item_bias = np.asarray(centred.sum(axis=0) / (col_nnz + lambda_item)).ravel()
    centred.data -= np.repeat(item_bias, col_nnz)
    rows = centred.tocsr()
    user_bias = np.asarray(rows.sum(axis=1)).ravel() / (np.diff(rows.indptr) + lambda_user)
    return mu, item_bias, user_bias


def fit_rows(train):
    ref_top = ref_loader.load_python_reference("Base.NonPersonalizedRecommender", "TopPop")
    ref_ge = ref_loader.load_python_reference("Base.NonPersonalizedRecommender", "GlobalEffects")
    source = "reference classes" if ref_top is not None else "host NumPy / SciPy statement of the reference's steps (no reference tree here)"
    resident = ResidentURM(train)
    rows = []
    for name, cls, ref_cls, host in (("TopPop", TopPop, ref_top, host_top_pop), ("GlobalEffects", GlobalEffects, ref_ge, host_global_effects)):
        rec = cls(train, verbose=False)
        row = {"model": name, "host_fit_source": source}
        row["device_host_csr_runs_s"] = runs_of(rec.fit)
        row["device_resident_runs_s"] = runs_of(lambda: rec.fit(resident_urm=resident))
        if ref_cls is not None:
            ref = ref_cls(train)
            row["host_fit_runs_s"] = runs_of(ref.fit, 5)
        else:
            row["host_fit_runs_s"] = runs_of(lambda: host(rec.URM_train), 5)
        for key in ("device_host_csr", "device_resident", "host_fit"):
            row[key + "_s"] = statistics.median(row[key + "_runs_s"])
        print(json.dumps(row), flush=True)
        rows.append(row)
    resident.close()
    return rows


def blocks_of(ev, rec):
    """The blocks of an evaluation alone (after one whole evaluateRecommender has begun it)."""
    ev.evaluateRecommender(rec)
    return runs_of(lambda: ev._run(rec, None))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "non_personalized_time.json"))
    args = ap.parse_args()
    urm = named_urm("ml20m")
    train, test = holdout_split(urm)
    record = {"device": _native.device_name(), "shape": "ml20m", "n_users": train.shape[0], "n_items": train.shape[1],
              "train_nnz": int(train.nnz), "cpu_threads": os.environ.get("OMP_NUM_THREADS", "unset"),
              "timing": "seconds (rank_ms: milliseconds); median of %d runs after one warm-up, each ending in a device synchronise" % REPEATS}
    record["fit"] = fit_rows(train)

    cutoffs = [10]
    top = TopPop(train, verbose=False)
    top.fit()
    one_factor = FactorModel(train, verbose=False)
    one_factor.USER_factors = np.ones((train.shape[0], 1), np.float32)
    one_factor.ITEM_factors = np.ascontiguousarray(top.item_pop.astype(np.float32)[:, None])
    ev = EvaluatorHoldout_MI355X(test, cutoffs, verbose=False)
    head = sps.csr_matrix(sps.vstack([test[:LISTS_USERS], sps.csr_matrix((test.shape[0] - LISTS_USERS, test.shape[1]), dtype=test.dtype)]))
    head_ev = EvaluatorHoldout_MI355X(head, cutoffs, verbose=False)
    holdout = {"cutoffs": cutoffs, "users": len(ev.users_to_evaluate)}
    for key, rec in (("item_scorer", top), ("one_factor", one_factor), ("item_scorer_again", top), ("one_factor_again", one_factor)):
        holdout[key + "_evaluate_runs_s"] = runs_of(lambda: ev.evaluateRecommender(rec))
        holdout[key + "_blocks_runs_s"] = blocks_of(ev, rec)
    for key in ("item_scorer", "one_factor"):
        for part in ("evaluate", "blocks"):
            holdout["%s_%s_s" % (key, part)] = statistics.median(holdout["%s_%s_runs_s" % (key, part)] + holdout["%s_again_%s_runs_s" % (key, part)])
    holdout["blocks_speedup_over_one_factor"] = holdout["one_factor_blocks_s"] / holdout["item_scorer_blocks_s"]
    holdout["same_result"] = ev.evaluateRecommender(top)[0] == ev.evaluateRecommender(one_factor)[0]
    holdout["host_users"] = len(head_ev.users_to_evaluate)
    holdout["host_2000_runs_s"] = runs_of(lambda: head_ev.evaluateRecommender(HostLists(top)), 5)
    holdout["host_2000_s"] = statistics.median(holdout["host_2000_runs_s"])
    holdout["host_all_users_extrapolated_s"] = holdout["host_2000_s"] * holdout["users"] / holdout["host_users"]
    holdout["host_extrapolation"] = "host_2000_s x users / host_users: an extrapolation, not a measurement"
    print(json.dumps(holdout), flush=True)
    record["holdout"] = holdout

    scorer = top._get_item_scorer()
    users = np.ascontiguousarray(ev.users_to_evaluate)
    shapes = {}
    for round_ in range(2):                                 # the two shapes alternate
        for bits in (2048, 8192):
            scorer.set_window_bits(bits)
            row = shapes.setdefault(str(bits), {"threads_per_user": bits // 32, "blocks_runs_s": [], "rank_runs_ms": []})
            row["blocks_runs_s"] += blocks_of(ev, top)
            for _ in range(REPEATS + 1):
                ms = 0.0
                for start in range(0, len(users), RANK_BLOCK):
                    scorer.recommend(users[start:start + RANK_BLOCK], cutoffs[0])
                    ms += scorer.stats()["kernel_ms"]
                row["rank_runs_ms"].append(ms)
            row["rank_runs_ms"].pop(-REPEATS - 1)           # (the warm-up of this round)
    for row in shapes.values():
        row["blocks_s"], row["rank_ms"] = statistics.median(row["blocks_runs_s"]), statistics.median(row["rank_runs_ms"])
    default = TopPop(train, verbose=False)
    default.item_pop, default.n_items = top.item_pop, top.n_items
    shapes["default_window_bits"] = default._get_item_scorer().window_bits()
    print(json.dumps(shapes), flush=True)
    record["kernel_shapes"] = shapes
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(record, f, indent=1)
        f.write("\n")
    print("written", args.out)


if __name__ == "__main__":
    main()
