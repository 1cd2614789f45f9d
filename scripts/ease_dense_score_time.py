"""Time of scoring EASE_R's dense W (topK=None) on the device, at the ML-1M and ML-20M shapes (named_urm, binary; leave-one-out
split as bench.py's holdout_split; l2_norm 1000; cutoff [10]).  Per shape, in one process:
  holdout_fused_s / negative_fused_s   one EvaluatorHoldout_MI355X / EvaluatorNegativeItemSample_MI355X (1 test item + 99 sampled
                     negatives per user) evaluation of EASE_R_MI355X_Recommender(dense_scoring="device") through the fused dense path
                     (csrc/densescore.hip): all test users, best of 3 after one warm-up, every run ends in a device synchronise;
  *_lists_2000_s     the route without the dense scorer, in the SAME run: the same evaluators' lists path over the host
                     _compute_item_score (SciPy csr @ ndarray) of a default-constructed recommender holding the same W, on the
                     first 2 000 test users, one run each (host work: no warm-up to speak of);
  *_fused_2000_s     the fused dense path on those same 2 000 users (best of 3): what the bar compares the line above with;
  *_lists_all_users_extrapolated_s   lists_2000_s x users / 2000 -- an extrapolation, not a measurement;
  lists_equals_fused_2000 / exact_lists_of_host_scores_equal_fused_2000   whether the two routes gave the same result dictionary on
                     those users, and whether the host scores ranked by the package's tie rule (lower item id first) did;
  kernel             the scoring kernel alone: every test user once, in the evaluator's blocks, dispatch times summed (get_stats'
                     kernel_ms), for both unroll depths the library builds (MI355REC_DSCORE_UNROLL), and its algorithmic bytes per
                     second -- nnz x n_out x 4 B over that time -- next to the guides' figures for HBM, the Infinity Cache and L2;
  weights            filling the scorer from the MI355XEase handle inside fit (device to device) against uploading the host array.
Every shape runs in a child process of its own under `timeout`; after a child that failed nothing more is started on the device.

    python scripts/ease_dense_score_time.py --out profiles/ease_dense_score_time.json
"""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "scripts"))

L2_NORM, CUTOFFS, N_NEGATIVES, LISTS_USERS = 1e3, [10], 99, 2000
# what the guides give for MI355X: achievable HBM3E streaming, uniformly gathered rows of a table inside the Infinity Cache, rows
# shared by every workgroup of an XCD (L2)
RATES = {"hbm_streaming_bytes_per_s": 6.3e12, "infinity_cache_gather_bytes_per_s": 8.6e12, "l2_shared_rows_bytes_per_s": 17e12}


def best_of(fn, sync, repeats=3):
    fn()
    times = []
    for _ in range(repeats):
        t0 = time.perf_counter()
        fn()
        sync()
        times.append(time.perf_counter() - t0)
    return times


def kernel_alone(scorer, users, block):
    """Dispatch time of the scoring kernel over all users (blocks of the evaluator's size), and the bytes its stored cells stream."""
    ms, nbytes = 0.0, 0.0
    for start in range(0, len(users), block):
        scorer.recommend(users[start:start + block], CUTOFFS[0], True, None)
        st = scorer.stats()
        ms += st["kernel_ms"]
        nbytes += st["algorithmic_bytes"]
    return ms, nbytes


def exact_lists_recommender(host):
    """The lists path fed with the ranking contract's own lists of the host scores: value descending, ties towards the lower item id."""
    import numpy as np
    import scipy.sparse as sps
    from recsys2019_deeplearning_evaluation_amd import recommender_base as RB

    class ExactLists(RB.BaseRecommender):
        def recommend(self, user_id_array, cutoff=None, remove_seen_flag=True, items_to_compute=None, remove_top_pop_flag=False,
                      remove_custom_items_flag=False, return_scores=False):
            users = np.atleast_1d(user_id_array)
            scores = np.array(host._compute_item_score(users, items_to_compute=items_to_compute), dtype=np.float32)
            X = sps.csr_matrix(self.URM_train)
            lists = []
            for r, u in enumerate(users):
                row = scores[r]
                if remove_seen_flag:
                    row[X.indices[X.indptr[u]:X.indptr[u + 1]]] = -np.inf
                order = np.argsort(-row, kind="stable")[:cutoff]
                lists.append(order[row[order] > -np.inf].tolist())
            return lists

    return ExactLists(host.URM_train, verbose=False)


def measure(shape):
    import numpy as np
    import scipy.sparse as sps
    from bench import holdout_split
    from eval_negative_time import sample_negatives
    from recsys2019_deeplearning_evaluation_amd import (EASE_R_MI355X_Recommender, EvaluatorHoldout_MI355X,
                                                        EvaluatorNegativeItemSample_MI355X, MI355XDenseScorer, _native)
    from recsys2019_deeplearning_evaluation_amd.synthetic import named_urm
    sync = _native.load().mi355rec_device_synchronize
    urm = named_urm(shape)
    urm.data[:] = 1.0
    train, test = holdout_split(urm)
    negative = sample_negatives(np.random.default_rng(11), train, test, N_NEGATIVES)
    head = sps.csr_matrix(sps.vstack([test[:LISTS_USERS], sps.csr_matrix((test.shape[0] - LISTS_USERS, test.shape[1]), dtype=test.dtype)]))

    copies = []
    real_set = MI355XDenseScorer.set_weights_from

    def timed_set(self, ease):
        t0 = time.perf_counter()
        real_set(self, ease)
        copies.append({"wall_ms": 1e3 * (time.perf_counter() - t0), "device_ms": self.stats()["call_ms"]})

    MI355XDenseScorer.set_weights_from = timed_set
    rec = EASE_R_MI355X_Recommender(train, verbose=False, dense_scoring="device")
    fits = []
    for _ in range(2):                              # (the second fit finds the scorer's buffers in place)
        t0 = time.perf_counter()
        rec.fit(topK=None, l2_norm=L2_NORM, verbose=False)
        fits.append(time.perf_counter() - t0)
    MI355XDenseScorer.set_weights_from = real_set
    assert rec.fit_info["scoring"] == "device" and rec.dense_device_scorable()
    scorer = rec._dense_scorer
    uploads = []
    for _ in range(2):
        t0 = time.perf_counter()
        scorer.update(rec.W_sparse)
        uploads.append(1e3 * (time.perf_counter() - t0))

    host = EASE_R_MI355X_Recommender(train, verbose=False)          # the default: scored by _compute_item_score on the host
    host.W_sparse = rec.W_sparse
    assert not host.device_scorable() and not host.dense_device_scorable()
    evaluators = {"holdout": (EvaluatorHoldout_MI355X(test, CUTOFFS, verbose=False), EvaluatorHoldout_MI355X(head, CUTOFFS, verbose=False)),
                  "negative": (EvaluatorNegativeItemSample_MI355X(test, negative, CUTOFFS, verbose=False),
                               EvaluatorNegativeItemSample_MI355X(head, negative, CUTOFFS, verbose=False))}
    out = {"shape": shape, "device": _native.device_name(), "n_users": train.shape[0], "n_items": train.shape[1], "train_nnz": int(train.nnz),
           "l2_norm": L2_NORM, "cutoffs": CUTOFFS, "negatives_per_user": N_NEGATIVES, "fit_wall_s": fits, "fit_route": rec.fit_info["inverse"],
           "weights": {"from_ease_handle_ms": copies, "upload_host_array_ms": uploads, "bytes": 4.0 * train.shape[1] ** 2}}
    for name, (full, first) in evaluators.items():
        users = len(full.users_to_evaluate)
        row = {"users": users, "lists_users": len(first.users_to_evaluate), "block": full._block_size()}
        row["fused_runs_s"] = best_of(lambda: full.evaluateRecommender(rec), sync)
        row["fused_s"] = min(row["fused_runs_s"])
        row["MAP@10"] = full.evaluateRecommender(rec)[0][CUTOFFS[0]]["MAP"]
        row["fused_2000_runs_s"] = best_of(lambda: first.evaluateRecommender(rec), sync)
        row["fused_2000_s"] = min(row["fused_2000_runs_s"])
        fused_2000 = first.evaluateRecommender(rec)[0]
        t0 = time.perf_counter()
        lists_2000 = first.evaluateRecommender(host)[0]
        row["lists_2000_s"] = time.perf_counter() - t0
        row["lists_all_users_extrapolated_s"] = row["lists_2000_s"] * users / max(1, row["lists_users"])
        row["lists_extrapolation"] = "lists_2000_s x users / lists_users: an extrapolation, not a measurement"
        row["fused_faster_than_lists_on_2000"] = row["fused_2000_s"] < row["lists_2000_s"]
        row["lists_equals_fused_2000"] = lists_2000 == fused_2000     # (the host ranking breaks ties its own way: reported, not required)
        row["exact_lists_of_host_scores_equal_fused_2000"] = first.evaluateRecommender(exact_lists_recommender(host))[0] == fused_2000
        out[name] = row
        print(shape, name, json.dumps(row), file=sys.stderr, flush=True)

    full = evaluators["holdout"][0]
    users, block = full.users_to_evaluate, full._block_size()
    kernel = {"users": len(users), "block": block, "rates_of_the_guides": RATES, "by_unroll": {}}
    default_ms, nbytes = min(kernel_alone(scorer, users, block) for _ in range(3))
    kernel["default"] = {"kernel_ms": default_ms, "algorithmic_bytes": nbytes, "bytes_per_s": nbytes / (1e-3 * default_ms)}
    for unroll in (4, 8):
        os.environ["MI355REC_DSCORE_UNROLL"] = str(unroll)
        other = MI355XDenseScorer(train, rec.W_sparse, train)
        try:
            ms, nb = min(kernel_alone(other, users, block) for _ in range(3))
            kernel["by_unroll"][str(unroll)] = {"kernel_ms": ms, "bytes_per_s": nb / (1e-3 * ms)}
        finally:
            other.close()
            os.environ.pop("MI355REC_DSCORE_UNROLL", None)
    out["kernel"] = kernel
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ease_dense_score_time.json"))
    ap.add_argument("--shapes", nargs="+", default=["ml1m", "ml20m"])
    ap.add_argument("--measure", help="(child) SHAPE")
    a = ap.parse_args()
    if a.measure:
        print(json.dumps(measure(a.measure)))
        return
    result = {"shapes": [], "timing": "seconds unless a key says ms; fused times: best of 3 after one warm-up, each run ends in a device "
                                      "synchronise; lists times: one run"}
    for shape in a.shapes:
        p = subprocess.run(["timeout", "-k", "10", "900", sys.executable, os.path.abspath(__file__), "--measure", shape], stdout=subprocess.PIPE,
                           text=True)
        if p.returncode != 0:
            result["shapes"].append({"shape": shape, "failed": p.returncode})
            print("%s failed (%d): nothing more is started" % (shape, p.returncode), flush=True)
            break
        r = json.loads(p.stdout.strip().splitlines()[-1])
        result["shapes"].append(r)
        print("%-6s holdout fused %.3f s (2000 users: fused %.3f s, lists %.2f s), negative fused %.3f s (2000: %.3f s / %.2f s), kernel %.1f ms = "
              "%.2f TB/s, weights from the EASE handle %.1f ms vs upload %.1f ms" % (
                  shape, r["holdout"]["fused_s"], r["holdout"]["fused_2000_s"], r["holdout"]["lists_2000_s"], r["negative"]["fused_s"],
                  r["negative"]["fused_2000_s"], r["negative"]["lists_2000_s"], r["kernel"]["default"]["kernel_ms"],
                  r["kernel"]["default"]["bytes_per_s"] / 1e12, r["weights"]["from_ease_handle_ms"][-1]["wall_ms"],
                  min(r["weights"]["upload_host_array_ms"])), flush=True)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(result, f, indent=1, sort_keys=True)
        f.write("\n")
    print("written", a.out)


if __name__ == "__main__":
    main()
