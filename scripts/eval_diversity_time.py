"""Cost of DIVERSITY_SIMILARITY in the device evaluator, and the proof that an evaluation WITHOUT a diversity object did not get
slower.  The ML-20M shape (named_urm("ml20m"), leave-one-out split as bench.py's holdout_split: 138 493 test users, 26 744 items), a
BPR-shaped k = 128 factor model, the fused path, cutoffs [10] and [5, 10, 20, 50].  All in ONE run, every figure the median of 7
repeats after one warm-up, every repeat ending in a device synchronise (all repeats are kept in the file):
  evaluation_s     one EvaluatorHoldout_MI355X.evaluateRecommender with no diversity object, with a float32 item diversity matrix
                   (2.9 GB) and with a float64 one (5.7 GB);
  kernel_alone_s   eval_diversity_kernel alone, as a difference: the lists of all users (read back from the device scorer) through
                   mi355rec_eval_add_lists as one block, on an evaluator with the matrix and on one without -- the call uploads the
                   lists, runs the metric kernel, on the first also the diversity kernel, and waits for the stream;
  construction     set_diversity's host time split into allocation + upload and the device range check (mi355rec_eval_diversity_info),
                   next to the time of the whole constructor;
  host             Diversity_similarity.add_recommendations on the host for the same lists of the first 2 000 users: the
                   reference's own class where the reference tree is present, else this repository's row-by-row restatement of it
                   (the same NumPy calls per list position); `host_implementation` says which.  The figure for all users is that time
                   multiplied up and is labelled an extrapolation.
`--parent-root DIR` names a checkout of the PARENT commit with its library built: the evaluation without a diversity object is then
measured on it in a child process of its own in the same run, and `no_diversity_not_slower` says, per cutoff list, whether this
tree's median lies above the slowest of the parent's seven repeats.  Every measurement runs in a child process under `timeout`;
after a child that failed nothing more is started on the device.

    python scripts/eval_diversity_time.py --parent-root ../parent --out profiles/eval_diversity_time.json
"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

HERE = os.path.dirname(os.path.abspath(__file__))
CUTOFF_LISTS, REPEATS, K, HOST_USERS = ([10], [5, 10, 20, 50]), 7, 128, 2000


def runs_of(fn, sync, repeats=REPEATS):
    fn()
    sync()
    times = []
    for _ in range(repeats):
        t0 = time.perf_counter()
        fn()
        sync()
        times.append(time.perf_counter() - t0)
    return times


def tag(cutoffs):
    return "cutoffs_" + "_".join(str(c) for c in cutoffs)


def setup():
    import numpy as np
    from bench import holdout_split
    from recsys2019_deeplearning_evaluation_amd import _native
    from recsys2019_deeplearning_evaluation_amd import recommender_base as RB
    from recsys2019_deeplearning_evaluation_amd.scoring import GpuScoringMixin
    from recsys2019_deeplearning_evaluation_amd.synthetic import named_urm

    class FactorModel(GpuScoringMixin, RB.BaseMatrixFactorizationRecommender):
        RECOMMENDER_NAME = "FactorModel"

    train, test = holdout_split(named_urm("ml20m"))
    rng = np.random.default_rng(11)
    rec = FactorModel(train, verbose=False)
    rec.USER_factors = rng.normal(0, 0.1, (train.shape[0], K)).astype(np.float32)
    rec.ITEM_factors = rng.normal(0, 0.1, (train.shape[1], K)).astype(np.float32)
    return train, test, rec, _native.load().mi355rec_device_synchronize, _native.device_name()


def measure_plain():
    """The evaluation without a diversity object: runs on this tree and on the parent's."""
    from recsys2019_deeplearning_evaluation_amd import EvaluatorHoldout_MI355X
    train, test, rec, sync, device = setup()
    out = {"device": device, "n_users": train.shape[0], "n_items": train.shape[1], "factors": K, "repeats": REPEATS}
    for cutoffs in CUTOFF_LISTS:
        ev = EvaluatorHoldout_MI355X(test, cutoffs, verbose=False)
        runs = runs_of(lambda: ev.evaluateRecommender(rec), sync)
        out[tag(cutoffs)] = {"evaluation_s_runs": runs, "evaluation_s": statistics.median(runs), "users": len(ev.users_to_evaluate),
                             "MAP": ev.evaluateRecommender(rec)[0][cutoffs[0]]["MAP"]}
        ev.close()
    return out


def host_add_recommendations():
    """(implementation, function(D, items) -> value)"""
    sys.path.insert(0, os.path.dirname(HERE))
    from oracle import ref_loader
    cls = ref_loader.load_python_reference("Base.Evaluation.metrics", "Diversity_similarity")
    if cls is not None:
        def reference(D, items):
            metric = cls.__new__(cls)                   # (the constructor's range assertion reads the whole matrix: not what is timed)
            metric.item_diversity_matrix, metric.n_evaluated_users, metric.diversity = D, 0, 0.0
            metric.add_recommendations(items)
            return metric.diversity
        return "the reference's Diversity_similarity.add_recommendations", reference
    import numpy as np

    def restatement(D, items):
        total = 0.0
        for index in range(len(items) - 1):
            row = D[items[index], items]
            row[index] = 0.0
            total += np.sum(row)
        return total / (len(items) * (len(items) - 1))
    return "this repository's row-by-row restatement (no reference tree on this machine)", restatement


def measure_diversity():
    import ctypes as C
    import numpy as np
    from recsys2019_deeplearning_evaluation_amd import EvaluatorHoldout_MI355X
    from recsys2019_deeplearning_evaluation_amd import _native as N
    from recsys2019_deeplearning_evaluation_amd.evaluation import item_terms
    train, test, rec, sync, device = setup()
    n_items = train.shape[1]
    D32 = np.random.default_rng(21).random((n_items, n_items), dtype=np.float32)
    out = {"device": device, "matrix": "uniform random in [0, 1), asymmetric", "matrix_bytes": {}}
    novelty, popularity = item_terms(rec.get_URM_train())
    for name in ("float32", "float64"):
        D = D32 if name == "float32" else D32.astype(np.float64)
        out["matrix_bytes"][name] = int(D.nbytes)
        for cutoffs in CUTOFF_LISTS:
            row = {}
            t0 = time.perf_counter()
            ev = EvaluatorHoldout_MI355X(test, cutoffs, verbose=False, diversity_object=D)
            sync()
            row["constructor_s"] = time.perf_counter() - t0
            elem, upload, check = C.c_int32(), C.c_double(), C.c_double()
            ev._call("diversity_info", C.byref(elem), C.byref(upload), C.byref(check))
            row["set_diversity_upload_ms"], row["set_diversity_range_check_ms"] = upload.value, check.value
            uploads, checks = [], []
            for _ in range(REPEATS if cutoffs == CUTOFF_LISTS[0] else 0):      # (the matrix, not the cutoffs, decides these)
                ev._call("set_diversity", N.ptr(D), D.dtype.itemsize)
                ev._call("diversity_info", C.byref(elem), C.byref(upload), C.byref(check))
                uploads.append(upload.value)
                checks.append(check.value)
            if uploads:
                row.update(set_diversity_upload_ms_runs=uploads, set_diversity_range_check_ms_runs=checks,
                           set_diversity_upload_ms=statistics.median(uploads), set_diversity_range_check_ms=statistics.median(checks))
            runs = runs_of(lambda: ev.evaluateRecommender(rec), sync)
            results, _ = ev.evaluateRecommender(rec)
            device_values = ev.per_user_values()
            row.update(evaluation_s_runs=runs, evaluation_s=statistics.median(runs),
                       DIVERSITY_SIMILARITY={str(c): results[c]["DIVERSITY_SIMILARITY"] for c in cutoffs})
            # the kernel alone, by difference: the same lists as one add_lists block with and without the matrix
            users = ev.users_to_evaluate
            table = np.full((len(users), ev.width), -1, np.int32)
            for start in range(0, len(users), 4096):
                for r, items in enumerate(rec.recommend(users[start:start + 4096], cutoff=ev.width, remove_seen_flag=True)):
                    table[start + r, :len(items)] = items
            plain = EvaluatorHoldout_MI355X(test, cutoffs, verbose=False)
            for which, e in (("with_matrix", ev), ("without_matrix", plain)):
                e._call("begin", N.ptr(novelty), N.ptr(popularity), N.ptr(users), len(users))
                r = runs_of(lambda: e._call("add_lists", 0, len(users), N.ptr(table)), sync)
                row["add_lists_%s_s_runs" % which], row["add_lists_%s_s" % which] = r, statistics.median(r)
            row["kernel_alone_s"] = row["add_lists_with_matrix_s"] - row["add_lists_without_matrix_s"]
            row["gathers"] = (ev.width - 1) ** 2 * len(users)         # every cell of the widest cutoff once, whatever the cutoffs
            plain.close()
            if name == "float64":                       # the host, on the same lists of the first HOST_USERS users
                implementation, add = host_add_recommendations()
                lists = [[int(i) for i in r[r >= 0]] for r in table[:HOST_USERS]]
                t0 = time.perf_counter()
                host = [[add(D, items[:c]) for c in cutoffs] for items in lists]
                seconds = time.perf_counter() - t0
                worst = max(abs(host[r][c] - device_values[cutoff]["DIVERSITY_SIMILARITY"][r]) for r in range(HOST_USERS) for c, cutoff in enumerate(cutoffs))
                row["host"] = {"host_implementation": implementation, "users": HOST_USERS, "seconds": seconds,
                               "seconds_all_users_EXTRAPOLATED": seconds * len(users) / HOST_USERS,
                               "largest_difference_from_the_device": worst}
            ev.close()
            out.setdefault(name, {})[tag(cutoffs)] = row
            print(name, cutoffs, json.dumps({k: v for k, v in row.items() if not k.endswith("_runs")}), file=sys.stderr, flush=True)
    return out


def measure_host_reference():
    """The host leg once more where the reference tree is present (it is not on the GPU machines): no device, so the lists are seeded
    random lists of the same shape, HOST_USERS users, from a float64 matrix of the ML-20M item count."""
    import platform
    import numpy as np
    implementation, add = host_add_recommendations()
    n_items = 26744
    rng = np.random.default_rng(21)
    D = rng.random((n_items, n_items), dtype=np.float32).astype(np.float64)
    out = {"host_implementation": implementation, "lists": "seeded random lists, distinct items", "users": HOST_USERS, "n_items": n_items,
           "machine": platform.processor() or platform.machine(), "all_users": 138493}
    for cutoffs in CUTOFF_LISTS:
        lists = [[int(i) for i in rng.choice(n_items, max(cutoffs), replace=False)] for _ in range(HOST_USERS)]
        t0 = time.perf_counter()
        for items in lists:
            for c in cutoffs:
                add(D, items[:c])
        seconds = time.perf_counter() - t0
        out[tag(cutoffs)] = {"seconds": seconds, "seconds_all_users_EXTRAPOLATED": seconds * out["all_users"] / HOST_USERS}
    return out


def child(root, what, seconds):
    """One measuring process over the tree at `root` (this script, that tree's package and bench.py)."""
    env = dict(os.environ, PYTHONPATH=root + os.pathsep + os.environ.get("PYTHONPATH", ""))
    p = subprocess.run(["timeout", "-k", "10", str(seconds), sys.executable, os.path.abspath(__file__), "--measure", what],
                       stdout=subprocess.PIPE, text=True, env=env, cwd=root)
    if p.returncode != 0:
        return None, p.returncode
    return json.loads(p.stdout.strip().splitlines()[-1]), 0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(os.path.dirname(HERE), "profiles", "eval_diversity_time.json"))
    ap.add_argument("--parent-root", help="a checkout of the parent commit with libmi355rec.so built: its evaluation is measured too")
    ap.add_argument("--seconds", type=int, default=400, help="time limit of each measuring process")
    ap.add_argument("--measure", help="(child) plain | diversity; the package is taken from PYTHONPATH")
    ap.add_argument("--host-reference", action="store_true", help="no device: time the host leg with the reference's own class, where its "
                    "tree is present, and add it to the file at --out as `host_reference`")
    a = ap.parse_args()
    if a.host_reference:
        with open(a.out) as f:
            result = json.load(f)
        result["host_reference"] = measure_host_reference()
        with open(a.out, "w") as f:
            json.dump(result, f, indent=1, sort_keys=True)
            f.write("\n")
        print(json.dumps(result["host_reference"]))
        return
    if a.measure:
        print(json.dumps(measure_plain() if a.measure == "plain" else measure_diversity()))
        return
    root = os.path.dirname(HERE)
    result = {"timing": "seconds unless a key says ms; median of %d repeats after one warm-up, each repeat ends in a device synchronise" % REPEATS}
    for key, tree, what in (("no_diversity", root, "plain"), ("parent_no_diversity", a.parent_root and os.path.abspath(a.parent_root), "plain"),
                            ("diversity", root, "diversity")):
        if tree is None:
            continue
        got, rc = child(tree, what, a.seconds)
        if got is None:
            print("measuring %s failed (%d): nothing more is started" % (key, rc), flush=True)
            sys.exit(1)
        result[key] = got
    if a.parent_root:
        result["no_diversity_not_slower"] = {}
        for cutoffs in CUTOFF_LISTS:
            mine, theirs = result["no_diversity"][tag(cutoffs)], result["parent_no_diversity"][tag(cutoffs)]
            result["no_diversity_not_slower"][tag(cutoffs)] = {
                "this_median": mine["evaluation_s"], "parent_median": theirs["evaluation_s"], "parent_min": min(theirs["evaluation_s_runs"]),
                "parent_max": max(theirs["evaluation_s_runs"]), "not_above_parent_max": mine["evaluation_s"] <= max(theirs["evaluation_s_runs"])}
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(result, f, indent=1, sort_keys=True)
        f.write("\n")
    for cutoffs in CUTOFF_LISTS:
        t = tag(cutoffs)
        print("%-22s none %.4f s, float32 %.4f s, float64 %.4f s; kernel alone %.4f / %.4f s" % (
            t, result["no_diversity"][t]["evaluation_s"], result["diversity"]["float32"][t]["evaluation_s"],
            result["diversity"]["float64"][t]["evaluation_s"], result["diversity"]["float32"][t]["kernel_alone_s"],
            result["diversity"]["float64"][t]["kernel_alone_s"]), flush=True)
    if "no_diversity_not_slower" in result:
        print("no diversity, not slower:", json.dumps(result["no_diversity_not_slower"]), flush=True)
    print("written", a.out)


if __name__ == "__main__":
    main()
