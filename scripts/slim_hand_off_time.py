"""What one validation of an early-stopping SLIM-BPR fit costs around the evaluation itself, with `validation_hand_off` "host" and
"device" (DESIGN section 19), and the proof that host mode did not get slower.  The ML-20M-shaped synthetic URM of bench.py (binary,
leave-one-out split as bench.py's holdout_split), BASELINE config 3's SLIM settings (adagrad, learning rate 1e-4, topK 100) on both
stores, EvaluatorHoldout_MI355X at cutoff [10], 20 epochs with a validation every 5:
  dense       symmetric=False (float64 cells);
  symmetric   symmetric=True (the packed triangle).
Every fit is run REPEATS = 7 times after one warm-up fit; inside a fit the recommender's hooks are timed where they are called, each
ending in a device synchronise, and a fit gives per validation (sums over the fit divided by its validations):
  prepare_s       _prepare_model_for_validation: host mode's get_S_and_W -- the download and two SciPy assemblies -- device mode's
                  update_from (its first validation of a fit runs the host path, and is in the sum);
  scorer_s        device_scorer() as the evaluator asks for it: host mode's fingerprint and a new scorer with URM_train, the seen CSR
                  and W uploaded; device mode returns the scorer it has;
  best_s          _update_best_model: host mode's copy, device mode's get_S of a new best -- spread over all validations;
  overhead_s      prepare_s + scorer_s + best_s: everything but the evaluation;
  validation_s    overhead_s + the rest of evaluateRecommender.
The figures of a leg are the medians over the 7 fits (all repeats are kept in the file).  `hand_off` times the call alone on a trained
handle -- MI355XSparseScorer.update_from, wall, and the device work and the bytes its get_stats reports.
`--parent-root DIR` names a checkout of the PARENT commit with its library built: its fits are then measured in a child process of
their own in the same run, and `conditions` says, store by store, whether host mode's validation_s is not above the parent's slowest
repeat and whether device mode's overhead_s is below the parent's.  Every measurement runs in a child process under `timeout`; after
a child that failed nothing more is started on the device.  Nothing is extrapolated.

    python scripts/slim_hand_off_time.py --parent-root ../parent --out profiles/slim_hand_off_time.json
"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

HERE = os.path.dirname(os.path.abspath(__file__))
CUTOFFS, REPEATS, TOPK = [10], 7, 100
FITS = {"dense": dict(symmetric=False), "symmetric": dict(symmetric=True)}
SLIM = dict(epochs=20, validation_every_n=5, sgd_mode="adagrad", learning_rate=1e-4, topK=TOPK, random_seed=42)
FIGURES = ("prepare_s", "scorer_s", "best_s", "overhead_s", "validation_s")


class Timed:
    """Seconds spent inside one bound method of an object, each call ending in a device synchronise."""

    def __init__(self, obj, name, sync):
        self.total, self.calls = 0.0, 0
        inner = getattr(obj, name)

        def timed(*args, **kwargs):
            t0 = time.perf_counter()
            try:
                return inner(*args, **kwargs)
            finally:
                sync()
                self.total += time.perf_counter() - t0
                self.calls += 1

        setattr(obj, name, timed)


def one_fit(spec, mode, train, evaluator, sync):
    from recsys2019_deeplearning_evaluation_amd import SLIM_BPR_MI355X
    rec = SLIM_BPR_MI355X(train, verbose=False)
    if mode != "parent":                            # (the parent commit has no such attribute: its only mode is left alone)
        rec.validation_hand_off = mode
    prepare, scorer, best = Timed(rec, "_prepare_model_for_validation", sync), Timed(rec, "device_scorer", sync), Timed(rec, "_update_best_model", sync)
    evaluate = Timed(evaluator, "evaluateRecommender", sync)
    try:
        # (no early stop: every fit makes the same number of validations)
        rec.fit(stop_on_validation=False, validation_metric="MAP", evaluator_object=evaluator, **SLIM, **spec)
    finally:
        del evaluator.evaluateRecommender          # (the instance attribute that shadows the method)
    n = evaluate.calls
    row = {"validations": n, "prepare_s": prepare.total / n, "scorer_s": scorer.total / n, "best_s": best.total / n,
           "map": float(rec.best_validation_metric), "W_sparse_nnz": int(rec.W_sparse.nnz)}
    row["overhead_s"] = row["prepare_s"] + row["scorer_s"] + row["best_s"]
    row["validation_s"] = row["prepare_s"] + row["best_s"] + evaluate.total / n     # (evaluate contains device_scorer())
    rec.invalidate_scorer()
    return row


def time_hand_off(train, sync):
    """update_from alone on trained handles of the two stores."""
    import scipy.sparse as sps
    from recsys2019_deeplearning_evaluation_amd import MI355XSparseScorer, SLIM_BPR_MI355X_Epoch
    n_items = train.shape[1]
    scorer = MI355XSparseScorer(train, sps.csr_matrix((n_items, n_items), dtype="float32"), train)
    out = {}
    for name, spec in FITS.items():
        handle = SLIM_BPR_MI355X_Epoch(train, sgd_mode=SLIM["sgd_mode"], learning_rate=SLIM["learning_rate"], topK=TOPK, random_seed=SLIM["random_seed"], **spec)
        handle.epochIteration_Cython(5)
        scorer.update_from(handle)
        wall, kernel = [], []
        for _ in range(REPEATS):
            t0 = time.perf_counter()
            scorer.update_from(handle)
            sync()
            wall.append(time.perf_counter() - t0)
            st = scorer.stats()
            kernel.append(st["kernel_ms"] * 1e-3)
        out[name] = {"bytes": st["algorithmic_bytes"], "launches": st["n_launches"], "W_nnz": int(scorer.weights().nnz), "wall_s_runs": wall,
                     "wall_s": statistics.median(wall), "kernel_s_runs": kernel, "kernel_s": statistics.median(kernel),
                     "bytes_per_s": st["algorithmic_bytes"] / statistics.median(kernel)}
        handle.close()
    scorer.close()
    return out


def measure(modes):
    from bench import holdout_split, load_urm
    from recsys2019_deeplearning_evaluation_amd import EvaluatorHoldout_MI355X, _native
    sync = _native.load().mi355rec_device_synchronize
    urm = load_urm("ml20m")
    urm.data[:] = 1.0
    train, test = holdout_split(urm)
    evaluator = EvaluatorHoldout_MI355X(test, CUTOFFS, verbose=False)
    out = {"device": _native.device_name(), "n_users": train.shape[0], "n_items": train.shape[1], "train_nnz": int(train.nnz), "cutoffs": CUTOFFS,
           "repeats": REPEATS, "slim": SLIM, "fits": FITS, "modes": {}}
    for mode in modes:
        out["modes"][mode] = {}
        for name, spec in FITS.items():
            one_fit(spec, mode, train, evaluator, sync)                 # warm-up
            runs = [one_fit(spec, mode, train, evaluator, sync) for _ in range(REPEATS)]
            row = {"runs": runs, "validations": runs[0]["validations"], "map": runs[0]["map"], "W_sparse_nnz": runs[0]["W_sparse_nnz"]}
            for figure in FIGURES:
                row[figure] = statistics.median(r[figure] for r in runs)
            out["modes"][mode][name] = row
            print(mode, name, json.dumps({k: v for k, v in row.items() if k != "runs"}), file=sys.stderr, flush=True)
    if "device" in modes:
        out["hand_off"] = time_hand_off(train, sync)
    return out


def child(root, modes, seconds):
    """One measuring process over the tree at `root` (this script, that tree's package and bench.py)."""
    env = dict(os.environ, PYTHONPATH=root + os.pathsep + os.environ.get("PYTHONPATH", ""))
    p = subprocess.run(["timeout", "-k", "10", str(seconds), sys.executable, os.path.abspath(__file__), "--measure", ",".join(modes)],
                       stdout=subprocess.PIPE, text=True, env=env, cwd=root)
    if p.returncode != 0:
        return None, p.returncode
    return json.loads(p.stdout.strip().splitlines()[-1]), 0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(os.path.dirname(HERE), "profiles", "slim_hand_off_time.json"))
    ap.add_argument("--parent-root", help="a checkout of the parent commit with libmi355rec.so built: its fits are measured too")
    ap.add_argument("--seconds", type=int, default=400, help="time limit of each measuring process")
    ap.add_argument("--measure", help="(child) MODES, comma separated; the package is taken from PYTHONPATH")
    a = ap.parse_args()
    if a.measure:
        print(json.dumps(measure(a.measure.split(","))))
        return
    root = os.path.dirname(HERE)
    result = {"timing": "seconds per validation; medians over %d fits after one warm-up fit, every timed hook ends in a device synchronise" % REPEATS}
    this, rc = child(root, ["host", "device"], a.seconds)
    if this is None:
        print("this tree's measurement failed (%d): nothing more is started" % rc, flush=True)
        sys.exit(1)
    result["this_tree"] = this
    host, device = this["modes"]["host"], this["modes"]["device"]
    if a.parent_root:
        parent, rc = child(os.path.abspath(a.parent_root), ["parent"], a.seconds)
        if parent is None:
            print("the parent's measurement failed (%d)" % rc, flush=True)
            result["parent"] = {"failed": rc}
        else:
            result["parent"] = parent
            par = parent["modes"]["parent"]
            result["conditions"] = {name: {
                "host_validation_s": host[name]["validation_s"], "parent_validation_s": par[name]["validation_s"],
                "parent_validation_s_slowest_repeat": max(r["validation_s"] for r in par[name]["runs"]),
                "host_not_above_parent_slowest_repeat": host[name]["validation_s"] <= max(r["validation_s"] for r in par[name]["runs"]),
                "host_overhead_s": host[name]["overhead_s"], "device_overhead_s": device[name]["overhead_s"],
                "parent_overhead_s": par[name]["overhead_s"],
                "device_overhead_below_host": device[name]["overhead_s"] < host[name]["overhead_s"],
                "device_overhead_below_parent": device[name]["overhead_s"] < par[name]["overhead_s"]} for name in FITS}
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(result, f, indent=1, sort_keys=True)
        f.write("\n")
    for name in FITS:
        print("%-10s per validation: host %.4f s (overhead %.4f), device %.4f s (overhead %.4f)" % (
            name, host[name]["validation_s"], host[name]["overhead_s"], device[name]["validation_s"], device[name]["overhead_s"]), flush=True)
        h = this["hand_off"][name]
        print("%-10s hand-off alone: %.3f ms wall, %.3f ms device work, %.0f bytes, W nnz %d" % (
            name, h["wall_s"] * 1e3, h["kernel_s"] * 1e3, h["bytes"], h["W_nnz"]), flush=True)
    if "conditions" in result:
        print("conditions:", json.dumps(result["conditions"]), flush=True)
    print("written", a.out)


if __name__ == "__main__":
    main()
