"""What one validation of an early-stopping fit costs around the evaluation itself, with `validation_hand_off` "host" and "device"
(DESIGN section 18), and the proof that host mode did not get slower.  The ML-20M-shaped synthetic URM of bench.py (binary,
leave-one-out split as bench.py's holdout_split), k = 128, EvaluatorHoldout_MI355X at cutoff [10], three fits:
  bpr_sgd      MatrixFactorization_BPR_MI355X, sgd (float32 state), 50 epochs, validation every 5;
  bpr_adagrad  the same with adagrad (float64 state);
  ials         IALSRecommender, 10 epochs, validation every 2 (float64 state).
Every fit is run REPEATS = 7 times after one warm-up fit; inside a fit the recommender's hooks are timed where they are called, each
ending in a device synchronise, and a fit gives per validation (sums over the fit divided by its validations):
  prepare_s       _prepare_model_for_validation: host mode's download, device mode's hand-off;
  scorer_s        device_scorer() as the evaluator asks for it: host mode's fingerprint, float32 pass and upload; device mode returns
                  the scorer it has (the first validation of a fit builds it in both modes);
  best_s          _update_best_model: host mode's copies, device mode's download of a new best -- spread over all validations;
  overhead_s      prepare_s + scorer_s + best_s: everything but the evaluation;
  validation_s    overhead_s + the rest of evaluateRecommender.
The figures of a leg are the medians over the 7 fits (all repeats are kept in the file).  `hand_off` times the call alone on a
trained handle -- MI355XScorer.update_from, wall and the copy kernels' own time -- with its bytes per second next to the 6.29 TB/s
a float4 copy streams on this device.
`--parent-root DIR` names a checkout of the PARENT commit with its library built: its fits are then measured in a child process of
their own in the same run, and `conditions` says, leg by leg, whether host mode's validation_s is not above the parent's slowest
repeat and whether device mode's overhead_s is below the parent's.  Every measurement runs in a child process under `timeout`; after
a child that failed nothing more is started on the device.

    python scripts/validation_hand_off_time.py --parent-root ../parent --out profiles/validation_hand_off_time.json
"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

HERE = os.path.dirname(os.path.abspath(__file__))
K, CUTOFFS, REPEATS = 128, [10], 7
HBM_STREAM_BYTES_PER_S = 6.29e12
FITS = {
    "bpr_sgd": dict(kind="bpr", epochs=50, validation_every_n=5, sgd_mode="sgd"),
    "bpr_adagrad": dict(kind="bpr", epochs=50, validation_every_n=5, sgd_mode="adagrad"),
    "ials": dict(kind="ials", epochs=10, validation_every_n=2),
}
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
    import numpy as np
    from recsys2019_deeplearning_evaluation_amd import IALSRecommender, MatrixFactorization_BPR_MI355X
    if spec["kind"] == "bpr":
        rec = MatrixFactorization_BPR_MI355X(train, verbose=False)
        kwargs = dict(batch_size=1024, num_factors=K, learning_rate=0.05, sgd_mode=spec["sgd_mode"], random_seed=5)
    else:
        rec = IALSRecommender(train, verbose=False)
        kwargs = dict(num_factors=K, reg=1e-2, alpha=2.0)
        np.random.seed(5)
    if mode != "parent":                            # (the parent commit has no such attribute: its only mode is left alone)
        rec.validation_hand_off = mode
    prepare, scorer, best = Timed(rec, "_prepare_model_for_validation", sync), Timed(rec, "device_scorer", sync), Timed(rec, "_update_best_model", sync)
    evaluate = Timed(evaluator, "evaluateRecommender", sync)
    try:
        # (no early stop: every fit makes the same number of validations)
        rec.fit(epochs=spec["epochs"], validation_every_n=spec["validation_every_n"], stop_on_validation=False, validation_metric="MAP",
                evaluator_object=evaluator, **kwargs)
    finally:
        del evaluator.evaluateRecommender          # (the instance attribute that shadows the method)
    n = evaluate.calls
    # BPR's fit calls the two hooks once before training: that call is part of both modes' fit, not of a validation -- the hooks'
    # totals are spread over the validations as they are, the same way in every leg
    row = {"validations": n, "prepare_s": prepare.total / n, "scorer_s": scorer.total / n, "best_s": best.total / n,
           "map": float(rec.best_validation_metric)}
    row["overhead_s"] = row["prepare_s"] + row["scorer_s"] + row["best_s"]
    row["validation_s"] = row["prepare_s"] + row["best_s"] + evaluate.total / n     # (evaluate contains device_scorer())
    scorer_obj = getattr(rec, "_scorer", None)
    if scorer_obj is not None:
        rec.invalidate_scorer()
    return row


def time_hand_off(train, sync):
    """update_from alone on trained handles of the three fits' shapes."""
    import numpy as np
    from recsys2019_deeplearning_evaluation_amd import MI355XScorer, MatrixFactorization_MI355X_Epoch
    from recsys2019_deeplearning_evaluation_amd.ials import IALS_MI355X_Epoch
    n_users, n_items = train.shape
    scorer = MI355XScorer(np.zeros((n_users, K), np.float32), np.zeros((n_items, K), np.float32), train)
    out = {}
    for name in FITS:
        if name == "ials":
            C = train.copy()
            C.data = 1.0 + 2.0 * C.data
            handle = IALS_MI355X_Epoch(C, K, 1e-2, K ** -0.5 * np.random.default_rng(5).random((n_items, K)))
            handle.run_epochs(1)
        else:
            handle = MatrixFactorization_MI355X_Epoch(train, n_factors=K, algorithm_name="MF_BPR", batch_size=1024, learning_rate=0.05,
                                                      sgd_mode=FITS[name]["sgd_mode"], random_seed=5)
            handle.epochIteration_Cython()
        scorer.update_from(handle)
        wall, kernel = [], []
        for _ in range(REPEATS):
            t0 = time.perf_counter()
            scorer.update_from(handle)
            sync()
            wall.append(time.perf_counter() - t0)
            st = scorer.stats()
            kernel.append(st["kernel_ms"] * 1e-3)
        rate = st["algorithmic_bytes"] / statistics.median(kernel)
        out[name] = {"bytes": st["algorithmic_bytes"], "launches": st["n_launches"], "wall_s_runs": wall, "wall_s": statistics.median(wall),
                     "kernel_s_runs": kernel, "kernel_s": statistics.median(kernel), "bytes_per_s": rate,
                     "share_of_hbm_stream_rate": rate / HBM_STREAM_BYTES_PER_S}
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
    out = {"device": _native.device_name(), "n_users": train.shape[0], "n_items": train.shape[1], "train_nnz": int(train.nnz), "k": K,
           "cutoffs": CUTOFFS, "repeats": REPEATS, "fits": {name: {k: v for k, v in spec.items() if k != "kind"} for name, spec in FITS.items()},
           "modes": {}}
    for mode in modes:
        out["modes"][mode] = {}
        for name, spec in FITS.items():
            one_fit(spec, mode, train, evaluator, sync)                 # warm-up
            runs = [one_fit(spec, mode, train, evaluator, sync) for _ in range(REPEATS)]
            row = {"runs": runs, "validations": runs[0]["validations"], "map": runs[0]["map"]}
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
    ap.add_argument("--out", default=os.path.join(os.path.dirname(HERE), "profiles", "validation_hand_off_time.json"))
    ap.add_argument("--parent-root", help="a checkout of the parent commit with libmi355rec.so built: its fits are measured too")
    ap.add_argument("--seconds", type=int, default=500, help="time limit of each measuring process")
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
    result["same_map"] = {name: host[name]["map"] == device[name]["map"] for name in FITS}
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
                "device_overhead_s": device[name]["overhead_s"], "parent_overhead_s": par[name]["overhead_s"],
                "device_overhead_below_parent": device[name]["overhead_s"] < par[name]["overhead_s"]} for name in FITS}
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(result, f, indent=1, sort_keys=True)
        f.write("\n")
    for name in FITS:
        print("%-12s per validation: host %.4f s (overhead %.4f), device %.4f s (overhead %.4f)" % (
            name, host[name]["validation_s"], host[name]["overhead_s"], device[name]["validation_s"], device[name]["overhead_s"]), flush=True)
        h = this["hand_off"][name]
        print("%-12s hand-off alone: %.3f ms wall, %.3f ms kernels, %.2f TB/s (%.0f%% of the stream rate)" % (
            name, h["wall_s"] * 1e3, h["kernel_s"] * 1e3, h["bytes_per_s"] * 1e-12, 100 * h["share_of_hbm_stream_rate"]), flush=True)
    if "conditions" in result:
        print("conditions:", json.dumps(result["conditions"]), flush=True)
    print("written", a.out)


if __name__ == "__main__":
    main()
