"""Time of NMFRecommender.fit at the ML-20M shape (named_urm("ml20m"): 138 493 x 26 744, 20 M cells) for the three solver / loss pairs
at num_factors 50 and 200: device milliseconds per iteration by phase (sparse products, GEMM, sweep, element-wise pass, SDDMM,
reductions) for both stages, the host's share of an iteration (wall time of the loop minus the device time: the call chain, the
permutation draws and the wait for the stop statistic), the whole fit, and on the same machine sklearn's seconds per iteration of the
same solver -- from two runs capped at 1 and at 1 + N iterations with tol=0, so that the initialisation cancels; a full sklearn fit at
this shape is not expected to finish in a session.  Every measurement runs in a child process of its own under `timeout`.

    python scripts/nmf_time.py --out profiles/nmf_time.json
"""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

PAIRS = {"cd": ("coordinate_descent", "frobenius", "cd"), "mu-fro": ("multiplicative_update", "frobenius", "mu"),
         "mu-kl": ("multiplicative_update", "kullback-leibler", "mu")}


def device_fit(pair, k):
    from recsys2019_deeplearning_evaluation_amd import NMFRecommender, _native
    from recsys2019_deeplearning_evaluation_amd.nmf import PHASES
    from recsys2019_deeplearning_evaluation_amd.synthetic import named_urm
    X = named_urm("ml20m")
    solver, loss, _ = PAIRS[pair]
    rec = NMFRecommender(X, verbose=False)
    t0 = time.perf_counter()
    rec.fit(num_factors=k, solver=solver, init_type="random", beta_loss=loss, random_seed=1)
    wall = time.perf_counter() - t0
    st = rec.fit_stats
    out = {"pair": pair, "num_factors": k, "device": _native.device_name(), "fit_wall_s": wall, "nnz": st["nnz"], "all_ones": st["all_ones"],
           "init_s": st["init_s"], "create_s": st["create_s"], "download_s": st["download_s"], "draw_s": st["draw_s"],
           "create_bytes": st["create_bytes"], "h2d_bytes": st["h2d_bytes"], "d2h_bytes": st["d2h_bytes"], "launches": st["launches"],
           "calls": st["calls"]}
    for stage, n_iter, loop_s in (("fit", st["n_iter_fit"], st["fit_s"]), ("transform", st["n_iter_transform"], st["transform_s"])):
        phases = st[stage + "_phase_ms"]
        device_ms = sum(phases.values())
        out[stage] = {"n_iter": n_iter, "loop_s": loop_s, "device_ms_per_iter": device_ms / n_iter,
                      "host_ms_per_iter": (1e3 * loop_s - device_ms) / n_iter, "phase_ms_per_iter": {p: phases[p] / n_iter for p in PHASES},
                      "last_stop_statistic": st["trajectory_" + stage][-1]}
    # algorithmic traffic and arithmetic of one stage-1 iteration: both sides
    n = X.shape[0] + X.shape[1]
    nnz = st["nnz"]
    product = nnz * (4.0 * k + (4.0 if st["all_ones"] else 8.0))
    out["algorithmic_per_iteration"] = {
        "product_bytes": 2 * product, "product_flops": 4.0 * nnz * k,
        "sweep_bytes": 12.0 * n * k, "sweep_flops": 2.0 * n * k * k,
        "gemm_bytes": 8.0 * n * k, "gemm_flops": 2.0 * n * k * k,
        "scale_bytes": 16.0 * n * k,
        "sddmm_bytes": 2 * nnz * (4.0 * k + 8.0 + (0.0 if st["all_ones"] else 4.0)), "sddmm_flops": 4.0 * nnz * k,
        "gram_bytes": 4.0 * n * k, "gram_flops": 2.0 * n * k * k}
    return out


def sklearn_fit(pair, k, iterations):
    import numpy as np
    from sklearn.decomposition import NMF
    from recsys2019_deeplearning_evaluation_amd.synthetic import named_urm
    import warnings
    warnings.filterwarnings("ignore")
    X = named_urm("ml20m").astype(np.float32)
    _, loss, solver = PAIRS[pair]
    walls = {}
    for max_iter in (1, 1 + iterations):
        model = NMF(n_components=k, init="random", solver=solver, beta_loss=loss, random_state=1, l1_ratio=0.5, shuffle=True, max_iter=max_iter,
                    tol=0)
        t0 = time.perf_counter()
        model.fit(X)
        walls[max_iter] = time.perf_counter() - t0
        assert model.n_iter_ == max_iter
    return {"pair": pair, "num_factors": k, "what": "sklearn.decomposition.NMF.fit, tol=0", "threads": os.environ.get("OMP_NUM_THREADS"),
            "wall_s": {str(m): w for m, w in walls.items()}, "iterations": iterations,
            "seconds_per_iteration": (walls[1 + iterations] - walls[1]) / iterations}


def child(args, limit):
    cmd = ["timeout", "-k", "10", str(limit), sys.executable, os.path.abspath(__file__)] + args
    p = subprocess.run(cmd, capture_output=True, text=True)
    if p.returncode != 0:
        return {"failed": p.returncode, "stderr": p.stderr[-2000:]}
    return json.loads(p.stdout.strip().splitlines()[-1])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "nmf_time.json"))
    ap.add_argument("--factors", type=int, nargs="+", default=[50, 200])
    ap.add_argument("--pairs", nargs="+", default=list(PAIRS))
    ap.add_argument("--sklearn-iterations", type=int, default=2)
    ap.add_argument("--no-sklearn", action="store_true")
    ap.add_argument("--no-device", action="store_true")
    ap.add_argument("--device-fit", nargs=2)
    ap.add_argument("--sklearn-fit", nargs=3)
    a = ap.parse_args()
    if a.device_fit:
        print(json.dumps(device_fit(a.device_fit[0], int(a.device_fit[1]))))
        return
    if a.sklearn_fit:
        print(json.dumps(sklearn_fit(a.sklearn_fit[0], int(a.sklearn_fit[1]), int(a.sklearn_fit[2]))))
        return
    result = {"shape": "named_urm('ml20m')", "device_fits": [], "sklearn": []}
    faulted = a.no_device
    for k in a.factors:
        for pair in a.pairs:
            if faulted:                                 # after a device run that failed or ran out of time nothing more is started on the device
                break
            r = child(["--device-fit", pair, str(k)], 300)
            result["device_fits"].append(dict(r, pair=pair, num_factors=k))
            if "failed" in r:
                faulted = True
                break
            print("device %s k = %d: %.2f s, fit %d iterations at %.2f ms device + %.2f ms host, transform %d at %.2f + %.2f" % (
                pair, k, r["fit_wall_s"], r["fit"]["n_iter"], r["fit"]["device_ms_per_iter"], r["fit"]["host_ms_per_iter"],
                r["transform"]["n_iter"], r["transform"]["device_ms_per_iter"], r["transform"]["host_ms_per_iter"]), flush=True)
    if not a.no_sklearn:
        for k in a.factors:
            for pair in a.pairs:
                r = child(["--sklearn-fit", pair, str(k), str(a.sklearn_iterations)], 900)
                result["sklearn"].append(dict(r, pair=pair, num_factors=k))
                print("sklearn %s k = %d: %s" % (pair, k, r.get("seconds_per_iteration", r)), flush=True)
    with open(a.out, "w") as f:
        json.dump(result, f, indent=1, sort_keys=True)
        f.write("\n")
    print("written", a.out)


if __name__ == "__main__":
    main()
