"""Time of an EASE_R fit on explicit-rating URMs at the ML-1M, Netflix and ML-20M shapes (named_urm(..., "real")): the same class
with indefinite="device" -- the unpivoted attempt that refuses, the rebuilt Gram matrix, the pivoted float64 inverse (pivot search +
row swaps, update GEMM, the rest), scaling + top-K -- against indefinite="host", the float32 `np.linalg.inv` on the host's threads
(OMP_NUM_THREADS, 16 where this was recorded), in the same run.  The device fit runs twice: the first allocates the float64 working
matrix and loads the kernels.  A handle-level run adds a sampled residual max |G P[:, j] - e_j| in float64 over 64 random columns (a
float64 host inverse is too slow to serve as truth at these sizes).  Every measurement runs in a child process of its own under
`timeout`; after a device run that failed nothing more is started on the device.

    python scripts/ease_pivoted_time.py --out profiles/ease_r_pivoted_time.json [--shapes ml1m netflix ml20m] [--skip-host ml20m]
"""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

F64_MFMA_FLOPS = 78.6e12        # v_mfma_f64_16x16x4_f64, peak
L2_NORM, TOPK = 1e3, 100


def device_fit(shape):
    import numpy as np
    from recsys2019_deeplearning_evaluation_amd import Compute_Similarity_MI355X, EASE_R_MI355X_Recommender, MI355XEase, _native
    from recsys2019_deeplearning_evaluation_amd.synthetic import named_urm
    X = named_urm(shape, "real")
    n = X.shape[1]
    fits = []
    for _ in range(2):
        rec = EASE_R_MI355X_Recommender(X, verbose=False, indefinite="device")
        t0 = time.perf_counter()
        rec.fit(topK=TOPK, l2_norm=L2_NORM, verbose=False)
        info = dict(rec.fit_info, fit_wall_s=time.perf_counter() - t0)
        fits.append(info)
    # the handle alone: the inverse's own time and a sampled residual of what it returns
    diagonal = (np.diff(X.tocsc().indptr) + L2_NORM).astype(np.float32)
    builder = Compute_Similarity_MI355X(X, topK=0, shrink=0, normalize=False, similarity="cosine")
    ease = MI355XEase(n)
    try:
        ease.set_gram_from(builder)
        ease.set_diagonal(diagonal)
        t0 = time.perf_counter()
        ease.invert(pivoted=True)
        invert_wall_s = time.perf_counter() - t0
        handle = dict(ease.fit_info(), invert_wall_s=invert_wall_s, **ease.pivot_info())
        P = ease.get_matrix()
    finally:
        ease.close()
        builder.close()
    rng = np.random.RandomState(7)
    cols = rng.choice(n, size=min(64, n), replace=False)
    X64 = X.astype(np.float64).tocsr()
    Pc = np.ascontiguousarray(P[:, cols], dtype=np.float64)
    squares = np.asarray(X64.multiply(X64).sum(axis=0)).ravel()
    R = X64.T @ (X64 @ Pc) + (diagonal.astype(np.float64) - squares)[:, None] * Pc        # the diagonal of G is popularity + l2
    R[cols, np.arange(len(cols))] -= 1.0
    flops = 2.0 * n ** 3
    return {"shape": shape, "n_items": n, "n_users": X.shape[0], "nnz": int(X.nnz), "device": _native.device_name(), "topK": TOPK,
            "l2_norm": L2_NORM, "first_fit": fits[0], "second_fit": fits[1], "handle": handle, "sampled_residual": float(np.abs(R).max()),
            "inverse_flops": flops, "update_flops_per_s": flops / (1e-3 * handle["update_ms"]),
            "update_fraction_of_f64_mfma_peak": flops / (1e-3 * handle["update_ms"]) / F64_MFMA_FLOPS}


def host_fit(shape):
    import numpy as np
    from recsys2019_deeplearning_evaluation_amd import EASE_R_MI355X_Recommender
    from recsys2019_deeplearning_evaluation_amd.synthetic import named_urm
    X = named_urm(shape, "real")
    spent = {"inv_s": 0.0}
    real_inv = np.linalg.inv

    def timed_inv(a):
        t = time.perf_counter()
        r = real_inv(a)
        spent["inv_s"] += time.perf_counter() - t
        return r

    rec = EASE_R_MI355X_Recommender(X, verbose=False, indefinite="host")
    np.linalg.inv = timed_inv
    try:
        t0 = time.perf_counter()
        rec.fit(topK=TOPK, l2_norm=L2_NORM, verbose=False)
        wall = time.perf_counter() - t0
    finally:
        np.linalg.inv = real_inv
    return {"shape": shape, "n_items": X.shape[1], "what": "EASE_R_MI355X_Recommender(indefinite=\"host\").fit: device Gram, refused unpivoted "
            "elimination, host float32 np.linalg.inv, host scaling and top-K", "threads": os.environ.get("OMP_NUM_THREADS"),
            "fit_info": rec.fit_info, "fit_wall_s": wall, "inverse_s": spent["inv_s"]}


def child(args, limit):
    cmd = ["timeout", "-k", "10", str(limit), sys.executable, os.path.abspath(__file__)] + args
    p = subprocess.run(cmd, capture_output=True, text=True)
    if p.returncode != 0:
        return {"failed": p.returncode, "stderr": p.stderr[-2000:]}
    return json.loads(p.stdout.strip().splitlines()[-1])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ease_r_pivoted_time.json"))
    ap.add_argument("--shapes", nargs="+", default=["ml1m", "netflix", "ml20m"])
    ap.add_argument("--skip-host", nargs="*", default=[], help="shapes whose host fit is not run")
    ap.add_argument("--device-fit", help="(child) SHAPE")
    ap.add_argument("--host-fit", help="(child) SHAPE")
    a = ap.parse_args()
    if a.device_fit:
        print(json.dumps(device_fit(a.device_fit)))
        return
    if a.host_fit:
        print(json.dumps(host_fit(a.host_fit)))
        return
    result = {"device_fits": [], "host_fits": [], "host_skipped": list(a.skip_host), "f64_mfma_flops": F64_MFMA_FLOPS}
    faulted = False
    for shape in a.shapes:
        r = child(["--device-fit", shape], 500)
        result["device_fits"].append(dict(r, shape=shape))
        if "failed" in r:
            faulted = True
            print("device %s failed: %s" % (shape, r), flush=True)
            break
        f, h = r["second_fit"], r["handle"]
        print("device %-8s n %6d: fit() %.2f s (%s; unpivoted attempt %.2f s, inverse %.1f ms = pivot search + swaps %.1f + update %.1f "
              "(%.1f Tflop/s) + rest, %d launches, %d rows moved, min |pivot| %.3g), residual %.1e" % (
                  shape, r["n_items"], f["fit_wall_s"], f["inverse"], f.get("unpivoted_s", 0.0), h["invert_ms"], h["pivot_ms"], h["update_ms"],
                  r["update_flops_per_s"] / 1e12, h["launches"], h["moved_rows"], h["min_pivot"], r["sampled_residual"]), flush=True)
    for shape in a.shapes:
        if shape in a.skip_host or faulted:
            continue
        r = child(["--host-fit", shape], 500)
        result["host_fits"].append(dict(r, shape=shape))
        if "failed" in r:
            faulted = True
        print("host   %-8s: fit() %s s, np.linalg.inv %s s, %s threads" % (shape, r.get("fit_wall_s"), r.get("inverse_s"), r.get("threads")), flush=True)
    with open(a.out, "w") as f:
        json.dump(result, f, indent=1, sort_keys=True)
        f.write("\n")
    print("written", a.out)


if __name__ == "__main__":
    main()
