"""Time of an EASE_R fit on binary URMs at the ML-1M, Netflix and ML-20M shapes (named_urm): the device path phase by phase -- Gram
matrix, inverse, scaling + top-K, download of the slabs, and the download of the dense W -- after one warm-up, best and median of
`--repeats`; the achieved flop/s of the inverse over 2 n^3 as a fraction of the 155 Tflop/s the f32 MFMA path reaches; a sampled
residual max |G P[:, j] - e_j| in float64 over 64 random columns of the device's inverse (a float64 host inverse is too slow to serve
as truth at these sizes); and, in the same run, the same fit through EASE_R_Recommender -- the host float32 `np.linalg.inv` -- with
the inverse's share of it.  Every measurement runs in a child process of its own under `timeout`; after a device run that failed
nothing more is started on the device.

    python scripts/ease_time.py --out profiles/ease_r_time.json [--skip-host ml20m] [--blocks 64 128]
"""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

F32_MFMA_FLOPS = 155e12         # v_mfma_f32_32x32x2_f32, measured
L2_NORM, TOPK = 1e3, 100


def device_fit(shape, repeats, blocks):
    """One result per block size (MI355REC_EASE_BLOCK, read when a handle is created; 0: the library's default), on one URM."""
    from recsys2019_deeplearning_evaluation_amd.synthetic import named_urm
    X = named_urm(shape)
    out = []
    for block in blocks:
        if block:
            os.environ["MI355REC_EASE_BLOCK"] = str(block)
        else:
            os.environ.pop("MI355REC_EASE_BLOCK", None)
        out.append(dict(device_fit_once(X, shape, repeats), block_asked=block))
    return out


def device_fit_once(X, shape, repeats):
    import numpy as np
    from recsys2019_deeplearning_evaluation_amd import Compute_Similarity_MI355X, EASE_R_MI355X_Recommender, MI355XEase, _native
    n = X.shape[1]
    diagonal = (np.diff(X.tocsc().indptr) + L2_NORM).astype(np.float32)
    phases = {k: [] for k in ("create_ms", "gram_ms", "invert_ms", "scale_topk_ms", "topk_call_ms", "total_ms")}
    info = None
    P = None
    for it in range(repeats + 1):                   # the first pass is the warm-up
        t0 = time.perf_counter()
        builder = Compute_Similarity_MI355X(X, topK=0, shrink=0, normalize=False, similarity="cosine")
        ease = MI355XEase(n)
        t1 = time.perf_counter()
        ease.set_gram_from(builder)
        ease.set_diagonal(diagonal)
        t2 = time.perf_counter()
        ease.invert()
        t3 = time.perf_counter()
        if it == repeats:
            P = ease.get_matrix()
            t3 = time.perf_counter()
        idx, val = ease.get_topk(TOPK)
        t4 = time.perf_counter()
        info = ease.fit_info()
        if it > 0:
            phases["create_ms"].append(1e3 * (t1 - t0))
            phases["gram_ms"].append(1e3 * (t2 - t1))
            phases["invert_ms"].append(info["invert_ms"])
            phases["scale_topk_ms"].append(info["topk_ms"])
            phases["topk_call_ms"].append(1e3 * (t4 - t3))
            phases["total_ms"].append(1e3 * (t2 - t0) + info["invert_ms"] + 1e3 * (t4 - t3))
        if it == repeats:
            t5 = time.perf_counter()
            W = ease.get_dense()
            dense_download_ms = 1e3 * (time.perf_counter() - t5)
            del W
        ease.close()
        builder.close()
    # sampled residual of the inverse: G = X^T X + l2 I for a binary URM (the diagonal of X^T X is the popularity)
    rng = np.random.RandomState(7)
    cols = rng.choice(n, size=min(64, n), replace=False)
    X64 = X.astype(np.float64).tocsr()
    Pc = np.ascontiguousarray(P[:, cols], dtype=np.float64)
    R = X64.T @ (X64 @ Pc) + L2_NORM * Pc
    R[cols, np.arange(len(cols))] -= 1.0
    worst = float(np.abs(R).max())
    del P
    # the recommender's own fit, as a user calls it
    rec = EASE_R_MI355X_Recommender(X, verbose=False)
    t0 = time.perf_counter()
    rec.fit(topK=TOPK, l2_norm=L2_NORM, verbose=False)
    fit_wall = time.perf_counter() - t0
    out = {"shape": shape, "n_items": n, "n_users": X.shape[0], "nnz": int(X.nnz), "device": _native.device_name(), "topK": TOPK,
           "l2_norm": L2_NORM, "block": info["block"], "steps": info["steps"], "launches": info["launches"], "repeats": repeats,
           "dense_download_ms": dense_download_ms, "sampled_residual": worst, "fit_wall_s": fit_wall, "fit_route": rec.fit_info["inverse"]}
    for k, v in phases.items():
        out[k] = {"best": min(v), "median": sorted(v)[len(v) // 2], "all": v}
    flops = 2.0 * n ** 3
    out["inverse_flops"] = flops
    out["inverse_flops_per_s"] = flops / (1e-3 * out["invert_ms"]["best"])
    out["inverse_fraction_of_f32_mfma_rate"] = out["inverse_flops_per_s"] / F32_MFMA_FLOPS
    return out


def host_fit(shape):
    import numpy as np
    from recsys2019_deeplearning_evaluation_amd import EASE_R_Recommender
    from recsys2019_deeplearning_evaluation_amd.synthetic import named_urm
    X = named_urm(shape)
    spent = {"inv_s": 0.0}
    real_inv = np.linalg.inv

    def timed_inv(a):
        t = time.perf_counter()
        r = real_inv(a)
        spent["inv_s"] += time.perf_counter() - t
        return r

    rec = EASE_R_Recommender(X, verbose=False)
    np.linalg.inv = timed_inv
    try:
        t0 = time.perf_counter()
        rec.fit(topK=TOPK, l2_norm=L2_NORM, verbose=False)
        wall = time.perf_counter() - t0
    finally:
        np.linalg.inv = real_inv
    return {"shape": shape, "n_items": X.shape[1], "what": "EASE_R_Recommender.fit: device Gram, host float32 np.linalg.inv, host scaling and top-K",
            "threads": os.environ.get("OMP_NUM_THREADS"), "fit_wall_s": wall, "inverse_s": spent["inv_s"],
            "inverse_flops_per_s": 2.0 * X.shape[1] ** 3 / spent["inv_s"]}


def child(args, limit):
    cmd = ["timeout", "-k", "10", str(limit), sys.executable, os.path.abspath(__file__)] + args
    p = subprocess.run(cmd, capture_output=True, text=True)
    if p.returncode != 0:
        return {"failed": p.returncode, "stderr": p.stderr[-2000:]}
    return json.loads(p.stdout.strip().splitlines()[-1])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ease_r_time.json"))
    ap.add_argument("--shapes", nargs="+", default=["ml1m", "netflix", "ml20m"])
    ap.add_argument("--blocks", type=int, nargs="+", default=[0], help="MI355REC_EASE_BLOCK values to time (0: the library's default)")
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--skip-host", nargs="*", default=[], help="shapes whose host fit is not run")
    ap.add_argument("--no-device", action="store_true", help="host fits only")
    ap.add_argument("--device-fit", nargs="+", help="(child) SHAPE REPEATS BLOCK...")
    ap.add_argument("--host-fit")
    a = ap.parse_args()
    if a.device_fit:
        print(json.dumps(device_fit(a.device_fit[0], int(a.device_fit[1]), [int(b) for b in a.device_fit[2:]])))
        return
    if a.host_fit:
        print(json.dumps(host_fit(a.host_fit)))
        return
    result = {"device_fits": [], "host_fits": [], "host_skipped": list(a.skip_host), "f32_mfma_flops": F32_MFMA_FLOPS}
    faulted = False
    for shape in a.shapes:
        if faulted or a.no_device:
            break
        rs = child(["--device-fit", shape, str(a.repeats)] + [str(b) for b in a.blocks], 900)
        if isinstance(rs, dict):                 # the child failed
            result["device_fits"].append(dict(rs, shape=shape))
            faulted = True
            print("device %s failed: %s" % (shape, rs), flush=True)
            break
        for r in rs:
            result["device_fits"].append(r)
            print("device %-8s n %6d block %3d: Gram %.1f ms, inverse %.1f ms (%.1f Tflop/s, %.2f of the f32 MFMA rate), scale + top-%d %.1f ms, "
                  "dense download %.0f ms, residual %.1e, fit() %.2f s" % (
                      shape, r["n_items"], r["block"], r["gram_ms"]["best"], r["invert_ms"]["best"], r["inverse_flops_per_s"] / 1e12,
                      r["inverse_fraction_of_f32_mfma_rate"], TOPK, r["scale_topk_ms"]["best"], r["dense_download_ms"], r["sampled_residual"],
                      r["fit_wall_s"]), flush=True)
    for shape in a.shapes:
        if shape in a.skip_host or faulted:
            continue
        r = child(["--host-fit", shape], 600)
        result["host_fits"].append(dict(r, shape=shape))
        if "failed" in r:
            faulted = True
        print("host   %-8s: %s" % (shape, {k: v for k, v in r.items() if k != "what"}), flush=True)
    with open(a.out, "w") as f:
        json.dump(result, f, indent=1, sort_keys=True)
        f.write("\n")
    print("written", a.out)


if __name__ == "__main__":
    main()
