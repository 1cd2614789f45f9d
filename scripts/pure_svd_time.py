"""Wall time of PureSVDRecommender.fit at the ML-20M shape (named_urm("ml20m"): 138 493 x 26 744, 20 M cells) for num_factors 50, 200 and
350, its split into the device phases (products, Gram builds, applies) and everything else (host preparation, uploads, the chain of
step-wise calls with their r x r copies and LAPACK calls), the bytes a product pass moves against the algorithmic nnz (4 r + 8), and on
the same machine the time of the reference's solver: sklearn's randomized_svd where it imports, otherwise the float32 restatement of
tests/pure_svd_cases.py (labelled as such).  Every fit runs in a child process of its own under `timeout`; the device time is the
best of two fits after one warm-up, the reference is run once.

    python scripts/pure_svd_time.py --out profiles/pure_svd_time.json
"""
import argparse
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def device_fit(k):
    from recsys2019_deeplearning_evaluation_amd import PureSVDRecommender, _native
    from recsys2019_deeplearning_evaluation_amd.synthetic import named_urm
    X = named_urm("ml20m")
    rec = PureSVDRecommender(X, verbose=False)
    walls = []
    for _ in range(3):                       # the first one warms the device up
        t0 = time.perf_counter()
        rec.fit(num_factors=k, random_seed=1)
        walls.append(time.perf_counter() - t0)
    st = rec.fit_stats
    r, nnz, products = st["r"], st["nnz"], st["products"]
    device_ms = st["product_ms"] + st["gram_ms"] + st["apply_ms"]
    per_pass_ms = st["product_ms"] / products
    algorithmic = nnz * (4.0 * r + 8.0)
    return {"num_factors": k, "r": r, "n_iter": st["n_iter"], "device": _native.device_name(), "fit_wall_s": min(walls[1:]),
            "fit_wall_s_all": walls, "product_ms": st["product_ms"], "gram_ms": st["gram_ms"], "apply_ms": st["apply_ms"],
            "kernels_s": device_ms / 1e3, "draw_s": st["draw_s"], "create_s": st["create_s"], "chain_s": st["chain_s"],
            "chain_minus_kernels_s": st["chain_s"] - device_ms / 1e3, "download_s": st["download_s"], "products": products, "gram_apply_pairs": st["gram_apply_pairs"],
            "calls": st["calls"], "launches": st["launches"], "host_fallbacks": st["host_fallbacks"],
            "product_pass_ms": per_pass_ms, "algorithmic_bytes_per_pass": algorithmic,
            "algorithmic_TB_per_s": algorithmic / per_pass_ms / 1e9, "create_bytes": st["create_bytes"], "h2d_bytes": st["h2d_bytes"],
            "d2h_bytes": st["d2h_bytes"], "sigma_first_last": [float(st["singular_values"][0]), float(st["singular_values"][-1])]}


def reference_fit(k):
    from recsys2019_deeplearning_evaluation_amd.synthetic import named_urm
    X = named_urm("ml20m")
    try:
        from sklearn.utils.extmath import randomized_svd
        label = "sklearn.utils.extmath.randomized_svd"
        t0 = time.perf_counter()
        _, s, _ = randomized_svd(X, n_components=k, random_state=1)
    except ImportError:
        import pure_svd_cases as P
        label = "float32 restatement (tests/pure_svd_cases.replay)"
        t0 = time.perf_counter()
        _, _, s = P.replay(X, k, 1, np.float32, return_s=True)
    return {"num_factors": k, "solver": label, "wall_s": time.perf_counter() - t0, "threads": os.environ.get("OMP_NUM_THREADS"),
            "sigma_first_last": [float(s[0]), float(s[-1])]}


def child(mode, k, seconds):
    cmd = ["timeout", "-k", "10", str(seconds), sys.executable, os.path.abspath(__file__), "--" + mode, str(k)]
    out = subprocess.run(cmd, capture_output=True, text=True)
    if out.returncode != 0:
        return {"num_factors": k, "failed": out.returncode, "stderr": out.stderr[-400:]}
    return json.loads(out.stdout.strip().splitlines()[-1])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "pure_svd_time.json"))
    ap.add_argument("--factors", default="50,200,350")
    ap.add_argument("--reference-factors", default="50,200,350")
    ap.add_argument("--device", type=int)
    ap.add_argument("--reference", type=int)
    args = ap.parse_args()
    if args.device is not None:
        print(json.dumps(device_fit(args.device)))
        return
    if args.reference is not None:
        print(json.dumps(reference_fit(args.reference)))
        return
    record = {"shape": "ml20m (synthetic.named_urm)", "device_fits": [], "reference_fits": []}
    for k in [int(v) for v in args.factors.split(",") if v]:
        record["device_fits"].append(child("device", k, 300))
        if record["device_fits"][-1].get("failed"):          # nothing more on the device after a failure
            break
        print(json.dumps(record["device_fits"][-1]), flush=True)
    for k in [int(v) for v in args.reference_factors.split(",") if v]:
        record["reference_fits"].append(child("reference", k, 900))
        print(json.dumps(record["reference_fits"][-1]), flush=True)
    with open(args.out, "w") as f:
        json.dump(record, f, indent=1)
    print("written", args.out)


if __name__ == "__main__":
    main()
