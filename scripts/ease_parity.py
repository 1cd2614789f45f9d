"""Accuracy of EASE_R_MI355X_Recommender against the float64 closed form, case by case (tests/ease_cases.py), next to the error of the
reference's own float32 `np.linalg.inv` on the same float32 Gram matrix: both as max |W - W64| / max |W64|, their ratio, the block size
of the elimination and the route the fit took (device inverse, or host inverse after the device refused an indefinite matrix).

    python scripts/ease_parity.py --out profiles/ease_r_parity.json
"""
import argparse
import json
import os
import sys

import numpy as np
import scipy.sparse as sps

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ease_r_parity.json"))
    a = ap.parse_args()
    import ease_cases as EC
    from recsys2019_deeplearning_evaluation_amd import EASE_R_MI355X_Recommender, _native
    rows = []
    cases = dict(EC.fit_cases(), **EC.indefinite_cases())
    for name in sorted(cases):
        X, kw = cases[name]
        if kw["topK"] is not None:
            continue
        G = EC.gram_f32(X, kw["l2_norm"], kw["normalize_matrix"])
        W64 = EC.weights_f64(G)
        scale = float(np.abs(W64).max())
        rec = EASE_R_MI355X_Recommender(sps.csr_matrix(X).copy(), verbose=False)
        rec.fit(verbose=False, **kw)
        device = float(np.abs(rec.W_sparse - W64).max() / scale)
        lu = float(np.abs(EC.weights_from_precision(np.linalg.inv(G)) - W64).max() / scale)
        info = rec.fit_info
        rows.append({"case": name, "n_items": int(len(G)), "l2_norm": kw["l2_norm"], "normalize_matrix": kw["normalize_matrix"],
                     "condition_number": float(np.linalg.cond(G.astype(np.float64))), "inverse": info["inverse"], "block": info["block"],
                     "failed_step": info["failed_step"], "device_error": device, "float32_lu_error": lu, "ratio": device / lu})
        print("%-40s n %5d  %-6s  device %.2e  float32 LU %.2e  ratio %.1f" % (name, len(G), info["inverse"], device, lu, device / lu), flush=True)
    result = {"device": _native.device_name(), "what": "max |W - W64| / max |W64|, W64 = float64 closed form of the float32 Gram matrix",
              "bar": EC.BAR, "cases": rows}
    with open(a.out, "w") as f:
        json.dump(result, f, indent=1, sort_keys=True)
        f.write("\n")
    print("written", a.out)


if __name__ == "__main__":
    main()
