"""Accuracy of the pivoted float64 device inverse of EASE_R, case by case (tests/ease_pivoted_cases.py, both block sizes), as
max |W - W64| / max |W64| with W64 the float64 closed form of the same float32 matrix -- beside the distance of the route it
replaces (float32 `np.linalg.inv` on the host), of LAPACK's float32 `sgetrf` + `sgetri`, and of the NumPy restatement of the device
method; then the three explicit-rating fits through EASE_R_MI355X_Recommender(indefinite="device").

    python scripts/ease_pivoted_parity.py --out profiles/ease_r_pivoted_parity.json
"""
import argparse
import json
import os
import sys

import numpy as np
import scipy.linalg.lapack as lapack
import scipy.sparse as sps

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def sgetri_inverse(G):
    lu, piv, info = lapack.sgetrf(np.asarray(G, dtype=np.float32))
    assert info == 0
    inv, info = lapack.sgetri(lu, piv)
    assert info == 0
    return inv


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ease_r_pivoted_parity.json"))
    a = ap.parse_args()
    import ease_cases as EC
    import ease_pivoted_cases as PC
    from recsys2019_deeplearning_evaluation_amd import EASE_R_MI355X_Recommender, MI355XEase, _native
    rows = []
    for block in PC.BLOCKS:
        os.environ["MI355REC_EASE_BLOCK"] = str(block)
        for name, G in PC.all_matrices(block):
            if len(G) == 1:
                continue
            W64 = PC.weights_f64_of(name, block)
            scale = float(np.abs(W64).max())
            ease = MI355XEase(len(G))
            try:
                ease.set_matrix(G)
                ease.invert(pivoted=True)
                info = dict(ease.fit_info(), **ease.pivot_info())
                W = ease.get_dense()
            finally:
                ease.close()

            def distance(V):
                return float(np.abs(V - W64).max() / scale)

            row = {"case": name, "n_items": int(len(G)), "block": info["block"], "moved_rows": info["moved_rows"], "min_pivot": info["min_pivot"],
                   "condition_number": float(np.linalg.cond(G.astype(np.float64))), "device_pivoted": distance(W),
                   "host_float32_inv": distance(EC.weights_from_precision(np.linalg.inv(G))),
                   "sgetri": distance(EC.weights_from_precision(sgetri_inverse(G))),
                   "restatement_float64": distance(PC.restated_weights(G, block)),
                   "restatement_rounded_to_float32": distance(PC.restated_weights(G, block).astype(np.float32))}
            rows.append(row)
            print("block %3d  %-24s n %5d  device %.2e  host inv %.2e  sgetri %.2e  restatement %.2e" % (
                block, name, len(G), row["device_pivoted"], row["host_float32_inv"], row["sgetri"], row["restatement_float64"]), flush=True)
        # the structured cases (their W is not defined: zeros on the diagonal of the inverse), measured on the inverse itself
        for name, G in PC.structured_matrices(block):
            P64 = np.linalg.inv(G.astype(np.float64))
            scale = float(np.abs(P64).max())
            ease = MI355XEase(len(G))
            try:
                ease.set_matrix(G)
                ease.invert(pivoted=True)
                info = dict(ease.fit_info(), **ease.pivot_info())
                P = ease.get_matrix()
            finally:
                ease.close()
            row = {"case": name, "n_items": int(len(G)), "block": info["block"], "moved_rows": info["moved_rows"], "min_pivot": info["min_pivot"],
                   "measured_on": "the inverse", "device_pivoted": float(np.abs(P - P64).max() / scale),
                   "host_float32_inv": float(np.abs(np.linalg.inv(G) - P64).max() / scale),
                   "sgetri": float(np.abs(sgetri_inverse(G) - P64).max() / scale),
                   "device_equals_the_rounded_float64_inverse": bool(np.array_equal(P, P64.astype(np.float32)))}
            rows.append(row)
            print("block %3d  %-24s n %5d  device %.2e  host inv %.2e  sgetri %.2e  (inverse; bit-equal to float64 rounded: %s)" % (
                block, name, len(G), row["device_pivoted"], row["host_float32_inv"], row["sgetri"],
                row["device_equals_the_rounded_float64_inverse"]), flush=True)
    os.environ.pop("MI355REC_EASE_BLOCK", None)
    fits = []
    for name, (X, kw) in sorted(PC.fit_cases().items()):
        W64 = PC.weights_f64_of(name, PC.BLOCKS[-1])
        scale = float(np.abs(W64).max())
        out = {"case": name, "n_items": int(len(W64))}
        for route in ("device", "host"):
            rec = EASE_R_MI355X_Recommender(sps.csr_matrix(X).copy(), verbose=False, indefinite=route)
            rec.fit(verbose=False, **dict(kw, topK=None))
            out["fit_indefinite_" + route] = float(np.abs(rec.W_sparse - W64).max() / scale)
            out["inverse_" + route] = rec.fit_info["inverse"]
        fits.append(out)
        print("fit  %-24s n %5d  indefinite=device %.2e (%s)  indefinite=host %.2e (%s)" % (
            name, out["n_items"], out["fit_indefinite_device"], out["inverse_device"], out["fit_indefinite_host"], out["inverse_host"]), flush=True)
    result = {"device": _native.device_name(), "what": "max |W - W64| / max |W64|, W64 = float64 closed form of the float32 matrix",
              "bound": PC.ROUNDED_BOUND, "cases": rows, "fits": fits}
    with open(a.out, "w") as f:
        json.dump(result, f, indent=1, sort_keys=True)
        f.write("\n")
    print("written", a.out)


if __name__ == "__main__":
    main()
