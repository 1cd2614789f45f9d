"""Device time of the SLIM ElasticNet fit (slim_elasticnet.py) at the ml1m, ml20m and netflix shapes, three points of the reference's
search space (ParameterTuning/run_parameter_search.py:693-698: topK 5..1000, l1_ratio log-uniform 1e-5..1, alpha uniform 1e-3..1).

Targets are fitted in contiguous chunks until a time budget per point is spent; targets/s comes from the chunks that ran and the
time of the whole catalogue is extrapolated from it (marked "estimated" in the record when not every target ran).  Reported per
point: Gram build time, accepted coordinate changes, sweeps, block steps, targets/s, bytes of G streamed (one row of G per accepted
change) and their fraction of the 8 TB/s HBM peak.

    python scripts/slim_en_time.py --out profiles/slim_en_time.json [--budget 60] [--shapes ml1m,ml20m,netflix]
    python scripts/slim_en_time.py --cpu-reference 4 --out profiles/slim_en_cpu_reference.json   # sklearn on the host, per item
"""
import argparse
import json
import os
import platform
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from recsys2019_deeplearning_evaluation_amd.synthetic import named_urm          # noqa: E402

POINTS = [dict(topK=1000, l1_ratio=1e-3, alpha=0.05), dict(topK=500, l1_ratio=3e-3, alpha=0.5), dict(topK=5, l1_ratio=0.1, alpha=1.0)]
HBM_PEAK = 8.0e12


def device(shapes, budget, chunk):
    from recsys2019_deeplearning_evaluation_amd import _native
    from recsys2019_deeplearning_evaluation_amd.slim_elasticnet import RAND_R_MAX, SLIMElasticNet_MI355X_Fit
    records = []
    for shape in shapes:
        X = named_urm(shape, "binary")
        n = X.shape[1]
        t0 = time.time()
        solver = SLIMElasticNet_MI355X_Fit(X)
        create_s = time.time() - t0
        gram_ms = solver.fit_info()["gram_ms"]
        try:
            for p in POINTS:
                seeds = np.random.RandomState(7).randint(0, RAND_R_MAX, size=n)
                tot = dict(ms=0.0, changes=0, sweeps=0, steps=0, gap_tests=0, targets=0, converged=0, kept=0)
                start = 0
                while start < n and tot["ms"] < 1e3 * budget:
                    end = min(n, start + chunk)
                    _, _, counts, _, conv = solver.fit_range(start, end, seeds[start:end], positive_only=True, **p)
                    st, info = solver.stats(), solver.fit_info()
                    tot["ms"] += st["kernel_ms"]
                    for k in ("changes", "sweeps", "steps", "gap_tests"):
                        tot[k] += info[k]
                    tot["targets"] += end - start
                    tot["converged"] += int(conv.sum())
                    tot["kept"] += int(counts.sum())
                    start = end
                rate = tot["targets"] / (tot["ms"] / 1e3)
                bytes_g = tot["changes"] * n * 4.0
                rec = dict(shape=shape, n_users=X.shape[0], n_items=n, nnz=int(X.nnz), point=p, device=_native.device_name(),
                           gram_ms=gram_ms, create_s=create_s, h_in_lds=info["h_in_lds"], targets_fitted=tot["targets"],
                           fit_ms_measured=tot["ms"], targets_per_s=rate, whole_fit_s=n / rate,
                           whole_fit_s_is="measured" if tot["targets"] == n else "estimated from %d of %d targets" % (tot["targets"], n),
                           accepted_changes=tot["changes"], sweeps=tot["sweeps"], block_steps=tot["steps"], gap_tests=tot["gap_tests"],
                           converged_fraction=tot["converged"] / tot["targets"], kept_per_target=tot["kept"] / tot["targets"],
                           sweeps_per_target=tot["sweeps"] / tot["targets"], changes_per_target=tot["changes"] / tot["targets"],
                           G_bytes_streamed=bytes_g, G_stream_GBps=bytes_g / (tot["ms"] / 1e3) / 1e9,
                           hbm_fraction=bytes_g / (tot["ms"] / 1e3) / HBM_PEAK)
                print(json.dumps(rec), flush=True)
                records.append(rec)
        finally:
            solver.close()
    return records


def cpu_reference(shapes, n_sample):
    """sklearn ElasticNet exactly as the reference configures it (SLIMElasticNetRecommender.py:55-63, :88-95), on a sample of items."""
    import sklearn
    import warnings
    from sklearn.linear_model import ElasticNet
    records = []
    for shape in shapes:
        Xc = named_urm(shape, "binary").tocsc().astype(np.float32)
        n = Xc.shape[1]
        items = np.random.RandomState(3).choice(n, n_sample, replace=False)
        for p in POINTS:
            model = ElasticNet(alpha=p["alpha"], l1_ratio=p["l1_ratio"], positive=True, fit_intercept=False, copy_X=False, precompute=True,
                               selection="random", max_iter=100, tol=1e-4)
            times = []
            for j in items:
                y = Xc[:, j].toarray()
                a, b = Xc.indptr[j], Xc.indptr[j + 1]
                keep = Xc.data[a:b].copy()
                Xc.data[a:b] = 0.0
                t0 = time.time()
                with warnings.catch_warnings():
                    warnings.simplefilter("ignore")
                    model.fit(Xc, y)
                times.append(time.time() - t0)
                Xc.data[a:b] = keep
            rec = dict(shape=shape, n_items=n, point=p, items=items.tolist(), seconds_per_item=times, mean_s_per_item=float(np.mean(times)),
                       whole_fit_s_estimated=float(np.mean(times)) * n, sklearn=sklearn.__version__, numpy=np.__version__,
                       host=platform.processor() or platform.machine(), threads="single process, one item at a time like the reference")
            print(json.dumps(rec), flush=True)
            records.append(rec)
    return records


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="ml1m,ml20m,netflix")
    ap.add_argument("--budget", type=float, default=60.0, help="device seconds per shape and point")
    ap.add_argument("--chunk", type=int, default=2048)
    ap.add_argument("--cpu-reference", type=int, default=0, help="sklearn per-item CPU time on this many sampled items instead")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    shapes = args.shapes.split(",")
    recs = cpu_reference(shapes, args.cpu_reference) if args.cpu_reference else device(shapes, args.budget, args.chunk)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(recs, f, indent=1)


if __name__ == "__main__":
    main()
