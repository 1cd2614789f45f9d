"""Wall time of one ItemKNN_CFCBF_Hybrid_Recommender fit at the ML-20M shape (named_urm("ml20m", "real"): 138 493 x 26 744, 20 M
cells) with a synthetic ICM (about 20 of ~1 100 features of mildly skewed popularity per item, real values, plus four genre-like features held by 10,
20, 30 and 40 % of the items), three ways in one process, alternating:

  parent    what a caller had to do before the hybrid classes existed: SciPy `ICM * w`, hstack with URM.T, transpose, then the existing
            Compute_Similarity on the result (every call of this leg exists in the parent commit);
  host      ItemKNN_CFCBF_Hybrid_Recommender.fit(ICM_weight=w): the same stacking inside the class (reference behaviour);
  resident  fit(ICM_weight=w, resident_blocks=...): the blocks were uploaded once, the stack is scaled and made in HBM; one
            recommender object is fitted again and again, so the blocks' full verification is paid in the warm-up round only;
  resident_fresh  the same with a NEW recommender for every fit, as the reference's search makes one: its copies of URM_train and
            ICM_train are buffers the blocks have not seen, so every fit pays the checksum of every stored cell.

Every fit is split into host preparation (SciPy stacking, or the verification of the resident blocks), the device stack (resident
only), the similarity constructor (upload or device copy, norms, schedule), the column kernel (the library's own dispatch timing)
and the rest of compute_similarity (CSR assembly on the device + download).  Host clocks around calls that end in a device
synchronise; median and best of `--repeats` after one warm-up round.  Also recorded: the one-off cost of uploading the blocks, the
recommender's constructor (paid once per fit by a search, whichever way the class is fitted) and the largest difference between the three W_sparse.

    python scripts/knn_hybrid_time.py --out profiles/knn_hybrid_time.json
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import scipy.sparse as sps

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from recsys2019_deeplearning_evaluation_amd import Compute_Similarity, ItemKNN_CFCBF_Hybrid_Recommender, ResidentURM, _native     # noqa: E402
from recsys2019_deeplearning_evaluation_amd import knn_cbf                                                                        # noqa: E402
from recsys2019_deeplearning_evaluation_amd.recommender_base import check_matrix                                                  # noqa: E402
from recsys2019_deeplearning_evaluation_amd.synthetic import named_urm                                                            # noqa: E402

FIT = dict(topK=100, shrink=10, similarity="cosine", normalize=True)
WEIGHT = 0.3


def synthetic_icm(n_items, n_features=1100, per_item=20, genres=(0.1, 0.2, 0.3, 0.4), seed=5):
    rng = np.random.default_rng(seed)
    p = 1.0 / np.power(np.arange(1, n_features + 1, dtype=np.float64), 0.25)
    cdf = np.cumsum(p / p.sum())
    rows = np.repeat(np.arange(n_items), per_item)
    cols = np.minimum(np.searchsorted(cdf, rng.random(len(rows))), n_features - 1)
    for g, share in enumerate(genres):
        items = np.flatnonzero(rng.random(n_items) < share)
        rows, cols = np.concatenate([rows, items]), np.concatenate([cols, np.full(len(items), n_features + g)])
    key = np.unique(rows.astype(np.int64) * (n_features + len(genres)) + cols)
    rows, cols = key // (n_features + len(genres)), key % (n_features + len(genres))
    vals = (rng.random(len(rows)) * 2.8 + 0.2).astype(np.float32)
    return sps.csr_matrix((vals, (rows, cols)), shape=(n_items, n_features + len(genres)), dtype=np.float32)


def now():
    return time.perf_counter()


def synchronise():
    _native.check(_native.load().mi355rec_device_synchronize())


def parent_way(URM, ICM):
    """The parent commit's calls only."""
    t0 = now()
    stacked = sps.hstack([ICM * WEIGHT, URM.T], format="csr")
    data_matrix = stacked.T
    t1 = now()
    builder = Compute_Similarity(data_matrix, feature_weighting="none", weighting_documents="columns", **FIT)
    synchronise()
    t2 = now()
    W = check_matrix(builder.compute_similarity(), format="csr")
    synchronise()
    t3 = now()
    kernel = builder.compute_similarity_object.stats()["kernel_ms"] / 1e3
    builder.compute_similarity_object.close()
    return W, {"host_prepare_s": t1 - t0, "device_stack_s": 0.0, "constructor_s": t2 - t1, "kernel_s": kernel,
               "assemble_and_download_s": t3 - t2 - kernel, "fit_s": t3 - t0}


class Probes:
    """Host clocks around the three calls a class fit is made of (the class itself carries no timing code)."""

    def __init__(self):
        self.t = {}
        self._real = (knn_cbf.Compute_Similarity, knn_cbf.Compute_Similarity_MI355X.from_resident, knn_cbf.N.ResidentStack,
                      knn_cbf._KNNCBFLogic._finish_build)
        probes = self

        def timed(name, fn):
            def call(*args, **kwargs):
                t0 = now()
                out = fn(*args, **kwargs)
                synchronise()
                probes.t[name] = probes.t.get(name, 0.0) + now() - t0
                return out
            return call

        class TimedDispatcher(self._real[0]):              # (a class, not a function: the fit also asks it `check_request`)
            __init__ = timed("constructor_s", self._real[0].__init__)

        knn_cbf.Compute_Similarity = TimedDispatcher
        knn_cbf.Compute_Similarity_MI355X.from_resident = timed("constructor_s", self._real[1])
        knn_cbf.N.ResidentStack = timed("device_stack_s", self._real[2])
        knn_cbf._KNNCBFLogic._finish_build = timed("finish_s", self._real[3])

    def restore(self):
        (knn_cbf.Compute_Similarity, knn_cbf.Compute_Similarity_MI355X.from_resident, knn_cbf.N.ResidentStack,
         knn_cbf._KNNCBFLogic._finish_build) = self._real


def class_way(rec, probes, resident_blocks):
    probes.t.clear()
    t0 = now()
    rec.fit(ICM_weight=WEIGHT, resident_blocks=resident_blocks, **FIT)
    synchronise()
    total = now() - t0
    kernel = rec.similarity_stats["kernel_ms"] / 1e3
    t = probes.t
    stack, ctor, finish = t.get("device_stack_s", 0.0), t["constructor_s"], t["finish_s"]
    return rec.W_sparse, {"host_prepare_s": total - stack - ctor - finish, "device_stack_s": stack, "constructor_s": ctor,
                          "kernel_s": kernel, "assemble_and_download_s": finish - kernel, "fit_s": total}


def summary(rows):
    return {key: {"median": statistics.median(r[key] for r in rows), "best": min(r[key] for r in rows)} for key in rows[0]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "knn_hybrid_time.json"))
    ap.add_argument("--scale", type=float, default=1.0, help="shrink the ML-20M shape (rehearsals)")
    ap.add_argument("--repeats", type=int, default=5)
    args = ap.parse_args()
    URM = named_urm("ml20m", "real", scale=args.scale)
    ICM = synthetic_icm(URM.shape[1])
    print("URM %s nnz %d, ICM %s nnz %d, genre features held by %s items" % (
        URM.shape, URM.nnz, ICM.shape, ICM.nnz, np.diff(ICM.tocsc().indptr)[-4:].tolist()), flush=True)
    record = {"device": _native.device_name(), "shape": "ml20m" if args.scale == 1.0 else "ml20m x %g" % args.scale,
              "URM": [int(URM.shape[0]), int(URM.shape[1]), int(URM.nnz)], "ICM": [int(ICM.shape[0]), int(ICM.shape[1]), int(ICM.nnz)],
              "fit": dict(FIT, ICM_weight=WEIGHT),
              "timing": "seconds, host clock around calls that end in a device synchronise; kernel_s is the library's dispatch timing; "
                        "median and best of %d alternating rounds after one warm-up round" % args.repeats}

    def fresh():
        t0 = now()
        rec = ItemKNN_CFCBF_Hybrid_Recommender(URM, ICM, verbose=False)
        return rec, now() - t0

    t0 = now()
    blocks = (ResidentURM(ICM.T), ResidentURM(URM))
    synchronise()
    record["upload_blocks_once_s"] = now() - t0
    probes = Probes()
    rows = {"parent": [], "host": [], "resident": [], "resident_fresh": []}
    constructors = []
    resident_rec, _ = fresh()
    W = {}
    for round_ in range(args.repeats + 1):
        host_rec, t_ctor = fresh()               # (a host-stacked fit replaces ICM_train: one recommender per fit, as in a search)
        constructors.append(t_ctor)
        got = {}
        W["parent"], got["parent"] = parent_way(URM, ICM)
        W["host"], got["host"] = class_way(host_rec, probes, None)
        W["resident"], got["resident"] = class_way(resident_rec, probes, blocks)
        W["resident_fresh"], got["resident_fresh"] = class_way(fresh()[0], probes, blocks)
        print("round %d: %s" % (round_, {k: round(v["fit_s"], 4) for k, v in got.items()}), flush=True)
        if round_:                               # round 0 warms up: code objects, the block cache, the first full verification
            for k in rows:
                rows[k].append(got[k])
    probes.restore()
    record["recommender_constructor_s"] = {"median": statistics.median(constructors), "best": min(constructors)}
    record["ways"] = {k: summary(v) for k, v in rows.items()}
    scale = abs(W["parent"]).max()
    record["w_sparse"] = {"nnz": int(W["parent"].nnz), "max_value": float(scale),
                          "host_vs_parent_max_abs_diff": float(abs(W["host"] - W["parent"]).max()),
                          "resident_vs_parent_max_abs_diff": float(abs(W["resident"] - W["parent"]).max()),
                          "resident_fresh_vs_parent_max_abs_diff": float(abs(W["resident_fresh"] - W["parent"]).max()),
                          "resident_nnz": int(W["resident"].nnz)}
    stacked = resident_rec.stacked_matrix()
    record["stacked_matrix_equals_the_host_stack"] = bool(abs(stacked - sps.hstack([ICM * WEIGHT, URM.T], format="csr")).max() == 0)
    for b in blocks:
        b.close()
    print(json.dumps(record["ways"], indent=1), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(record, f, indent=1)
    print("written", args.out)


if __name__ == "__main__":
    main()
