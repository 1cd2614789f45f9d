"""What AsySVD's user-factor estimate costs before a validation, on the host and on the device, and the proof that
host mode did not get slower.  The ML-20M-shaped synthetic URM (ratings 1 .. 5), k = 128 (or the ASY_SVD handle's maximum, if that is
lower), a training handle as the constructor leaves it -- an AsySVD epoch at this shape is 20 M strictly ordered steps and is no part
of what is measured; the estimate reads Y whatever it holds.  All legs run in ONE run, each as the median of REPEATS = 7 calls after
one warm-up call, every timed call ending in a device synchronise:
  kernel          MatrixFactorization_MI355X_Epoch.estimate_user_factors(): the kernel's own time (the start/stop events its
                  dispatch carries), its algorithmic bytes per second next to the 8.6 TB/s a 38 MB table gathers at from the Infinity
                  Cache (Y is 27 MB), and the call's wall time with the divisor's upload and the 142 MB download;
  prepare_device  _AsySVDLogic._prepare_model_for_validation with user_factor_estimate = "device";
  prepare_host    the same with "host" (SciPy's URM_train.dot(Y), single-threaded, and the row division);
  prepare_parent  the statements of the parent commit's _prepare_model_for_validation, kept below as a function of this script, on
                  the same objects.
The three prepare legs take turns inside every repeat, in a rotating order, so that a drift of the host is shared by all of them.
`conditions` says whether prepare_host is not above prepare_parent's slowest repeat and whether prepare_device is below prepare_host;
`same_bytes` whether the device estimate is the host estimate bit for bit at this shape.

    python scripts/asysvd_estimate_time.py --out profiles/asysvd_estimate_time.json
"""
import argparse
import json
import os
import statistics
import sys
import time

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
K, REPEATS = 128, 7
ASY_KMAX = 256                              # csrc/mf_plan.h
INFINITY_CACHE_GATHER_BYTES_PER_S = 8.6e12


def parent_prepare(rec):
    """_AsySVDLogic._prepare_model_for_validation as the parent commit has it."""
    rec.ITEM_factors_Y, rec.ITEM_factors = rec.epoch_kernel.get_factors()
    rec.USER_factors = rec._estimate_user_factors(rec.ITEM_factors_Y)
    rec._forget_device_scorer()
    if rec.use_bias:
        rec.USER_bias = rec.epoch_kernel.get_USER_bias()
        rec.ITEM_bias = rec.epoch_kernel.get_ITEM_bias()
        rec.GLOBAL_bias = rec.epoch_kernel.get_GLOBAL_bias()


def measure(scale):
    from recsys2019_deeplearning_evaluation_amd import MatrixFactorization_AsySVD_MI355X, MatrixFactorization_MI355X_Epoch, _native
    from recsys2019_deeplearning_evaluation_amd.synthetic import named_urm
    sync = _native.load().mi355rec_device_synchronize
    k = min(K, ASY_KMAX)
    train = named_urm("ml20m", "real", scale=scale)
    rec = MatrixFactorization_AsySVD_MI355X(train, verbose=False)
    rec.use_bias = True
    rec.epoch_kernel = MatrixFactorization_MI355X_Epoch(rec.URM_train, n_factors=k, algorithm_name="ASY_SVD", batch_size=1, use_bias=True,
                                                        learning_rate=1e-3, sgd_mode="sgd", random_seed=5)
    handle = rec.epoch_kernel
    out = {"device": _native.device_name(), "n_users": train.shape[0], "n_items": train.shape[1], "nnz": int(train.nnz), "k": k,
           "repeats": REPEATS, "y_bytes": train.shape[1] * k * 8, "legs": {}}

    kernel, wall = [], []
    handle.estimate_user_factors()          # warm-up (and the rows' order, which the first call makes)
    for _ in range(REPEATS):
        t0 = time.perf_counter()
        handle.estimate_user_factors()
        sync()
        wall.append(time.perf_counter() - t0)
        st = handle.stats()
        kernel.append(st["kernel_ms"] * 1e-3)
    rate = st["algorithmic_bytes"] / statistics.median(kernel)
    out["legs"]["kernel"] = {"algorithmic_bytes": st["algorithmic_bytes"], "launches": st["n_launches"], "kernel_s_runs": kernel,
                             "kernel_s": statistics.median(kernel), "bytes_per_s": rate,
                             "share_of_infinity_cache_gather_rate": rate / INFINITY_CACHE_GATHER_BYTES_PER_S,
                             "wall_s_runs": wall, "wall_s": statistics.median(wall)}
    print("kernel", json.dumps({n: v for n, v in out["legs"]["kernel"].items() if not n.endswith("_runs")}), file=sys.stderr, flush=True)

    # the three legs take turns, in an order that rotates from repeat to repeat: whatever drifts on the host (the SciPy product is
    # one thread's work on a machine that is not empty) drifts under all of them alike
    legs = [("prepare_device", "device", rec._prepare_model_for_validation), ("prepare_host", "host", rec._prepare_model_for_validation),
            ("prepare_parent", "host", lambda: parent_prepare(rec))]
    estimates, runs = {}, {leg: [] for leg, _, _ in legs}
    for repeat in range(-1, REPEATS):       # (-1: the warm-up round)
        for leg, mode, call in legs[repeat % 3:] + legs[:repeat % 3]:
            rec.user_factor_estimate = mode
            sync()
            t0 = time.perf_counter()
            call()
            sync()
            if repeat >= 0:
                runs[leg].append(time.perf_counter() - t0)
            estimates[leg] = rec.USER_factors
    for leg, _, _ in legs:
        out["legs"][leg] = {"seconds_runs": runs[leg], "seconds": statistics.median(runs[leg]), "slowest_s": max(runs[leg])}
        print(leg, json.dumps({"seconds": statistics.median(runs[leg]), "slowest_s": max(runs[leg])}), file=sys.stderr, flush=True)
    out["same_bytes"] = bool(estimates["prepare_device"].tobytes() == estimates["prepare_host"].tobytes() == estimates["prepare_parent"].tobytes())
    legs = out["legs"]
    out["conditions"] = {
        "host_s": legs["prepare_host"]["seconds"], "parent_slowest_repeat_s": legs["prepare_parent"]["slowest_s"],
        "host_not_above_parent_slowest_repeat": legs["prepare_host"]["seconds"] <= legs["prepare_parent"]["slowest_s"],
        "device_s": legs["prepare_device"]["seconds"], "device_below_host": legs["prepare_device"]["seconds"] < legs["prepare_host"]["seconds"],
        "host_over_device": legs["prepare_host"]["seconds"] / legs["prepare_device"]["seconds"]}
    handle.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(os.path.dirname(HERE), "profiles", "asysvd_estimate_time.json"))
    ap.add_argument("--scale", type=float, default=1.0, help="shrink the ML-20M shape (a quick look; the committed figures are at 1.0)")
    a = ap.parse_args()
    result = {"timing": "seconds per call; medians over %d calls after one warm-up call, every timed call ends in a device synchronise" % REPEATS}
    result.update(measure(a.scale))
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(result, f, indent=1, sort_keys=True)
        f.write("\n")
    legs = result["legs"]
    print("estimate kernel: %.3f ms, %.2f TB/s algorithmic (%.0f%% of the Infinity Cache gather rate); the call %.1f ms wall" % (
        legs["kernel"]["kernel_s"] * 1e3, legs["kernel"]["bytes_per_s"] * 1e-12, 100 * legs["kernel"]["share_of_infinity_cache_gather_rate"],
        legs["kernel"]["wall_s"] * 1e3), flush=True)
    print("_prepare_model_for_validation: device %.3f s, host %.3f s, parent %.3f s (slowest repeat %.3f s); same bytes: %s" % (
        legs["prepare_device"]["seconds"], legs["prepare_host"]["seconds"], legs["prepare_parent"]["seconds"], legs["prepare_parent"]["slowest_s"],
        result["same_bytes"]), flush=True)
    print("conditions:", json.dumps(result["conditions"]), flush=True)
    print("written", a.out)


if __name__ == "__main__":
    main()
