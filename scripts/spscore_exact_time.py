"""Cost of the sparse scorer's exact mode next to the default atomic mode, and the proof that the default did
not get slower.  The ML-20M-shaped synthetic URM of bench.py (binary, leave-one-out split as bench.py's holdout_split), ItemKNN cosine
at topK=100 (shrink 0), cutoff [10].  Both modes in ONE run, every figure the median of 7 repeats after one warm-up, every repeat
ending in a device synchronise (all repeats are kept in the file):
  recommend_block_s    recommend() of the recommender for blocks of 1 000 users: the first 20 000 users, seconds per block;
  holdout_s            one EvaluatorHoldout_MI355X evaluation, all test users, fused path;
  negative_s           one EvaluatorNegativeItemSample_MI355X evaluation (1 test item + 99 sampled negatives per user), fused path;
  kernel_ms_per_block  the scoring dispatch alone (get_stats' kernel_ms) over the same 20 blocks: for the exact mode that is
                       spexact_rows_kernel WITHOUT the ranking, for the atomic mode score + rank are one kernel -- not comparable,
                       both are recorded for what they are;
  lanes                exact mode, a host model of the kernel's two phases over those 20 000 users: the share of lanes that hold a
                       cell of B in the load + multiply steps (64 cells of the laid-out pieces per step) and in the ordered LDS
                       add steps (the lanes of one profile cell's piece inside one load step; bounded from both sides, see
                       lane_shares).  Counted from the matrices, not measured.
  lists_equal          whether the two modes returned the same lists for those users (they need not: near-ties).
`--parent-root DIR` names a checkout of the PARENT commit with its library built: its atomic legs are then measured in a child
process of their own in the same run, and `default_not_slower` says, leg by leg, whether this tree's atomic median lies inside the
spread (min .. max) of the parent's seven repeats.  Every measurement runs in a child process under `timeout`; after a child that
failed nothing more is started on the device.

    python scripts/spscore_exact_time.py --parent-root ../parent --out profiles/spscore_exact_time.json
"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

HERE = os.path.dirname(os.path.abspath(__file__))
TOPK, CUTOFFS, N_NEGATIVES, BLOCK, N_BLOCKS, REPEATS = 100, [10], 99, 1000, 20, 7
LEGS = ("recommend_block_s", "holdout_s", "negative_s")


def runs_of(fn, sync, repeats=REPEATS):
    fn()
    times = []
    for _ in range(repeats):
        t0 = time.perf_counter()
        fn()
        sync()
        times.append(time.perf_counter() - t0)
    return times


def sample_negatives(rng, train, test, per_user, draws=128):
    """Up to `per_user` distinct items per user outside train | test: the first admissible ones of `draws` uniform draws."""
    import numpy as np
    import scipy.sparse as sps
    n_users, n_items = train.shape
    users = np.repeat(np.arange(n_users, dtype=np.int64), draws)
    keys = users * n_items + rng.integers(0, n_items, n_users * draws)
    taken = sps.csr_matrix(train) + sps.csr_matrix(test)
    taken_keys = np.repeat(np.arange(n_users, dtype=np.int64), np.diff(taken.indptr)) * n_items + taken.indices
    keys = keys[~np.isin(keys, taken_keys)]
    _, first = np.unique(keys, return_index=True)
    keys = keys[np.sort(first)]
    users = keys // n_items
    rank = np.arange(len(keys)) - np.searchsorted(users, users, side="left")
    keep = rank < per_user
    return sps.csr_matrix((np.ones(int(keep.sum()), np.float32), (users[keep], keys[keep] % n_items)), shape=train.shape)


def lane_model(A, users, B, tile=32256, owners=16):
    """The exact kernel's lane use over `users`, from the matrices: per (user, slice) the profile is taken 64 cells at a time, their
    pieces of B are laid end to end and loaded 64 cells per step; then one LDS add step per profile cell that has a cell there."""
    import numpy as np
    import scipy.sparse as sps
    n_out = B.shape[1]
    tile = min(n_out, tile)
    slice_w = -(-tile // owners)
    B = sps.csr_matrix(B)
    rows = np.repeat(np.arange(B.shape[0]), np.diff(B.indptr))
    slices = (B.indices // tile) * owners + (B.indices % tile) // slice_w
    S = sps.csr_matrix((np.ones(B.nnz, np.float64), (rows, slices)), shape=(B.shape[0], int(slices.max()) + 1 if B.nnz else 1))
    S.sum_duplicates()                              # S[m, k]: cells of row m inside slice k
    lens = np.diff(A.indptr)[users]
    starts = A.indptr[users]
    cell_pos = np.concatenate([np.arange(s, s + n) for s, n in zip(starts, lens)] + [np.empty(0, np.int64)]).astype(np.int64)
    batch_of_user = np.concatenate([[0], np.cumsum(-(-lens // 64))])
    batch = np.concatenate([batch_of_user[r] + np.arange(n) // 64 for r, n in enumerate(lens)] + [np.empty(0, np.int64)]).astype(np.int64)
    P = sps.csr_matrix((np.ones(len(cell_pos)), (batch, A.indices[cell_pos])), shape=(int(batch_of_user[-1]), B.shape[0]))
    T = (P @ S).toarray()                           # cells per (batch of 64 profile cells, slice)
    cells = float(T.sum())
    load_steps = float(np.ceil(T / 64.0).sum())
    pieces = float((P @ (S > 0).astype(np.float64)).sum())
    return lane_shares(cells, load_steps, pieces)


def lane_shares(cells, load_steps, pieces):
    """An add step takes the lanes of ONE piece inside ONE load step: a piece longer than 64 cells, or one that crosses the end of a
    load step, takes several.  Every end of a load step cuts at most one piece, so the add steps lie between max(pieces, load_steps)
    and pieces + load_steps: the share of busy lanes is given for both ends."""
    most, fewest = pieces + load_steps, max(pieces, load_steps)
    return {"cells_of_b": cells, "load_steps": load_steps, "pieces": pieces, "cells_per_piece": cells / pieces if pieces else 0.0,
            "load_lane_share": cells / (64.0 * load_steps) if load_steps else 0.0,
            "add_steps_at_most": most, "add_steps_at_least": fewest,
            "add_lane_share_at_least": cells / (64.0 * most) if most else 0.0,
            "add_lane_share_at_most": cells / (64.0 * fewest) if fewest else 0.0,
            "how": "counted on the host from A and B (a model of the kernel's steps), not measured on the device"}


def measure(modes):
    import numpy as np
    import scipy.sparse as sps
    from bench import holdout_split, load_urm
    from recsys2019_deeplearning_evaluation_amd import (EvaluatorHoldout_MI355X, EvaluatorNegativeItemSample_MI355X, ItemKNNCFRecommender,
                                                        _native)
    sync = _native.load().mi355rec_device_synchronize
    urm = load_urm("ml20m")
    urm.data[:] = 1.0
    train, test = holdout_split(urm)
    negative = sample_negatives(np.random.default_rng(11), train, test, N_NEGATIVES)
    rec = ItemKNNCFRecommender(train)
    rec.fit(topK=TOPK, shrink=0, similarity="cosine")
    holdout = EvaluatorHoldout_MI355X(test, CUTOFFS, verbose=False)
    sampled = EvaluatorNegativeItemSample_MI355X(test, negative, CUTOFFS, verbose=False)
    users = np.arange(BLOCK * N_BLOCKS, dtype=np.int32)
    blocks = [users[a:a + BLOCK] for a in range(0, len(users), BLOCK)]
    out = {"device": _native.device_name(), "n_users": train.shape[0], "n_items": train.shape[1], "train_nnz": int(train.nnz),
           "w_nnz": int(rec.W_sparse.nnz), "topK": TOPK, "cutoffs": CUTOFFS, "negatives_per_user": N_NEGATIVES, "block": BLOCK,
           "blocks": N_BLOCKS, "repeats": REPEATS, "modes": {}}
    lists = {}
    for mode in modes:
        if mode != "atomic":                        # (the parent commit has no such attribute: its only mode is left alone)
            rec.sparse_scoring = mode
        row = {}
        runs = runs_of(lambda: [rec.recommend(b, cutoff=CUTOFFS[0]) for b in blocks], sync)
        row["recommend_block_s_runs"] = [t / N_BLOCKS for t in runs]
        row["holdout_s_runs"] = runs_of(lambda: holdout.evaluateRecommender(rec), sync)
        row["negative_s_runs"] = runs_of(lambda: sampled.evaluateRecommender(rec), sync)
        for leg in LEGS:
            row[leg] = statistics.median(row[leg + "_runs"])
        row["MAP@10_holdout"] = holdout.evaluateRecommender(rec)[0][CUTOFFS[0]]["MAP"]
        row["MAP@10_negative"] = sampled.evaluateRecommender(rec)[0][CUTOFFS[0]]["MAP"]
        scorer = rec.device_scorer()
        kernel = []
        for _ in range(REPEATS):
            ms = 0.0
            for b in blocks:
                scorer.recommend(b, CUTOFFS[0], True, None)
                ms += scorer.stats()["kernel_ms"]
            kernel.append(ms / N_BLOCKS)
        row["kernel_ms_per_block_runs"] = kernel
        row["kernel_ms_per_block"] = statistics.median(kernel)
        row["kernel_is"] = "spexact_rows_kernel, scoring only" if mode == "exact" else "spscore_kernel, scoring + ranking"
        lists[mode] = np.concatenate([scorer.recommend(b, CUTOFFS[0], True, None)[0] for b in blocks])
        out["modes"][mode] = row
        print(mode, json.dumps({k: v for k, v in row.items() if not k.endswith("_runs")}), file=sys.stderr, flush=True)
    if "exact" in modes:
        out["lanes"] = lane_model(sps.csr_matrix(train), users, sps.csr_matrix(rec.W_sparse).sorted_indices())
        twice = np.concatenate([rec.device_scorer().recommend(b, CUTOFFS[0], True, None)[0] for b in blocks])
        out["exact_lists_repeat"] = bool(np.array_equal(twice, lists["exact"]))
    if len(lists) == 2:
        same = (lists["atomic"] == lists["exact"]).all(axis=1)
        out["lists_equal"] = {"users": int(len(same)), "users_with_the_same_list": int(same.sum())}
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
    ap.add_argument("--out", default=os.path.join(os.path.dirname(HERE), "profiles", "spscore_exact_time.json"))
    ap.add_argument("--parent-root", help="a checkout of the parent commit with libmi355rec.so built: its atomic legs are measured too")
    ap.add_argument("--seconds", type=int, default=500, help="time limit of each measuring process")
    ap.add_argument("--measure", help="(child) MODES, comma separated; the package is taken from PYTHONPATH")
    a = ap.parse_args()
    if a.measure:
        print(json.dumps(measure(a.measure.split(","))))
        return
    root = os.path.dirname(HERE)
    result = {"timing": "seconds unless a key says ms; median of %d repeats after one warm-up, each repeat ends in a device synchronise" % REPEATS}
    this, rc = child(root, ["atomic", "exact"], a.seconds)
    if this is None:
        print("this tree's measurement failed (%d): nothing more is started" % rc, flush=True)
        sys.exit(1)
    result["this_tree"] = this
    at, ex = this["modes"]["atomic"], this["modes"]["exact"]
    result["exact_over_atomic"] = {leg: ex[leg] / at[leg] for leg in LEGS}
    if a.parent_root:
        parent, rc = child(os.path.abspath(a.parent_root), ["atomic"], a.seconds)
        if parent is None:
            print("the parent's measurement failed (%d)" % rc, flush=True)
            result["parent"] = {"failed": rc}
        else:
            result["parent"] = parent
            pa = parent["modes"]["atomic"]
            result["default_not_slower"] = {leg: {"this_median": at[leg], "parent_median": pa[leg], "parent_min": min(pa[leg + "_runs"]),
                                                  "parent_max": max(pa[leg + "_runs"]),
                                                  "inside_parent_spread": min(pa[leg + "_runs"]) <= at[leg] <= max(pa[leg + "_runs"]),
                                                  "not_above_parent_max": at[leg] <= max(pa[leg + "_runs"])} for leg in LEGS}
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(result, f, indent=1, sort_keys=True)
        f.write("\n")
    for leg in LEGS:
        print("%-18s atomic %.4f s, exact %.4f s (x%.2f)" % (leg, at[leg], ex[leg], ex[leg] / at[leg]), flush=True)
    print("exact kernel alone %.3f ms per block of %d users; lanes: load %.3f, add at least %.3f" % (
        ex["kernel_ms_per_block"], BLOCK, this["lanes"]["load_lane_share"], this["lanes"]["add_lane_share_at_least"]), flush=True)
    if "default_not_slower" in result:
        print("default not slower:", json.dumps(result["default_not_slower"]), flush=True)
    print("written", a.out)


if __name__ == "__main__":
    main()
