"""Helpers of the non-personalized recommenders' tests (NumPy / SciPy only, nothing from the native library): the fixture of
tests/golden/make_non_personalized_fixture.py, a NumPy restatement of the shared-vector scorer's algorithm (csrc/itemscore.hip: one
global order, mask compaction, windowed bitmap of the seen positions), a float64 restatement of GlobalEffects.fit with the
reference's element-wise roundings, and the profiles the exact tests rank."""
import json

import numpy as np
import scipy.sparse as sps

from _util import GOLDEN

FIXTURE = np.load(GOLDEN + "/non_personalized.npz")
META = json.loads(str(FIXTURE["cases"]))
CASES = META["cases"]
LAMBDAS = [tuple(p) for p in META["lambdas"]]
CUTOFFS = META["cutoffs"]


def case_urm(name):
    """The URM of a fixture case AS PASSED to the reference's constructors (the `holes` case stores one explicit zero)."""
    shape = tuple(int(x) for x in FIXTURE[name + "_shape"])
    return sps.csr_matrix((FIXTURE[name + "_data"], FIXTURE[name + "_indices"], FIXTURE[name + "_indptr"]), shape=shape)


# ------------------------------------------------------------------------------------------ the scorer's algorithm in NumPy
def model_order(vector):
    """Item ids of the finite entries by (value descending, id ascending)."""
    v = np.asarray(vector, dtype=np.float32)
    ids = np.flatnonzero(np.isfinite(v))
    return ids[np.argsort(-v[ids], kind="stable")]


def windowed_lists(vector, seen_rows, cutoff, remove_seen=True, allowed=None, W=2048):
    """The lists of users whose seen items are `seen_rows` (arrays of item ids, unsorted, repeats allowed), the way the ranking
    kernel finds them: windows of W positions of the (mask-compacted) order, the seen positions marked in a bitmap, the clear ones
    emitted until `cutoff` items are out; nothing past position cutoff + len(seen row) is looked at."""
    n_items = len(vector)
    order = model_order(vector)
    if allowed is not None:
        order = order[np.asarray(allowed)[order] != 0]
    rank_of = np.full(n_items, -1, np.int64)
    rank_of[order] = np.arange(len(order))
    out = np.full((len(seen_rows), cutoff), -1, np.int32)
    for r, seen in enumerate(seen_rows):
        seen = np.asarray(seen, dtype=np.int64) if remove_seen else np.empty(0, np.int64)
        bound = min(len(order), cutoff + len(seen))
        emitted, base = 0, 0
        while base < bound and emitted < cutoff:
            wlen = min(W, bound - base)
            bitmap = np.zeros(wlen, bool)
            rel = rank_of[seen] - base
            bitmap[rel[(rel >= 0) & (rel < wlen)]] = True
            clear = np.flatnonzero(~bitmap)[:cutoff - emitted]
            out[r, emitted:emitted + len(clear)] = order[base + clear]
            emitted += len(clear)
            base += W
    return out


def broadcast_rows(vector, n_rows):
    """The score block of a shared vector, non-finite entries as -inf (they are never listed)."""
    v = np.asarray(vector, dtype=np.float32)
    return np.repeat(np.where(np.isfinite(v), v, -np.inf).astype(np.float32)[None, :], n_rows, axis=0)


# ------------------------------------------------------------------------------------------------------- vectors and profiles
def vectors(n_items, rng):
    """name -> float32 vector: counts with -inf entries, constant, two-level, small-integer counts, distinct, and counts with -inf and NaN
    entries."""
    counts = rng.integers(0, 12, n_items).astype(np.float32)
    holes = counts.copy()
    holes[rng.random(n_items) < 0.2] = -np.inf
    holes[rng.random(n_items) < 0.1] = np.nan
    return {"minus_inf": np.where(rng.random(n_items) < 0.3, -np.inf, counts).astype(np.float32),
            "constant": np.full(n_items, 3.0, np.float32),
            "two_levels": rng.integers(1, 3, n_items).astype(np.float32),
            "counts": counts,
            "distinct": (rng.permutation(n_items).astype(np.float32) - np.float32(n_items // 2)) / np.float32(4),
            "non_finite": holes}


def profiles(order, cutoffs, rng):
    """Seen rows relative to an order (best item first): empty; everything; exactly the c best items; all but c - 1 items (the
    c - 1 worst stay); every second item of the order; an unsorted row with repeats."""
    n = len(order)
    rows = [np.empty(0, np.int64), np.array(order)]
    for c in cutoffs:
        rows.append(np.array(order[:c]))
        rows.append(np.array(order[:n - (c - 1)]))
    rows.append(np.array(order[::2]))
    some = rng.choice(n, min(n, 40), replace=False)
    rows.append(rng.permutation(np.concatenate([some, some[:len(some) // 2], some[:3]])))
    return rows


def seen_matrix(rows, n_items):
    """CSR whose rows hold exactly the given index sequences -- unsorted, repeats kept."""
    indptr = np.concatenate([[0], np.cumsum([len(r) for r in rows])]).astype(np.int32)
    indices = np.concatenate(rows).astype(np.int32) if indptr[-1] else np.empty(0, np.int32)
    return sps.csr_matrix((np.ones(len(indices), np.float32), indices, indptr), shape=(len(rows), n_items))


def masks(n_items, order, rng):
    """name -> uint8 mask or None: none, half, all-zero, the best 100 items excluded."""
    half = (rng.random(n_items) < 0.5).astype(np.uint8)
    no_head = np.ones(n_items, np.uint8)
    no_head[order[:100]] = 0
    return {"none": None, "half": half, "all_zero": np.zeros(n_items, np.uint8), "no_head": no_head}


# ------------------------------------------------------------------------------------- GlobalEffects.fit, restated in float64
def global_effects_f64(URM, lambda_user, lambda_item):
    """mu, item_bias, user_bias with the reference's element-wise roundings (float32 x - mu; float32 of the float64 difference to the
    item bias) and float64 sums (math.fsum would give the same: the tests' data make every sum exact or bound the difference)."""
    X = sps.csr_matrix(URM, dtype=np.float32, copy=True)
    X.eliminate_zeros()
    n_users, n_items = X.shape
    x = X.data.astype(np.float32)
    mu = np.float32(x.astype(np.float64).sum() / len(x))
    d = (x - mu).astype(np.float32)
    cols = X.indices
    rows = np.repeat(np.arange(n_users), np.diff(X.indptr))
    col_nnz = np.bincount(cols, minlength=n_items)
    item_bias = np.bincount(cols, weights=d.astype(np.float64), minlength=n_items) / (col_nnz + float(lambda_item))
    left = (d.astype(np.float64) - item_bias[cols]).astype(np.float32)
    row_nnz = np.diff(X.indptr)
    user_bias = np.bincount(rows, weights=left.astype(np.float64), minlength=n_users) / (row_nnz + float(lambda_user))
    return mu, item_bias, user_bias


def float32_summation_bounds(URM, lambda_user, lambda_item):
    """Worst-case distance between float64-summed biases and the reference's float32-summed ones (its sums run in float32: NumPy's
    pairwise sum of the values, depth <= 13 + ceil(log2 nnz) roundings; scipy's column and row sums, one rounding per stored cell and
    two for the quotient), each rounding at most 2^-24 relative to the magnitudes summed:
      |d mu|        <= (13 + ceil(log2 nnz)) 2^-24 mean|x|
      |d item_bias| <= (L_max + 2) 2^-24 max|x - mu| + |d mu|
      |d user_bias| <= that + (R_max + 2) 2^-24 max|d'|
    L_max, R_max: the longest column and row.  Returns (mu_bound, item_bound, user_bound)."""
    X = sps.csr_matrix(URM, dtype=np.float32, copy=True)
    X.eliminate_zeros()
    mu, item_bias, _ = global_effects_f64(X, lambda_user, lambda_item)
    x = X.data.astype(np.float64)
    u = 2.0 ** -24
    mu_bound = (13 + int(np.ceil(np.log2(len(x))))) * u * np.abs(x).mean()
    L_max = int(np.bincount(X.indices, minlength=X.shape[1]).max())
    R_max = int(np.diff(X.indptr).max())
    d = np.abs(x - float(mu))
    item_bound = (L_max + 2) * u * d.max() + mu_bound
    left = np.abs((x - float(mu)) - item_bias[X.indices])
    user_bound = item_bound + (R_max + 2) * u * left.max()
    return mu_bound, item_bound, user_bound
