"""Device-ranking test helper (NumPy / SciPy only, nothing from the native library): the exact oracle of the ranking contract
(DESIGN.md section 3.5), a host restatement of the dispatch inside `score_rank_kernel` / `spscore_kernel` that names the route a
filtered score row takes, and the named cases of tests/test_ranking_oracle.py (CPU) and tests/test_ranking_exact_gpu.py (device).

Contract: the list of a row is the `cutoff` best FINITE scores, value descending, ties towards the lower item id, -1 padded --
whichever route produced it.  Given the filtered float32 row the correct list is fully determined, so the tests compare with no
tolerance.  Out of scope: -0.0 (the GEMM accumulates from +0.f and the sparse scorer's atomics add onto +0.f, so it cannot reach a
score row; the in-LDS key and rocPRIM would order it differently), NaN and +inf scores.

Routes (`predict_route`), in the order the kernels decide them:
  wide                 the row does not fit LDS or the cut-off is above MAX_TOPK: rows in HBM, one segmented radix sort
  threshold_first      rank_threshold_first emitted the list (bound from the thread maxima, candidates ranked exactly)
  fallback_ineligible  ... it did not start: fewer finite scores than the cut-off, or THRESHOLD_FACTOR * cutoff > THREADS
  fallback_overflow    ... it collected more than AUX_WORDS / 2 candidates and gave up
  take_all             block_topk_emit: no more finite scores than the cut-off, nothing to select
  select_superset      block_select left early with a superset of at most `cap` candidates
  select_exact         block_select resolved all 32 key bits and the cells equal to the K-th key all belong to the list
  select_partial_ties  ... only some of them do: a second radix select, on the item id, picks the lowest
  rank_counting        block_rank_emit_lds ranked <= COUNTING_MAX candidates by counting
  rank_bitonic         ... more than that with the bitonic sort

Row cases are written in score space: a recipe returns the filtered float32 row itself (-inf where a filter applies).  Both scorers
reproduce any such rows bit for bit -- `realise_dense`: U = identity, V = the rows as columns, every score is one product by 1.0
plus exact zeros; `realise_sparse`: A = identity, B = the rows, one atomic add onto +0.f per cell -- with -inf cells shared by all
rows of the case going through the item mask and the others through the seen-items CSR.  Model cases (`int_dense_model`,
`int_sparse_model`) use small integers, so every partial sum is exact in float32 in any order and the host predicts the scores.
"""
import os
import re
import zlib
from collections import namedtuple

import numpy as np
import scipy.sparse as sps

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "recsys2019_deeplearning_evaluation_amd", "csrc")

ROUTES = ("wide", "threshold_first", "fallback_ineligible", "fallback_overflow", "take_all", "select_superset", "select_exact",
          "select_partial_ties", "rank_counting", "rank_bitonic")
# the candidate ranking is reached from both block-level entry points: each of the two must see both of its methods
ENTRY_RANKS = (("threshold_first", "rank_counting"), ("threshold_first", "rank_bitonic"),
               ("block_topk_emit", "rank_counting"), ("block_topk_emit", "rank_bitonic"))

_PATTERNS = {
    # name: (file, regular expression with one group per number)
    "AUX_WORDS": ("topk.cuh", r"constexpr int AUX_WORDS = (\d+);"),
    "MAX_TOPK": ("topk.cuh", r"constexpr int MAX_TOPK = (\d+);"),
    "COUNTING_MAX": ("topk.cuh", r"if \(ncand <= (\d+)\) \{"),
    "CAP_FLOOR": ("topk.cuh", r"const uint32_t cap = \(uint32_t\)min\(AUX_WORDS / 2, max\((\d+), \d+ \* topK\)\);"),
    "CAP_PER_K": ("topk.cuh", r"const uint32_t cap = \(uint32_t\)min\(AUX_WORDS / 2, max\(\d+, (\d+) \* topK\)\);"),
    "THREADS": ("score.hip", r"auto k = score_rank_kernel<(\d+)>;"),
    "THREADS_SPARSE": ("score.hip", r"auto k = spscore_kernel<(\d+)>;"),
    "THRESHOLD_FACTOR": ("score.hip", r"nfinite >= \(uint32_t\)cutoff && (\d+) \* cutoff <= THREADS"),
    "LDS_BUDGET": ("score.hip", r"return lds <= (\d+) \* (\d+) && cutoff <= MAX_TOPK;"),
    "LDS_SLACK": ("score.hip", r"\(size_t\)AUX_WORDS \* 4 \+ (\d+);"),
}


def parse_constants(csrc=CSRC):
    """The numbers the dispatch depends on, read from the sources (exactly one match each, or an AssertionError)."""
    text, out = {}, {}
    for name, (fname, pattern) in _PATTERNS.items():
        if fname not in text:
            with open(os.path.join(csrc, fname)) as f:
                text[fname] = f.read()
        found = re.findall(pattern, text[fname])
        assert len(found) == 1, "%s: %d matches of %r in %s" % (name, len(found), pattern, fname)
        groups = found[0] if isinstance(found[0], tuple) else (found[0],)
        out[name] = int(np.prod([int(g) for g in groups]))
    assert out["THREADS"] == out["THREADS_SPARSE"], "the two ranking kernels are launched with different block sizes"
    return out


class _Constants(dict):
    """Parsed on first use, so that importing the oracle alone does not depend on the layout of the kernel sources."""

    def __missing__(self, name):
        self.update(parse_constants())
        return dict.__getitem__(self, name)


C = _Constants()


# ---------------------------------------------------------------------------------------------------------------- oracle
def exact_ranking(row, cutoff):
    """Ids of the finite cells of a float32 row by (value descending, id ascending), cut to `cutoff`, -1 padded."""
    row = np.asarray(row, dtype=np.float32)
    order = np.argsort(-row, kind="stable")                  # stable: equal values keep the ascending ids; -inf cells go last
    out = np.full(cutoff, -1, np.int32)
    k = min(cutoff, int((row > -np.inf).sum()))
    out[:k] = order[:k]
    return out


def exact_rankings(rows, cutoff):
    return np.stack([exact_ranking(r, cutoff) for r in rows]) if len(rows) else np.empty((0, cutoff), np.int32)


# ------------------------------------------------------------------------------------------------------- route predictor
def float_key(v):
    """topk.cuh float_key: order-preserving float32 -> uint32."""
    b = np.ascontiguousarray(v, dtype=np.float32).view(np.uint32)
    return np.where(b & np.uint32(0x80000000), ~b, b | np.uint32(0x80000000)).astype(np.uint32)


def fits_lds_rank(n_items, cutoff):
    lds = ((n_items + 3) & ~3) * 4 + C["AUX_WORDS"] * 4 + C["LDS_SLACK"]
    return lds <= C["LDS_BUDGET"] and cutoff <= C["MAX_TOPK"]


def route_detail(row, cutoff):
    """(set of route names, number of candidates handed to the final ranking -- None on the wide path) of one filtered row."""
    row = np.asarray(row, dtype=np.float32)
    n = len(row)
    assert 1 <= cutoff <= n
    if not fits_lds_rank(n, cutoff):
        return {"wide"}, None
    threads, cand_max = C["THREADS"], C["AUX_WORDS"] // 2
    finite = row > -np.inf
    nfinite = int(finite.sum())
    keys = float_key(row).astype(np.int64)
    fkeys = keys[finite]
    routes = set()

    def ranked(ncand):
        routes.add("rank_counting" if ncand <= C["COUNTING_MAX"] else "rank_bitonic")
        return routes, ncand

    # rank_threshold_first
    if nfinite >= cutoff and C["THRESHOLD_FACTOR"] * cutoff <= threads:
        padded = np.full(-(-n // threads) * threads, -np.inf, np.float32)
        padded[:n] = row
        tmax = padded.reshape(-1, threads).max(axis=0)                 # cell j belongs to thread j mod THREADS
        kth = np.sort(float_key(tmax).astype(np.int64))[::-1][cutoff - 1]
        T = (kth >> 16) << 16                                          # block_kth_largest_prefix16
        ncand = int((fkeys >= T).sum())
        if ncand <= cand_max:
            routes.add("threshold_first")
            return ranked(ncand)
        routes.add("fallback_overflow")
    else:
        routes.add("fallback_ineligible")
    # block_topk_emit, TOPK_FINITE
    K = min(cutoff, nfinite)
    if nfinite <= cutoff:
        routes.add("take_all")
        return ranked(nfinite)
    cap = min(cand_max, max(C["CAP_FLOOR"], C["CAP_PER_K"] * cutoff))
    kth = np.sort(fkeys)[::-1][K - 1]
    # block_select over the full key range: 8-bit windows from the top; after each window the prefix is that of the K-th key
    for remaining in (24, 16, 8, 0):
        prefix = kth >> remaining
        above = int(((fkeys >> remaining) > prefix).sum())
        in_bin = int(((fkeys >> remaining) == prefix).sum())
        if remaining > 0 and above + in_bin <= cap:
            routes.add("select_superset")
            return ranked(above + in_bin)
    need_eq, eq_total = K - above, in_bin
    routes.add("select_partial_ties" if need_eq < eq_total else "select_exact")
    return ranked(K)


def predict_route(row, cutoff):
    return route_detail(row, cutoff)[0]


def entry_ranks(routes):
    """The (entry point, ranking method) pair of a non-wide route set."""
    entry = "threshold_first" if "threshold_first" in routes else "block_topk_emit"
    return {(entry, r) for r in routes if r.startswith("rank_")}


# --------------------------------------------------------------------------------------------------------------- recipes
# recipe(n, cutoff, rng) -> float32 row of n scores, -inf where a filter applies.  Every recipe works for every 1 <= cutoff <= n.
ULP1 = np.float32(2.0 ** -23)             # spacing of float32 in [1, 2)


def _descending_with_tie(n, lo, hi, rng):
    """Distinct integer scores n, n-1, ... in a random item order, the ranks [lo, hi) all set to one value."""
    v = (n - np.arange(n)).astype(np.float32)
    v[max(lo, 0):min(hi, n)] = v[max(lo, 0)] if max(lo, 0) < n else v[-1]
    row = np.empty(n, np.float32)
    row[rng.permutation(n)] = v
    return row


def _keep_finite(row, count, rng):
    out = np.full(len(row), -np.inf, np.float32)
    keep = rng.choice(len(row), min(max(count, 0), len(row)), replace=False)
    out[keep] = row[keep]
    return out


def _int_levels(n, rng):
    return rng.integers(-10, 10, n).astype(np.float32)


RECIPES = {
    "gaussian": lambda n, c, rng: rng.normal(size=n).astype(np.float32),
    "seen_only": lambda n, c, rng: np.where(rng.random(n) < 0.05, -np.inf, rng.normal(size=n)).astype(np.float32),
    "constant": lambda n, c, rng: np.full(n, 3.0, np.float32),
    "two_levels": lambda n, c, rng: rng.integers(1, 3, n).astype(np.float32),
    "int_levels": lambda n, c, rng: _int_levels(n, rng),
    "small_tie_at_cut": lambda n, c, rng: _descending_with_tie(n, c - 3, c + 2, rng),
    "wide_tie_at_cut": lambda n, c, rng: _descending_with_tie(n, max(c - 2500, 0), max(c - 2500, 0) + 5000, rng),   # > MAX_TOPK cells
                                                                                                    # where the row has room
    # all scores inside one 16-bit key prefix (1 + j ulp, j < 2^16)
    "narrow_ties": lambda n, c, rng: (np.float32(1) + rng.integers(0, 8, n).astype(np.float32) * ULP1).astype(np.float32),
    "narrow_distinct": lambda n, c, rng: (np.float32(1) + rng.permutation(n).astype(np.float32) * ULP1).astype(np.float32),
    # exactly `cutoff` cells two ulps above the rest: the K-th key's ties end at the cut
    "narrow_tie_ends_at_cut": lambda n, c, rng: _keep_level(n, c, rng),
    # negatives, zeros and positives; fewer positives than the cut-off, so the zeros straddle it
    "zeros_straddle_cut": lambda n, c, rng: _signs(n, c, rng),
    # zeros everywhere but the last cutoff // 2 cells, which hold distinct positive scores: the cut falls inside the zeros
    "top_scores_behind_a_tie": lambda n, c, rng: _tail_scores(n, c, rng),
    "mask_fewer": lambda n, c, rng: _keep_finite(_int_levels(n, rng), c - 1, rng),
    "mask_exactly": lambda n, c, rng: _keep_finite(_int_levels(n, rng), c, rng),
    "mask_one_more": lambda n, c, rng: _keep_finite(_int_levels(n, rng), c + 1, rng),
    "nothing_finite": lambda n, c, rng: np.full(n, -np.inf, np.float32),
    # every admissible item in ONE residue class mod THREADS: a single thread holds every finite maximum
    "one_residue_class": lambda n, c, rng: _residue(n, rng),
}


def _keep_level(n, c, rng):
    row = np.ones(n, np.float32)
    row[rng.choice(n, c, replace=False)] = np.float32(1) + 2 * ULP1
    return row


def _signs(n, c, rng):
    row = np.zeros(n, np.float32)
    where = rng.permutation(n)
    npos, nneg = c // 2, n // 4
    row[where[:npos]] = rng.integers(1, 4, npos).astype(np.float32)
    row[where[npos:npos + nneg]] = -rng.integers(1, 4, nneg).astype(np.float32)
    return row


def _tail_scores(n, c, rng):
    row = np.zeros(n, np.float32)
    top = min(c // 2, n - 1)
    if top:
        row[n - top:] = rng.permutation(top).astype(np.float32) + 1
    return row


def _residue(n, rng):
    row = np.full(n, -np.inf, np.float32)
    cls = np.arange(7 % n, n, C["THREADS"])
    row[cls] = rng.integers(-3, 4, len(cls)).astype(np.float32)
    return row


ALL_RECIPES = tuple(RECIPES)

# ------------------------------------------------------------------------------------------------------------ case table
Case = namedtuple("Case", "name n_items cutoff recipes routes entry_ranks")


def _case(name, n_items, cutoff, recipes, routes, ranks=()):
    recipes = (recipes,) if isinstance(recipes, str) else tuple(recipes)
    assert set(routes) <= set(ROUTES) and set(ranks) <= set(ENTRY_RANKS) and set(recipes) <= set(RECIPES), name
    return Case(name, n_items, cutoff, recipes, frozenset(routes), frozenset(ranks))


TF_C, TF_B = ENTRY_RANKS[0], ENTRY_RANKS[1]
BT_C, BT_B = ENTRY_RANKS[2], ENTRY_RANKS[3]

# Named cases: each states the routes (and entry point x ranking method pairs) it is there to reach; test_ranking_oracle.py checks
# the statement against predict_route and that together they leave no route out.
NAMED = [
    _case("gaussian_ml20m_c20", 26744, 20, "gaussian", {"threshold_first", "rank_counting"}, {TF_C}),
    _case("int_levels_last_lds_row_c20", 32256, 20, "int_levels", {"threshold_first", "rank_bitonic"}, {TF_B}),
    _case("wide_tie_c100", 20000, 100, "wide_tie_at_cut", {"fallback_overflow", "select_partial_ties", "rank_counting"}, {BT_C}),
    _case("small_tie_c100", 20000, 100, "small_tie_at_cut", {"threshold_first", "rank_counting"}, {TF_C}),
    _case("constant_c20", 5000, 20, "constant", {"fallback_overflow", "select_partial_ties", "rank_counting"}, {BT_C}),
    _case("constant_c2000", 5000, 2000, "constant", {"fallback_ineligible", "select_partial_ties", "rank_bitonic"}, {BT_B}),
    _case("two_levels_c256", 9000, 256, "two_levels", {"fallback_overflow", "select_partial_ties"}),
    _case("narrow_ties_c20", 26744, 20, "narrow_ties", {"fallback_overflow", "select_partial_ties"}),
    _case("narrow_distinct_c20", 26744, 20, "narrow_distinct", {"fallback_overflow", "select_superset", "rank_counting"}, {BT_C}),
    _case("narrow_tie_ends_at_cut_c20", 26744, 20, "narrow_tie_ends_at_cut", {"fallback_overflow", "select_exact", "rank_counting"}, {BT_C}),
    _case("narrow_tie_ends_at_cut_c1025", 26744, 1025, "narrow_tie_ends_at_cut", {"fallback_ineligible", "select_exact", "rank_bitonic"}, {BT_B}),
    _case("zeros_straddle_c20", 26744, 20, "zeros_straddle_cut", {"fallback_overflow", "select_partial_ties"}),
    # the few scores above the tie sit at the END of the row: a selection that took every zero (no second select on the item id)
    # would have filled the AUX_WORDS / 2 candidate slots long before it reached them
    _case("top_scores_behind_the_zeros_c20", 26744, 20, "top_scores_behind_a_tie", {"fallback_overflow", "select_partial_ties", "rank_counting"}, {BT_C}),
    _case("top_scores_behind_the_zeros_c600", 32256, 600, "top_scores_behind_a_tie", {"fallback_ineligible", "select_partial_ties"}),
    _case("zeros_straddle_c600", 5000, 600, "zeros_straddle_cut", {"fallback_ineligible", "select_partial_ties"}),
    _case("gaussian_c257", 26744, 257, "gaussian", {"fallback_ineligible", "select_superset", "rank_counting"}, {BT_C}),
    _case("gaussian_c1025", 26744, 1025, "gaussian", {"fallback_ineligible", "select_superset", "rank_bitonic"}, {BT_B}),
    _case("gaussian_c4096", 26744, 4096, "gaussian", {"fallback_ineligible", "rank_bitonic"}, {BT_B}),
    _case("gaussian_c4097", 26744, 4097, "gaussian", {"wide"}),
    _case("first_wide_row_c20", 32257, 20, ALL_RECIPES, {"wide"}),
    _case("mask_fewer_c20", 26744, 20, "mask_fewer", {"fallback_ineligible", "take_all", "rank_counting"}, {BT_C}),
    _case("mask_exactly_c20", 26744, 20, "mask_exactly", {"threshold_first", "rank_counting"}, {TF_C}),
    _case("mask_exactly_c300", 26744, 300, "mask_exactly", {"fallback_ineligible", "take_all"}),
    _case("mask_one_more_c20", 26744, 20, "mask_one_more", {"threshold_first"}),
    _case("mask_fewer_c2000", 26744, 2000, "mask_fewer", {"fallback_ineligible", "take_all", "rank_bitonic"}, {BT_B}),
    _case("nothing_finite_c20", 26744, 20, "nothing_finite", {"fallback_ineligible", "take_all", "rank_counting"}),
    _case("one_residue_class_c20", 26744, 20, "one_residue_class", {"threshold_first", "rank_counting"}, {TF_C}),
    _case("one_residue_class_c30", 26744, 30, "one_residue_class", {"fallback_ineligible", "take_all"}),
    _case("seen_only_c100", 26744, 100, "seen_only", {"threshold_first"}),
]

# Boundary sweep: every size against every cut-off that fits, each case a batch of all recipes (so one launch mixes users that take
# different routes).  The only route stated is the one the sizes are there for: the literal limits of the wide path.
SIZES = (1, 2, 63, 64, 65, 1023, 1024, 1025, 4097, 32255, 32256, 32257, 40000)
CUTOFFS = (1, 2, 255, 256, 257, 511, 512, 513, 1024, 1025, 4095, 4096, 4097)


def _sweep():
    out = []
    for n in SIZES:
        for c in sorted({x for x in CUTOFFS + (n - 1, n) if 1 <= x <= n}):
            out.append(_case("sweep_n%d_c%d" % (n, c), n, c, ALL_RECIPES, {"wide"} if n > 32256 or c > 4096 else set()))
    return out


SWEEP = _sweep()
CASES = NAMED + SWEEP
CASE_BY_NAME = {c.name: c for c in CASES}
assert len(CASE_BY_NAME) == len(CASES)


def case_rows(case):
    """The filtered float32 score rows of a case, one per recipe (seeded by the case's name)."""
    rng = np.random.default_rng(zlib.crc32(case.name.encode()))
    return np.stack([RECIPES[r](case.n_items, case.cutoff, rng) for r in case.recipes]).astype(np.float32)


# ---------------------------------------------------------------------------------------- rows -> models that score to them
def split_filters(rows):
    """-inf cells of a batch of rows -> (item mask uint8 or None: the cells no row admits; seen CSR: the others)."""
    blocked = rows == -np.inf
    everywhere = blocked.all(axis=0)
    allowed = None if not everywhere.any() else (~everywhere).astype(np.uint8)
    seen = sps.csr_matrix((blocked & ~everywhere).astype(np.float32))
    return allowed, seen


def realise_dense(rows):
    """(U, V): U = identity, V[i, r] = rows[r, i] (0 where filtered): row r's scores are rows[r] bit for bit."""
    R = len(rows)
    V = np.ascontiguousarray(np.where(rows == -np.inf, np.float32(0), rows).T, dtype=np.float32)
    return np.eye(R, dtype=np.float32), V


def realise_sparse(rows):
    """(A, B): A = identity, B = the rows' non-zero finite cells."""
    R = len(rows)
    B = sps.csr_matrix(np.where(rows == -np.inf, np.float32(0), rows), dtype=np.float32)
    B.eliminate_zeros()
    return sps.identity(R, dtype=np.float32, format="csr"), B


# ------------------------------------------------------------------------------------------------------ integer models
EXACT_LIMIT = 2 ** 24


def random_seen(n_users, n_items, per_user, rng):
    rows = np.repeat(np.arange(n_users), per_user)
    cols = rng.integers(0, n_items, n_users * per_user)
    X = sps.csr_matrix((np.ones(len(rows), np.float32), (rows, cols)), shape=(n_users, n_items))
    X.data[:] = 1
    return X


def int_dense_model(n_users, n_items, k, use_bias, seed):
    """Small-integer factors (and biases): dict with U, V, bias (bu, bi, mu) or None, X (seen)."""
    rng = np.random.default_rng(seed)
    U = rng.integers(-2, 3, (n_users, k)).astype(np.float32)
    V = rng.integers(-2, 3, (n_items, k)).astype(np.float32)
    bias = (rng.integers(-3, 4, n_users).astype(np.float32), rng.integers(-3, 4, n_items).astype(np.float32), 2.0) if use_bias else None
    return dict(U=U, V=V, bias=bias, X=random_seen(n_users, n_items, min(5, n_items), rng))


def dense_scores(m, users):
    """Host scores of an integer dense model in int64, as float32 (exact: see dense_premise)."""
    s = m["U"][users].astype(np.int64) @ m["V"].astype(np.int64).T
    if m["bias"] is not None:
        bu, bi, mu = m["bias"]
        s = s + bi.astype(np.int64) + int(mu) + bu[users].astype(np.int64)[:, None]
    return s.astype(np.float32)


def dense_premise(m):
    """Integers everywhere, and a bound on the magnitude of every partial sum in any order."""
    arrays = [m["U"], m["V"]] + ([m["bias"][0], m["bias"][1], np.float32(m["bias"][2])] if m["bias"] is not None else [])
    integral = all((np.asarray(a) == np.rint(a)).all() for a in arrays)
    bound = np.abs(m["U"]).astype(np.int64).max(axis=0) @ np.abs(m["V"]).astype(np.int64).max(axis=0)
    if m["bias"] is not None:
        bound += int(np.abs(m["bias"][0]).max() + np.abs(m["bias"][1]).max() + abs(m["bias"][2]))
    return integral, int(bound)


SPECIAL_USERS = (0, 1, 2, 3, 6, 7, 8)
FEW_SCORES = {6: 1, 7: 4, 8: 19}              # user: number of non-zero scores


def int_sparse_model(n_users, n_items, user_based, seed, urm_values=(1,)):
    """ItemKNN (A = URM, B = W items x items) or UserKNN (A = W users x users, B = URM) with small-integer weights, negative ones
    included.  SPECIAL_USERS are the special profiles:
      0  empty row of A: every score is zero, the list is the lowest admissible ids
      1  a single stored cell of A whose row of B has 3 non-zeros: 3 non-zero scores
      2  (ItemKNN) profile {a, b} with W[a] = {b}, W[b] = {a}: the seen items cover all non-zero scores
         (UserKNN) W[2] = {3} and URM[3] is a subset of URM[2]: likewise
      3  a plain user (UserKNN: the neighbour of user 2)
      6, 7, 8  a single stored cell of A whose row of B has 1, 4 and 19 non-zeros (FEW_SCORES): from one non-zero score up to one
         fewer than the cut-offs 5 and 20 the models are ranked at"""
    rng = np.random.default_rng(seed)
    n_w = n_users if user_based else n_items
    X = _random_int_csr(n_users, n_items, max(1, n_items // 50), urm_values, rng)
    W = _random_int_csr(n_w, n_w, max(1, min(n_w // 50, 30)), (-2, -1, 1, 2, 3), rng)
    a, b, c = 5 % n_items, 11 % n_items, 17 % n_items
    few = {u: {60 + j: (-1, 2, 1)[j % 3] for j in range(count)} for u, count in FEW_SCORES.items()}      # the rows of B they receive
    if user_based:
        W = _with_rows(W, {0: {}, 1: {4: 2}, 2: {3: 3}, 6: {9: 1}, 7: {10: 2}, 8: {11: -1}})
        X = _with_rows(X, {4: {a: 1, b: 1, (b + 6) % n_items: 1}, 2: {a: 1, b: 1, (a + 1) % n_items: 1}, 3: {a: 1, b: 1},
                           6: {2: 1}, 7: {2: 1}, 8: {2: 1}, 9: few[6], 10: few[7], 11: few[8]})
    else:
        X = _with_rows(X, {0: {}, 1: {c: 1}, 2: {a: 1, b: 1}, 6: {23: 1}, 7: {29: 1}, 8: {37: 1}})
        W = _with_rows(W, {c: {a: 2, b: -1, (b + 6) % n_items: 1}, a: {b: 2}, b: {a: 3}, 23: few[6], 29: few[7], 37: few[8]})
    return dict(X=X, W=W, user_based=user_based, A=W if user_based else X, B=X if user_based else W)


def _random_int_csr(n_rows, n_cols, per_row, values, rng):
    """`per_row` cells per row at random columns (a column drawn twice keeps one cell), values drawn from `values`."""
    r = np.repeat(np.arange(n_rows), per_row)
    c = rng.integers(0, n_cols, len(r))
    _, first = np.unique(r * n_cols + c, return_index=True)
    v = rng.choice(values, len(first)).astype(np.float32)
    return sps.csr_matrix((v, (r[first], c[first])), shape=(n_rows, n_cols))


def _with_rows(M, rows):
    """CSR matrix M with the given rows replaced: {row: {column: value}}."""
    keep = np.ones(M.shape[0], np.float32)
    keep[list(rows)] = 0
    r = [i for i, cells in rows.items() for _ in cells]
    c = [j for cells in rows.values() for j in cells]
    v = [x for cells in rows.values() for x in cells.values()]
    out = sps.diags(keep).dot(M) + sps.csr_matrix((np.array(v, np.float32), (r, c)), shape=M.shape)
    out = sps.csr_matrix(out, dtype=np.float32)
    out.eliminate_zeros()
    out.sort_indices()
    return out


def sparse_scores(m, users):
    A, B = m["A"].astype(np.int64), m["B"].astype(np.int64)
    return np.asarray(A[users].dot(B).todense()).astype(np.float32)


def sparse_premise(m):
    integral = (m["A"].data == np.rint(m["A"].data)).all() and (m["B"].data == np.rint(m["B"].data)).all()
    bound = abs(m["A"]).astype(np.int64).dot(abs(m["B"]).astype(np.int64))
    return bool(integral), int(bound.max()) if bound.nnz else 0


def apply_filters(scores, X, users, remove_seen=True, allowed=None):
    out = np.array(scores, dtype=np.float32)
    if allowed is not None:
        out[:, ~np.asarray(allowed, bool)] = -np.inf
    if remove_seen:
        for r, u in enumerate(users):
            out[r, X.indices[X.indptr[u]:X.indptr[u + 1]]] = -np.inf
    return out


# (name, n_users, n_items, k, use_bias, cutoffs): the integer dense models of the device tests
DENSE_MODELS = [
    ("k1", 300, 3000, 1, False, (1, 20, 256, 257)),
    ("k1_bias", 300, 3000, 1, True, (2, 20, 511)),
    ("k3", 300, 12000, 3, False, (20, 512)),
    ("k3_bias", 300, 12000, 3, True, (100, 513)),
    ("k33", 300, 5000, 33, False, (20, 1025)),
    ("k33_bias", 300, 5000, 33, True, (2, 255, 4096)),
]
# (name, n_users, n_items, user_based, urm_values, cutoffs)
SPARSE_MODELS = [
    ("itemknn_binary", 300, 2000, False, (1,), (5, 20, 300)),
    ("itemknn_ratings", 300, 6000, False, (1, 2, 3, 4, 5), (20, 1025)),
    ("userknn_binary", 300, 2000, True, (1,), (5, 20, 300)),
    ("userknn_ratings", 200, 6000, True, (1, 2, 3), (20, 257)),
]


def dense_model(name):
    _, n_users, n_items, k, use_bias, _ = next(m for m in DENSE_MODELS if m[0] == name)
    return int_dense_model(n_users, n_items, k, use_bias, zlib.crc32(name.encode()))


def sparse_model(name):
    _, n_users, n_items, user_based, values, _ = next(m for m in SPARSE_MODELS if m[0] == name)
    return int_sparse_model(n_users, n_items, user_based, zlib.crc32(name.encode()) % 100000, values)
