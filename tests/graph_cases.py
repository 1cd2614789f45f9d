"""P3alpha / RP3beta test helper (NumPy / SciPy only): the seeded URM and the cases of tests/golden/graph_based_search.npz (written by
tests/golden/make_graph_based_fixture.py from the reference's own recommenders), the comparison of a finished W_sparse with the
float64 walk of oracle.oracle_random_walk through BOTH cuts with their tie classes, and the float32 error bound of the reference's path.

The URM: 150 users x 90 items, ratings 1 .. 5, with
  two cold items (COLD_ITEMS), two empty users (EMPTY_USERS), one item that a single user holds (LONELY_ITEM) and one user who
  rated every item that is not cold (FULL_USER, who is therefore that single user) -- through that user every pair of warm items
  co-occurs, so every warm row of the walk is full and topK = 90 / 1000 reach past its non-zero cells (87 at most).
The cases span the range the hyper-parameter search draws from: alpha in {0.05, 0.4, 1, 2}, beta in {0, 0.6, 2} (RP3beta; P3alpha is the
beta = None walk), topK in {1, 5, 90, 1000}, normalize_similarity on and off, min_rating = 3 with implicit off and on -- every value with
each of the two classes at least once.  alpha = 0 is NOT in the fixture: the reference cannot run it (SciPy's sparse .power refuses the
exponent 0); the package accepts it and tests/test_graph_gpu.py pins what it computes there.
"""
import json
import os
import sys

import numpy as np
import scipy.sparse as sps

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

GOLDEN = os.path.join(ROOT, "tests", "golden", "graph_based_search.npz")
N_USERS, N_ITEMS = 150, 90
COLD_ITEMS, EMPTY_USERS = (13, 57), (4, 99)
LONELY_ITEM, FULL_USER = 30, 7
LONELY_USER = FULL_USER          # who rated every item holds the single-user item, too
F32 = 2.0 ** -24                # half a float32 ulp: the relative error of one float32 rounding


def search_urm():
    rng = np.random.default_rng(190)
    pop = 0.03 + 0.3 * rng.random(N_ITEMS) ** 2
    dense = rng.random((N_USERS, N_ITEMS)) < pop[None, :]
    dense[:, LONELY_ITEM] = False
    dense[FULL_USER, :] = True
    dense[:, list(COLD_ITEMS)] = False
    dense[list(EMPTY_USERS), :] = False
    ratings = rng.integers(1, 6, size=dense.shape)
    X = sps.csr_matrix(np.where(dense, ratings, 0).astype(np.float32))
    X.sort_indices()
    return X


def _case(cls, **kw):
    return dict(cls=cls, kw=kw)


CASES = [
    _case("P3", alpha=0.05, topK=5, normalize_similarity=False),
    _case("P3", alpha=0.4, topK=1, normalize_similarity=True),
    _case("P3", alpha=1.0, topK=90, normalize_similarity=False),
    _case("P3", alpha=2.0, topK=1000, normalize_similarity=True),
    _case("P3", alpha=1.0, topK=5, normalize_similarity=True, min_rating=3, implicit=False),
    _case("P3", alpha=0.4, topK=5, normalize_similarity=False, min_rating=3, implicit=True),
    _case("P3", alpha=2.0, topK=1, normalize_similarity=False),
    _case("P3", alpha=0.05, topK=90, normalize_similarity=True),
    _case("P3", alpha=1.0, topK=1000, normalize_similarity=False, min_rating=3, implicit=True),
    _case("P3", alpha=2.0, topK=5, normalize_similarity=True),
    _case("RP3", alpha=0.05, beta=0.0, topK=5, normalize_similarity=True),
    _case("RP3", alpha=0.4, beta=0.6, topK=1, normalize_similarity=False),
    _case("RP3", alpha=1.0, beta=2.0, topK=90, normalize_similarity=True),
    _case("RP3", alpha=2.0, beta=0.6, topK=1000, normalize_similarity=False),
    _case("RP3", alpha=1.0, beta=0.6, topK=5, normalize_similarity=True, min_rating=3, implicit=False),
    _case("RP3", alpha=0.4, beta=2.0, topK=5, normalize_similarity=False, min_rating=3, implicit=True),
    _case("RP3", alpha=2.0, beta=2.0, topK=5, normalize_similarity=True),
    _case("RP3", alpha=2.0, beta=0.0, topK=1, normalize_similarity=True),
    _case("RP3", alpha=0.05, beta=2.0, topK=1000, normalize_similarity=True),
    _case("RP3", alpha=1.0, beta=0.0, topK=90, normalize_similarity=False),
    _case("RP3", alpha=0.4, beta=0.6, topK=90, normalize_similarity=True, min_rating=3, implicit=True),
]


def load_cases():
    """(X, cases) of the fixture: every case a dict with cls, kw and W, the reference's W_sparse (csr, its own dtype)."""
    z = np.load(GOLDEN, allow_pickle=False)
    X = sps.csr_matrix((z["X_data"], z["X_indices"], z["X_indptr"]), shape=tuple(int(v) for v in z["X_shape"]))
    cases = json.loads(str(z["cases"]))
    for n, c in enumerate(cases):
        shape = tuple(int(v) for v in z["W_%d_shape" % n])
        c["W"] = sps.csr_matrix((z["W_%d_data" % n], z["W_%d_indices" % n], z["W_%d_indptr" % n]), shape=shape)
        c["index"] = n
    return X, cases


def walk_arguments(case):
    """The arguments of oracle.oracle_random_walk for a case (of either fixture)."""
    kw = case["kw"]
    return dict(alpha=kw.get("alpha", 1.0), beta=kw.get("beta", 0.6) if case["cls"] == "RP3" else None,
                min_rating=kw.get("min_rating", 0), implicit=kw.get("implicit", False))


def reference_float32_bound(X, case):
    """Relative error of a cell of the REFERENCE's W_sparse against the exact walk, from the float32 operations of its path (the URM is
    float32, so sklearn's normalize, .power and the sparse product all stay float32), with u = 2^-24 per rounding, n_u = the longest
    user profile, n_i = the most users of an item (both after the min_rating filter):
      Pui = r / sum|r|        the float32 row sum of n_u terms and the division          (n_u + 1) u
      Pui^alpha               amplifies that by alpha, and rounds                        alpha (n_u + 1) u + u
      Piu = (1 / n_i)^alpha   exact count, division, power                               (alpha + 1) u
      Piu . Pui               one product and a float32 sum of at most n_i terms         (n_i + 1) u
      (RP3beta) * degree      in float64, stored as float32                              u
    normalize_similarity divides by the float32 sum of a row's (at most min(topK, n_items)) cells, each off by the bound so far:
    the bound doubles, plus (cells + 1) u."""
    kw = case["kw"]
    Xf = sps.csr_matrix(X, dtype=np.float64, copy=True)
    if kw.get("min_rating", 0) > 0:
        Xf.data[Xf.data < kw["min_rating"]] = 0
        Xf.eliminate_zeros()
    n_u = int(np.diff(Xf.indptr).max())
    n_i = int(np.bincount(Xf.indices, minlength=Xf.shape[1]).max())
    alpha = kw.get("alpha", 1.0)
    bound = (alpha * (n_u + 1) + 1) * F32 + (alpha + 1) * F32 + (n_i + 1) * F32 + (F32 if case["cls"] == "RP3" else 0.0)
    if kw.get("normalize_similarity", case["cls"] == "RP3"):
        bound = 2 * bound + (min(kw.get("topK", 100), X.shape[1]) + 1) * F32
    return bound


def check_w_sparse_against_walk(W, walk, topK, normalize_similarity, rtol, value_rtol=None, value_atol_of_row_max=None):
    """A finished W_sparse (rows = source items) against the full float64 walk `walk` (oracle_random_walk), through the two cuts the
    reference makes, each with the tie class of _util.check_topk_against_dense taken relative to the cut (|x - t| <= rtol max(|x|, |t|)):
      row cut     the topK largest cells of a row (zeros compete, then are dropped); a cell is SURE when it lies above the class of
                  the K-th value, MAYBE when inside it;
      rows        optionally divided by the sum of their kept cells (= the sum of the K largest: whichever tied cells were kept);
      column cut  the topK largest non-zero cells of a column among those the row cut kept.  Which MAYBE cells it saw is not known,
                  so its K-th value lies between that of the SURE cells alone and that of SURE and MAYBE together.
    Every cell of W must be SURE or MAYBE and not below the lower column bar; every SURE cell above the upper column bar must be in W.
    Values: within value_rtol of the walk's (normalised) cell, or within value_atol_of_row_max of the largest of the row.  Returns the
    largest relative error met."""
    F = np.asarray(walk.todense(), dtype=np.float64)
    n = F.shape[0]
    K = min(int(topK), n)
    G = np.asarray(sps.csr_matrix(W).todense(), dtype=np.float64)
    top = -np.sort(-F, axis=1)[:, :K]                          # the K largest of every row, descending
    t = top[:, K - 1][:, None]
    band = rtol * np.maximum(np.abs(F), np.abs(t))
    sure = (F - t > band) & (F != 0)
    maybe = (np.abs(F - t) <= band) & (F != 0)
    norm = np.abs(top).sum(axis=1) if normalize_similarity else np.ones(n)
    Nrm = F / np.where(norm != 0, norm, 1.0)[:, None]
    worst = 0.0
    for j in range(n):
        col, s, m, g = Nrm[:, j], sure[:, j], maybe[:, j], G[:, j] != 0
        assert not (g & ~(s | m)).any(), "column %d holds a cell the row cut drops" % j
        desc_sure, desc_all = -np.sort(-col[s]), -np.sort(-col[s | m])
        lo = desc_sure[K - 1] if len(desc_sure) >= K else -np.inf
        hi = desc_all[K - 1] if len(desc_all) >= K else -np.inf
        if np.isfinite(lo):
            assert (col[g] - lo >= -rtol * np.maximum(np.abs(col[g]), abs(lo))).all(), "column %d holds a cell below its K-th value" % j
        must = s & ((col - hi > rtol * np.maximum(np.abs(col), abs(hi))) if np.isfinite(hi) else True)
        assert g[must].all(), "column %d misses a cell above its K-th value" % j
        assert g.sum() <= K
        assert g.sum() >= min(K, int(s.sum())), "column %d: too few cells" % j
        if g.any():
            err = np.abs(G[g, j] - col[g])
            if value_rtol is not None:
                assert (err <= value_rtol * np.abs(col[g])).all(), "column %d: relative error %.3g > %.3g" % (
                    j, (err / np.abs(col[g])).max(), value_rtol)
            if value_atol_of_row_max is not None:
                row_max = np.abs(Nrm[g]).max(axis=1)
                assert (err <= value_atol_of_row_max * row_max).all(), "column %d: error %.3g of the row's largest" % (j, (err / row_max).max())
            worst = max(worst, float((err / np.abs(col[g])).max()))
    return worst
