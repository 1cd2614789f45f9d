"""oracle.oracle_random_walk / oracle_random_walk_topk (the float64 restatement of P3alpha / RP3beta) against the reference's own
W_sparse: every case of tests/golden/graph_based_search.npz (tests/graph_cases.py) and of the older tests/golden/graph_based.npz.
CPU only.  This is what lets the GPU tests trust the oracle at shapes the reference is too slow for.

Support: through the row cut and the column cut with their tie classes (graph_cases.check_w_sparse_against_walk); the class is twice
the reference's float32 bound wide, since the reference ranks float32 sums, each of two neighbours off by that bound.
Values: within graph_cases.reference_float32_bound, stated from the reference's float32 operations."""
import numpy as np
import pytest

from oracle import oracle as O
from _util import load_golden, unpack_csr
import graph_cases as G


def _search_cases():
    X, cases = G.load_cases()
    return [(X, c) for c in cases]


def _old_cases():
    z, cases = load_golden("graph_based")
    X = unpack_csr(z, "X")
    for n, c in enumerate(cases):
        c["W"], c["index"] = z["W_%d" % n], n
    return [(X, c) for c in cases]


def _id(prefix):
    return lambda pair: "%s%d-%s" % (prefix, pair[1]["index"], pair[1]["cls"])


def _check(X, case):
    kw = case["kw"]
    topK, normalize = kw["topK"], kw["normalize_similarity"]
    walk = O.oracle_random_walk(X, **G.walk_arguments(case))
    assert walk.dtype == np.float64 and walk.diagonal().max() == 0
    bound = G.reference_float32_bound(X, case)
    assert bound < 1e-4                                     # (a few hundred roundings: the bound says something)
    worst = G.check_w_sparse_against_walk(case["W"], walk, topK, normalize, rtol=2 * bound, value_rtol=bound)
    # the oracle's own post-steps: it passes the same check with no tie class to speak of, and agrees with the reference on every cell both keep
    # (topK = 1 with normalisation makes every kept cell 1.0: the column cut then picks among exact ties)
    mine = O.oracle_random_walk_topk(walk, topK, normalize)
    G.check_w_sparse_against_walk(mine, walk, topK, normalize, rtol=1e-14, value_rtol=1e-12)
    ref = np.asarray(case["W"].todense() if hasattr(case["W"], "todense") else case["W"], dtype=np.float64)
    both = (mine.toarray() != 0) & (ref != 0)
    assert (np.abs(mine.toarray()[both] - ref[both]) <= bound * np.abs(mine.toarray()[both])).all()
    return worst


def test_fixture_holds_the_urm_of_the_case_file_and_spans_the_search_range():
    X, cases = G.load_cases()
    Y = G.search_urm()
    assert (X != Y).nnz == 0 and X.dtype == np.float32
    assert [dict(cls=c["cls"], kw=c["kw"]) for c in cases] == G.CASES
    for cls in ("P3", "RP3"):
        mine = [c["kw"] for c in cases if c["cls"] == cls]
        assert {k["alpha"] for k in mine} == {0.05, 0.4, 1.0, 2.0}
        assert {k["topK"] for k in mine} == {1, 5, 90, 1000}
        assert {k["normalize_similarity"] for k in mine} == {False, True}
        assert {(k.get("min_rating", 0), k.get("implicit", False)) for k in mine} == {(0, False), (3, False), (3, True)}
    assert {c["kw"]["beta"] for c in cases if c["cls"] == "RP3"} == {0.0, 0.6, 2.0}
    counts = np.bincount(X.indices, minlength=X.shape[1])
    assert (counts[list(G.COLD_ITEMS)] == 0).all() and counts[G.LONELY_ITEM] == 1 and (np.diff(X.indptr)[list(G.EMPTY_USERS)] == 0).all()
    assert np.diff(X.indptr)[G.FULL_USER] == G.N_ITEMS - len(G.COLD_ITEMS)


@pytest.mark.parametrize("pair", _search_cases(), ids=_id("search"))
def test_oracle_walk_equals_the_reference_over_the_search_range(pair):
    _check(*pair)


@pytest.mark.parametrize("pair", _old_cases(), ids=_id("old"))
def test_oracle_walk_equals_the_reference_on_the_first_fixture(pair):
    _check(*pair)


def test_oracle_walk_quirks():
    """implicit acts only inside min_rating > 0; the degree counts stored entries; the walk given float32 M values uses them."""
    X = G.search_urm()
    a = O.oracle_random_walk(X, 0.7, 0.3, min_rating=0, implicit=True)
    b = O.oracle_random_walk(X, 0.7, 0.3, min_rating=0, implicit=False)
    assert (a != b).nnz == 0
    c = O.oracle_random_walk(X, 0.7, 0.3, min_rating=3, implicit=True)
    d = O.oracle_random_walk(X, 0.7, 0.3, min_rating=3, implicit=False)
    assert (c != d).nnz > 0 and ((c != 0) != (d != 0)).nnz == 0
    B, M, item_count = O.oracle_walk_inputs(X, 1.0)
    assert (item_count == np.bincount(X.indices, minlength=X.shape[1])).all() and (B.data == 1).all()
    assert np.allclose(np.asarray(M.sum(axis=1)).ravel()[np.diff(X.indptr) > 0], 1.0, rtol=1e-14)
    # cold items: empty rows and columns; the single-user item walks to everything its user holds
    w = O.oracle_random_walk(X, 1.0).toarray()
    assert (w[list(G.COLD_ITEMS)] == 0).all() and (w[:, list(G.COLD_ITEMS)] == 0).all()
    held = X[G.LONELY_USER].indices
    assert set(np.flatnonzero(w[G.LONELY_ITEM])) == set(held) - {G.LONELY_ITEM}
    M32 = M.astype(np.float32)
    w32 = O.oracle_random_walk(X, 1.0, M=M32).toarray()
    assert (w32 != w).any() and np.allclose(w32, w, rtol=1e-6)
    # alpha = 0 (the reference cannot run it): integer co-occurrence counts
    w0 = O.oracle_random_walk(X, 0.0).toarray()
    Xb = (X != 0).astype(np.float64)
    co = (Xb.T @ Xb).toarray()
    np.fill_diagonal(co, 0)
    assert (w0 == co).all()
