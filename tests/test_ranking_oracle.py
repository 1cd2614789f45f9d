"""The host side of the exact ranking tests (tests/ranking_cases.py), checked without a device: the oracle against a brute-force
sort, the route predictor against what every named case states it reaches, the coverage of the case table, the premises of the
integer-exact models and the constants read from the kernel sources."""
import numpy as np
import pytest

import ranking_cases as R


def test_constants_parse_and_are_the_ones_the_case_table_was_written_for():
    c = R.parse_constants()
    assert set(c) == set(R._PATTERNS)
    assert all(isinstance(v, int) and v > 0 for v in c.values())
    # the literal limits the named cases and the sweep are placed around: a changed constant must fail here, not lose a route
    assert c["THREADS"] == 1024 and c["THRESHOLD_FACTOR"] * 256 == c["THREADS"]
    assert c["MAX_TOPK"] == 4096 == c["AUX_WORDS"] // 2 and c["COUNTING_MAX"] == 1024
    assert (c["CAP_FLOOR"], c["CAP_PER_K"]) == (256, 2)
    assert R.fits_lds_rank(32256, 4096) and not R.fits_lds_rank(32257, 1) and not R.fits_lds_rank(32256, 4097)


def test_a_constant_that_moves_is_noticed(tmp_path):
    import os
    import shutil
    for f in ("topk.cuh", "score.hip"):
        shutil.copy(os.path.join(R.CSRC, f), tmp_path / f)
    text = (tmp_path / "topk.cuh").read_text()
    (tmp_path / "topk.cuh").write_text(text.replace("constexpr int MAX_TOPK = 4096;", "constexpr int MAX_TOPK = 2048;"))
    assert R.parse_constants(str(tmp_path))["MAX_TOPK"] == 2048
    (tmp_path / "topk.cuh").write_text(text.replace("constexpr int MAX_TOPK = 4096;", "constexpr int MAX_TOPK = kMax;"))
    with pytest.raises(AssertionError):
        R.parse_constants(str(tmp_path))


def test_exact_ranking_equals_a_brute_force_sort():
    rng = np.random.default_rng(0)
    for trial in range(400):
        n = int(rng.integers(1, 40))
        row = rng.integers(-3, 4, n).astype(np.float32)
        if trial % 3:
            row += rng.choice([0.0, 0.5, 0.25], n).astype(np.float32)
        row[rng.random(n) < rng.choice([0.0, 0.2, 0.9, 1.0])] = -np.inf
        cutoff = int(rng.integers(1, n + 1))
        want = sorted((j for j in range(n) if row[j] != -np.inf), key=lambda j: (-float(row[j]), j))[:cutoff]
        want = want + [-1] * (cutoff - len(want))
        assert R.exact_ranking(row, cutoff).tolist() == want
    assert R.exact_ranking(np.array([0.0, 0.0, 0.0], np.float32), 2).tolist() == [0, 1]
    assert R.exact_ranking(np.array([-np.inf, -np.inf], np.float32), 2).tolist() == [-1, -1]


def test_float_key_preserves_order():
    v = np.array([-np.inf, -3e38, -2.0, -1.0, -1e-30, 0.0, 1e-30, 1.0, 1.0 + 2.0 ** -23, 2.0, 3e38], np.float32)
    k = R.float_key(v).astype(np.int64)
    assert (np.diff(k) > 0).all() and k[5] == 0x80000000


def test_route_predictor_on_the_rows_it_was_first_sketched_with():
    rng = np.random.default_rng(5)
    routes, ncand = R.route_detail(rng.normal(size=26744).astype(np.float32), 20)
    assert routes == {"threshold_first", "rank_counting"} and 20 <= ncand < 200
    band = (1 + 0.007 * rng.random(26744)).astype(np.float32)
    assert "fallback_overflow" in R.predict_route(band, 20)
    sparse_user = np.zeros(5000, np.float32); sparse_user[[3, 700, 1500, 2900, 4100]] = [5, 4, 3, 2, 1]
    assert R.predict_route(sparse_user, 20) == {"fallback_overflow", "select_partial_ties", "rank_counting"}
    factors = rng.integers(-2, 3, (20000, 3)).astype(np.float32) @ rng.integers(-2, 3, 3).astype(np.float32)
    assert "threshold_first" in R.predict_route(factors, 20)


@pytest.mark.parametrize("case", R.NAMED, ids=lambda c: c.name)
def test_named_case_reaches_the_routes_it_states(case):
    rows = R.case_rows(case)
    assert rows.shape == (len(case.recipes), case.n_items) and rows.dtype == np.float32
    assert not np.isnan(rows).any() and not (rows == np.inf).any() and not (np.signbit(rows) & (rows == 0)).any()
    reached, ranks = set(), set()
    for row in rows:
        routes = R.predict_route(row, case.cutoff)
        reached |= routes
        ranks |= R.entry_ranks(routes)
    assert case.routes <= reached, (case.name, sorted(case.routes - reached), sorted(reached))
    assert case.entry_ranks <= ranks, (case.name, sorted(case.entry_ranks - ranks), sorted(ranks))


def test_the_sweep_crosses_the_wide_path_where_it_states_and_nowhere_else():
    for case in R.SWEEP:
        reached = set()
        for row in R.case_rows(case):
            assert not np.isnan(row).any() and not (row == np.inf).any() and not (np.signbit(row) & (row == 0)).any()
            reached |= R.predict_route(row, case.cutoff)
        assert ("wide" in reached) == ("wide" in case.routes) and (reached == {"wide"} or "wide" not in reached), case.name


def test_the_named_cases_leave_no_route_out():
    stated = set().union(*(c.routes for c in R.NAMED))
    assert stated == set(R.ROUTES), sorted(set(R.ROUTES) - stated)
    ranks = set().union(*(c.entry_ranks for c in R.NAMED))
    assert ranks == set(R.ENTRY_RANKS), sorted(set(R.ENTRY_RANKS) - ranks)


def test_the_table_holds_every_size_cutoff_tie_structure_and_filter():
    sizes = {c.n_items for c in R.CASES}
    assert set(R.SIZES) <= sizes and set(R.SIZES) == {1, 2, 63, 64, 65, 1023, 1024, 1025, 4097, 32255, 32256, 32257, 40000}
    for n in R.SIZES:
        fitting = {x for x in (1, 2, 255, 256, 257, 511, 512, 513, 1024, 1025, 4095, 4096, 4097, n - 1, n) if 1 <= x <= n}
        assert fitting == {c.cutoff for c in R.SWEEP if c.n_items == n}, n
    assert all(set(c.recipes) == set(R.RECIPES) for c in R.SWEEP)
    # the tie group of "wide_tie_at_cut" is above MAX_TOPK where the row has room for it
    row = R.RECIPES["wide_tie_at_cut"](20000, 100, np.random.default_rng(0))
    assert np.unique(row, return_counts=True)[1].max() > R.C["MAX_TOPK"]
    # narrow-band rows: one 16-bit key prefix, with and without ties
    for name, ties in (("narrow_ties", True), ("narrow_distinct", False), ("narrow_tie_ends_at_cut", True)):
        row = R.RECIPES[name](40000, 20, np.random.default_rng(1))
        assert len(np.unique(R.float_key(row) >> 16)) == 1 and (len(np.unique(row)) < len(row)) == ties
    # the masks leave one fewer than, exactly and one more than `cutoff` finite cells
    for name, extra in (("mask_fewer", -1), ("mask_exactly", 0), ("mask_one_more", 1)):
        assert np.isfinite(R.RECIPES[name](5000, 300, np.random.default_rng(2))).sum() == 300 + extra
    row = R.RECIPES["one_residue_class"](26744, 20, np.random.default_rng(3))
    assert len(set(np.flatnonzero(np.isfinite(row)) % R.C["THREADS"])) == 1 and np.isfinite(row).sum() == 27
    row = R.RECIPES["zeros_straddle_cut"](5000, 20, np.random.default_rng(4))
    assert (row > 0).sum() < 20 < (row >= 0).sum() and (row < 0).any()


def test_realised_models_score_to_the_rows():
    """U = identity / A = identity reproduce the rows exactly in float32 arithmetic (one product by 1.0, the rest exact zeros)."""
    case = R.CASE_BY_NAME["sweep_n1025_c256"]
    rows = R.case_rows(case)
    allowed, seen = R.split_filters(rows)
    U, V = R.realise_dense(rows)
    A, B = R.realise_sparse(rows)
    for scores in ((U @ V.T).astype(np.float32), np.asarray(A.dot(B).todense(), dtype=np.float32)):
        got = R.apply_filters(scores, seen, np.arange(len(rows)), True, allowed)
        assert got.tobytes() == rows.tobytes()
    assert allowed is None and seen.nnz > 0                         # a batch of all recipes: per-user filters only
    allowed, seen = R.split_filters(R.case_rows(R.CASE_BY_NAME["mask_fewer_c20"]))
    assert allowed.sum() == 19 and seen.nnz == 0                    # a single row: its filter is the item mask


@pytest.mark.parametrize("name", [m[0] for m in R.DENSE_MODELS])
def test_integer_dense_model_premise(name):
    m = R.dense_model(name)
    integral, bound = R.dense_premise(m)
    assert integral and bound < R.EXACT_LIMIT
    users = np.arange(m["U"].shape[0])
    s = R.dense_scores(m, users)
    assert np.abs(s).max() <= bound and (s == np.rint(s)).all()
    # the models are there for ties: many cells share a score
    assert len(np.unique(s[0])) < s.shape[1] // 10


@pytest.mark.parametrize("name", [m[0] for m in R.SPARSE_MODELS])
def test_integer_sparse_model_premise_and_special_users(name):
    m = R.sparse_model(name)
    integral, bound = R.sparse_premise(m)
    assert integral and bound < R.EXACT_LIMIT
    assert (m["W"].data < 0).any()
    users = np.arange(4)
    raw = R.sparse_scores(m, users)
    filtered = R.apply_filters(raw, m["X"], users)
    assert not raw[0].any()                                          # empty profile
    assert 1 <= np.count_nonzero(raw[1]) <= 3                        # fewer non-zero scores than any cut-off used with it
    assert np.count_nonzero(raw[2]) > 0 and not np.where(np.isfinite(filtered[2]), filtered[2], 0).any()
    assert R.exact_ranking(filtered[0], 5).tolist() == np.flatnonzero(np.isfinite(filtered[0]))[:5].tolist()
    # one non-zero score ... one fewer than the cut-offs 5 and 20, none of them hidden by the user's seen items
    assert sorted(R.FEW_SCORES.values()) == [1, 4, 19] and {5, 20} & set(next(s[5] for s in R.SPARSE_MODELS if s[0] == name))
    for u, count in R.FEW_SCORES.items():
        row = R.apply_filters(R.sparse_scores(m, [u]), m["X"], [u])[0]
        assert np.count_nonzero(np.where(np.isfinite(row), row, 0)) == count
