"""PureSVD on the device against the reference's own fits (tests/golden/pure_svd.npz, made by tests/golden/make_pure_svd_fixture.py
with scikit-learn's randomized_svd) and against the float64 restatement of tests/pure_svd_cases.py.

Bars of the fixture parity.  d of a case is the distance between replay(float32) and replay(float64), an estimate of the reference's
own float32 rounding distance from the exact result (test_pure_svd_spec prints it).  The device's rounding is independent of it and of
similar size, so 2 d is the expected distance and the bar is max(4 d, floor): a factor two for another summation order.  The floor
covers cases whose d happens to be small: 1e-5 of the largest score for the score matrix, 2e-6 relative for the singular values
(32 float32 ulps of a column norm summed over a few hundred rows).  Factor columns are compared up to sign, and only where the
singular value is separated from both neighbours by more than 1 %: by Wedin's theorem the angle between the computed and the
reference's singular vector is at most |E|_F / gap, with E the difference of the two score matrices (<= sqrt(cells) * bar * largest
score) and gap the distance to the nearest other singular value.

Measured on an MI355X (first device run; sigma: relative distance of the singular values, scores: distance of the score matrices
over the largest score, each with its bar; separated columns compared, their worst distance as a fraction of its bound; fall-backs):
  case  0 clusters k = 8    sigma 4.31e-07 (2.00e-06)  scores 9.02e-07 (1.00e-05)   8 columns 1.0e-03   -
  case  1 clusters k = 20   sigma 5.64e-07 (2.40e-06)  scores 6.10e-06 (2.39e-05)  14 columns 7.6e-04   -
  case  2 ratings  k = 6    sigma 4.09e-07 (2.02e-06)  scores 7.66e-07 (1.00e-05)   6 columns 9.6e-04   -
  case  3 ratings  k = 25   sigma 6.33e-07 (2.47e-06)  scores 2.01e-06 (1.00e-05)  10 columns 1.5e-03   -
  case  4 wide     k = 5    sigma 4.57e-07 (2.00e-06)  scores 7.57e-07 (1.00e-05)   5 columns 1.2e-03   -
  case  5 wide     k = 5    sigma 4.74e-07 (2.00e-06)  scores 7.14e-07 (1.00e-05)   5 columns 1.7e-03   -   (random_seed=None)
  case  6 clusters k = 8    sigma 4.65e-07 (2.00e-06)  scores 7.15e-07 (1.00e-05)   8 columns 6.6e-04   -   (random_seed=None)
  case  7 kron     k = 20   sigma 6.78e-07 (2.12e-06)  scores 8.72e-06 (1.61e-05)   9 columns 1.6e-02   9 host QR, host SVD
  case  8 tiny     k = 20   sigma 1.19e-06 (4.73e-06)  scores 1.04e-06 (1.00e-05)  20 columns 3.0e-03   -
  case  9 tiny     k = 40   sigma 1.05e-06 (4.26e-06)  scores 2.51e-06 (1.00e-05)  25 columns 8.9e-03   -
  case 10 zipf     k = 20   sigma 1.13e-06 (4.39e-06)  scores 1.31e-05 (1.25e-04)   scores of 64 users only
  case 11 zipf     k = 100  sigma 6.58e-07 (2.45e-06)  scores 1.06e-05 (1.19e-04)   scores of 64 users only
The distances sit at 1.0 - 1.3 d (2.2 d on case 7): the reference's own rounding, not the device's, is most of them -- which is also
why the floors were left where the reasoning above put them.  Orthonormality: |V^T V - I| 7e-08 .. 1.4e-07 (5.4e-07 on case 7, where
LAPACK's V is returned), |U^T U - diag(s^2)| / s0^2 3e-09 .. 3.3e-08; the float32 restatement reaches 3.4e-07 .. 1.2e-06 and
1.2e-08 .. 2.4e-07.  Full size: ml1m k = 50 / 200 sigma 4.2e-08 / 8.6e-08, scores 2.0e-06 / 1.2e-06 against replay(float64) (d 1.5e-04 /
6.3e-04: the tail of a flat spectrum is ill-determined in float32); ML-20M shape k = 50: sigma 1.05e-07 against replay(float64) (the
restatement takes 20 s on 16 cores, so it is compared at k = 50 itself), |V^T V - I| 1.5e-07, |U^T U - diag| / s0^2 3.1e-09.
Item variant: values within 6.3e-07 / 7.6e-07 / 2.8e-06 / 4.6e-07 of the largest |W|; case 0 keeps 595 cells where the reference keeps
600 (the five rounding-residue cells of the empty item, see supports_match).
"""
import numpy as np
import pytest
import scipy.sparse as sps

import pure_svd_cases as P
from recsys2019_deeplearning_evaluation_amd import (EvaluatorHoldout_MI355X, PureSVDItemRecommender, PureSVDRecommender)
from recsys2019_deeplearning_evaluation_amd import recommender_base as RB
from recsys2019_deeplearning_evaluation_amd.pure_svd import PureSVD_MI355X_Steps
from recsys2019_deeplearning_evaluation_amd.scoring import GpuScoringMixin
from recsys2019_deeplearning_evaluation_amd.synthetic import named_urm
from test_scoring_gpu import _check_ranking

pytestmark = pytest.mark.gpu

FLOOR_SCORES = 1e-5
FLOOR_SIGMA = 2e-6
U32 = 2.0 ** -24


def fit_case(case, cls=PureSVDRecommender, **extra):
    rec = cls(case["X"].copy(), verbose=False)
    if case["seed"] is None:
        np.random.seed(case["np_seed"])
    rec.fit(num_factors=case["num_factors"], random_seed=case["seed"], **extra)
    return rec, (np.random.rand() if case["seed"] is None else None)


def bars(case):
    d_sigma, d_scores, U32_, V32_ = P.noise_floor(case)
    return max(4 * d_sigma, FLOOR_SIGMA), max(4 * d_scores, FLOOR_SCORES), U32_, V32_


def distances(case, U, V):
    if case["store"] == "factors":
        got, want = P.scores_of(U, V), P.scores_of(case["U"], case["V"])
    else:
        got, want = P.scores_of(U, V, case["users"]), case["scores"]
    return P.sigma_distance(P.singular_values(U), case["s"]), P.score_distance(got, want), np.abs(want).max(), want.size


def test_fixture_parity(gpu):
    cases, _ = P.load_cases()
    report = []
    for case in cases:
        rec, after = fit_case(case)
        U, V = rec.USER_factors, rec.ITEM_factors
        bar_sigma, bar_scores, _, _ = bars(case)
        e_sigma, e_scores, largest, cells = distances(case, U, V)
        n_compared, worst = 0, 0.0
        if case["store"] == "factors":
            assert U.shape == case["U"].shape and V.shape == case["V"].shape, case["index"]
            columns, gap = P.separated_columns(case["s"])
            for j in columns:
                for mine, ref in ((U[:, j], case["U"][:, j]), (V[:, j], case["V"][:, j])):
                    mine, ref = mine.astype(np.float64), ref.astype(np.float64)
                    err = min(np.linalg.norm(mine - ref), np.linalg.norm(mine + ref)) / np.linalg.norm(ref)
                    bound = np.sqrt(cells) * bar_scores * largest / gap[j]
                    worst = max(worst, err / bound)
                n_compared += 1
        else:
            assert tuple(U.shape + V.shape) == tuple(case["shapes"]), case["index"]
        assert U.dtype == np.float32 and V.dtype == np.float32 and isinstance(U, np.ndarray) and isinstance(V, np.ndarray)
        assert np.isfinite(U).all() and np.isfinite(V).all()
        report.append((case["index"], case["urm"], case["num_factors"], e_sigma, bar_sigma, e_scores, bar_scores, n_compared, worst,
                       rec.fit_stats["host_fallbacks"], rec.fit_stats["svd_on_host"], after, case.get("after")))
    print("\n".join("case %d (%s, k = %d): sigma %.2e (bar %.2e), scores %.2e (bar %.2e), %d separated columns at %.2e of their bound, "
                    "%d host QR, %d host SVD" % r[:11] for r in report))
    for r in report:
        assert r[3] <= r[4] and r[5] <= r[6], r
        assert r[8] <= 1.0, r
        assert r[11] == r[12], ("np.random after the fit", r)
    assert report[0][7] > 0 and report[1][7] > 0, "separated columns on the planted-cluster cases"


def test_orthonormality(gpu):
    cases, _ = P.load_cases()
    lines = []
    for case in cases:
        rec, _ = fit_case(case)
        _, _, U32_, V32_ = bars(case)
        ref_v, ref_u = P.orthonormality(U32_, V32_)
        got_v, got_u = P.orthonormality(rec.USER_factors, rec.ITEM_factors)
        lines.append((case["index"], got_v, ref_v, got_u, ref_u))
    print("\n".join("case %d: |V^T V - I| %.2e (replay %.2e), |U^T U - diag| / s0^2 %.2e (replay %.2e)" % l for l in lines))
    for index, got_v, ref_v, got_u, ref_u in lines:
        assert got_v <= 4 * ref_v and got_u <= 4 * ref_u, (index, got_v, ref_v, got_u, ref_u)


def test_repeatability(gpu):
    cases, _ = P.load_cases()
    for case in (cases[1], cases[4], cases[10]):
        a, _ = fit_case(case)
        b, _ = fit_case(case)
        assert a.USER_factors.tobytes() == b.USER_factors.tobytes() and a.ITEM_factors.tobytes() == b.ITEM_factors.tobytes()
        U, V = a.USER_factors.copy(), a.ITEM_factors.copy()
        a.fit(num_factors=case["num_factors"], random_seed=case["seed"])
        assert a.USER_factors.tobytes() == U.tobytes() and a.ITEM_factors.tobytes() == V.tobytes()


def test_rank_deficiency_and_traffic(gpu):
    cases, _ = P.load_cases()
    for n in P.DEGENERATE:
        case = cases[n]
        rec, _ = fit_case(case)
        bar_sigma, bar_scores, _, _ = bars(case)
        e_sigma, e_scores, _, _ = distances(case, rec.USER_factors, rec.ITEM_factors)
        print("case %d: %d host QR, host SVD %d, sigma %.2e scores %.2e" % (n, rec.fit_stats["host_fallbacks"], rec.fit_stats["svd_on_host"],
                                                                           e_sigma, e_scores))
        assert np.isfinite(rec.USER_factors).all() and np.isfinite(rec.ITEM_factors).all()
        assert e_sigma <= bar_sigma and e_scores <= bar_scores
    assert cases[P.DEGENERATE[0]]["s"][-1] < P.SIGMA_SMALL * cases[P.DEGENERATE[0]]["s"][0]
    case = cases[0]                                     # planted clusters, num_factors at the gap
    rec, _ = fit_case(case)
    st = rec.fit_stats
    n_users, n_items = case["X"].shape
    r, nnz = st["r"], case["X"].nnz
    assert st["host_fallbacks"] == 0 and st["svd_on_host"] == 0 and r == case["num_factors"] + 10
    pieces = n_users + n_items                          # every row here is one piece (no row has more than 512 cells)
    urm_upload = 2 * 8 * nnz + 4 * 4 * pieces           # both layouts (indices and values), four words of piece table per row
    applies = st["gram_apply_pairs"] + 2                # + the two of the last step
    grams = st["gram_apply_pairs"] + 1                  # + B B^T
    assert st["create_bytes"] <= urm_upload
    assert st["h2d_bytes"] <= 4 * n_items * r + applies * 4 * r * r            # the Gaussian block and the r x r matrices
    assert st["d2h_bytes"] <= grams * 8 * r * r + 4 * (n_users + n_items) * r    # the Gram matrices and the two factor blocks
    assert st["products"] == 2 * st["n_iter"] + 2


def _product_urm(values):
    rng = np.random.default_rng(5)
    n_rows, n_cols = 400, 25000
    lengths = rng.integers(0, 700, n_rows)              # some above one piece (512 cells), some empty
    lengths[3], lengths[10:14], lengths[399] = 20000, 0, 0
    rows = np.repeat(np.arange(n_rows), lengths)
    cols = np.concatenate([np.sort(rng.choice(n_cols, n, replace=False)) for n in lengths])
    data = np.ones(len(rows), np.float32) if values == "ones" else rng.normal(size=len(rows)).astype(np.float32)
    return sps.csr_matrix((data, (rows, cols)), shape=(n_rows, n_cols), dtype=np.float32)


@pytest.mark.parametrize("values", ["ones", "real"])
@pytest.mark.parametrize("r", [11, 64, 110, 360, 522])
def test_product_kernels_alone(gpu, r, values):
    """S X against SciPy in float64; every cell within the float32 summation bound of its row: (length + 2) * 2^-24 * sum |s| |x|."""
    base = _product_urm(values)
    rng = np.random.default_rng(r)
    for A in (base, sps.csr_matrix(base.T)):            # the long row once in the CSR layout, once in the CSC layout
        steps = PureSVD_MI355X_Steps(A, r)
        try:
            assert steps.fit_info()["all_ones"] == (values == "ones")
            blocks = [rng.normal(size=(A.shape[0], r)).astype(np.float32), rng.normal(size=(A.shape[1], r)).astype(np.float32)]
            for dst in (0, 1):
                S = sps.csr_matrix(A if dst == 0 else A.T, dtype=np.float64)
                X = blocks[1 - dst]
                steps.set_block(1 - dst, X)
                steps.product(dst)
                got = steps.get_block(dst)
                want = S @ X.astype(np.float64)
                bound = (np.diff(S.indptr)[:, None] + 2) * U32 * (abs(S) @ np.abs(X).astype(np.float64))
                assert (np.abs(got - want) <= bound).all(), (r, values, dst, float((np.abs(got - want) - bound).max()))
                assert (got[np.diff(S.indptr) == 0] == 0).all()
                assert steps.stats()["algorithmic_bytes"] == A.nnz * (4.0 * r + 8.0)
                steps.product(dst)
                assert steps.get_block(dst).tobytes() == got.tobytes()
            # Gram matrix and apply through the same entries
            G = steps.gram(1)
            X = steps.get_block(1).astype(np.float64)
            assert np.abs(G - X.T @ X).max() <= 1e-12 * np.abs(G).max()
            T = rng.normal(size=(r, r)).astype(np.float32)
            steps.apply(1, T)
            want = X @ T.astype(np.float64)
            assert np.abs(steps.get_block(1) - want).max() <= (r + 2) * U32 * (np.abs(X) @ np.abs(T).astype(np.float64)).max()
            with pytest.raises(ValueError):
                steps.set_block(0, blocks[1][:, :r - 1] if r > 1 else blocks[1])
            with pytest.raises(ValueError):
                steps.set_block(2, blocks[0])
        finally:
            steps.close()


@pytest.mark.parametrize("num_factors", [50, 200])
def test_full_size_ml1m_shape(gpu, num_factors):
    X = named_urm("ml1m", "binary")
    case = dict(X=X, num_factors=num_factors, seed=17, index=("ml1m", num_factors))
    d_sigma, d_scores, _, _ = P.noise_floor(case)
    U64, V64 = P.replay(X, num_factors, 17, np.float64)
    rec = PureSVDRecommender(X, verbose=False)
    rec.fit(num_factors=num_factors, random_seed=17)
    users = np.sort(np.random.default_rng(3).choice(X.shape[0], 256, replace=False))
    want = P.scores_of(U64, V64, users)
    e_sigma = P.sigma_distance(P.singular_values(rec.USER_factors), P.singular_values(U64))
    e_scores = P.score_distance(P.scores_of(rec.USER_factors, rec.ITEM_factors, users), want)
    bar_sigma, bar_scores = max(4 * d_sigma, FLOOR_SIGMA), max(4 * d_scores, FLOOR_SCORES)
    print("ml1m k = %d: sigma %.2e (d %.2e), scores %.2e (d %.2e), stats %s" % (num_factors, e_sigma, d_sigma, e_scores, d_scores,
                                                                            {k: v for k, v in rec.fit_stats.items() if k != "singular_values"}))
    assert e_sigma <= bar_sigma and e_scores <= bar_scores
    assert rec.fit_stats["host_fallbacks"] == 0 and rec.fit_stats["svd_on_host"] == 0
    lists = rec.recommend(users, cutoff=10)
    tol = 2 * bar_scores * np.abs(want).max()
    for row, u in enumerate(users):
        score_row = want[row].copy()
        score_row[X.indices[X.indptr[u]:X.indptr[u + 1]]] = -np.inf
        _check_ranking(np.asarray(lists[row], dtype=np.int64), score_row, 10, tol)


def test_full_size_ml20m_shape(gpu):
    X = named_urm("ml20m", "binary")
    k = 50
    rec = PureSVDRecommender(X, verbose=False)
    rec.fit(num_factors=k, random_seed=23)
    U, V, st = rec.USER_factors, rec.ITEM_factors, rec.fit_stats
    print("ml20m k = %d: %s" % (k, {key: v for key, v in st.items() if key != "singular_values"}))
    assert U.shape == (X.shape[0], k) and V.shape == (X.shape[1], k) and np.isfinite(U).all() and np.isfinite(V).all()
    assert st["host_fallbacks"] == 0 and st["svd_on_host"] == 0 and st["all_ones"]
    s = P.singular_values(U)
    assert (np.diff(s) <= 0).all()
    assert float(X.nnz) - float((s * s).sum()) >= 0.0            # |A|_F^2 = nnz for a binary URM
    ortho_v, ortho_u = P.orthonormality(U, V)
    print("ml20m: |V^T V - I| %.2e, |U^T U - diag| / s0^2 %.2e" % (ortho_v, ortho_u))
    assert ortho_v <= 6e-6 and ortho_u <= 6e-6                   # 4 x the 1.4e-6 the float32 restatement reaches on the fixture cases
    # singular values against the float64 restatement (sixteen SciPy products of 20 M cells x 60)
    U64, _ = P.replay(X, k, 23, np.float64)
    e_sigma = P.sigma_distance(s, P.singular_values(U64))
    print("ml20m: sigma against replay(float64) %.2e" % e_sigma)
    assert e_sigma <= 1e-5          # the fixture cases' d is 4e-7 .. 1.2e-6; rows here are up to 100 x longer (error ~ sqrt(length))
    users = np.sort(np.random.default_rng(4).choice(X.shape[0], 1000, replace=False))
    lists = rec.recommend(users, cutoff=10)
    host = RB.BaseMatrixFactorizationRecommender._compute_item_score(rec, users).astype(np.float64)
    tol = 1e-5 * np.abs(host).max()
    for row, u in enumerate(users):
        host[row, X.indices[X.indptr[u]:X.indptr[u + 1]]] = -np.inf
        _check_ranking(np.asarray(lists[row], dtype=np.int64), host[row], 10, tol)


def supports_match(got, want, tol):
    """Same support per column, except (the comparator of test_slim_elasticnet_gpu is the model) at the selection cut -- a cell kept by
    one side only holds, within tol, the smallest value the reference kept in that column: a tie, which the reference breaks in no fixed
    order -- and at zero: the reference drops cells that are exactly 0.0, and the row of an EMPTY item in its ITEM_factors is rounding
    residue of LAPACK (1e-10) where the device's is exactly zero, so a cell kept by one side only may also be zero within tol."""
    for j in np.flatnonzero(((got != 0) != (want != 0)).any(axis=0)):
        kept = want[:, j][want[:, j] != 0]
        only_one = np.flatnonzero((got[:, j] != 0) != (want[:, j] != 0))
        v = np.where(got[only_one, j] != 0, got[only_one, j], want[only_one, j])
        at_cut = np.abs(v - kept.min()) <= tol if len(kept) else np.zeros(len(v), bool)
        if not (at_cut | (np.abs(v) <= tol)).all():
            return False
    return True


def test_item_variant(gpu):
    _, item_cases = P.load_cases()
    for case in item_cases:
        rec, after = fit_case(case, PureSVDItemRecommender, topK=case["topK"])
        W, want = rec.W_sparse, case["W"].toarray()
        assert sps.isspmatrix_csr(W) and W.dtype == np.float32 and W.shape == want.shape
        got = W.toarray()
        topK = want.shape[0] if case["topK"] is None else case["topK"]
        err = np.abs(got - want)[(got != 0) & (want != 0)].max() / np.abs(want).max()
        print("item case %d: nnz %d (reference %d), max err / max %.2e" % (case["index"], W.nnz, case["W"].nnz, err))
        assert (got != 0).sum(axis=0).max() <= topK
        assert supports_match(got, want, 1e-5 * np.abs(want).max()) and err <= 1e-5
        assert after == case.get("after")
        lists = rec.recommend(np.arange(20), cutoff=5)
        scores = np.asarray((sps.csr_matrix(case["X"][:20], dtype=np.float64) @ sps.csr_matrix(W, dtype=np.float64)).todense())
        tol = 1e-5 * np.abs(scores).max()
        for u in range(20):
            scores[u, case["X"].indices[case["X"].indptr[u]:case["X"].indptr[u + 1]]] = -np.inf
            _check_ranking(np.asarray(lists[u], dtype=np.int64), scores[u], 5, tol)
    with pytest.raises(ValueError):
        PureSVDItemRecommender(item_cases[1]["X"], verbose=False).fit(num_factors=8, topK=26, random_seed=1)


class _MF(GpuScoringMixin, RB.BaseMatrixFactorizationRecommender):
    RECOMMENDER_NAME = "MF_shell"


class _ListsOnly:
    def __init__(self, rec):
        self._rec = rec

    def __getattr__(self, name):
        return getattr(self._rec, name)


def test_evaluator_harness(gpu):
    from eval_cases import make_case
    case = make_case("binary")
    rec = PureSVDRecommender(case["train"], verbose=False)
    rec.fit(num_factors=12, random_seed=5)
    shell = _MF(case["train"], verbose=False)
    shell.USER_factors, shell.ITEM_factors = rec.USER_factors.copy(), rec.ITEM_factors.copy()
    ev = EvaluatorHoldout_MI355X(case["test"], case["cutoffs"], verbose=False, **case["kwargs"])
    fused, _ = ev.evaluateRecommender(rec)
    same_factors, _ = ev.evaluateRecommender(shell)
    lists, _ = ev.evaluateRecommender(_ListsOnly(rec))
    for cutoff in fused:
        for metric, value in fused[cutoff].items():
            for other in (same_factors, lists):
                assert value == other[cutoff][metric] or (value != value and other[cutoff][metric] != other[cutoff][metric]), (cutoff, metric)
    assert max(fused[c]["RECALL"] for c in fused) > 0.0
