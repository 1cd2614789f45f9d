"""PureSVD without a device: the NumPy restatement of tests/pure_svd_cases.py against the reference's own fits
(tests/golden/pure_svd.npz, made by tests/golden/make_pure_svd_fixture.py with scikit-learn's randomized_svd), the noise floor d of
every case, and the package's surface.

d of a case = max |replay(float32) - replay(float64)|, for the singular values (relative) and for the score matrix USER_factors
ITEM_factors^T (relative to its largest entry).  Where the fixture was made the float32 restatement is bit-identical to sklearn;
another BLAS may sum in another order, so the bar of the restatement against the fixture is d itself.  Measured (case: d_sigma,
d_scores): 0: 4.0e-7, 8.8e-7; 1: 6.0e-7, 6.0e-6; 2: 5.1e-7, 6.8e-7; 3: 6.2e-7, 2.0e-6; 4: 4.2e-7, 6.5e-7; 5: 5.0e-7, 6.6e-7;
6: 4.1e-7, 6.0e-7; 7: 5.3e-7, 4.0e-6; 8: 1.2e-6, 1.0e-6; 9: 1.1e-6, 2.5e-6; 10: 1.1e-6, 3.1e-5; 11: 6.1e-7, 3.0e-5."""
import os
import re

import numpy as np
import pytest
import scipy.sparse as sps

import pure_svd_cases as P
import test_native_abi as abi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _reference_scores(case, U, V):
    if case["store"] == "factors":
        return P.scores_of(U, V), P.scores_of(case["U"], case["V"])
    return P.scores_of(U, V, case["users"]), case["scores"]


def test_replay_reproduces_the_reference_fixture_within_its_noise_floor():
    cases, _ = P.load_cases()
    assert len(cases) == len(P.CASES)
    for case in cases:
        d_sigma, d_scores, U, V = P.noise_floor(case)
        got, want = _reference_scores(case, U, V)
        e_sigma, e_scores = P.sigma_distance(P.singular_values(U), case["s"]), P.score_distance(got, want)
        print("case %d (%s, k = %d): d sigma %.2e scores %.2e; replay(float32) against the fixture: sigma %.2e scores %.2e"
              % (case["index"], case["urm"], case["num_factors"], d_sigma, d_scores, e_sigma, e_scores))
        assert 0.0 < d_sigma < 1e-4 and 0.0 < d_scores < 1e-3, case["index"]
        assert e_sigma <= d_sigma and e_scores <= d_scores, case["index"]
        if case["store"] == "factors":
            assert U.shape == case["U"].shape and V.shape == case["V"].shape and case["U"].dtype == np.float32


def test_replay_leaves_numpy_random_state_where_the_reference_leaves_it():
    cases, _ = P.load_cases()
    seen = 0
    for case in cases:
        if case["seed"] is not None:
            continue
        np.random.seed(case["np_seed"])
        P.replay(case["X"], case["num_factors"], None)
        assert np.random.rand() == case["after"]
        seen += 1
    assert seen >= 2


def test_cases_cover_the_branches():
    cases, item_cases = P.load_cases()
    n_iter = {7 if c["num_factors"] < 0.1 * min(c["X"].shape) else 4 for c in cases}
    assert n_iter == {4, 7}
    assert any(c["X"].shape[0] < c["X"].shape[1] for c in cases), "transpose branch"
    assert any(c["num_factors"] > c["X"].shape[1] for c in cases) and any(c["num_factors"] + 10 > c["X"].shape[1] >= c["num_factors"] for c in cases)
    assert any((np.diff(c["X"].indptr) == 0).any() and (np.diff(c["X"].tocsc().indptr) == 0).any() for c in cases), "an empty user and item"
    assert any((c["X"].data != 1.0).any() for c in cases), "real values"
    kron = cases[P.DEGENERATE[0]]
    assert np.linalg.matrix_rank(kron["X"].toarray()) == 9 and kron["s"][9] < 1e-4 * kron["s"][0]
    for case in (cases[0], cases[1]):
        columns, _ = P.separated_columns(case["s"])
        assert len(columns) > 0
    assert {c["topK"] for c in item_cases} >= {None, 5} and any(c["topK"] is not None and c["topK"] > c["X"].shape[1] - 1 for c in item_cases)


def test_item_fixture_is_the_column_topk_of_v_vt():
    cases, item_cases = P.load_cases()
    for case in item_cases:
        if case["seed"] is None:
            np.random.seed(case["np_seed"])
        _, V = P.replay(case["X"], case["num_factors"], case["seed"])
        topK = case["X"].shape[1] if case["topK"] is None else case["topK"]
        W = P.w_sparse_of(V, topK)
        want = case["W"].toarray()
        assert (W != 0).sum(axis=0).max() <= topK and np.abs(W - want).max() <= 1e-5 * np.abs(want).max()


# ---- (c) the package's surface: fails before the feature exists ---------------------------------------------------------------------
def test_package_exports_and_binds_both_classes():
    import recsys2019_deeplearning_evaluation_amd as pkg
    from recsys2019_deeplearning_evaluation_amd import recommender_base as RB
    from recsys2019_deeplearning_evaluation_amd.reference_binding import bind
    from recsys2019_deeplearning_evaluation_amd.scoring import GpuScoringMixin, GpuSimilarityScoringMixin
    assert "PureSVDRecommender" in pkg.__all__ and "PureSVDItemRecommender" in pkg.__all__
    assert issubclass(pkg.PureSVDRecommender, (GpuScoringMixin, RB.BaseMatrixFactorizationRecommender))
    assert issubclass(pkg.PureSVDItemRecommender, (GpuSimilarityScoringMixin, RB.BaseItemSimilarityMatrixRecommender))

    class MF(RB.BaseMatrixFactorizationRecommender):
        pass

    class ItemSim(RB.BaseItemSimilarityMatrixRecommender):
        pass

    class UserSim(RB.BaseUserSimilarityMatrixRecommender):
        pass

    R = bind(MF, ItemSim, UserSim, RB.Incremental_Training_Early_Stopping)
    assert issubclass(R.PureSVDRecommender, MF) and issubclass(R.PureSVDRecommender, GpuScoringMixin)
    assert issubclass(R.PureSVDItemRecommender, ItemSim) and issubclass(R.PureSVDItemRecommender, GpuSimilarityScoringMixin)
    assert R.PureSVDRecommender.RECOMMENDER_NAME == "PureSVDRecommender"
    assert R.PureSVDItemRecommender.RECOMMENDER_NAME == "PureSVDItemRecommender"
    import inspect
    assert list(inspect.signature(pkg.PureSVDRecommender.fit).parameters) == ["self", "num_factors", "random_seed"]
    assert list(inspect.signature(pkg.PureSVDItemRecommender.fit).parameters) == ["self", "num_factors", "topK", "random_seed"]


def test_header_declares_the_svd_group():
    names = abi.declared_symbols()
    for entry in ("create", "set_block", "get_block", "product", "gram", "apply", "get_stats", "fit_info", "destroy"):
        assert "mi355rec_svd_" + entry in names, entry
    abi.test_library_exports_every_declared_symbol()
    abi.test_binding_covers_header_exactly()


def test_bad_arguments_raise_value_error_before_touching_the_device():
    from recsys2019_deeplearning_evaluation_amd.pure_svd import PureSVD_MI355X_Steps, randomized_svd_device
    X = sps.random(20, 10, 0.3, format="csr", dtype=np.float32, random_state=0)
    with pytest.raises(ValueError):
        PureSVD_MI355X_Steps(X, 0)
    with pytest.raises(ValueError):
        randomized_svd_device(X, 0)
    bad = X.copy()
    bad.indices = bad.indices.copy()
    bad.indices[0] = 10                       # a column outside the matrix: refused by create, never handed to the gather
    with pytest.raises(ValueError):
        from recsys2019_deeplearning_evaluation_amd import _native as N
        import ctypes as C
        h = C.c_void_p()
        Xc = sps.csc_matrix(X)
        arrays = (N.as_i32(bad.indptr), N.as_i32(bad.indices), N.as_f32(bad.data), N.as_i32(Xc.indptr), N.as_i32(Xc.indices), N.as_f32(Xc.data))
        N.check(N.load().mi355rec_svd_create(C.byref(h), 20, 10, 4, *[N.ptr(a) for a in arrays]))
    # every refusal of create, word for word: the ones both handle types share and the width with PureSVD's noun
    from _util import block_pair_create_refusals
    assert len(block_pair_create_refusals("svd", "block width r")) == 18


def test_no_cpu_fallback_without_device():
    from recsys2019_deeplearning_evaluation_amd import PureSVDItemRecommender, PureSVDRecommender, _native
    if _native.device_count() > 0:
        pytest.skip("a device is present")
    X = sps.random(40, 30, 0.3, format="csr", dtype=np.float32, random_state=0)
    with pytest.raises(_native.NativeLibraryError):
        PureSVDRecommender(X, verbose=False).fit(num_factors=4, random_seed=1)
    with pytest.raises(_native.NativeLibraryError):
        PureSVDItemRecommender(X, verbose=False).fit(num_factors=4, topK=5, random_seed=1)


def test_source_of_the_kernels_names_nothing_per_width():
    """One product kernel for every block width: the template parameters of its kernel-only header are the all-ones switch only."""
    text = open(os.path.join(ROOT, "recsys2019_deeplearning_evaluation_amd", "csrc", "blocks_kernels.cuh")).read()
    assert re.findall(r"template <([^>]*)>", text) == ["bool ONES"]
