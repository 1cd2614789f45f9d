"""The content-based and CF+CBF hybrid KNN recommenders on the device: the CSR stack made in HBM (csrc/stack.hip) bit for bit
against SciPy's, the similarity build started from it against the build from the host-stacked matrix, every case of the
reference-generated fixture (tests/golden/knn_cbf.npz) through the four recommenders, the shapes a content matrix brings to the column
kernels -- few long rows, real values, empty columns, a wide user base -- against the CPU oracle, and scoring / evaluation.

Tolerance: 1e-5 relative on similarity values, neighbour sets exact up to the tie class (_util.check_topk_against_dense)."""
import ctypes as C

import numpy as np
import pytest
import scipy.sparse as sps

import recsys2019_deeplearning_evaluation_amd as pkg
from oracle import oracle as O
from recsys2019_deeplearning_evaluation_amd import (Compute_Similarity_MI355X, EvaluatorHoldout_MI355X, ItemKNN_CFCBF_Hybrid_Recommender,
                                                    ItemKNNCBFRecommender, MI355XSparseScorer, ResidentStack, ResidentURM,
                                                    UserKNN_CFCBF_Hybrid_Recommender, UserKNNCBFRecommender, _native)
from recsys2019_deeplearning_evaluation_amd import recommender_base as RB
from recsys2019_deeplearning_evaluation_amd.synthetic import synthetic_urm
from _util import check_topk_against_dense, csr_columns_as_slabs, load_golden, unpack_csr

pytestmark = pytest.mark.gpu
RTOL = 1e-5
N_COLS = 37


# ---- the stack kernel ---------------------------------------------------------------------------------------------------------------

def _block(rng, n_rows, nnz, first_row=0, last_row=None, n_cols=N_COLS):
    """n_rows x n_cols CSR with exactly nnz cells in rows [first_row, last_row): real values of both signs, sorted indices."""
    last_row = n_rows if last_row is None else last_row
    cells = rng.choice((last_row - first_row) * n_cols, nnz, replace=False)
    vals = (rng.standard_normal(nnz) * 3).astype(np.float32)
    vals[vals == 0] = 1.0
    M = sps.csr_matrix((vals, (first_row + cells // n_cols, cells % n_cols)), shape=(n_rows, n_cols), dtype=np.float32)
    M.sort_indices()
    assert M.nnz == nnz
    return M


def _scipy_stack(blocks, scales):
    S = sps.vstack([b * s for b, s in zip(blocks, scales)], format="csr")       # (float32 array * Python float: one float32 product)
    assert S.dtype == np.float32
    return S


def _assert_same_arrays(got, want):
    assert got.shape == want.shape and got.nnz == want.nnz
    np.testing.assert_array_equal(np.asarray(got.indptr, np.int64), np.asarray(want.indptr, np.int64))
    np.testing.assert_array_equal(got.indices, want.indices)
    np.testing.assert_array_equal(got.data.view(np.uint32), np.asarray(want.data, np.float32).view(np.uint32))      # bit for bit


def _device_stack(blocks, scales):
    residents = [ResidentURM(b) for b in blocks]
    stack = ResidentStack(residents, scales)
    got = stack.download()
    assert stack.shape == got.shape and stack.nnz == got.nnz
    stack.close()
    for r in residents:
        r.close()
    return got


@pytest.mark.parametrize("n_blocks", [2, 3])
@pytest.mark.parametrize("first_nnz", [0, 1, 2, 3, 4, 5, 63, 64, 65, 1025])
def test_stack_is_bit_identical_to_scipy(gpu, n_blocks, first_nnz):
    """A block's cells start at the nnz of the blocks before it: every alignment of the second block's source against the 16-byte
    quads of the destination, quads that straddle two blocks, a tail shorter than a quad, more than one workgroup (1025 cells), a
    block with rows and no cells (first_nnz = 0), leading and trailing empty rows, a one-row block."""
    rng = np.random.default_rng(100 * n_blocks + first_nnz)
    blocks = [_block(rng, 40, first_nnz), _block(rng, 9, 70, first_row=2, last_row=6)]
    scales = [(0.3, 1.0), (-2.5, 1.0), (1.0, 0.3)][first_nnz % 3]
    if n_blocks == 3:
        blocks.append(_block(rng, 1, 11))
        scales = [(0.3, 1.0, -2.5), (1.0, -2.5, 0.3), (-2.5, 0.3, 1.0)][first_nnz % 3]
    want = _scipy_stack(blocks, scales)
    assert want.shape == (sum(b.shape[0] for b in blocks), N_COLS)
    _assert_same_arrays(_device_stack(blocks, scales), want)


def test_stack_scales_touch_their_own_block_only_and_one_is_a_copy(gpu):
    rng = np.random.default_rng(5)
    blocks = [_block(rng, 6, 50), _block(rng, 7, 61), _block(rng, 5, 42)]
    blocks[1].data[:4] = np.array([1e-38, -1e-38, 1.1754944e-38, 3e-39], np.float32)          # products and inputs below the normal range
    got = _device_stack(blocks, [1.0, 0.3, -2.5])
    _assert_same_arrays(got, _scipy_stack(blocks, [1.0, 0.3, -2.5]))
    assert got.data[:50].tobytes() == blocks[0].data.tobytes()
    np.testing.assert_array_equal(got.data[50:111], blocks[1].data * np.float32(0.3))
    np.testing.assert_array_equal(got.data[111:], blocks[2].data * np.float32(-2.5))
    # a scale of exactly 1 leaves every bit pattern alone, a NaN's payload included (x * 1.0f would quieten a signalling NaN)
    odd = _block(rng, 3, 20)
    odd.data.view(np.uint32)[:3] = [0x7FA00001, 0xFFC12345, 0x00000001]
    same = _device_stack([odd, blocks[0]], [1.0, 1.0])
    assert same.data[:20].tobytes() == odd.data.tobytes()


def test_stack_with_a_scale_of_zero_has_scipys_arrays(gpu):
    rng = np.random.default_rng(6)
    blocks = [_block(rng, 5, 33), _block(rng, 4, 21)]
    want = _scipy_stack(blocks, [0.0, 1.0])
    _assert_same_arrays(_device_stack(blocks, [0.0, 1.0]), want)
    want = _scipy_stack(blocks, [1.0, -0.0])
    _assert_same_arrays(_device_stack(blocks, [1.0, -0.0]), want)


def test_stack_into_a_destination_that_is_not_16_byte_aligned_and_bad_column_ids(gpu):
    """The C entry point with output arrays one word past an allocation: the word-by-word route, same arrays.  A column id outside
    [0, n_cols) is copied and reported (MI355REC_E_INVALID)."""
    rng = np.random.default_rng(7)
    blocks = [_block(rng, 6, 67), _block(rng, 3, 30)]
    want = _scipy_stack(blocks, [0.3, 1.0])
    residents = [ResidentURM(b) for b in blocks]
    table = (_native.CsrBlock * 2)(*[_native.CsrBlock(r.shape[0], r.nnz, r.indptr.ptr, r.indices.ptr, r.data.ptr, s)
                                     for r, s in zip(residents, (0.3, 1.0))])
    out = [_native.DeviceArray(n + 1) for n in (want.shape[0] + 1, want.nnz, want.nnz)]
    lib = _native.load()
    _native.check(lib.mi355rec_csr_stack_device(2, table, N_COLS, *[C.c_void_p(a.address(1)) for a in out]))
    indptr, indices, data = [a.to_host()[1:] for a in out]
    _assert_same_arrays(sps.csr_matrix((data.view(np.float32), indices, indptr), shape=want.shape), want)
    widest = int(max(b.indices.max() for b in blocks))
    assert lib.mi355rec_csr_stack_device(2, table, widest, *[C.c_void_p(a.address(1)) for a in out]) == _native.E_INVALID
    assert lib.mi355rec_csr_stack_device(2, table, widest + 1, *[a.ptr for a in out]) == 0
    for a in out + residents:
        a.close()


# ---- the two ways to the same build ---------------------------------------------------------------------------------------------------

def _content_and_interactions(values, seed=3, n_items=300, n_features=6, n_users=40):
    """ICM (n_items x n_features, real values in (0.1, 3.1)) and a URM of the given kind; 20 items without features."""
    rng = np.random.default_rng(seed)
    dense = rng.random((n_items, n_features)) < np.linspace(0.15, 0.6, n_features)[None, :]
    dense[rng.choice(n_items, 20, replace=False)] = False
    ICM = sps.csr_matrix(np.where(dense, rng.random(dense.shape) * 3 + 0.1, 0).astype(np.float32))
    URM = synthetic_urm(n_users, n_items, 2500, 3, 150, seed=seed + 1, values=values)
    return ICM, URM


def _both_builds(ICM, URM, weight, **kw):
    host = sps.hstack([ICM * weight, URM.T], format="csr").T                                       # the reference's dataMatrix: CSC
    blocks = [ResidentURM(ICM.T), ResidentURM(URM)]
    stack = ResidentStack(blocks, [weight, 1.0])
    _assert_same_arrays(stack.download(), sps.csr_matrix(host))
    a = Compute_Similarity_MI355X(host, **kw)
    b = Compute_Similarity_MI355X.from_resident(stack, 1, **kw)
    return host, a, b, [stack] + blocks


def test_build_from_the_resident_stack_equals_the_build_from_the_host_stack(gpu):
    ICM, URM = _content_and_interactions("real")
    kw = dict(topK=20, shrink=2, similarity="cosine")
    host, a, b, held = _both_builds(ICM, URM, 0.3, **kw)
    orc = O.OracleSimilarity(host, topK=0, shrink=2)
    for dev in (a, b):
        idx, val, _ = dev.compute_slabs()
        for c in range(host.shape[1]):
            check_topk_against_dense(idx[c], val[c], orc.column(c)[0], 20, RTOL)
    assert a.accumulator_info() == b.accumulator_info()
    for o in [a, b] + held:
        o.close()


def test_build_from_the_resident_stack_is_identical_on_binary_data(gpu):
    """All-ones blocks and a scale of 1: integer co-occurrence counts, repeatable bit for bit
    (test_sim_gpu.py::test_deterministic_across_runs_on_binary_data) -- so the two paths give the SAME slabs."""
    ICM, URM = _content_and_interactions("binary")
    ICM.data[:] = 1.0
    for similarity in ("cosine", "jaccard"):
        host, a, b, held = _both_builds(ICM, URM, 1.0, topK=20, shrink=1, similarity=similarity)
        ia, va, _ = a.compute_slabs()
        ib, vb, _ = b.compute_slabs()
        np.testing.assert_array_equal(ia, ib)
        np.testing.assert_array_equal(va, vb)
        assert a.accumulator_info() == b.accumulator_info()
        for o in [a, b] + held:
            o.close()


@pytest.mark.parametrize("weighting", ["TF-IDF", "BM25"])
def test_weighted_matrix_of_both_paths(gpu, weighting):
    """Equal bit for bit.  TF-IDF reads counts only.  BM25 divides by document sums that the pre-pass adds with float64 atomics in
    whatever order the wavefronts arrive, but here every sum is exact: the addends are float32 values (24 bits) of magnitude 0.07 to
    5, at most 46 per document and a few thousand in the total, so no partial sum needs more than 24 + 7 + 12 = 43 of the 53 bits,
    and every output depends on the input bits alone -- which the two paths share."""
    ICM, URM = _content_and_interactions("real")
    host, a, b, held = _both_builds(ICM, URM, 0.7, topK=10, shrink=0, feature_weighting=weighting, weighting_documents="columns")
    wa, wb = a.weighted_matrix(), b.weighted_matrix()
    assert wa.shape == wb.shape == host.shape and wb.dtype == np.float32
    np.testing.assert_array_equal(wa.indptr, wb.indptr)
    np.testing.assert_array_equal(wa.indices, wb.indices)
    np.testing.assert_array_equal(wa.data.view(np.uint32), wb.data.view(np.uint32))
    assert abs(wa - sps.csr_matrix(host)).max() > 0
    for o in [a, b] + held:
        o.close()


def test_from_resident_judges_tf_idf_by_the_blocks_and_the_signs_of_the_scales(gpu):
    ICM, URM = _content_and_interactions("real")
    blocks = [ResidentURM(ICM.T), ResidentURM(URM)]
    for scales, fine in (((0.5, 1.0), True), ((0.0, 1.0), True), ((-0.5, 1.0), False), ((0.5, -1.0), False)):
        stack = ResidentStack(blocks, scales)
        assert stack.values_nonnegative() == fine
        if not fine:
            with pytest.raises(AssertionError, match="TF_IDF"):
                Compute_Similarity_MI355X.from_resident(stack, 1, topK=5, feature_weighting="TF-IDF")
        stack.close()
    stack = ResidentStack(blocks, [float("nan"), 1.0])
    with pytest.raises(ValueError, match="non finite"):                  # the library's own pass over the values
        Compute_Similarity_MI355X.from_resident(stack, 1, topK=5)
    with pytest.raises(ValueError, match="norm_sum_order"):
        Compute_Similarity_MI355X.from_resident(stack, 2, topK=5)
    for o in [stack] + blocks:
        o.close()


# ---- the reference's fits -------------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def golden():
    z, cases = load_golden("knn_cbf")
    matrices = {name: unpack_csr(z, name) for name in ("URM", "icm_real", "icm_all", "ucm_real", "ucm_all")}
    return z, cases, matrices


def _check_w_sparse(W, data_matrix, fit, reference_W=None):
    """W's columns against the oracle's dense columns on `data_matrix` (the transpose of the post-fit content matrix, CSC)."""
    kw = {k: v for k, v in fit.items() if k not in ("feature_weighting", "topK")}
    n = data_matrix.shape[1]
    topK = min(fit["topK"], n)
    assert sps.isspmatrix_csr(W) and W.dtype == np.float32 and W.shape == (n, n)
    assert np.diff(sps.csc_matrix(W).indptr).max() <= topK
    orc = O.OracleSimilarity(data_matrix, topK=0, **kw)
    idx, val = csr_columns_as_slabs(W, topK)
    for c in range(n):
        check_topk_against_dense(idx[c], val[c], orc.column(c)[0], topK, RTOL)
    if reference_W is not None:         # the cells both hold carry the reference's values
        both = W.multiply(reference_W != 0) - reference_W.multiply(W != 0)
        assert abs(both).max() <= RTOL * abs(reference_W).max()


def _check_post_fit_matrix(got, want):
    """As tests/test_sim_gpu.py::test_knn_with_feature_weighting compares the re-weighted URM."""
    assert sps.isspmatrix_csr(got) and got.dtype == np.float32 and got.shape == want.shape
    got = got.copy()
    got.sort_indices()
    np.testing.assert_array_equal(got.indptr, want.indptr)
    np.testing.assert_array_equal(got.indices, want.indices)
    np.testing.assert_allclose(got.toarray(), want.toarray(), rtol=RTOL, atol=1e-7)


def _resident_blocks(rec):
    if isinstance(rec, ItemKNN_CFCBF_Hybrid_Recommender):
        return ResidentURM(rec.ICM_train.T), ResidentURM(rec.URM_train)
    return ResidentURM(rec.UCM_train.T), ResidentURM(rec.URM_train.T)


def _one_ulp_sensitivity(CM, kw, seeds=3):
    """How far one float32 ulp of the stored weights moves the similarities: every value of CM goes one ulp up or down at random,
    and the largest movement of a column of the oracle, relative to that column's largest value, is returned."""
    base = O.OracleSimilarity(CM.T, topK=0, **kw).compute_similarity()
    top = np.abs(base).max(axis=0)
    worst = 0.0
    for seed in range(seeds):
        moved = CM.copy()
        up = np.random.default_rng(seed).random(CM.nnz) < 0.5
        moved.data = np.nextafter(CM.data, np.where(up, np.inf, -np.inf).astype(np.float32))
        other = O.OracleSimilarity(moved.T, topK=0, **kw).compute_similarity()
        worst = max(worst, float((np.abs(other - base).max(axis=0)[top > 0] / top[top > 0]).max()))
    return worst


@pytest.mark.parametrize("n", range(16))
def test_fixture_parity(gpu, golden, n):
    """Every case of the reference-generated fixture.  W_sparse is checked column by column against the oracle's dense columns with
    the tie-aware comparator, and its cells against the reference's W_sparse where both hold one; the post-fit content matrix
    against the reference's as test_sim_gpu.py::test_knn_with_feature_weighting compares the re-weighted URM.

    The oracle's input is the fixture's post-fit matrix, with one exception.  With BM25 / TF-IDF the device's float32 weights and
    the float32 rounding of the reference's float64 weights may differ in the last bit, and where a similarity does not forgive
    that, a build from one rounding cannot be held to 1e-5 of an oracle on the other.  `_one_ulp_sensitivity` measures it: a
    case whose columns move by more than RTOL under one ulp of the weights is checked against the oracle on the recommender's OWN
    post-fit matrix, as test_knn_with_feature_weighting does (the two roundings themselves are compared at RTOL by the post-fit
    check).  That is case 7 alone (adjusted cosine on TF-IDF weights, 2.2e-5): user 37 holds one feature whose weight, 2.6176, lies
    0.4 % from the feature's mean, so one ulp of that mean (2.4e-7) is 2.2e-5 of the centred value and of every similarity of the
    column.  The other weighted cases move by 3.8e-6 (case 1), 1.3e-6 (case 11) and below 3e-7."""
    z, cases, M = golden
    assert len(cases) == 16
    case = cases[n]
    want_W, want_CM = unpack_csr(z, "W_%d" % n), unpack_csr(z, "CM_%d" % n)
    weighted = case["fit"].get("feature_weighting", "none") != "none"
    own = weighted and _one_ulp_sensitivity(want_CM, {k: v for k, v in case["fit"].items() if k not in ("feature_weighting", "topK")}) > RTOL
    assert own == (n == 7)
    weight = {("ICM_weight" if case["cls"].startswith("Item") else "UCM_weight"): case["weight"]} if "weight" in case else {}
    rec = getattr(pkg, case["cls"])(M["URM"], M[case["cm"]], verbose=False)
    rec.fit(**case["fit"], **weight)
    _check_post_fit_matrix(getattr(rec, rec._CM), want_CM)
    _check_w_sparse(rec.W_sparse, (getattr(rec, rec._CM) if own else want_CM).T, case["fit"], want_W)
    if not weight:
        return
    assert rec.stacked_matrix() is getattr(rec, rec._CM)
    res = getattr(pkg, case["cls"])(M["URM"], M[case["cm"]], verbose=False)
    blocks = _resident_blocks(res)
    res.fit(**case["fit"], **weight, resident_blocks=blocks)
    assert abs(getattr(res, res._CM) - M[case["cm"]]).max() == 0 and getattr(res, res._CM).shape == M[case["cm"]].shape      # the constructor's matrix
    stacked = res.stacked_matrix()
    _check_post_fit_matrix(stacked, want_CM)
    _check_w_sparse(res.W_sparse, (stacked if own else want_CM).T, case["fit"], want_W)
    if not weighted:
        stacked.sort_indices()
        assert stacked.data.tobytes() == want_CM.data.tobytes()
    for b in blocks:
        b.close()


# ---- shapes that stress the kernel routes ---------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def thin_icms():
    """300 items x 6 features.  "every": feature 0 is held by all 300 items (a row as long as the matrix is wide); "empty": 20 items hold
    no feature (empty columns) and feature 0 is held by the other 280.  Real values; the binary variants take their pattern."""
    rng = np.random.default_rng(11)
    dense = rng.random((300, 6)) < np.array([1.0, 0.3, 0.2, 0.1, 0.05, 0.4])[None, :]
    dense[:, 0] = True
    every = sps.csr_matrix(np.where(dense, rng.random(dense.shape) * 4 + 0.05, 0).astype(np.float32))
    dense[rng.choice(300, 20, replace=False)] = False
    empty = sps.csr_matrix(np.where(dense, every.toarray(), 0).astype(np.float32))
    assert (np.diff(every.tocsc().indptr)[0], (np.diff(empty.indptr) == 0).sum(), np.diff(empty.tocsc().indptr)[0]) == (300, 20, 280)
    return {"every": every, "empty": empty}


@pytest.mark.parametrize("values", ["binary", "real"])
@pytest.mark.parametrize("topK", [5, 50])
@pytest.mark.parametrize("layout", ["every", "empty"])
def test_thin_content_matrix(gpu, thin_icms, layout, topK, values):
    ICM = thin_icms[layout].copy()
    if values == "binary":
        ICM.data[:] = 1.0
    URM = synthetic_urm(50, 300, 1500, 3, 100, seed=4)
    rec = ItemKNNCBFRecommender(URM, ICM, verbose=False)
    fit = dict(topK=topK, shrink=1, similarity="cosine")
    rec.fit(**fit)
    _check_w_sparse(rec.W_sparse, rec.ICM_train.T, fit)
    cold = np.flatnonzero(rec._cold_item_CBF_mask)
    assert len(cold) == (20 if layout == "empty" else 0)
    assert rec.W_sparse[:, cold].nnz == 0 and rec.W_sparse[cold, :].nnz == 0
    positive = np.diff(sps.csc_matrix(rec.W_sparse).indptr)
    assert positive.max() == topK and (layout == "every" or positive.min() == 0)


@pytest.mark.parametrize("resident", [False, True])
def test_hybrid_stack_of_a_binary_urm_under_a_real_valued_icm(gpu, thin_icms, resident):
    """(6 + 40) x 300: binary and real values in one matrix -- neither the all-ones nor the small-integer accumulators apply."""
    ICM = thin_icms["empty"]
    URM = synthetic_urm(40, 300, 2500, 3, 150, seed=9, values="binary")
    rec = ItemKNN_CFCBF_Hybrid_Recommender(URM, ICM, verbose=False)
    fit = dict(topK=25, shrink=2, similarity="cosine")
    blocks = _resident_blocks(rec) if resident else None
    rec.fit(ICM_weight=0.45, resident_blocks=blocks, **fit)
    stacked = rec.stacked_matrix()
    assert stacked.shape == (300, 46) and stacked.nnz == ICM.nnz + URM.nnz
    _check_w_sparse(rec.W_sparse, stacked.T, fit)
    for b in blocks or ():
        b.close()


def test_user_cbf_on_a_user_base_wider_than_the_lds_accumulator(gpu):
    """33 000 users x 4 features: two accumulator tiles (32 256 cells each), rows of ~10 000 cells.  A sample of columns against the
    oracle, as tests/test_sim_gpu.py::test_userknn_recommender_on_a_wide_user_base does."""
    rng = np.random.default_rng(13)
    n_users = 33000
    dense = rng.random((n_users, 4)) < 0.3
    UCM = sps.csr_matrix(np.where(dense, rng.random(dense.shape) * 2 + 0.5, 0).astype(np.float32))
    assert 9000 < np.diff(UCM.tocsc().indptr).min() and (np.diff(UCM.indptr) == 0).sum() > 1000
    URM = synthetic_urm(n_users, 50, 100000, 1, 40, seed=14)
    rec = UserKNNCBFRecommender(URM, UCM, verbose=False)
    rec.fit(topK=15, shrink=1, similarity="cosine")
    assert rec.W_sparse.shape == (n_users, n_users) and (np.diff(rec.W_sparse.tocsc().indptr) <= 15).all()
    orc = O.OracleSimilarity(rec.UCM_train.T, topK=0, shrink=1)
    Wc = rec.W_sparse.tocsc()
    have_features = np.flatnonzero(np.diff(UCM.indptr) > 0)
    sample = [0, 17, 32255, 32256, n_users - 1] + have_features[[0, len(have_features) // 2, -1]].tolist()
    for c in sample:
        s, e = Wc.indptr[c], Wc.indptr[c + 1]
        order = np.argsort(-Wc.data[s:e], kind="stable")
        idx = -np.ones(15, np.int32); val = np.zeros(15, np.float32)
        idx[:e - s] = Wc.indices[s:e][order]; val[:e - s] = Wc.data[s:e][order]
        check_topk_against_dense(idx, val, orc.column(int(c))[0], 15, RTOL)
        assert (e - s == 0) == (UCM.indptr[c + 1] == UCM.indptr[c])
    assert rec._compute_item_score(np.arange(5)).shape == (5, 50)


# ---- scoring and evaluation -------------------------------------------------------------------------------------------------------------

def _check_ranking(ranked_row, score_row, cutoff, tol):
    """A device list against the host's scores, tie-aware (as tests/test_scoring_gpu.py)."""
    got = ranked_row[ranked_row >= 0]
    finite = np.isfinite(score_row)
    k = min(cutoff, int(finite.sum()))
    assert len(got) == k and len(set(got.tolist())) == k
    if k == 0:
        return
    t = np.sort(score_row[finite])[::-1][k - 1]
    assert np.isfinite(score_row[got]).all()
    assert (score_row[got] >= t - tol).all()
    assert np.isin(np.flatnonzero(score_row > t + tol), got).all()
    assert (np.diff(score_row[got]) <= tol).all()


class _ListsOnly:
    """The recommender's own recommend() behind an object the evaluator cannot score on the device."""

    def __init__(self, rec):
        self.rec = rec

    def recommend(self, *args, **kwargs):
        return self.rec.recommend(*args, **kwargs)

    def get_URM_train(self):
        return self.rec.get_URM_train()

    def set_items_to_ignore(self, items):
        self.rec.set_items_to_ignore(items)

    def reset_items_to_ignore(self):
        self.rec.reset_items_to_ignore()


@pytest.mark.parametrize("model", ["cbf", "hybrid"])
def test_recommend_and_the_evaluator_run_on_the_device(gpu, thin_icms, model, monkeypatch):
    ICM = thin_icms["empty"]
    full = synthetic_urm(200, 300, 9000, 8, 150, seed=21, values="real")
    rng = np.random.default_rng(22)
    held_out = rng.random(full.nnz) < 0.25
    train, test = full.copy(), full.copy()
    train.data[held_out] = 0; test.data[~held_out] = 0
    train.eliminate_zeros(); test.eliminate_zeros()
    if model == "cbf":
        rec = ItemKNNCBFRecommender(train, ICM, verbose=False)
        rec.fit(topK=30, shrink=1, similarity="cosine", feature_weighting="TF-IDF")
    else:
        rec = ItemKNN_CFCBF_Hybrid_Recommender(train, ICM, verbose=False)
        rec.fit(ICM_weight=0.5, topK=30, shrink=1, similarity="cosine")
    users = np.arange(0, 200, 3)
    dev_lists, dev_scores = rec.recommend(users, cutoff=12, return_scores=True)
    assert isinstance(rec._sp_scorer, MI355XSparseScorer)
    host_lists, host_scores = RB.BaseRecommender.recommend(rec, users, cutoff=12, return_scores=True)
    fin = np.isfinite(host_scores)
    assert (np.isfinite(dev_scores) == fin).all()
    scale = np.abs(host_scores[fin]).max()
    assert np.abs(dev_scores[fin] - host_scores[fin]).max() < RTOL * scale
    for r in range(len(users)):
        _check_ranking(np.array(dev_lists[r] + [-1] * (12 - len(dev_lists[r]))), host_scores[r].astype(np.float64), 12, RTOL * scale)
    ev = EvaluatorHoldout_MI355X(test, [5, 10], verbose=False)
    taken = []
    for name in ("_run_fused", "_run_lists"):
        monkeypatch.setattr(ev, name, (lambda inner, name: lambda *a, **k: (taken.append(name), inner(*a, **k))[1])(getattr(ev, name), name))
    fused, _ = ev.evaluateRecommender(rec)
    assert taken == ["_run_fused"]
    lists, _ = ev.evaluateRecommender(_ListsOnly(rec))
    assert taken == ["_run_fused", "_run_lists"]
    assert fused == lists and fused[10]["MAP"] > 0


def test_resident_blocks_of_another_matrix_are_refused(gpu, golden):
    _, _, M = golden
    URM, ICM, UCM = M["URM"], M["icm_real"], M["ucm_real"]
    other_icm = ICM.copy(); other_icm.data[7] += 0.5
    other_urm = URM.copy(); other_urm.data[11] += 1
    good = [ResidentURM(ICM.T), ResidentURM(URM), ResidentURM(UCM.T), ResidentURM(URM.T)]
    bad = [ResidentURM(other_icm.T), ResidentURM(other_urm), ResidentURM(sps.csr_matrix(ICM.T)), ResidentURM(other_urm.T)]
    rec = ItemKNN_CFCBF_Hybrid_Recommender(URM, ICM, verbose=False)
    for blocks in ((bad[0], good[1]), (good[0], bad[1]), (good[1], good[0]), (bad[2], good[1])):      # (bad[2]: the right cells, made from a CSR)
        with pytest.raises(ValueError, match="resident_blocks"):
            rec.fit(ICM_weight=0.5, topK=5, resident_blocks=blocks)
    assert not hasattr(rec, "W_sparse")
    rec.fit(ICM_weight=0.5, topK=5, resident_blocks=(good[0], good[1]))
    assert rec.W_sparse.nnz > 0
    urec = UserKNN_CFCBF_Hybrid_Recommender(URM, UCM, verbose=False)
    for blocks in ((good[2], bad[3]), (good[2], good[1]), (good[0], good[3])):
        with pytest.raises(ValueError, match="resident_blocks"):
            urec.fit(UCM_weight=0.5, topK=5, resident_blocks=blocks)
    urec.fit(UCM_weight=0.5, topK=5, resident_blocks=(good[2], good[3]))
    assert urec.W_sparse.nnz > 0
    with pytest.raises(NotImplementedError):
        urec.fit(UCM_weight=0.5, topK=5, resident_blocks=(good[2], good[3]), use_implementation="python")
    for b in good + bad:
        b.close()
