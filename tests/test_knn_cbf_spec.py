"""Content-based and CF+CBF hybrid KNN recommenders without a device: their surface (names, signatures, assertions, cold masks), the
binding onto given base classes, the host stacking of the hybrids against the reference-generated fixture
(tests/golden/knn_cbf.npz, made by tests/golden/make_knn_cbf_fixture.py), the CPU oracle against that fixture's W_sparse on the
tall-thin and stacked matrices, and the C ABI of the device stack (struct layout, the host-side refusals)."""
import ctypes as C
import inspect
import os
import subprocess

import numpy as np
import pytest
import scipy.sparse as sps

import recsys2019_deeplearning_evaluation_amd as pkg
from oracle import oracle as O
from oracle.feature_weighting import TF_IDF, okapi_BM_25
from recsys2019_deeplearning_evaluation_amd import (ItemKNN_CFCBF_Hybrid_Recommender, ItemKNNCBFRecommender, ItemKNNCustomSimilarityRecommender,
                                                    UserKNN_CFCBF_Hybrid_Recommender, UserKNNCBFRecommender, _native)
from recsys2019_deeplearning_evaluation_amd import recommender_base as RB
from recsys2019_deeplearning_evaluation_amd.reference_binding import bind
from _util import check_topk_against_dense, csr_columns_as_slabs, load_golden, unpack_csr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RTOL = 1e-5
FIVE = ["ItemKNNCBFRecommender", "UserKNNCBFRecommender", "ItemKNN_CFCBF_Hybrid_Recommender", "UserKNN_CFCBF_Hybrid_Recommender",
        "ItemKNNCustomSimilarityRecommender"]
CBF_FIT = [("topK", 50), ("shrink", 100), ("similarity", "cosine"), ("normalize", True), ("feature_weighting", "none")]


@pytest.fixture(scope="module")
def golden():
    z, cases = load_golden("knn_cbf")
    matrices = {name: unpack_csr(z, name) for name in ("URM", "icm_real", "icm_all", "ucm_real", "ucm_all")}
    return z, cases, matrices


def _recommender(case, matrices):
    return getattr(pkg, case["cls"])(matrices["URM"], matrices[case["cm"]], verbose=False)


def _parameters(fit):
    return [(p.name, p.default) for p in inspect.signature(fit).parameters.values()
            if p.kind is p.POSITIONAL_OR_KEYWORD and p.name != "self"]


def _var_keyword(fit):
    return [p.name for p in inspect.signature(fit).parameters.values() if p.kind is p.VAR_KEYWORD]


# ---- surface ------------------------------------------------------------------------------------------------------------------

def test_the_five_classes_are_exported():
    for name in FIVE + ["ResidentStack"]:
        assert name in pkg.__all__ and hasattr(pkg, name), name


def test_names_and_fit_signatures_are_the_references():
    assert ItemKNNCBFRecommender.RECOMMENDER_NAME == "ItemKNNCBFRecommender"
    assert UserKNNCBFRecommender.RECOMMENDER_NAME == "UserKNNCBFRecommender"
    assert ItemKNN_CFCBF_Hybrid_Recommender.RECOMMENDER_NAME == "ItemKNN_CFCBF_HybridRecommender"       # (sic: the reference's string)
    assert UserKNN_CFCBF_Hybrid_Recommender.RECOMMENDER_NAME == "UserKNN_CFCBF_Hybrid_Recommender"
    assert ItemKNNCustomSimilarityRecommender.RECOMMENDER_NAME == "ItemKNNCustomSimilarityRecommender"
    for cls in (ItemKNNCBFRecommender, UserKNNCBFRecommender):
        assert _parameters(cls.fit) == CBF_FIT and _var_keyword(cls.fit) == ["similarity_args"]
        assert cls.FEATURE_WEIGHTING_VALUES == ["BM25", "TF-IDF", "none"]
    # the hybrids: the reference's weight, then the one documented extra keyword
    assert _parameters(ItemKNN_CFCBF_Hybrid_Recommender.fit) == [("ICM_weight", 1.0), ("resident_blocks", None)]
    assert _parameters(UserKNN_CFCBF_Hybrid_Recommender.fit) == [("UCM_weight", 1.0), ("resident_blocks", None)]
    for cls in (ItemKNN_CFCBF_Hybrid_Recommender, UserKNN_CFCBF_Hybrid_Recommender):
        assert _var_keyword(cls.fit) == ["fit_args"]
    assert _parameters(ItemKNNCustomSimilarityRecommender.fit) == [("W_sparse", inspect.Parameter.empty), ("selectTopK", False), ("topK", 100)]
    assert _parameters(ItemKNNCBFRecommender.__init__) == [("URM_train", inspect.Parameter.empty), ("ICM_train", inspect.Parameter.empty), ("verbose", True)]
    assert _parameters(UserKNNCBFRecommender.__init__) == [("URM_train", inspect.Parameter.empty), ("UCM_train", inspect.Parameter.empty), ("verbose", True)]
    assert UserKNNCBFRecommender._SCORER_USER_BASED and UserKNN_CFCBF_Hybrid_Recommender._SCORER_USER_BASED
    assert not ItemKNNCBFRecommender._SCORER_USER_BASED and not ItemKNN_CFCBF_Hybrid_Recommender._SCORER_USER_BASED


def test_feature_weighting_value_error(golden):
    _, _, M = golden
    for cls, cm in ((ItemKNNCBFRecommender, "icm_real"), (ItemKNN_CFCBF_Hybrid_Recommender, "icm_real"),
                    (UserKNNCBFRecommender, "ucm_real"), (UserKNN_CFCBF_Hybrid_Recommender, "ucm_real")):
        with pytest.raises(ValueError, match="Value for 'feature_weighting' not recognized"):
            cls(M["URM"], M[cm], verbose=False).fit(feature_weighting="nope")


def test_constructor_shape_assertions_and_float32_copies(golden):
    _, _, M = golden
    with pytest.raises(AssertionError, match="ICM_train has 70 rows for the 60 items"):
        ItemKNNCBFRecommender(M["URM"], M["ucm_real"], verbose=False)
    with pytest.raises(AssertionError, match="UCM_train has 60 rows for the 70 users"):
        UserKNNCBFRecommender(M["URM"], M["icm_real"], verbose=False)
    icm = sps.csc_matrix(M["icm_real"], dtype=np.float64)
    icm.data[:3] = 0.0                                       # explicit zeros go
    rec = ItemKNNCBFRecommender(M["URM"], icm, verbose=False)
    assert sps.isspmatrix_csr(rec.ICM_train) and rec.ICM_train.dtype == np.float32 and rec.ICM_train.nnz == icm.nnz - 3
    assert rec.n_features == icm.shape[1] and icm.nnz == M["icm_real"].nnz       # (a copy: the caller's matrix is untouched)
    urec = UserKNNCBFRecommender(M["URM"], M["ucm_real"].astype(np.float64), verbose=False)
    assert sps.isspmatrix_csr(urec.UCM_train) and urec.UCM_train.dtype == np.float32 and urec.n_features == M["ucm_real"].shape[1]


def test_cold_masks_and_their_and_on_the_hybrids(golden):
    _, _, M = golden
    URM, ICM, UCM = M["URM"], M["icm_real"], M["ucm_real"]
    no_features = np.diff(ICM.indptr) == 0
    no_interactions = np.diff(URM.tocsc().indptr) == 0
    assert no_features[5] and no_features[17] and no_interactions[17] and no_interactions[30] and not no_features[30]
    cbf = ItemKNNCBFRecommender(URM, ICM, verbose=False)
    np.testing.assert_array_equal(cbf._cold_item_CBF_mask, no_features)
    np.testing.assert_array_equal(cbf._get_cold_item_mask(), no_interactions)
    hyb = ItemKNN_CFCBF_Hybrid_Recommender(URM, ICM, verbose=False)
    np.testing.assert_array_equal(hyb._get_cold_item_mask(), no_features & no_interactions)
    assert hyb._get_cold_item_mask()[17] and not hyb._get_cold_item_mask()[5] and not hyb._get_cold_item_mask()[30]
    u_no_features = np.diff(UCM.indptr) == 0
    u_no_interactions = np.diff(URM.indptr) == 0
    assert u_no_features[3] and u_no_features[11] and u_no_interactions[11] and not u_no_interactions[3]
    ucbf = UserKNNCBFRecommender(URM, UCM, verbose=False)
    np.testing.assert_array_equal(ucbf._cold_user_CBF_mask, u_no_features)
    np.testing.assert_array_equal(ucbf._get_cold_user_mask(), u_no_interactions)
    uhyb = UserKNN_CFCBF_Hybrid_Recommender(URM, UCM, verbose=False)
    np.testing.assert_array_equal(uhyb._get_cold_user_mask(), u_no_features & u_no_interactions)
    assert uhyb._get_cold_user_mask()[11] and not uhyb._get_cold_user_mask()[3]


def test_custom_similarity_recommender(golden):
    _, _, M = golden
    URM = M["URM"]
    n = URM.shape[1]
    rec = ItemKNNCustomSimilarityRecommender(URM, verbose=False)
    with pytest.raises(AssertionError, match="not square"):
        rec.fit(sps.random(n, n + 1, 0.1, format="csr"))
    with pytest.raises(AssertionError, match="not consistent"):
        rec.fit(sps.random(n + 1, n + 1, 0.1, format="csr"))
    W = sps.random(n, n, 0.4, format="csc", dtype=np.float32, random_state=3)
    rec.fit(W)
    assert sps.isspmatrix_csr(rec.W_sparse) and abs(rec.W_sparse - W).max() == 0
    rec.fit(W, selectTopK=True, topK=5)
    assert sps.isspmatrix_csr(rec.W_sparse) and np.diff(rec.W_sparse.tocsc().indptr).max() == 5
    assert abs(rec.W_sparse - RB.similarityMatrixTopK(W, k=5)).max() == 0
    np.testing.assert_allclose(rec._compute_item_score(np.arange(4)), URM[:4].dot(rec.W_sparse).toarray(), rtol=1e-6)


# ---- binding ------------------------------------------------------------------------------------------------------------------

def test_bind_builds_the_classes_on_the_given_bases():
    class MF(RB.BaseMatrixFactorizationRecommender): pass                        # noqa: E701
    class ItemSim(RB.BaseItemSimilarityMatrixRecommender): pass                  # noqa: E701
    class UserSim(RB.BaseUserSimilarityMatrixRecommender): pass                  # noqa: E701
    class ItemCBF(RB.BaseItemCBFRecommender): pass                               # noqa: E701
    class UserCBF(RB.BaseUserCBFRecommender): pass                               # noqa: E701
    old = bind(MF, ItemSim, UserSim, RB.Incremental_Training_Early_Stopping)
    assert sorted(vars(old)) == sorted([
        "MatrixFactorization_BPR_MI355X", "MatrixFactorization_FunkSVD_MI355X", "MatrixFactorization_AsySVD_MI355X", "IALSRecommender",
        "SLIM_BPR_MI355X", "SLIMElasticNetRecommender", "PureSVDRecommender", "PureSVDItemRecommender", "EASE_R_MI355X_Recommender",
        "NMFRecommender", "ItemKNNCFRecommender", "UserKNNCFRecommender", "P3alphaRecommender", "RP3betaRecommender"])
    R = bind(MF, ItemSim, UserSim, RB.Incremental_Training_Early_Stopping, BaseItemCBFRecommender=ItemCBF, BaseUserCBFRecommender=UserCBF)
    assert sorted(set(vars(R)) - set(vars(old))) == sorted(FIVE)
    for name in ("ItemKNNCBFRecommender", "ItemKNN_CFCBF_Hybrid_Recommender"):
        assert issubclass(getattr(R, name), ItemCBF) and issubclass(getattr(R, name), ItemSim) and issubclass(getattr(R, name), pkg.GpuSimilarityScoringMixin)
    for name in ("UserKNNCBFRecommender", "UserKNN_CFCBF_Hybrid_Recommender"):
        assert issubclass(getattr(R, name), UserCBF) and issubclass(getattr(R, name), UserSim) and getattr(R, name)._SCORER_USER_BASED
    assert issubclass(R.ItemKNNCustomSimilarityRecommender, ItemSim)
    for name in FIVE:
        assert getattr(R, name).RECOMMENDER_NAME == getattr(pkg, name).RECOMMENDER_NAME
        assert _parameters(getattr(R, name).fit) == _parameters(getattr(pkg, name).fit)
    host = bind(MF, ItemSim, UserSim, RB.Incremental_Training_Early_Stopping, device_scoring=False, BaseItemCBFRecommender=ItemCBF,
                BaseUserCBFRecommender=UserCBF)
    assert not issubclass(host.ItemKNNCBFRecommender, pkg.GpuSimilarityScoringMixin)
    z, cases = load_golden("knn_cbf")
    rec = R.ItemKNN_CFCBF_Hybrid_Recommender(unpack_csr(z, "URM"), unpack_csr(z, "icm_real"), verbose=False)
    assert rec.n_features == 12 and rec._get_cold_item_mask()[17]


# ---- the hybrids' host stack and the oracle, against the reference's fits -------------------------------------------------------

def test_host_stack_is_the_references_post_fit_matrix(golden):
    z, cases, M = golden
    weighted = 0
    for n, case in enumerate(cases):
        rec = _recommender(case, M)
        stack = rec._host_stack(case["weight"]) if "weight" in case else getattr(rec, rec._CM)
        want = unpack_csr(z, "CM_%d" % n)
        assert sps.isspmatrix_csr(stack) and stack.dtype == np.float32 and stack.shape == want.shape
        stack.sort_indices()
        np.testing.assert_array_equal(stack.indptr, want.indptr)
        np.testing.assert_array_equal(stack.indices, want.indices)
        weighting = case["fit"].get("feature_weighting", "none")
        if weighting == "none":
            assert stack.data.tobytes() == want.data.tobytes(), case                    # bit for bit
        else:       # the weighting's documents are the rows of the content matrix (ItemKNNCBFRecommender.py:39-45)
            after = sps.csr_matrix((okapi_BM_25 if weighting == "BM25" else TF_IDF)(stack)).astype(np.float32)
            np.testing.assert_array_equal(after.indptr, want.indptr)
            np.testing.assert_allclose(after.toarray(), want.toarray(), rtol=RTOL, atol=1e-7)
            weighted += 1
    assert weighted >= 6


def test_oracle_reproduces_the_references_w_sparse_on_tall_thin_and_stacked_matrices(golden):
    """The data matrix is the transpose of the post-fit content matrix: CSC, so the norms are summed in the CSC order."""
    z, cases, _ = golden
    seen = set()
    for n, case in enumerate(cases):
        kw = {k: v for k, v in case["fit"].items() if k != "feature_weighting"}
        data_matrix = unpack_csr(z, "CM_%d" % n).T
        assert sps.isspmatrix_csc(data_matrix) and data_matrix.shape[0] < 90
        W = unpack_csr(z, "W_%d" % n)
        n_cols = data_matrix.shape[1]
        assert W.shape == (n_cols, n_cols)
        topK = min(kw.pop("topK"), n_cols)
        orc = O.OracleSimilarity(data_matrix, topK=0, **kw)
        idx, val = csr_columns_as_slabs(W, topK)
        for c in range(n_cols):
            check_topk_against_dense(idx[c], val[c], orc.column(c)[0], topK, RTOL)
        seen.add(case["fit"]["similarity"])
    assert seen == {"cosine", "pearson", "jaccard", "tanimoto", "asymmetric", "dice", "tversky", "adjusted"}


# ---- C ABI of the device stack --------------------------------------------------------------------------------------------------

def test_block_struct_has_the_layout_of_the_header(tmp_path):
    header = os.path.join(ROOT, "include", "mi355rec.h")
    cls = _native.CsrBlock
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "%s"' % header, 'int main(void) {',
             'printf("%zu %d", sizeof(mi355rec_csr_block), MI355REC_STACK_MAX_BLOCKS);']
    for field, _ in cls._fields_:
        lines.append('printf(" %s:%%zu", offsetof(mi355rec_csr_block, %s));' % (field, field))
    lines += ['printf("\\n");', 'return 0;', '}']
    src = tmp_path / "layout.c"
    src.write_text("\n".join(lines))
    exe = tmp_path / "layout"
    subprocess.run(["gcc", str(src), "-o", str(exe)], check=True)
    size, max_blocks, *fields = subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()
    assert int(size) == C.sizeof(cls) == 40 and int(max_blocks) == _native.STACK_MAX_BLOCKS
    assert len(fields) == len(cls._fields_) == 6
    for item in fields:
        name, off = item.split(":")
        assert getattr(cls, name).offset == int(off), (name, off)


def test_stack_entry_point_refuses_bad_tables_on_the_host():
    """Every one of these is turned down before the device is looked for: MI355REC_E_INVALID here and on a machine with a GPU alike
    (the pointers are never followed)."""
    lib = _native.load()
    somewhere = C.c_void_p(0x1000)

    def call(blocks, n_blocks=None, n_cols=37, out=(somewhere, somewhere, somewhere)):
        table = (_native.CsrBlock * max(1, len(blocks)))(*blocks)
        return lib.mi355rec_csr_stack_device(len(blocks) if n_blocks is None else n_blocks, table, n_cols, *out)

    def block(n_rows, nnz, scale=1.0):
        return _native.CsrBlock(n_rows, nnz, somewhere, somewhere, somewhere, scale)

    assert call([], n_blocks=0) == _native.E_INVALID
    assert call([block(1, 1)], n_blocks=-1) == _native.E_INVALID
    assert call([block(-1, 0)]) == _native.E_INVALID
    assert call([block(2, -5)]) == _native.E_INVALID
    assert call([block(2, 2)], n_cols=-1) == _native.E_INVALID
    assert call([block(2 ** 30, 5), block(2 ** 30, 5)]) == _native.E_INVALID                  # 2^31 rows
    assert call([block(2 ** 31 - 1, 5)]) == _native.E_INVALID                                  # (and 2^31 row pointers)
    assert call([block(10, 2 ** 30), block(10, 2 ** 30)]) == _native.E_INVALID                # 2^31 cells
    assert call([block(0, 3)]) == _native.E_INVALID                                            # cells in no rows
    assert call([block(2, 2)], out=(somewhere, None, somewhere)) == _native.E_INVALID
    assert call([_native.CsrBlock(2, 2, somewhere, None, somewhere, 1.0)]) == _native.E_INVALID
    assert lib.mi355rec_csr_stack_device(1, None, 37, somewhere, somewhere, somewhere) == _native.E_INVALID
    assert call([block(1, 0)] * 17) == _native.E_UNSUPPORTED
    with pytest.raises(ValueError, match="csr_stack"):
        _native.check(call([block(-1, 0)]))


def test_resident_stack_checks_its_arguments_before_the_device():
    class Block:                # (what ResidentStack reads of a ResidentURM before it allocates anything)
        def __init__(self, shape, nnz):
            self.shape, self.nnz = shape, nnz
    with pytest.raises(ValueError, match="blocks and"):
        _native.ResidentStack([], [])
    with pytest.raises(ValueError, match="blocks and"):
        _native.ResidentStack([Block((2, 3), 1)], [1.0, 2.0])
    with pytest.raises(ValueError, match="different numbers of columns"):
        _native.ResidentStack([Block((2, 3), 1), Block((2, 4), 1)], [1.0, 1.0])
    with pytest.raises(ValueError, match="do not fit int32"):
        _native.ResidentStack([Block((2 ** 30, 3), 1), Block((2 ** 30, 3), 1)], [1.0, 1.0])
