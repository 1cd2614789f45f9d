"""Dense-weight scoring without a GPU: the order contract pinned to the installed SciPy, the constructor keyword of
EASE_R_MI355X_Recommender, and the C ABI of the dense scorer (header, binding, library)."""
import os
import re

import numpy as np
import pytest
import scipy.sparse as sps

from recsys2019_deeplearning_evaluation_amd import _native
import dense_score_cases as DC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = {"mi355rec_dscorer_create", "mi355rec_dscorer_update", "mi355rec_dscorer_set_from_ease", "mi355rec_dscorer_recommend",
           "mi355rec_dscorer_recommend_candidates", "mi355rec_dscorer_get_stats", "mi355rec_dscorer_destroy"}


@pytest.mark.parametrize("name", sorted(DC.shapes()))
def test_the_oracle_is_the_scipy_product(name):
    """SciPy's csr @ ndarray walks a row's stored cells in storage order and rounds the product before the add: the recurrence the
    device kernel implements.  (A fused multiply-add recurrence differs from it by an ulp here and there.)"""
    m = DC.model(name)
    X, W, users = m["X"], m["W"], m["users"]
    product = X[users] @ W
    assert isinstance(product, np.ndarray) and product.dtype == np.float32
    assert np.array_equal(DC.oracle(X, users, W), product)
    # the order matters: this is not a statement about any order of the same cells
    if max(np.diff(X.indptr)) >= 60 and W.shape[1] >= 1000:
        S = X.copy()
        S.sort_indices()
        assert not np.array_equal(S[users] @ W, product)


def test_the_models_hold_what_they_are_there_for():
    m = DC.model("two_tiles_plus_3")
    X = m["X"]
    lengths = np.diff(X.indptr)
    assert set((0, 1, 2, 3, 63, 64, 65, 700)) <= set(lengths.tolist())
    assert lengths[DC.EMPTY_USER] == 0 and X.data[X.indptr[DC.ZERO_USER]] == 0.0 and X.nnz == lengths.sum()
    assert set(np.unique(X.data).tolist()) == {0.0, 1.0, 2.0, 3.0, 4.0, 5.0}
    assert (np.diag(m["W"]) == 0).all()
    T = DC.parse_tile()
    assert sorted(n for _, n in DC.shapes().values())[:5] == [5, T - 1, T, T + 1, 2 * T + 3]
    n_mid, n_wide = DC.shapes()["wide"]
    assert n_mid == 8 and not DC.RC.fits_lds_rank(n_wide, 10) and DC.RC.fits_lds_rank(n_wide - 1, 10)


def test_a_bogus_dense_scoring_is_refused_without_touching_the_device(monkeypatch):
    from recsys2019_deeplearning_evaluation_amd import EASE_R_MI355X_Recommender

    def no_library():
        raise AssertionError("the constructor loaded the native library")

    monkeypatch.setattr(_native, "load", no_library)
    X = sps.random(20, 10, 0.3, format="csr", dtype=np.float32, random_state=0)
    with pytest.raises(ValueError, match="dense_scoring"):
        EASE_R_MI355X_Recommender(X, verbose=False, dense_scoring="bogus")
    for mode in ("host", "device"):
        rec = EASE_R_MI355X_Recommender(X, verbose=False, dense_scoring=mode)
        assert rec.dense_scoring == mode and not rec.dense_device_scorable()         # (no W_sparse yet)
    assert EASE_R_MI355X_Recommender(X, verbose=False).dense_scoring == "host"


def test_the_mixin_tells_the_two_scorers_apart():
    from recsys2019_deeplearning_evaluation_amd import GpuSimilarityScoringMixin, MI355XDenseScorer

    class Model(GpuSimilarityScoringMixin):
        pass

    rec = Model()
    assert rec.dense_scoring == "host" and MI355XDenseScorer._PREFIX == "mi355rec_dscorer"
    rec.W_sparse = np.zeros((3, 3), np.float32)
    assert not rec.device_scorable() and not rec.dense_device_scorable()
    rec.dense_scoring = "device"
    assert not rec.device_scorable() and rec.dense_device_scorable()
    rec.W_sparse = sps.identity(3, format="csr")
    assert rec.device_scorable() and not rec.dense_device_scorable()


def test_header_binding_and_library_agree_on_the_dense_scorer():
    header = open(os.path.join(ROOT, "include", "mi355rec.h")).read()
    header = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    declared = set(re.findall(r"\b(mi355rec_dscorer_\w+)\s*\(", header))
    assert declared == SYMBOLS
    assert {"mi355rec_eval_add_dscorer", "mi355rec_eval_add_dscorer_candidates"} <= set(re.findall(r"\b(mi355rec_eval_\w+)\s*\(", header))
    lib = _native.load()
    for name in sorted(SYMBOLS) + ["mi355rec_eval_add_dscorer", "mi355rec_eval_add_dscorer_candidates"]:
        assert name in _native.SIGNATURES and hasattr(lib, name), name
