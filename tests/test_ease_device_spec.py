"""What the device EASE_R path rests on, checked without a GPU: the blocked, unpivoted float32 elimination (restated in NumPy,
tests/ease_cases.py) stays inside the model's 1e-4 bar on every test case at every block size, it refuses the indefinite matrices
explicit ratings produce, and the new class has the reference's surface."""
import inspect
import os
import re

import numpy as np
import pytest

import recsys2019_deeplearning_evaluation_amd as pkg
from recsys2019_deeplearning_evaluation_amd import _native
from recsys2019_deeplearning_evaluation_amd.ease_r import EASE_R_MI355X_Recommender, EASE_R_Recommender, MI355XEase
from recsys2019_deeplearning_evaluation_amd.reference_binding import bind
from recsys2019_deeplearning_evaluation_amd import recommender_base as RB
import ease_cases as EC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("block", [32, 64, 128])
def test_restatement_is_within_the_bar_of_float64(block):
    worst = 0.0
    for name, G in EC.all_gram_matrices(block):
        want = EC.weights_f64(G)
        got = EC.restated_weights(G, block)
        lu = EC.weights_from_precision(np.linalg.inv(G))            # the float32 LU's own error, for scale
        scale = max(np.abs(want).max(), 1e-300)
        err, err_lu = np.abs(got - want).max() / scale, np.abs(lu - want).max() / scale
        print("block %3d  %-36s n %5d  blocked %.2e  float32 LU %.2e" % (block, name, len(G), err, err_lu))
        assert got.dtype == np.float32
        if len(G) > 1:
            assert err < EC.BAR, (name, block, err)
        else:
            assert got.shape == (1, 1) and got[0, 0] == 0.0
        worst = max(worst, err)
    assert worst > 0.0


def test_restatement_keeps_the_top_50_supports():
    for name, (X, kw) in EC.fit_cases().items():
        if kw["topK"] is None:
            continue
        G = EC.gram_f32(X, kw["l2_norm"], kw["normalize_matrix"])
        want, got = EC.weights_f64(G), EC.restated_weights(G, 128)
        k = kw["topK"]
        differing = 0
        for c in range(len(G)):
            a = set(np.argsort(-want[:, c], kind="stable")[:k])
            b = set(np.argsort(-got[:, c].astype(np.float64), kind="stable")[:k])
            differing += a != b
        print("%-36s columns whose top-%d support differs from float64's: %d" % (name, k, differing))
        assert differing == 0, (name, differing)


def test_restatement_refuses_indefinite_matrices():
    for name, (X, kw) in EC.indefinite_cases().items():
        G = EC.gram_f32(X, kw["l2_norm"], kw["normalize_matrix"])
        assert np.linalg.eigvalsh(G.astype(np.float64)).min() < 0, name
        for block in (32, 64, 128):
            with pytest.raises(FloatingPointError):
                EC.blocked_inverse_f32(G, block)
    X, cases, _ = EC.fixture()
    for n in (1, 2):
        G = EC.gram_f32(X, cases[n]["l2_norm"], cases[n]["normalize_matrix"])
        EC.blocked_inverse_f32(G, 128)


def test_restatement_refuses_zero_pivot_and_nan():
    with pytest.raises(FloatingPointError):
        EC.blocked_inverse_f32(np.array([[0, 1], [1, 0]], np.float32), 64)
    G = EC.random_spd(70)
    G[3, 40] = np.nan
    with pytest.raises(FloatingPointError):
        EC.blocked_inverse_f32(G, 64)


def test_surface_matches_the_reference():
    want = ["self", "topK", "l2_norm", "normalize_matrix", "verbose"]         # EASE_R_Recommender.py:40
    sig = inspect.signature(EASE_R_MI355X_Recommender.fit)
    assert list(sig.parameters) == want
    assert [sig.parameters[p].default for p in want[1:]] == [None, 1e3, False, True]
    assert sig == inspect.signature(EASE_R_Recommender.fit)
    assert "EASE_R_MI355X_Recommender" in pkg.__all__ and pkg.EASE_R_MI355X_Recommender is EASE_R_MI355X_Recommender
    assert "EASE_R_Recommender" in pkg.__all__
    R = bind(RB.BaseMatrixFactorizationRecommender, RB.BaseItemSimilarityMatrixRecommender, RB.BaseUserSimilarityMatrixRecommender,
             RB.Incremental_Training_Early_Stopping)
    assert issubclass(R.EASE_R_MI355X_Recommender, RB.BaseItemSimilarityMatrixRecommender)
    assert inspect.signature(R.EASE_R_MI355X_Recommender.fit) == sig
    assert MI355XEase._PREFIX == "mi355rec_ease"
    assert EASE_R_MI355X_Recommender.RECOMMENDER_NAME == "EASE_R_MI355X_Recommender" != EASE_R_Recommender.RECOMMENDER_NAME


def test_every_ease_symbol_of_the_header_has_a_signature():
    header = open(os.path.join(ROOT, "include", "mi355rec.h")).read()
    declared = set(re.findall(r"\b(mi355rec_ease_\w+)\s*\(", header))
    assert declared >= {"mi355rec_ease_create", "mi355rec_ease_set_gram_from_sim", "mi355rec_ease_set_matrix", "mi355rec_ease_get_matrix",
                        "mi355rec_ease_set_diagonal", "mi355rec_ease_invert", "mi355rec_ease_get_dense", "mi355rec_ease_get_topk",
                        "mi355rec_ease_fit_info", "mi355rec_ease_get_stats", "mi355rec_ease_destroy"}
    assert declared <= set(_native.SIGNATURES)
    assert "mi355rec_sim_compute_dense_device" in header and "mi355rec_sim_compute_dense_device" in _native.SIGNATURES
