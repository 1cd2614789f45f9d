"""What the pivoted device inverse of EASE_R rests on, checked without a GPU: the blocked Gauss-Jordan elimination with partial
pivoting in float64 (restated in NumPy, tests/ease_pivoted_cases.py) is within 1e-7 of the float64 closed form on every indefinite
case at both block sizes (1e-6 once W is rounded to float32), the unpivoted float32 scheme refuses each of those matrices, a
singular or NaN matrix is refused, scaled permutations are inverted exactly, and the Python surface carries the new route."""
import inspect
import os
import re

import numpy as np
import pytest

from recsys2019_deeplearning_evaluation_amd import _native
from recsys2019_deeplearning_evaluation_amd.ease_r import EASE_R_MI355X_Recommender, EASE_R_Recommender, MI355XEase, _EASELogic
from recsys2019_deeplearning_evaluation_amd.reference_binding import bind
from recsys2019_deeplearning_evaluation_amd import recommender_base as RB
import ease_cases as EC
import ease_pivoted_cases as PC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("block", PC.BLOCKS)
def test_restatement_is_within_the_bounds_of_float64(block):
    worst = 0.0
    for name, G in PC.all_matrices(block):
        want = PC.weights_f64_of(name, block)
        got = PC.restated_weights(G, block)
        assert got.dtype == np.float64 and got.shape == want.shape
        if len(G) == 1:
            assert got[0, 0] == 0.0
            continue
        scale = np.abs(want).max()
        err = np.abs(got - want).max() / scale
        err32 = np.abs(got.astype(np.float32) - want).max() / scale
        print("block %3d  %-24s n %5d  float64 %.2e  rounded to float32 %.2e" % (block, name, len(G), err, err32))
        assert err <= PC.ELIMINATION_BOUND, (name, block, err)
        assert err32 <= PC.ROUNDED_BOUND, (name, block, err32)
        worst = max(worst, err)
    assert worst > 0.0


@pytest.mark.parametrize("block", PC.BLOCKS)
def test_the_unpivoted_scheme_refuses_every_one_of_these_matrices(block):
    for name, G in PC.all_matrices(block):
        if len(G) == 1 and G[0, 0] > 0:
            continue                                    # (a positive 1 x 1 matrix IS positive definite)
        with pytest.raises(FloatingPointError):
            EC.blocked_inverse_f32(G, block)


@pytest.mark.parametrize("block", PC.BLOCKS)
def test_scaled_permutations_are_inverted_exactly(block):
    G = PC.scaled_permutation()
    info = {}
    assert np.array_equal(PC.pivoted_inverse_f64(G, block, info).astype(np.float32), PC.exact_inverse_f32(G))
    assert info["moved"] > 0 and info["smallest_pivot"] == np.abs(G[G != 0]).min()
    for n in (block + 1, 2 * block + 3):
        R = PC.reversal(n)
        assert np.array_equal(PC.pivoted_inverse_f64(R, block).astype(np.float32), R)
    info = {}
    PC.pivoted_inverse_f64(PC.diagonally_dominant(2 * block + 3), block, info)
    assert info["moved"] == 0


@pytest.mark.parametrize("block", PC.BLOCKS)
def test_restatement_refuses_singular_and_nan_matrices(block):
    n = 2 * block + 3
    for at in (0, block + 5, n - 1):                    # column 0, inside a later block, the last column
        G = PC.random_symmetric(n).copy()
        G[:, at] = 0.0
        with pytest.raises(FloatingPointError):
            PC.pivoted_inverse_f64(G, block)
    G = PC.random_symmetric(n).copy()
    G[3, block + 9] = np.nan
    with pytest.raises(FloatingPointError):
        PC.pivoted_inverse_f64(G, block)


def test_ties_go_to_the_lowest_row():
    swaps = PC.panel_swaps(np.array([[1.0, 0.0], [-2.0, 1.0], [2.0, 5.0], [0.5, 0.0]]), 10)
    assert [(g, p) for g, p, _ in swaps] == [(10, 11), (11, 12)]


def test_the_indefinite_keyword_and_the_unchanged_fit_signature():
    sig = inspect.signature(_EASELogic.__init__)
    assert list(sig.parameters) == ["self", "URM_train", "verbose", "dense_scoring", "indefinite"]
    assert sig.parameters["indefinite"].default == "host" and sig.parameters["dense_scoring"].default == "host"
    X = EC.fixture()[0]
    for bad in ("gpu", None, True, ""):
        with pytest.raises(ValueError, match="indefinite"):
            EASE_R_MI355X_Recommender(X, verbose=False, indefinite=bad)
    assert EASE_R_MI355X_Recommender(X, verbose=False).indefinite == "host"
    assert EASE_R_MI355X_Recommender(X, verbose=False, indefinite="device").indefinite == "device"
    fit = inspect.signature(EASE_R_MI355X_Recommender.fit)
    assert list(fit.parameters) == ["self", "topK", "l2_norm", "normalize_matrix", "verbose"]
    assert fit == inspect.signature(EASE_R_Recommender.fit)
    R = bind(RB.BaseMatrixFactorizationRecommender, RB.BaseItemSimilarityMatrixRecommender, RB.BaseUserSimilarityMatrixRecommender,
             RB.Incremental_Training_Early_Stopping)
    assert R.EASE_R_MI355X_Recommender(X, verbose=False, indefinite="device").indefinite == "device"
    with pytest.raises(ValueError, match="indefinite"):
        R.EASE_R_MI355X_Recommender(X, verbose=False, indefinite="both")
    assert inspect.signature(R.EASE_R_MI355X_Recommender.fit) == fit
    assert list(inspect.signature(MI355XEase.invert).parameters) == ["self", "pivoted"]
    assert inspect.signature(MI355XEase.invert).parameters["pivoted"].default is False
    assert callable(MI355XEase.pivot_info)


def test_the_new_symbols_are_in_the_header_and_in_the_signatures():
    header = open(os.path.join(ROOT, "include", "mi355rec.h")).read()
    declared = set(re.findall(r"\b(mi355rec_ease_\w+)\s*\(", header))
    new = {"mi355rec_ease_invert_pivoted", "mi355rec_ease_pivot_info"}
    assert new <= declared and new <= set(_native.SIGNATURES)
    assert len(_native.SIGNATURES["mi355rec_ease_invert_pivoted"][1]) == 1
    assert len(_native.SIGNATURES["mi355rec_ease_pivot_info"][1]) == 5
    # mi355rec_ease_fit_info keeps its eight arguments
    assert len(_native.SIGNATURES["mi355rec_ease_fit_info"][1]) == 8
    makefile = open(os.path.join(ROOT, "recsys2019_deeplearning_evaluation_amd", "csrc", "Makefile")).read()
    assert "ease_pivot.hip" in makefile
