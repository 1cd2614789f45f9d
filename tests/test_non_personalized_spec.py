"""CPU checks of the non-personalized recommenders: Random against the reference's recorded np.random stream and lists, the
shared-vector scorer's algorithm (restated in NumPy, tests/non_personalized_cases.py) against the exact ranking oracle, and the
classes' place in the package and in reference_binding.bind."""
import zlib

import numpy as np
import pytest

import recsys2019_deeplearning_evaluation_amd as P
from non_personalized_cases import (CASES, FIXTURE, META, broadcast_rows, case_urm, float32_summation_bounds, global_effects_f64, masks,
                                    model_order, profiles, seen_matrix, vectors, windowed_lists)
from ranking_cases import apply_filters, exact_rankings
from recsys2019_deeplearning_evaluation_amd import recommender_base as RB
from recsys2019_deeplearning_evaluation_amd.reference_binding import bind


@pytest.mark.parametrize("name", CASES)
def test_random_reproduces_the_reference_stream_and_lists(name):
    users, subset = FIXTURE[name + "_users"], FIXTURE[name + "_subset"]
    saved = np.random.get_state()
    try:
        rec = P.Random(case_urm(name), verbose=False)
        rec.fit(random_seed=META["random_seed"])
        block0 = rec._compute_item_score(users[:3])
        block1 = rec._compute_item_score(users[3:5], items_to_compute=subset)
        state = np.random.get_state()
        for got, want in ((block0, FIXTURE[name + "_random_block0"]), (block1, FIXTURE[name + "_random_block1"])):
            assert got.dtype == want.dtype and np.array_equal(got, want)
        assert state[0] == "MT19937" and np.array_equal(state[1], FIXTURE[name + "_random_state_keys"])
        assert state[2] == int(FIXTURE[name + "_random_state_pos"])
        rec.fit(random_seed=META["random_seed"])
        lists = rec.recommend(users, cutoff=META["random_cutoff"])          # float64 draws have no ties: the lists are determined
        want = [[int(i) for i in row if i >= 0] for row in FIXTURE[name + "_random_lists"]]
        assert lists == want
    finally:
        np.random.set_state(saved)


def test_random_needs_no_device_scorer():
    assert not issubclass(P.Random, P.GpuItemScoreMixin)
    assert issubclass(P.TopPop, P.GpuItemScoreMixin) and issubclass(P.GlobalEffects, P.GpuItemScoreMixin)
    assert "host" in P.Random.__doc__ and "float32" in P.Random.__doc__


def _cutoffs(n_items):
    return sorted({c for c in (1, 2, 10, 64, 65, n_items - 1, n_items) if 1 <= c <= n_items})


@pytest.mark.parametrize("W", [64, 2048, 8192])
@pytest.mark.parametrize("n_items", [1, 2, 63, 64, 65, 1000, 4097])
def test_windowed_algorithm_equals_the_exact_oracle(n_items, W):
    rng = np.random.default_rng(zlib.crc32(b"windowed") + n_items)
    vecs = vectors(n_items, rng)
    del vecs["non_finite"]                                  # (NaN: the device test; the oracle's argsort has no place for it)
    base_order = model_order(vecs["distinct"])
    rows = profiles(base_order, [c for c in (1, 10) if c <= n_items], rng)
    X = seen_matrix(rows, n_items)
    users = np.arange(len(rows))
    checked = 0
    for vec_name, vec in vecs.items():
        for mask_name, mask in masks(n_items, model_order(vec), rng).items():
            if mask_name == "no_head":
                continue
            for remove_seen in (True, False):
                filtered = apply_filters(broadcast_rows(vec, len(rows)), X, users, remove_seen, mask)
                for cutoff in _cutoffs(n_items):
                    got = windowed_lists(vec, rows, cutoff, remove_seen, mask, W)
                    assert np.array_equal(got, exact_rankings(filtered, cutoff)), (vec_name, mask_name, remove_seen, cutoff)
                    checked += 1
    assert checked >= 5 * 3 * 2


def test_global_effects_restatement_is_within_float32_summation_of_the_reference():
    """The float64 restatement the device is held to against the reference's own (float32-summed) fit: inside the derived bounds."""
    for name in CASES:
        for lu, li in META["lambdas"]:
            mu, item_bias, user_bias = global_effects_f64(case_urm(name), lu, li)
            mu_bound, item_bound, user_bound = float32_summation_bounds(case_urm(name), lu, li)
            tag = "%s_ge_%d_%d" % (name, lu, li)
            assert abs(float(mu) - float(FIXTURE[tag + "_mu"])) <= mu_bound
            assert np.abs(item_bias - FIXTURE[tag + "_item_bias"]).max() <= item_bound
            assert np.abs(user_bias - FIXTURE[tag + "_user_bias"]).max() <= user_bound


def test_host_scores_follow_the_reference_dtypes():
    X = case_urm("ratings")
    top, ge = P.TopPop(X, verbose=False), P.GlobalEffects(X, verbose=False)
    top.item_pop, top.n_items = FIXTURE["ratings_item_pop"], X.shape[1]
    ge.item_bias, ge.n_items = FIXTURE["ratings_ge_10_25_item_bias"], X.shape[1]
    subset = FIXTURE["ratings_subset"]
    assert top._compute_item_score([0, 1]).dtype == np.float32 and ge._compute_item_score([0, 1]).dtype == np.float64
    block = ge._compute_item_score([0, 1, 2], items_to_compute=subset)
    assert block.shape == (3, X.shape[1]) and np.isneginf(np.delete(block[1], subset)).all()
    assert np.array_equal(block[2, subset], ge.item_bias[subset].astype(np.float32).astype(np.float64))
    # the host recommend() of the base class on the reference's vector gives lists with the reference's scores, position by position
    lists = RB.BaseRecommender.recommend(top, FIXTURE["ratings_users"], cutoff=20)
    want = FIXTURE["ratings_toppop_c20_s1_i0"]
    for got, ref in zip(lists, want):
        ref = ref[ref >= 0]
        assert len(got) == len(ref) and np.array_equal(top.item_pop[got], top.item_pop[ref])


def test_classes_are_exported():
    for name in ("TopPop", "GlobalEffects", "Random", "MI355XItemScorer", "GpuItemScoreMixin"):
        assert name in P.__all__ and hasattr(P, name)
    assert (P.TopPop.RECOMMENDER_NAME, P.GlobalEffects.RECOMMENDER_NAME, P.Random.RECOMMENDER_NAME) == (
        "TopPopRecommender", "GlobalEffectsRecommender", "RandomRecommender")


def test_bind_builds_the_three_classes_on_the_given_base():
    class ForeignBase(RB.BaseRecommender):
        pass

    args = (RB.BaseMatrixFactorizationRecommender, RB.BaseItemSimilarityMatrixRecommender, RB.BaseUserSimilarityMatrixRecommender,
            RB.Incremental_Training_Early_Stopping)
    assert not hasattr(bind(*args), "TopPop")
    R = bind(*args, BaseRecommender=ForeignBase)
    for name in ("TopPop", "GlobalEffects", "Random"):
        assert issubclass(getattr(R, name), ForeignBase), name
    assert issubclass(R.TopPop, P.GpuItemScoreMixin) and not issubclass(R.Random, P.GpuItemScoreMixin)
    host = bind(*args, device_scoring=False, BaseRecommender=ForeignBase)
    assert not issubclass(host.TopPop, P.GpuItemScoreMixin)


def test_bind_takes_the_reference_base_class():
    from oracle import ref_loader
    Base = ref_loader.load_python_reference("Base.BaseRecommender", "BaseRecommender")
    if Base is None:
        pytest.skip("the reference tree is not on this machine")
    R = bind(RB.BaseMatrixFactorizationRecommender, RB.BaseItemSimilarityMatrixRecommender, RB.BaseUserSimilarityMatrixRecommender,
             RB.Incremental_Training_Early_Stopping, BaseRecommender=Base)
    for name in ("TopPop", "GlobalEffects", "Random"):
        assert issubclass(getattr(R, name), Base), name
    saved = np.random.get_state()
    try:
        rec = R.Random(case_urm("binary"), verbose=False)
        rec.fit(random_seed=3)
        assert len(rec.recommend([0, 1], cutoff=5)) == 2
    finally:
        np.random.set_state(saved)
