"""TopPop and GlobalEffects on the device against the reference's own classes (tests/golden/non_personalized.npz, written by
tests/golden/make_non_personalized_fixture.py) and against a float64 restatement of GlobalEffects.fit.

Bounds.  Device against the restatement: the same float32 element-wise roundings and float64 sums on both sides, so only the order of
a sum differs -- at most n_cells 2^-53 relative to the magnitudes summed (n_cells: the cells of that column or row), and one more
rounding for the quotient; mu is bit-equal (sums of half-step ratings are exact in float64).  Device against the fixture: the
reference sums in float32 -- non_personalized_cases.float32_summation_bounds derives the worst case.  Lists are compared tie-aware:
same length, same reference score at every position -- exactly for TopPop, within one float32 ulp of max|item_bias| plus the bias
bound for GlobalEffects (which ranks float32(item_bias)).  Measured distances: profiles/non_personalized_parity.json."""
import json
import os

import numpy as np
import pytest
import scipy.sparse as sps

from non_personalized_cases import CASES, CUTOFFS, FIXTURE, LAMBDAS, case_urm, float32_summation_bounds, global_effects_f64
from recsys2019_deeplearning_evaluation_amd import GlobalEffects, ResidentURM, TopPop
from recsys2019_deeplearning_evaluation_amd import _native as N

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_parity = {}


@pytest.fixture(scope="module")
def fitted(gpu):
    """name -> (TopPop, GlobalEffects at the first lambda pair), fitted once from the host CSR."""
    out = {}
    for name in CASES:
        top, ge = TopPop(case_urm(name), verbose=False), GlobalEffects(case_urm(name), verbose=False)
        top.fit()
        ge.fit(lambda_user=LAMBDAS[0][0], lambda_item=LAMBDAS[0][1])
        out[name] = (top, ge)
    return out


@pytest.mark.gpu
@pytest.mark.parametrize("name", CASES)
def test_item_pop_equals_the_reference(fitted, name):
    top = fitted[name][0]
    want = FIXTURE[name + "_item_pop"]
    assert top.item_pop.dtype == np.int32 and np.array_equal(top.item_pop, want)
    assert top.n_items == len(want)
    resident = ResidentURM(top.URM_train)
    again = TopPop(case_urm(name), verbose=False)
    again.fit(resident_urm=resident)
    assert np.array_equal(again.item_pop, want)
    assert again.recommend(FIXTURE[name + "_users"], cutoff=20) == top.recommend(FIXTURE[name + "_users"], cutoff=20)
    with pytest.raises(ValueError, match="resident_urm"):
        TopPop(case_urm(name)[:, ::-1], verbose=False).fit(resident_urm=resident)
    resident.close()


def _order_bounds(URM, lambda_user, lambda_item):
    """Per column / per row: n_cells 2^-53 sum|terms| / denominator, plus 2^-53 |value| for the quotient's rounding."""
    X = sps.csr_matrix(URM, dtype=np.float32, copy=True)
    X.eliminate_zeros()
    mu, item_bias, user_bias = global_effects_f64(X, lambda_user, lambda_item)
    d = (X.data - mu).astype(np.float32).astype(np.float64)
    left = (d - item_bias[X.indices]).astype(np.float32).astype(np.float64)
    rows = np.repeat(np.arange(X.shape[0]), np.diff(X.indptr))
    col_nnz, row_nnz = np.bincount(X.indices, minlength=X.shape[1]), np.diff(X.indptr)
    u = 2.0 ** -53
    item = col_nnz * u * np.bincount(X.indices, weights=np.abs(d), minlength=X.shape[1]) / (col_nnz + lambda_item) + u * np.abs(item_bias)
    user = row_nnz * u * np.bincount(rows, weights=np.abs(left), minlength=X.shape[0]) / (row_nnz + lambda_user) + u * np.abs(user_bias)
    return (mu, item_bias, user_bias), item, user


@pytest.mark.gpu
@pytest.mark.parametrize("lambdas", LAMBDAS)
@pytest.mark.parametrize("name", CASES)
def test_global_effects_against_the_restatement_and_the_reference(gpu, name, lambdas):
    lu, li = lambdas
    rec = GlobalEffects(case_urm(name), verbose=False)
    rec.fit(lambda_user=lu, lambda_item=li)
    (mu, item_bias, user_bias), item_tol, user_tol = _order_bounds(case_urm(name), lu, li)
    assert isinstance(rec.mu, np.float32) and rec.mu == mu
    assert rec.item_bias.dtype == np.float64 and rec.item_bias.shape == (rec.n_items,) and rec.user_bias.shape == (rec.n_users,)
    d_item, d_user = np.abs(rec.item_bias - item_bias), np.abs(rec.user_bias - user_bias)
    print("%s %s: restatement item %.3g user %.3g" % (name, lambdas, d_item.max(), d_user.max()))
    assert (d_item <= item_tol).all() and (d_user <= user_tol).all()
    # the same from the device copy, bit for bit (fixed summation order), and on a second run
    resident = ResidentURM(rec.URM_train)
    again = GlobalEffects(case_urm(name), verbose=False)
    again.fit(lambda_user=lu, lambda_item=li, resident_urm=resident)
    assert again.mu == rec.mu and np.array_equal(again.item_bias, rec.item_bias) and np.array_equal(again.user_bias, rec.user_bias)
    resident.close()
    # the reference's own fit (float32 sums)
    tag = "%s_ge_%d_%d" % (name, lu, li)
    mu_bound, item_bound, user_bound = float32_summation_bounds(case_urm(name), lu, li)
    f_mu = abs(float(rec.mu) - float(FIXTURE[tag + "_mu"]))
    f_item = np.abs(rec.item_bias - FIXTURE[tag + "_item_bias"]).max()
    f_user = np.abs(rec.user_bias - FIXTURE[tag + "_user_bias"]).max()
    _parity["%s lambda_user=%d lambda_item=%d" % (name, lu, li)] = {
        "mu": [f_mu, mu_bound], "item_bias": [float(f_item), item_bound], "user_bias": [float(f_user), user_bound],
        "restatement_item_bias": float(d_item.max()), "restatement_user_bias": float(d_user.max())}
    print("%s %s: reference mu %.3g (<= %.3g) item %.3g (<= %.3g) user %.3g (<= %.3g)" % (
        name, lambdas, f_mu, mu_bound, f_item, item_bound, f_user, user_bound))
    assert f_mu <= mu_bound and f_item <= item_bound and f_user <= user_bound


@pytest.mark.gpu
def test_parity_report(gpu):
    """profiles/non_personalized_parity.json: [distance to the reference, bound] of every case, as measured in this run."""
    if len(_parity) != len(CASES) * len(LAMBDAS):
        for name in CASES:
            for lambdas in LAMBDAS:
                try:
                    test_global_effects_against_the_restatement_and_the_reference(None, name, lambdas)
                except AssertionError:
                    pass
    assert len(_parity) == len(CASES) * len(LAMBDAS)
    try:
        with open(os.path.join(ROOT, "profiles", "non_personalized_parity.json"), "w") as f:
            json.dump({"device": N.device_name(), "rule": "[distance to the reference's float32-summed fit, derived worst-case bound]",
                       "cases": _parity}, f, indent=1, sort_keys=True)
            f.write("\n")
    except OSError:
        pass                                            # a read-only tree: the figures are in the output above


def _same_scores(lists, table, scores, tol, where):
    for got, ref in zip(lists, table):
        ref = ref[ref >= 0]
        assert len(got) == len(ref), where
        assert len(set(got)) == len(got), where
        if len(ref):
            assert np.abs(scores[np.asarray(got, dtype=np.int64)] - scores[ref]).max() <= tol, where


@pytest.mark.gpu
@pytest.mark.parametrize("name", CASES)
def test_lists_carry_the_reference_scores(fitted, name):
    top, ge = fitted[name]
    users, subset = FIXTURE[name + "_users"], FIXTURE[name + "_subset"]
    ref_bias = FIXTURE["%s_ge_%d_%d_item_bias" % ((name,) + LAMBDAS[0])]
    ulp = float(np.spacing(np.float32(np.abs(ref_bias).max())))
    ge_tol = ulp + float32_summation_bounds(case_urm(name), *LAMBDAS[0])[1]
    for cutoff in CUTOFFS:
        for seen in (1, 0):
            for sub in (0, 1):
                kw = dict(cutoff=cutoff, remove_seen_flag=bool(seen), items_to_compute=subset if sub else None)
                key = "c%d_s%d_i%d" % (cutoff, seen, sub)
                got = top.recommend(users, **kw)
                _same_scores(got, FIXTURE["%s_toppop_%s" % (name, key)], FIXTURE[name + "_item_pop"].astype(np.float64), 0.0, ("toppop", key))
                if seen:
                    for u, items in zip(users, got):
                        assert not set(items) & set(top.URM_train.indices[top.URM_train.indptr[u]:top.URM_train.indptr[u + 1]])
                if sub:
                    assert all(set(items) <= set(subset.tolist()) for items in got)
                _same_scores(ge.recommend(users, **kw), FIXTURE["%s_ge_%s" % (name, key)], ref_bias, ge_tol, ("ge", key))
    single = top.recommend(int(users[0]), cutoff=5)
    assert single == top.recommend(users[:1], cutoff=5)[0]
    lists, scores = top.recommend(users[:4], cutoff=5, return_scores=True)
    assert scores.shape == (4, top.n_items) and lists == top.recommend(users[:4], cutoff=5)


@pytest.mark.gpu
@pytest.mark.parametrize("cls", [TopPop, GlobalEffects])
def test_saved_model_is_scored_without_a_fit(fitted, tmp_path, cls):
    name = "holes"
    rec = fitted[name][0 if cls is TopPop else 1]
    users = FIXTURE[name + "_users"]
    rec.save_model(str(tmp_path) + "/", file_name="model")
    fresh = cls(case_urm(name), verbose=False)
    fresh.load_model(str(tmp_path) + "/", file_name="model")
    for cutoff in CUTOFFS:
        assert fresh.recommend(users, cutoff=cutoff) == rec.recommend(users, cutoff=cutoff)
    vector = "item_pop" if cls is TopPop else "item_bias"
    assert np.array_equal(getattr(fresh, vector), getattr(rec, vector)) and getattr(fresh, vector).dtype == getattr(rec, vector).dtype


@pytest.mark.gpu
def test_scorer_cache_follows_the_vector_and_the_urm(fitted):
    top = TopPop(case_urm("binary"), verbose=False)
    top.fit()
    users = FIXTURE["binary_users"]
    first = top.recommend(users, cutoff=5, remove_seen_flag=False)
    scorer = top._item_scorer
    assert top.recommend(users, cutoff=5, remove_seen_flag=False) == first and top._item_scorer is scorer
    top.item_pop = top.item_pop[::-1].copy()                        # a new vector: an update of the same scorer
    flipped = top.recommend(users, cutoff=5, remove_seen_flag=False)
    assert top._item_scorer is scorer and flipped != first
    assert flipped[0] == np.argsort(-top.item_pop.astype(np.float32), kind="stable")[:5].tolist()
    top.set_URM_train(top.URM_train)                                # a new URM_train object: a new scorer
    assert top.recommend(users, cutoff=5, remove_seen_flag=False) == flipped and top._item_scorer is not scorer
    top.invalidate_scorer()
    assert top._item_scorer is None
