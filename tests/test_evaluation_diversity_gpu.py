"""DIVERSITY_SIMILARITY on the device, in both evaluators: against the reference's values (tests/golden/evaluator_diversity.npz, written
by tests/golden/make_diversity_fixture.py from the reference's own evaluators and Diversity_similarity) and against the float64
restatement of tests/diversity_cases.py; every path, block size and matrix layout against one another bit for bit.

Bounds (relative, L = min(cutoff, list length)): a per-user value within 4 L^2 2^-53 of the restatement -- both sum the same <= L^2
non-negative float64 terms, each in an order of its own, each within L^2 2^-53 of the exact sum, and the division adds 2^-53; the
metric within that bound at the longest list plus n_users 2^-53 for the sum over the users; against the reference's stored values
the bounds of tests/test_evaluation_diversity_cpu.py."""
import math

import numpy as np
import pytest
import scipy.sparse as sps

from diversity_cases import CASES, diversity_per_user, list_lengths, make_case
from eval_cases import make_case as make_eval_case, set_model
from recsys2019_deeplearning_evaluation_amd import (EASE_R_MI355X_Recommender, EvaluatorHoldout_MI355X, EvaluatorNegativeItemSample_MI355X,
                                                    TopPop)
from recsys2019_deeplearning_evaluation_amd import _native as N
from recsys2019_deeplearning_evaluation_amd.evaluation import METRICS, METRICS_WITH_DIVERSITY, PER_USER
from test_evaluation_diversity_cpu import FIXTURE, reference_bounds
from test_evaluation_gpu import FLOAT32_ACCUMULATED, _FixtureLists, _ItemSim, _ListsOnly, _MF

DS = "DIVERSITY_SIMILARITY"
EPS = 2.0 ** -53
HOLDOUT = [name for name in CASES if name.startswith("holdout")]


class _Diversity:
    """What the reference's scripts pass: an object with the matrix as `item_diversity_matrix`."""

    def __init__(self, matrix):
        self.item_diversity_matrix = matrix


def _evaluator(name, diversity=True, **kwargs):
    case = make_case(name)
    if diversity:
        kwargs["diversity_object"] = _Diversity(case["D"])
    if "negative" in case:
        return EvaluatorNegativeItemSample_MI355X(case["test"], case["negative"], case["cutoffs"], verbose=False, **kwargs)
    return EvaluatorHoldout_MI355X(case["test"], case["cutoffs"], verbose=False, **kwargs)


def _fixed(name):
    return _FixtureLists(make_case(name)["train"], FIXTURE[name + "_users"], FIXTURE[name + "_lists"])


def _per_user(ev):
    values = ev.per_user_values()
    return np.stack([values[cutoff][DS] for cutoff in ev.cutoff_list], axis=1)


def _same(a, b, metrics=METRICS_WITH_DIVERSITY):
    assert list(a) == list(b)
    for cutoff in a:
        assert list(a[cutoff]) == list(b[cutoff]) == metrics
        for metric in metrics:
            x, y = a[cutoff][metric], b[cutoff][metric]
            assert x == y or (math.isnan(x) and math.isnan(y)), (cutoff, metric, x, y)


def _same_eighteen(plain, with_object):
    """The metrics of an evaluator without the object, bit for bit, in the same order around the new key."""
    assert list(plain) == list(with_object)
    for cutoff in plain:
        assert list(plain[cutoff]) == METRICS == [m for m in with_object[cutoff] if m != DS]
        for metric in METRICS:
            x, y = plain[cutoff][metric], with_object[cutoff][metric]
            assert x == y or (math.isnan(x) and math.isnan(y)), (cutoff, metric, x, y)


def _check_against_restatement_and_reference(name, results, per_user):
    D, lists, cutoffs = FIXTURE[name + "_D"], FIXTURE[name + "_lists"], FIXTURE[name + "_cutoffs"].tolist()
    want = diversity_per_user(D, lists, cutoffs)
    L = list_lengths(lists, cutoffs).astype(np.float64)
    print(name, "worst per-user error over its bound:", np.max(np.abs(per_user - want) / (4 * L ** 2 * EPS * want)))
    assert np.all(np.abs(per_user - want) <= 4 * L ** 2 * EPS * want)
    got = np.array([results[cutoff][DS] for cutoff in cutoffs])
    mean = np.array([math.fsum(want[:, c]) for c in range(len(cutoffs))]) / len(want)
    assert np.all(np.abs(got - mean) <= (4 * L.max(axis=0) ** 2 + len(want)) * EPS * mean)
    per_user_bound, metric_bound = reference_bounds(name)
    ref = FIXTURE[name + "_per_user"]
    assert np.all(np.abs(per_user - ref) <= per_user_bound * np.abs(ref))
    assert np.all(np.abs(got - FIXTURE[name + "_metric"]) <= metric_bound * FIXTURE[name + "_metric"])


# ---- 1. the lists path against the fixture ------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def replayed(gpu):
    """The fixture's lists of every holdout case through the lists path, once: evaluator, results, text, per-user values."""
    out = {}
    for name in HOLDOUT:
        ev = _evaluator(name)
        assert np.array_equal(ev.users_to_evaluate, FIXTURE[name + "_users"])
        results, text = ev.evaluateRecommender(_fixed(name))
        out[name] = (ev, results, text, _per_user(ev))
    return out


@pytest.mark.gpu
@pytest.mark.parametrize("name", HOLDOUT)
def test_lists_path_matches_the_restatement_and_the_reference(replayed, name):
    ev, results, text, per_user = replayed[name]
    _check_against_restatement_and_reference(name, results, per_user)
    cutoffs = make_case(name)["cutoffs"]
    assert list(results) == cutoffs and all(list(results[c]) == METRICS_WITH_DIVERSITY for c in cutoffs)
    assert "AVERAGE_POPULARITY: %.7f, DIVERSITY_SIMILARITY: %.7f, DIVERSITY_MEAN_INTER_LIST: " % (
        results[cutoffs[0]]["AVERAGE_POPULARITY"], results[cutoffs[0]][DS]) in text.split("\n")[0]
    assert set(ev.per_user_values()[cutoffs[0]]) == set(PER_USER) | {DS}


@pytest.mark.gpu
@pytest.mark.parametrize("name", HOLDOUT)
def test_the_other_metrics_are_those_of_an_evaluator_without_the_object(replayed, name):
    _, results, _, _ = replayed[name]
    plain = _evaluator(name, diversity=False)
    without, text = plain.evaluateRecommender(_fixed(name))
    assert all(list(without[c]) == METRICS for c in without) and DS not in text
    assert set(plain.per_user_values()[plain.cutoff_list[0]]) == set(PER_USER)
    _same_eighteen(without, results)


@pytest.mark.gpu
def test_a_list_of_exactly_two_items_is_computed(replayed):
    for name in HOLDOUT:
        lists, D = FIXTURE[name + "_lists"], FIXTURE[name + "_D"].astype(np.float64)
        two = np.flatnonzero((lists >= 0).sum(axis=1) == 2)
        assert len(two) == 4
        for r in two:
            a, b = lists[r, :2]
            assert np.all(replayed[name][3][r] == D[a, b] / 2)            # one cell: the last position gives no row


# ---- 2. fused path = lists path, for each scorer type ---------------------------------------------------------------------------------
WIDE_CUTOFFS = [10, 2, 65, 64, 130]


@pytest.fixture(scope="module")
def binary(gpu):
    """The `binary` case of tests/eval_cases.py (exact-grid models: no list depends on rounding), a float64 matrix, one evaluator."""
    case = make_eval_case("binary")
    n_items = case["train"].shape[1]
    D = np.random.default_rng(11).random((n_items, n_items))
    ev = EvaluatorHoldout_MI355X(case["test"], WIDE_CUTOFFS, verbose=False, diversity_object=D)
    return case, D, ev


def _recommender(kind, case):
    if kind == "factor":
        return set_model(_MF(case["train"], verbose=False), case["models"]["mf_bias"])
    if kind == "sparse_exact":
        rec = set_model(_ItemSim(case["train"], verbose=False), case["models"]["item"])
        rec.sparse_scoring = "exact"
        return rec
    if kind == "dense":
        rec = EASE_R_MI355X_Recommender(sps.csr_matrix(case["train"], dtype=np.float32), verbose=False, dense_scoring="device")
        rec.fit(topK=None, l2_norm=20.0, verbose=False)
        return rec
    rec = TopPop(case["train"], verbose=False)
    rec.fit()
    return rec


@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["factor", "sparse_exact", "dense", "item_vector"])
def test_fused_path_equals_lists_path_bitwise(binary, kind, monkeypatch):
    case, D, ev = binary
    rec = _recommender(kind, case)
    calls = []
    real = ev._run_fused
    monkeypatch.setattr(ev, "_run_fused", lambda scorer, add, *a: (calls.append(add), real(scorer, add, *a))[1])
    fused, fused_text = ev.evaluateRecommender(rec)
    fused_users = _per_user(ev)
    assert calls == [{"factor": "add_scorer", "sparse_exact": "add_spscorer", "dense": "add_dscorer", "item_vector": "add_itemscorer"}[kind]]
    lists, lists_text = ev.evaluateRecommender(_ListsOnly(rec))
    assert len(calls) == 1
    _same(fused, lists)
    assert fused_text == lists_text and np.array_equal(fused_users, _per_user(ev))
    assert np.all(fused_users > 0) and np.all(fused_users <= 1)
    if kind == "factor":                                    # the device's lists, read back, against the restatement
        table = np.full((len(ev.users_to_evaluate), ev.width), -1, np.int32)
        for r, items in enumerate(rec.recommend(ev.users_to_evaluate, cutoff=ev.width, remove_seen_flag=True)):
            table[r, :len(items)] = items
        want = diversity_per_user(D, table, WIDE_CUTOFFS)
        L = list_lengths(table, WIDE_CUTOFFS).astype(np.float64)
        assert np.all(np.abs(fused_users - want) <= 4 * L ** 2 * EPS * want)


# ---- 3. block sizes and repeats --------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_block_sizes_and_repeats_give_the_same_bits(binary):
    case, _, ev = binary
    rec = _recommender("factor", case)
    first, _ = ev.evaluateRecommender(rec)
    users = _per_user(ev)
    for block in (None, 1, 7, len(ev.users_to_evaluate)):
        again, _ = ev.evaluateRecommender(rec, block_size=block)
        _same(first, again)
        assert np.array_equal(users, _per_user(ev)), block
    for block in (1, 7):
        again, _ = ev.evaluateRecommender(_ListsOnly(rec), block_size=block)
        _same(first, again)
        assert np.array_equal(users, _per_user(ev)), block


# ---- 4. short lists ---------------------------------------------------------------------------------------------------------------------
def _tiny(n_users=5, n_items=6, seen_by_user_0=5):
    rng = np.random.default_rng(3)
    train = np.zeros((n_users, n_items), np.float32)
    test = np.zeros((n_users, n_items), np.float32)
    train[0, :seen_by_user_0] = 1
    test[0, n_items - 1] = 1
    for u in range(1, n_users):
        train[u, rng.permutation(n_items)[:2]] = 1
        test[u, np.flatnonzero(train[u] == 0)[0]] = 1
    rec = _MF(sps.csr_matrix(train), verbose=False)
    rec.USER_factors = rng.integers(-8, 9, (n_users, 4)).astype(np.float32)
    rec.ITEM_factors = rng.integers(-8, 9, (n_items, 4)).astype(np.float32)
    return sps.csr_matrix(train), sps.csr_matrix(test), rec, rng.random((n_items, n_items))


@pytest.mark.gpu
def test_a_user_with_one_admissible_item_raises_zero_division(gpu):
    train, test, rec, D = _tiny()
    for path in (rec, _ListsOnly(rec)):
        ev = EvaluatorHoldout_MI355X(test, [2, 3], verbose=False, diversity_object=D)
        with pytest.raises(ZeroDivisionError, match="fewer than two items met a diversity_object"):
            ev.evaluateRecommender(path)
        short = _per_user(ev)
        assert np.isnan(short[0]).all() and not np.isnan(short[1:]).any()
    # two admissible items: computed
    train, test, rec, D = _tiny(seen_by_user_0=4)
    ev = EvaluatorHoldout_MI355X(test, [2, 3], verbose=False, diversity_object=D)
    results, _ = ev.evaluateRecommender(rec)
    a, b = rec.recommend(np.array([0]), cutoff=3, remove_seen_flag=True)[0]
    assert np.all(_per_user(ev)[0] == D[a, b] / 2) and 0 < results[3][DS] <= 1
    # without the object the same evaluation is fine
    assert EvaluatorHoldout_MI355X(_tiny()[1], [2, 3], verbose=False).evaluateRecommender(_tiny()[2])[0][2]["PRECISION"] >= 0


@pytest.mark.gpu
def test_a_cutoff_of_one_raises_zero_division(gpu):
    name = HOLDOUT[0]
    case = make_case(name)
    ev = EvaluatorHoldout_MI355X(case["test"], [5, 1], verbose=False, diversity_object=case["D"])
    with pytest.raises(ZeroDivisionError, match=r"fewer than two items met a diversity_object \(cutoffs \[1\]\)"):
        ev.evaluateRecommender(_fixed(name))
    values = _per_user(ev)
    assert np.isnan(values[:, 1]).all() and not np.isnan(values[:, 0]).any()


@pytest.mark.gpu
def test_no_evaluated_user_gives_zero(gpu):
    name = HOLDOUT[0]
    case = make_case(name)
    ev = EvaluatorHoldout_MI355X(case["test"], case["cutoffs"], verbose=False, diversity_object=case["D"], min_ratings_per_user=1000)
    assert len(ev.users_to_evaluate) == 0
    results, text = ev.evaluateRecommender(_fixed(name))
    assert all(list(results[c]) == METRICS_WITH_DIVERSITY and results[c][DS] == 0.0 for c in case["cutoffs"])
    assert "DIVERSITY_SIMILARITY: 0.0000000" in text and _per_user(ev).shape == (0, len(case["cutoffs"]))


# ---- 5. matrix storage and layout ------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_float32_and_fortran_ordered_matrices(replayed):
    name = "holdout_f32"
    case = make_case(name)
    _, results32, _, users32 = replayed[name]
    assert case["D"].dtype == np.float32
    as64 = EvaluatorHoldout_MI355X(case["test"], case["cutoffs"], verbose=False, diversity_object=case["D"].astype(np.float64))
    results64, _ = as64.evaluateRecommender(_fixed(name))
    users64 = _per_user(as64)
    L = list_lengths(FIXTURE[name + "_lists"], case["cutoffs"]).astype(np.float64)
    assert np.all(np.abs(users32 - users64) <= 4 * L ** 2 * EPS * users64)
    for c in case["cutoffs"]:
        assert abs(results32[c][DS] - results64[c][DS]) <= (4 * L.max() ** 2 + len(L)) * EPS * results64[c][DS]
    name = "holdout_f64"
    case = make_case(name)
    fortran = np.asfortranarray(case["D"])
    assert not fortran.flags["C_CONTIGUOUS"]
    ev = EvaluatorHoldout_MI355X(case["test"], case["cutoffs"], verbose=False, diversity_object=_Diversity(fortran))
    _same(ev.evaluateRecommender(_fixed(name))[0], replayed[name][1])
    assert np.array_equal(_per_user(ev), replayed[name][3])


# ---- 6. the negative-sample evaluator ---------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_negative_sample_evaluator_on_both_paths(gpu, monkeypatch):
    name = "negative_f64"
    case = make_case(name)
    ev = _evaluator(name)
    assert np.array_equal(ev.users_to_evaluate, FIXTURE[name + "_users"]) and ev.candidates_on_device
    rec = set_model(_MF(case["train"], verbose=False), case["model"])
    calls = []
    real = ev._run_fused
    monkeypatch.setattr(ev, "_run_fused", lambda scorer, add, *a: (calls.append(add), real(scorer, add, *a))[1])
    fused, _ = ev.evaluateRecommender(rec)
    assert calls == ["add_scorer_candidates"]
    fused_users = _per_user(ev)
    _check_against_restatement_and_reference(name, fused, fused_users)
    lists, _ = ev.evaluateRecommender(_ListsOnly(rec))                      # recommend() per user, the lists of a block uploaded
    assert len(calls) == 1
    _same(fused, lists)
    assert np.array_equal(fused_users, _per_user(ev))
    ref = FIXTURE[name + "_dict"]                                           # the reference's other metrics, as the existing tests bound them
    for c, cutoff in enumerate(case["cutoffs"]):
        for m, metric in enumerate(METRICS):
            rtol = len(fused_users) * 2.0 ** -24 if metric in FLOAT32_ACCUMULATED else 1e-9
            assert fused[cutoff][metric] == pytest.approx(ref[c, m], rel=rtol, abs=1e-300), (cutoff, metric)
    plain, _ = _evaluator(name, diversity=False).evaluateRecommender(rec)
    _same_eighteen(plain, fused)


# ---- 7. refusals -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_values_outside_the_range_are_refused_on_the_device(gpu, dtype):
    name = HOLDOUT[0]
    case = make_case(name)
    ev = EvaluatorHoldout_MI355X(case["test"], case["cutoffs"], verbose=False)
    good = np.ascontiguousarray(case["D"], dtype=dtype)
    for value in (1.5, np.nan, -0.1, np.inf):
        bad = good.copy()
        bad[-1, -1] = value
        with pytest.raises(ValueError, match="item_diversity_matrix contains value greater than 1.0 or lower than 0.0: 1 cells"):
            ev._call("set_diversity", N.ptr(bad), bad.dtype.itemsize)
        with pytest.raises(ValueError, match="item_diversity_matrix contains value"):
            EvaluatorHoldout_MI355X(case["test"], case["cutoffs"], verbose=False, diversity_object=bad)
    with pytest.raises(ValueError, match="cells of 2 bytes"):
        ev._call("set_diversity", N.ptr(good), 2)
    edge = good.copy()
    edge[0, 0], edge[1, 1] = 0.0, 1.0
    ev._call("set_diversity", N.ptr(edge), edge.dtype.itemsize)             # the ends of the range are inside
    ev._call("set_diversity", None, 0)                                      # and NULL takes the matrix away


@pytest.mark.gpu
def test_lists_wider_than_1024_are_refused(gpu):
    n_items = 1030
    test = sps.csr_matrix((np.ones(3, np.float32), (np.arange(3), np.arange(3))), shape=(3, n_items))
    D = np.zeros((n_items, n_items), np.float32)
    with pytest.raises(NotImplementedError, match="lists of 1025 entries: at most 1024"):
        EvaluatorHoldout_MI355X(test, [10, 1025], verbose=False, diversity_object=D)
    with pytest.raises(NotImplementedError, match="lists of 1025 entries: at most 1024"):
        EvaluatorNegativeItemSample_MI355X(test, test, [10, 1025], verbose=False, diversity_object=D)
    plain = EvaluatorHoldout_MI355X(test, [10, 1025], verbose=False)
    with pytest.raises(NotImplementedError, match="lists of 1025 entries: at most 1024"):
        plain._call("set_diversity", N.ptr(D), 4)
    EvaluatorHoldout_MI355X(test, [10, 1024], verbose=False, diversity_object=D)


# ---- 8. one evaluator, several recommenders ---------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_an_evaluator_used_twice_gives_each_recommender_its_own_result(replayed):
    name = "holdout_f64"
    case = make_case(name)
    ev, first, _, first_users = replayed[name]
    users, lists = FIXTURE[name + "_users"], FIXTURE[name + "_lists"]
    other = lists.copy()
    for row in other:                                       # the same items in reverse order, two items fewer where there are four
        n = (row >= 0).sum()
        keep = n - 2 if n >= 4 else n
        row[:keep] = row[:n][::-1][:keep]
        row[keep:] = -1
    second, _ = ev.evaluateRecommender(_FixtureLists(case["train"], users, other))
    second_users = _per_user(ev)
    want = diversity_per_user(case["D"], other, case["cutoffs"])
    L = list_lengths(other, case["cutoffs"]).astype(np.float64)
    assert np.all(np.abs(second_users - want) <= 4 * L ** 2 * EPS * want)
    assert not np.array_equal(second_users, first_users)
    third, _ = ev.evaluateRecommender(_fixed(name))
    _same(first, third)
    assert np.array_equal(_per_user(ev), first_users)
