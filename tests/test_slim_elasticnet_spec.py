"""SLIM ElasticNet: the specification the device fit implements, pinned on the CPU (no GPU needed).

The reference (SLIM_ElasticNet/SLIMElasticNetRecommender.py:41-149) runs sklearn's sparse coordinate descent once per item.  The
replay below is the same solver in Gram form, float64 NumPy: shared G = X^T X, H = G w, sklearn's xorshift coordinate sequence per
target (one seed per item from NumPy's global RandomState), the duality-gap stop test, and the reference's selection rule
local_topK = min(nnz - 1, topK).  It is evaluated the way the device kernel evaluates it -- a window of draws against the same H,
accept up to the first draw whose value changes -- which is exact because H only moves when w does.  Checked against
tests/golden/slim_elasticnet.npz (made by tests/golden/make_slim_elasticnet_fixture.py from the reference with scikit-learn)."""
import json
import os

import numpy as np
import scipy.sparse as sps

import slim_elasticnet_cases as cases
from slim_elasticnet_cases import RAND_R_MAX, coordinate_sweep, replay_target, select  # noqa: F401 (the oracle lives with the case builders)

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "slim_elasticnet.npz")


def load_cases():
    z = np.load(GOLDEN, allow_pickle=False)
    cases = json.loads(str(z["cases"]))

    def csr(prefix):
        shape = tuple(int(x) for x in z[prefix + "_shape"])
        return sps.csr_matrix((z[prefix + "_data"], z[prefix + "_indices"], z[prefix + "_indptr"]), shape=shape)

    out = []
    for n, case in enumerate(cases):
        out.append(dict(case, X=csr("X_" + case["urm"]), W=csr("W_%d" % n), n_iter=z["n_iter_%d" % n], after=float(z["after_%d" % n])))
    return out


def replay_fit(X, seed, l1_ratio, alpha, positive_only, topK):
    X = sps.csc_matrix(X, dtype=np.float64)
    n_users, n_items = X.shape
    G = (X.T @ X).toarray()
    d = np.asarray(X.multiply(X).sum(axis=0)).ravel()
    l1, l2 = alpha * l1_ratio * n_users, alpha * (1.0 - l1_ratio) * n_users
    np.random.seed(seed)
    seeds = np.random.randint(0, RAND_R_MAX, size=n_items)
    W = np.zeros((n_items, n_items))
    n_iter = np.zeros(n_items, np.int64)
    for j in range(n_items):
        w, n_iter[j], _, _ = replay_target(G, d, j, int(seeds[j]), l1, l2, positive_only)
        keep = select(w, topK)
        W[keep, j] = w[keep]
    return W, n_iter, np.random.rand()


def test_seed_draws_match_one_by_one_draws():
    """np.random.randint(0, 2**31 - 1, size=N) = N scalar draws, and leaves the global state in the same place."""
    np.random.seed(123)
    a = np.random.randint(0, RAND_R_MAX, size=57)
    after_a = np.random.rand()
    np.random.seed(123)
    b = np.array([np.random.randint(0, RAND_R_MAX) for _ in range(57)])
    assert (a == b).all() and np.random.rand() == after_a


def test_gram_replay_reproduces_the_reference_fixtures():
    for n, case in enumerate(load_cases()):
        W, n_iter, after = replay_fit(case["X"], case["seed"], case["l1_ratio"], case["alpha"], case["positive_only"], case["topK"])
        want = case["W"].toarray()
        assert after == case["after"], n
        assert ((W != 0) == (want != 0)).all(), (n, int(((W != 0) != (want != 0)).sum()))
        scale = np.maximum(np.abs(want).max(axis=0), 1e-30)
        assert (np.abs(W - want).max(axis=0) <= 1e-5 * scale).all(), (n, (np.abs(W - want).max(axis=0) / scale).max())
        same = n_iter == case["n_iter"]
        assert same.mean() >= 0.9 and (np.abs(n_iter - case["n_iter"]) <= 1).all(), (n, same.mean())


# ---- the one- and two-sweep cases of test_slim_elasticnet_sequence_gpu.py: what their bar can and cannot see ----------------------------
import pytest  # noqa: E402

SWEEP_GRID = [(n, "binary") for n in cases.SWEEP_N_ITEMS] + [(1300, "random")]


@pytest.mark.parametrize("n_items,values", SWEEP_GRID)
def test_float32_model_meets_a_tenth_of_the_one_sweep_bar(n_items, values):
    """Honest float32 rounding (the float32 host model against the float64 replay, same cases, same targets) stays below a tenth of
    the device tests' bar and leaves support, n_iter and converged alone.  Worst over all cases: 5.33e-6 of a column's max after one
    sweep (n_items = 1023, signed), 1.48e-5 after two (n_items = 1300, non-quantised values, signed)."""
    for params in cases.SWEEP_PARAMS:
        for max_iter in (1, 2):
            want = cases.sweep_case(n_items, params, max_iter, values)
            got = cases.sweep_case(n_items, params, max_iter, values, "float32")
            worst = 0.0
            for t, (w, n_iter, conv, changes) in want.items():
                w32, n_iter32, conv32, changes32 = got[t]
                assert ((w32 != 0) == (w != 0)).all() and (n_iter32, conv32) == (n_iter, conv), (params, max_iter, t)
                assert w[t] == 0 and (n_iter == max_iter or conv)
                worst = max(worst, cases.column_error(w32, w))
            print("n_items %d %s %s max_iter %d: float32 model err / column max %.2e" % (n_items, values, params, max_iter, worst))
            assert worst <= cases.SWEEP_BAR[max_iter] / 10, (params, max_iter, worst)
    assert max(cases.SWEEP_BAR.values()) <= 1e-3


@pytest.mark.parametrize("n_items", [n for n in cases.SWEEP_N_ITEMS if n >= 511])
def test_wrong_sequences_break_the_one_sweep_bar(n_items):
    """The condition that keeps the device test honest: a fit of one or two sweeps over a wrong coordinate sequence leaves the bar on
    every live target.  Parameter set "signed" (l1 = 0: every drawn live coordinate becomes nonzero, so every draw counts); the
    smallest effect is 3.6e-3 of a column's max (rotated tail, n_items = 1300, one sweep), 24 times the two-sweep bar."""
    live = [t for t in cases.sweep_targets(n_items) if t != cases.empty_item_of(n_items)]
    for name, (_, first_n) in cases.WRONG_SEQUENCES.items():
        if n_items < first_n:
            continue
        for max_iter in (1, 2):
            want = cases.sweep_case(n_items, "signed", max_iter)
            wrong = cases.sweep_case(n_items, "signed", max_iter, "binary", "float64", name)
            effect = [cases.column_error(wrong[t][0], want[t][0]) for t in live]
            print("n_items %d %s max_iter %d: smallest effect %.2e" % (n_items, name, max_iter, min(effect)))
            assert min(effect) > cases.SWEEP_BAR[max_iter], (name, max_iter, effect)


def test_wrong_sequences_differ_from_the_true_one_only_where_they_say():
    true, state = coordinate_sweep(12345, 1300)
    for name, (seq, first_n) in cases.WRONG_SEQUENCES.items():
        c, s = seq(12345, 1300)
        assert s == state and (c != true).any(), name
        assert (seq(12345, first_n - 1)[0] == coordinate_sweep(12345, first_n - 1)[0]).all(), name
    assert (np.flatnonzero(cases.rotated_tail(12345, 1300)[0] != true) >= 1260).all()
    assert set(np.flatnonzero(cases.early_wave3(12345, 1300)[0] != true) % 512 // 64) == {3}
    assert (cases.restarted_second_window(12345, 1300)[0][512:1024] == true[:512]).all()


def test_replay_on_a_sparse_gram_equals_the_dense_one():
    X = cases.urm(65)
    G, d = cases.gram64(X)
    Xc = sps.csc_matrix(X, dtype=np.float64)
    Gs = sps.csc_matrix(Xc.T @ Xc)
    l1, l2 = cases.penalties(X, 0.01, 0.1)
    for dtype in (np.float64, np.float32):
        for j in (0, 31, 64):
            a = replay_target(G, d, j, 99 + j, l1, l2, True, max_iter=3, dtype=dtype)
            b = replay_target(Gs, d, j, 99 + j, l1, l2, True, max_iter=3, dtype=dtype)
            assert (a[0] == b[0]).all() and a[1:] == b[1:] and a[0].dtype == dtype


@pytest.mark.parametrize("n_items,params,max_iter", [(65, "signed", 2), (65, "positive", 100), (513, "signed", 1), (513, "positive", 3)])
def test_c_replay_equals_the_numpy_replay(n_items, params, max_iter):
    """oracle.c's one-draw-at-a-time replay (the reference of the device tests) is bit-equal to replay_target, which the fixture test
    above pins to the reference: from a Gram matrix, and from the URM alone (Gram columns formed on demand)."""
    from oracle import oracle as O
    X, kw = cases.urm(n_items, "int"), cases.SWEEP_PARAMS[params]
    G, d = cases.gram64(X)
    l1, l2 = cases.penalties(X, kw["alpha"], kw["l1_ratio"])
    seeds = cases.sweep_seeds(n_items)
    for t in cases.sweep_targets(n_items):
        w, n_iter, conv, changes = replay_target(G, d, t, int(seeds[t]), l1, l2, kw["positive_only"], max_iter=max_iter)
        for operands in (dict(G=G), dict(G=sps.csr_matrix(G)), dict(X=X)):
            w_c, *rest = O.slimen_replay(t, int(seeds[t]), l1, l2, kw["positive_only"], d, max_iter=max_iter, **operands)
            assert (w_c == w).all() and tuple(rest) == (n_iter, conv, changes), (t, list(operands), rest, (n_iter, conv, changes))


@pytest.mark.parametrize("values,params", sorted(cases.CONVERGED_TARGETS))
def test_converged_targets_have_a_sweep_count_the_reference_determines(values, params):
    """The rule behind cases.CONVERGED_TARGETS, and the converged bars of the device test on the float32 host model: the float64 replay
    runs the same number of sweeps with the tolerance a quarter lower and a quarter higher, the float32 model runs that number, keeps the
    same 100 coefficients and stays within 2e-4 of the column's max."""
    want, model = cases.converged_case(params, values), cases.converged_case(params, values, "float32")
    assert len(want) == 8 and cases.empty_item_of(cases.CONVERGED_N_ITEMS) not in want
    for tol in (0.8e-4, 1.25e-4):
        other = cases.converged_case(params, values, tol=tol)
        assert [other[t][1] for t in want] == [want[t][1] for t in want], tol
    assert [model[t][1:3] for t in want] == [want[t][1:3] for t in want]
    for t in want:
        keep = select(want[t][0], cases.CONVERGED_TOPK)
        assert set(select(model[t][0], cases.CONVERGED_TOPK)) == set(keep), t
        assert cases.column_error(model[t][0][keep], want[t][0][keep]) <= 2e-4, t


def test_seed_zero_is_seed_one_and_the_edge_seeds_are_in_the_cases():
    assert (coordinate_sweep(0, 100)[0] == coordinate_sweep(1, 100)[0]).all()
    for n in cases.SWEEP_N_ITEMS:
        seeds, targets = cases.sweep_seeds(n), cases.sweep_targets(n)
        assert seeds[0] == 0 and seeds[n - 1] == RAND_R_MAX - 1 and 0 in targets and n - 1 in targets
        assert cases.empty_item_of(n) is None or cases.empty_item_of(n) in targets
        X = cases.urm(n)
        assert X.shape[1] == n and X[5].nnz == 0
        empty = np.flatnonzero(np.diff(X.tocsc().indptr) == 0)
        assert list(empty) == ([] if n == 2 else [n // 2])


def test_tie_construction_is_exact_in_both_dtypes():
    """The known answer of the selection test: every coefficient is exactly 0.25, 0.125 or -0.125, in float32 and in float64, under two
    different draw orders; the tied indices span many of the device's per-thread ranges of three cells."""
    X, want = cases.tie_case()
    assert X.shape == (cases.TIE_N_USERS, cases.TIE_N_ITEMS)
    l1, l2 = cases.penalties(X, cases.TIE_PARAMS["alpha"], cases.TIE_PARAMS["l1_ratio"])
    assert (np.float32(l1), np.float32(l2)) == (1.0, 4.0)
    G, d = cases.gram64(X)
    where = np.flatnonzero(want)
    assert len(where) == 90 and (G[np.ix_(where, where)] == 4 * np.eye(90)).all() and d[0] == 190
    assert sorted(np.unique(want[where], return_counts=True)[1]) == [10, 40, 40]
    for value in (0.25, 0.125, -0.125):
        assert len(set(np.flatnonzero(want == value) // 3)) >= 10
    for dtype in (np.float64, np.float32):
        for seed in (7, 2 ** 31 - 2):
            w, n_iter, conv, _ = replay_target(G, d, 0, seed, l1, l2, False, dtype=dtype)
            assert conv and (w == want).all(), (dtype, seed)
    for topK in cases.TIE_TOPKS:
        keep = select(want, topK)
        assert len(keep) == min(89, topK) and len(set(keep)) == len(keep)
        cut = want[keep].min()
        tied = np.flatnonzero(want == cut)
        assert (np.sort(keep[want[keep] == cut]) == tied[:(want[keep] == cut).sum()]).all() and set(where[want[where] > cut]) <= set(keep)
