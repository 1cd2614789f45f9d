"""The device ranking against its exact contract (tests/ranking_cases.py): the list of a row is the `cutoff`
best finite scores, value descending, ties towards the lower item id, -1 padded -- whichever route produced it.  No tolerance
anywhere in this module: given the filtered float32 row the device returns, the list is determined (`exact_ranking`), and with
integer-valued models or rows realised through identity operands the host predicts the scores bit for bit as well.  Every row of
every batch is checked."""
import numpy as np
import pytest
import scipy.sparse as sps

import ranking_cases as R
from recsys2019_deeplearning_evaluation_amd import (GpuScoringMixin, GpuSimilarityScoringMixin, MI355XScorer,
                                                    MI355XSparseScorer)
from recsys2019_deeplearning_evaluation_amd import recommender_base as RB
from recsys2019_deeplearning_evaluation_amd.synthetic import named_urm

pytestmark = pytest.mark.gpu

KINDS = ("dense", "sparse")


def _same_bits(got, want):
    return got.shape == want.shape and got.dtype == want.dtype == np.float32 and got.tobytes() == want.tobytes()


def _assert_lists(ranked, want, what):
    """Row by row, so that a failure names the row and the first position that differs."""
    assert ranked.shape == want.shape and ranked.dtype == np.int32, what
    for r in np.flatnonzero((ranked != want).any(axis=1)):
        at = int(np.flatnonzero(ranked[r] != want[r])[0])
        raise AssertionError("%s: row %d differs from position %d: device %s, expected %s"
                             % (what, r, at, ranked[r][at:at + 8].tolist(), want[r][at:at + 8].tolist()))


def _realise(rows, kind):
    """(scorer, item mask) whose scores for users 0 .. len(rows) - 1 are `rows`."""
    allowed, seen = R.split_filters(rows)
    if kind == "dense":
        return MI355XScorer(*R.realise_dense(rows), seen), allowed
    return MI355XSparseScorer(*R.realise_sparse(rows), seen), allowed


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("case", R.CASES, ids=lambda c: c.name)
def test_row_case_is_ranked_exactly(gpu, case, kind):
    """Every named case and every size x cut-off of the sweep, through both scorers: scores equal the rows bit for bit, -inf exactly
    where a filter applies, the list is the oracle's, `return_scores=False` (the evaluator's variant) gives the same list, and so
    does the same row filtered by the item mask instead of the seen items (batch of one, mask after no mask after mask)."""
    rows = R.case_rows(case)
    want = R.exact_rankings(rows, case.cutoff)
    sc, allowed = _realise(rows, kind)
    users = np.arange(len(rows))
    ranked, scores = sc.recommend(users, case.cutoff, remove_seen=True, allowed_items=allowed, return_scores=True)
    assert _same_bits(scores, rows)
    _assert_lists(ranked, R.exact_rankings(scores, case.cutoff), "self-consistency")
    _assert_lists(ranked, want, "host rows")
    quiet, none = sc.recommend(users, case.cutoff, remove_seen=True, allowed_items=allowed, return_scores=False)
    assert none is None
    _assert_lists(quiet, want, "return_scores=False")
    for r in np.flatnonzero((rows == -np.inf).any(axis=1)):
        mask = (rows[r] > -np.inf).astype(np.uint8)
        one, s = sc.recommend([r], case.cutoff, remove_seen=False, allowed_items=mask, return_scores=True)
        assert _same_bits(s, rows[r:r + 1])
        _assert_lists(one, want[r:r + 1], "item mask, row %d" % r)
        one, _ = sc.recommend([r], case.cutoff, remove_seen=True, allowed_items=allowed)
        _assert_lists(one, want[r:r + 1], "seen items after a mask, row %d" % r)
    sc.close()


@pytest.mark.parametrize("use_bias", [False, True])
@pytest.mark.parametrize("k", [7, 64])
def test_gaussian_factor_models_are_self_consistent(gpu, k, use_bias):
    """The continuous inputs of tests/test_scoring_gpu.py: whatever float32 scores the device returns, its list is the exact ranking of
    them -- and the list does not depend on whether the scores are written back."""
    X = named_urm("ml1m", "binary", scale=0.3)
    rng = np.random.default_rng(k)
    U = rng.normal(0, 0.3, (X.shape[0], k)).astype(np.float32); V = rng.normal(0, 0.3, (X.shape[1], k)).astype(np.float32)
    bias = (rng.normal(size=X.shape[0]).astype(np.float32), rng.normal(size=X.shape[1]).astype(np.float32), 0.7) if use_bias else ()
    sc = MI355XScorer(U, V, X, *bias)
    users = rng.choice(X.shape[0], 333, replace=False)
    allowed = (rng.random(X.shape[1]) < 0.5).astype(np.uint8)
    for cutoff, mask in ((25, None), (256, None), (257, allowed), (1025, None), (X.shape[1], allowed)):
        ranked, scores = sc.recommend(users, cutoff, remove_seen=True, allowed_items=mask, return_scores=True)
        assert not np.isnan(scores).any()
        for r, u in enumerate(users):
            blocked = np.zeros(X.shape[1], bool)
            blocked[X.indices[X.indptr[u]:X.indptr[u + 1]]] = True
            if mask is not None:
                blocked |= mask == 0
            assert ((scores[r] == -np.inf) == blocked).all()
        _assert_lists(ranked, R.exact_rankings(scores, ranked.shape[1]), "cutoff %d" % cutoff)
        quiet, _ = sc.recommend(users, cutoff, remove_seen=True, allowed_items=mask)
        _assert_lists(quiet, ranked, "return_scores=False, cutoff %d" % cutoff)
    sc.close()


@pytest.mark.parametrize("user_based", [False, True])
def test_gaussian_similarity_models_are_self_consistent(gpu, user_based):
    """Continuous similarity weights (no statement about `return_scores=False` here: the order of the float atomics may move a
    score by an ulp between two calls)."""
    X = named_urm("ml1m", "real", scale=0.2)
    n = X.shape[0] if user_based else X.shape[1]
    W = sps.random(n, n, 0.02, format="csr", random_state=7, dtype=np.float32)
    W.data[:] = np.random.default_rng(8).normal(size=W.nnz).astype(np.float32)
    sp = MI355XSparseScorer(*((W, X) if user_based else (X, W)), X)
    users = np.arange(0, X.shape[0], 3)
    for cutoff in (15, 300, X.shape[1]):
        ranked, scores = sp.recommend(users, cutoff, remove_seen=True, return_scores=True)
        assert not np.isnan(scores).any()
        _assert_lists(ranked, R.exact_rankings(scores, ranked.shape[1]), "cutoff %d" % cutoff)
    sp.close()


def _batches(n_users, rng):
    """Batch sizes {1, 127, 128, 129}: the special users first (one of them in the batch of one), then random users, with
    repeated ids."""
    special = np.array(R.SPECIAL_USERS)
    for size in (1, 127, 128, 129):
        users = rng.integers(0, n_users, size)
        if size == 1:
            users[0] = rng.choice(special)
        else:
            users[:len(special)] = special
            users[-3:] = users[len(special)]
        yield users


def _score_sequences(score_rows, lists, cutoff):
    """Scores along each list, padded with NaN: equal sequences <=> equal multisets, both lists being value-descending."""
    out = np.full((len(lists), cutoff), np.nan)
    for r, items in enumerate(lists):
        out[r, :len(items)] = score_rows[r, items]
    return out


@pytest.mark.parametrize("name", [m[0] for m in R.DENSE_MODELS])
def test_integer_factor_model(gpu, name):
    """Small-integer factors (and biases): the host knows the scores bit for bit.  Scorer object re-used across batch sizes and
    cut-offs; the recommender's `recommend()` against the host path of BaseRecommender.recommend by the scores along the lists."""
    cutoffs = next(m[5] for m in R.DENSE_MODELS if m[0] == name)
    m = R.dense_model(name)
    rng = np.random.default_rng(11)
    n_users, n_items = m["X"].shape
    sc = MI355XScorer(m["U"], m["V"], m["X"], *(m["bias"] or ()))
    allowed = (rng.random(n_items) < 0.3).astype(np.uint8)
    for cutoff in cutoffs:
        for users in _batches(n_users, rng):
            for remove_seen, mask in ((True, None), (False, allowed), (True, allowed)):
                host = R.apply_filters(R.dense_scores(m, users), m["X"], users, remove_seen, mask)
                want = R.exact_rankings(host, cutoff)
                ranked, scores = sc.recommend(users, cutoff, remove_seen=remove_seen, allowed_items=mask, return_scores=True)
                assert _same_bits(scores, host)
                _assert_lists(ranked, want, "cutoff %d, batch %d" % (cutoff, len(users)))
                quiet, _ = sc.recommend(users, cutoff, remove_seen=remove_seen, allowed_items=mask)
                _assert_lists(quiet, want, "return_scores=False, cutoff %d, batch %d" % (cutoff, len(users)))
    sc.close()
    rec = type("IntegerMF", (GpuScoringMixin, RB.BaseMatrixFactorizationRecommender), {})(m["X"], verbose=False)
    rec.USER_factors, rec.ITEM_factors = m["U"], m["V"]
    if m["bias"] is not None:
        rec.use_bias = True
        rec.USER_bias, rec.ITEM_bias, rec.GLOBAL_bias = m["bias"]
    users = np.arange(64)
    for cutoff in cutoffs:
        dev_lists, dev_scores = rec.recommend(users, cutoff=cutoff, return_scores=True)
        host_lists, host_scores = RB.BaseRecommender.recommend(rec, users, cutoff=cutoff, return_scores=True)
        assert _same_bits(dev_scores, host_scores.astype(np.float32))
        assert np.array_equal(_score_sequences(host_scores, dev_lists, cutoff), _score_sequences(host_scores, host_lists, cutoff), equal_nan=True)
    rec.invalidate_scorer()


@pytest.mark.parametrize("name", [m[0] for m in R.SPARSE_MODELS])
def test_integer_similarity_model(gpu, name):
    """ItemKNN and UserKNN operand order with small-integer ratings and weights, negative ones included; the special users are the
    empty profile (list = the lowest admissible ids), the users with 1, 3, 4 and 19 non-zero scores (down to one, up to one fewer
    than the cut-offs 5 and 20), and the user whose seen items cover all non-zero scores."""
    cutoffs = next(m[5] for m in R.SPARSE_MODELS if m[0] == name)
    m = R.sparse_model(name)
    rng = np.random.default_rng(12)
    n_users, n_items = m["X"].shape
    sp = MI355XSparseScorer(m["A"], m["B"], m["X"])
    allowed = (rng.random(n_items) < 0.3).astype(np.uint8)
    for cutoff in cutoffs:
        for users in _batches(n_users, rng):
            for remove_seen, mask in ((True, None), (False, allowed), (True, allowed)):
                host = R.apply_filters(R.sparse_scores(m, users), m["X"], users, remove_seen, mask)
                want = R.exact_rankings(host, cutoff)
                ranked, scores = sp.recommend(users, cutoff, remove_seen=remove_seen, allowed_items=mask, return_scores=True)
                assert _same_bits(scores, host)
                _assert_lists(ranked, want, "cutoff %d, batch %d" % (cutoff, len(users)))
                quiet, _ = sp.recommend(users, cutoff, remove_seen=remove_seen, allowed_items=mask)
                _assert_lists(quiet, want, "return_scores=False, cutoff %d, batch %d" % (cutoff, len(users)))
                for r in np.flatnonzero(users == 0):               # empty profile: zeros everywhere, the lowest admissible ids
                    assert ranked[r].tolist() == np.flatnonzero(host[r] > -np.inf)[:cutoff].tolist()
    sp.close()
    base = RB.BaseUserSimilarityMatrixRecommender if m["user_based"] else RB.BaseItemSimilarityMatrixRecommender
    rec = type("IntegerKNN", (GpuSimilarityScoringMixin, base), {"_SCORER_USER_BASED": m["user_based"]})(m["X"], verbose=False)
    rec.W_sparse = m["W"]
    users = np.arange(64)
    for cutoff in cutoffs:
        dev_lists, dev_scores = rec.recommend(users, cutoff=cutoff, return_scores=True)
        host_lists, host_scores = RB.BaseRecommender.recommend(rec, users, cutoff=cutoff, return_scores=True)
        assert _same_bits(dev_scores, host_scores.astype(np.float32))
        assert np.array_equal(_score_sequences(host_scores, dev_lists, cutoff), _score_sequences(host_scores, host_lists, cutoff), equal_nan=True)
    rec.invalidate_scorer()


@pytest.mark.parametrize("kind", KINDS)
def test_lists_do_not_depend_on_the_route_cutoff_4096_and_4097(gpu, kind):
    """One integer model at the last in-LDS cut-off and the first wide one: the common prefix of the lists is identical."""
    rng = np.random.default_rng(13)
    if kind == "dense":
        m = R.int_dense_model(40, 9000, 3, True, 21)
        sc = MI355XScorer(m["U"], m["V"], m["X"], *m["bias"])
        host = lambda users: R.dense_scores(m, users)
    else:
        m = R.int_sparse_model(40, 9000, False, 22, (1, 2, 3))
        sc = MI355XSparseScorer(m["A"], m["B"], m["X"])
        host = lambda users: R.sparse_scores(m, users)
    users = rng.permutation(40)[:24]
    assert R.fits_lds_rank(9000, 4096) and not R.fits_lds_rank(9000, 4097)
    in_lds, _ = sc.recommend(users, 4096, remove_seen=True)
    wide, _ = sc.recommend(users, 4097, remove_seen=True)
    _assert_lists(wide[:, :4096], in_lds, "wide against in-LDS")
    _assert_lists(wide, R.exact_rankings(R.apply_filters(host(users), m["X"], users), 4097), "wide against the host")
    sc.close()


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("cutoff", [20, 300, 4096])
def test_lists_do_not_depend_on_the_route_32256_and_32257_items(gpu, kind, cutoff):
    """The last catalogue that fits LDS, and the same rows with one always-masked item appended: in-LDS and wide lists are equal."""
    rows = R.case_rows(R.CASE_BY_NAME["sweep_n32256_c4096"])
    longer = np.concatenate([rows, np.full((len(rows), 1), -np.inf, np.float32)], axis=1)
    assert R.predict_route(rows[0], cutoff) != {"wide"} and R.predict_route(longer[0], cutoff) == {"wide"}
    users = np.arange(len(rows))
    lists = []
    for batch in (rows, longer):
        sc, allowed = _realise(batch, kind)
        ranked, scores = sc.recommend(users, cutoff, remove_seen=True, allowed_items=allowed, return_scores=True)
        assert _same_bits(scores, batch)
        lists.append(ranked)
        sc.close()
    assert allowed is not None and allowed[-1] == 0 and allowed[:-1].all()
    _assert_lists(lists[1], lists[0], "wide against in-LDS")
    _assert_lists(lists[0], R.exact_rankings(rows, cutoff), "in-LDS against the host")


@pytest.mark.parametrize("kind", KINDS)
def test_one_scorer_across_batches_cutoffs_routes_and_masks(gpu, kind):
    """Buffer regrowth and the wide ranker's offsets: one scorer object, batches growing then shrinking, cut-offs (and with them the
    in-LDS / wide route) changing, a mask, then none, then another one; repeated user ids in every batch."""
    rng = np.random.default_rng(14)
    if kind == "dense":
        m = R.int_dense_model(200, 6000, 3, False, 31)
        sc = MI355XScorer(m["U"], m["V"], m["X"])
        host = lambda users: R.dense_scores(m, users)
    else:
        m = R.int_sparse_model(200, 6000, True, 32, (1, 2))
        sc = MI355XSparseScorer(m["A"], m["B"], m["X"])
        host = lambda users: R.sparse_scores(m, users)
    mask_a = (rng.random(6000) < 0.5).astype(np.uint8)
    mask_b = (rng.random(6000) < 0.01).astype(np.uint8)
    steps = [(1, 20, None), (127, 20, mask_a), (128, 300, None), (129, 4097, mask_b), (40, 6000, None), (129, 20, mask_a),
             (128, 4097, None), (127, 5999, mask_b), (1, 4097, mask_a), (129, 2, None), (1, 1, mask_b)]
    for size, cutoff, mask in steps:
        users = rng.integers(0, 200, size)
        users[-1] = users[0]
        want_scores = R.apply_filters(host(users), m["X"], users, True, mask)
        want = R.exact_rankings(want_scores, cutoff)
        what = "batch %d, cutoff %d, %s" % (size, cutoff, "no mask" if mask is None else "mask of %d" % mask.sum())
        ranked, scores = sc.recommend(users, cutoff, remove_seen=True, allowed_items=mask, return_scores=True)
        assert _same_bits(scores, want_scores), what
        _assert_lists(ranked, want, what)
        quiet, _ = sc.recommend(users, cutoff, remove_seen=True, allowed_items=mask)
        _assert_lists(quiet, want, what + ", return_scores=False")
    sc.close()
