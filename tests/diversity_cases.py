"""DIVERSITY_SIMILARITY: a float64 restatement of the reference's formula (Base/Evaluation/metrics.py:664-680, written row by row as
the reference writes it) and the seeded cases of tests/golden/evaluator_diversity.npz (tests/golden/make_diversity_fixture.py runs
the reference's own evaluators on them, tests/test_evaluation_diversity_*.py rebuild the same inputs).

The matrices are random and ASYMMETRIC with a non-zero diagonal: a transposed index, an included diagonal and an included last row
each change the answer.  The holdout cases are evaluated on fixed lists (a recommender that answers with stored lists); the
negative-sample case on an exact-grid factor model of tests/eval_cases.py, so that the reference's recommender, the device scorer and
the host path of this package all give the same lists."""
import functools

import numpy as np

from eval_cases import _factors, _split
from negative_eval_cases import ALL, _admissible, _draw_negatives

CASES = ("holdout_f64", "holdout_f32", "negative_f64")
# unsorted, on both sides of the 64-lane edge, 130 above every list of holdout_f64's short users; [2, 3, 5] with lists of 2, 3 and 4
CUTOFFS = {"holdout_f64": [10, 2, 65, 64, 130], "holdout_f32": [2, 3, 5], "negative_f64": [5, 2, 30, 10]}
SEEDS = {"holdout_f64": 2026102101, "holdout_f32": 2026102102, "negative_f64": 2026102103}


# ---- the formula ------------------------------------------------------------------------------------------------------------------
def diversity_of_list(D, items):
    """Diversity_similarity.add_recommendations for one list, in float64: every row but the last one's, the row's own position
    zeroed, the sum divided by len * (len - 1).  Raises ZeroDivisionError for fewer than two items, as the reference does."""
    items = [int(i) for i in items]
    D = np.asarray(D)
    total = 0.0
    for index in range(len(items) - 1):
        row = D[items[index], items].astype(np.float64)
        row[index] = 0.0
        total += float(np.sum(row))
    return total / (len(items) * (len(items) - 1))


def diversity_per_user(D, table, cutoffs):
    """[n_lists][n_cutoffs] for a -1 padded table of lists."""
    out = np.zeros((len(table), len(cutoffs)))
    for r, row in enumerate(table):
        items = row[row >= 0]
        for c, cutoff in enumerate(cutoffs):
            out[r, c] = diversity_of_list(D, items[:cutoff])
    return out


def list_lengths(table, cutoffs):
    """[n_lists][n_cutoffs]: min(cutoff, list length)."""
    return np.minimum((np.asarray(table) >= 0).sum(axis=1)[:, None], np.asarray(cutoffs)[None, :])


# ---- the cases ----------------------------------------------------------------------------------------------------------------------
def _matrix(rng, n_items, dtype):
    D = rng.random((n_items, n_items), dtype=dtype)
    assert not np.allclose(D, D.T) and np.all(np.diag(D) > 0) and D.min() >= 0 and D.max() <= 1
    return D


def _fixed_lists(rng, train, width):
    """Per user a random order of the items outside its train row, cut at `width`; -1 padded."""
    X = train.toarray() != 0
    table = np.full((X.shape[0], width), -1, np.int32)
    for u in range(X.shape[0]):
        items = rng.permutation(np.flatnonzero(~X[u]))[:width]
        table[u, :len(items)] = items
    return table


@functools.lru_cache(maxsize=None)
def make_case(name):
    """dict(train, test, cutoffs, D, kwargs) and, for the holdout cases, lists (the fixed lists of ALL users, -1 padded); for the
    negative-sample case negative (URM_test_negative) and model (the attributes of a factor model)."""
    rng = np.random.default_rng(SEEDS[name])
    cutoffs = CUTOFFS[name]
    if name == "negative_f64":
        n_users, n_items = 150, 150
        n_test = rng.integers(1, 5, n_users)
        train, test = _split(rng, n_users, n_items, rng.integers(10, 30, n_users), n_test, False)
        from_train = np.where(np.arange(n_users) % 7 == 0, 3, 0)
        outside = np.full(n_users, 20)
        outside[:4] = 1                                     # users 0-3: two to five candidates, fewer than cutoffs 5, 10 and 30
        n_items_free = n_items - np.ediff1d(train.indptr) - n_test
        assert np.all(outside <= n_items_free)
        negative = _draw_negatives(rng, train, test, outside, from_train, np.zeros(n_users, np.int64))
        admissible = _admissible(train, test, negative, {})
        assert admissible.sum(axis=1).min() >= 2
        return dict(train=train, test=test, negative=negative, cutoffs=cutoffs, kwargs={}, D=_matrix(rng, n_items, np.float64),
                    model=_factors(rng, n_users, n_items, 16, admissible, ALL, False))
    n_users, n_items, dtype = (120, 160, np.float64) if name == "holdout_f64" else (90, 150, np.float32)
    n_train = rng.integers(5, 25, n_users)
    n_test = rng.integers(1, 6, n_users)
    short = (2, 3, 64, 65, 100) if name == "holdout_f64" else (2, 3, 4)      # list lengths of the first users, four users each
    for g, length in enumerate(short):
        n_train[4 * g:4 * g + 4] = n_items - length
        n_test[4 * g:4 * g + 4] = 1
    train, test = _split(rng, n_users, n_items, n_train, n_test, False)
    lists = _fixed_lists(rng, train, min(max(cutoffs), n_items))
    assert (lists >= 0).sum(axis=1).min() == 2
    return dict(train=train, test=test, cutoffs=cutoffs, kwargs={}, D=_matrix(rng, n_items, dtype), lists=lists)
