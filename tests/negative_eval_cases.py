"""Seeded inputs of the negative-sample evaluator fixture (tests/golden/make_negative_evaluator_fixture.py writes the reference's
results for them, tests/test_evaluation_negative_*.py rebuild the same inputs): train / test split, the sampled negatives, evaluator
arguments and the models.  Everything is drawn, nothing stored.

The models are the exact-grid models of tests/eval_cases.py (every score exact in float32 whatever the order of its terms).  Ties
are removed among ALL admissible candidates of every user, not only above the list width: a user with fewer candidates than the
cutoff is ranked to the end of its row."""
import functools

import numpy as np
import scipy.sparse as sps

from eval_cases import CUTOFFS, SIM_UNIT, _factors, _item_similarity, _split, _untie, _user_similarity, set_model  # noqa: F401

CASES = ("sampled", "sampled_graded", "long_rows", "long_rows_over", "wide")
FOUR = ("mf", "mf_bias", "item", "user")
MODELS = {"sampled": FOUR, "sampled_graded": FOUR, "long_rows": ("mf",), "long_rows_over": ("mf",), "wide": ("mf", "item")}
ROW_LIMIT = 4096                    # the longest candidate row the device ranks
ALL = 1 << 30                       # "list width" for the tie removal: every admissible candidate
SEEDS = {"sampled": 2026101801, "sampled_graded": 2026101802, "long_rows": 2026101803, "long_rows_over": 2026101803, "wide": 2026101804}


def _draw_negatives(rng, train, test, outside, from_train, from_test, explicit_zero=()):
    """URM_test_negative: per user `outside[u]` items outside train | test, `from_train[u]` of its train items and `from_test[u]` of
    its test items (as many as it has); users in `explicit_zero` get one more stored entry whose value is 0."""
    n_users, n_items = train.shape
    rows, cols, vals = [], [], []
    for u in range(n_users):
        seen = train.indices[train.indptr[u]:train.indptr[u + 1]]
        held = test.indices[test.indptr[u]:test.indptr[u + 1]]
        free = np.setdiff1d(np.arange(n_items), np.union1d(seen, held))
        extra = 1 if u in explicit_zero else 0
        picked = rng.choice(free, outside[u] + extra, replace=False)
        items = [picked, rng.choice(seen, min(from_train[u], len(seen)), replace=False),
                 rng.choice(held, min(from_test[u], len(held)), replace=False)]
        values = np.ones(sum(len(i) for i in items), np.float32)
        if extra:
            values[0] = 0.0
        rows.append(np.full(len(values), u))
        cols.append(np.concatenate(items))
        vals.append(values)
    m = sps.coo_matrix((np.concatenate(vals), (np.concatenate(rows), np.concatenate(cols))), shape=train.shape)
    return sps.csr_matrix(m)        # (explicit zeros stay stored: the evaluator has to drop them)


def candidate_mask(test, negative):
    """Dense bool: the non-zero stored cells of either matrix."""
    return (test.toarray() != 0) | (negative.toarray() != 0)


def _wide_item_similarity(rng, train, admissible):
    """An item-item matrix too large to draw densely: every admissible candidate of a user gets weight from one to three items of the
    user's profile, plus scattered entries; ties among a user's candidates are then removed one unit at a time."""
    X = sps.csr_matrix(train, dtype=np.int64)
    n_items = X.shape[1]
    rows, cols, vals = [], [], []
    for u in range(X.shape[0]):
        profile = X.indices[X.indptr[u]:X.indptr[u + 1]]
        cands = np.flatnonzero(admissible[u])
        for share in (1.0, 0.5, 0.25):
            take = cands[rng.random(len(cands)) < share]
            rows.append(rng.choice(profile, len(take)))
            cols.append(take)
            vals.append(rng.integers(1, 1 << 16, len(take)))
    rows.append(rng.integers(0, n_items, 200000))
    cols.append(rng.integers(0, n_items, 200000))
    vals.append(rng.integers(1, 1 << 16, 200000))
    entries = [np.concatenate(rows), np.concatenate(cols), np.concatenate(vals).astype(np.int64)]

    def matrix():
        K = sps.csr_matrix(sps.coo_matrix((entries[2], (entries[0], entries[1])), shape=(n_items, n_items)))
        K.sum_duplicates()
        return K

    def bump(u, j, other):          # one more unit from the first item of the user's profile
        entries[0] = np.append(entries[0], X.indices[X.indptr[u]])
        entries[1] = np.append(entries[1], j)
        entries[2] = np.append(entries[2], 1)
    _untie(lambda: (X @ matrix()).toarray(), bump, admissible, ALL)
    K = matrix()
    assert K.data.max() < 1 << 19
    return dict(W_sparse=sps.csr_matrix((K * SIM_UNIT).astype(np.float32)))


def _admissible(train, test, negative, kwargs):
    mask = candidate_mask(test, negative)
    if kwargs.get("exclude_seen", True):
        mask &= train.toarray() == 0
    mask[:, kwargs.get("ignore_items", [])] = False
    return mask


@functools.lru_cache(maxsize=None)
def make_case(name):
    """dict(train, test, negative, cutoffs, kwargs of the evaluator, models) -- models: name -> dict of the recommender attributes."""
    rng = np.random.default_rng(SEEDS[name])
    if name in ("long_rows", "long_rows_over"):
        # candidate rows at the two ranking branches' boundary (1024 | 1025), at the row limit and -- long_rows_over -- one past it
        n_users, n_items = 64, 6000
        n_train, n_test = np.full(n_users, 20), np.full(n_users, 3)
        train, test = _split(rng, n_users, n_items, n_train, n_test, False)
        total = np.full(n_users, 100)
        total[:3] = (1024, 1025, ROW_LIMIT)
        from_train = np.zeros(n_users, np.int64)
        from_train[:4] = 5
        if name == "long_rows_over":
            total[3] = ROW_LIMIT + 1
        negative = _draw_negatives(rng, train, test, total - n_test - from_train, from_train, np.zeros(n_users, np.int64))
        kwargs = {}
        admissible = _admissible(train, test, negative, kwargs)
        return dict(train=train, test=test, negative=negative, cutoffs=CUTOFFS, kwargs=kwargs,
                    models={"mf": _factors(rng, n_users, n_items, 8, admissible, ALL, False)})
    if name == "wide":
        n_users, n_items = 300, 40000
        n_test = rng.integers(1, 12, n_users)
        train, test = _split(rng, n_users, n_items, rng.integers(5, 40, n_users), n_test, False)
        from_train = np.where(np.arange(n_users) % 7 == 0, 3, 0)
        negative = _draw_negatives(rng, train, test, 200 - n_test - from_train, from_train, np.zeros(n_users, np.int64))
        kwargs = {}
        admissible = _admissible(train, test, negative, kwargs)
        return dict(train=train, test=test, negative=negative, cutoffs=CUTOFFS, kwargs=kwargs,
                    models={"mf": _factors(rng, n_users, n_items, 8, admissible, ALL, False),
                            "item": _wide_item_similarity(rng, train, admissible)})
    n_users, n_items = 400, 320
    users = np.arange(n_users)
    n_train = rng.integers(10, 40, n_users)
    graded = name == "sampled_graded"
    n_test = rng.integers(0, 12 if graded else 7, n_users)
    outside = np.full(n_users, 99)
    from_train = np.where(users % 7 == 0, 3, 0)         # every 7th user: three train items (exclude_seen) and two of its
    from_test = np.where(users % 7 == 0, 2, 0)          # test items (de-duplication) among the negatives
    explicit_zero = set(users[(users % 11 == 0) & (users >= 16)].tolist())
    if not graded:
        n_test[:4], outside[:4], from_train[:4], from_test[:4] = 2, 0, 10, 0        # users 0-3: every candidate in train (test moved below)
        n_test[4:8], outside[4:8], from_train[4:8], from_test[4:8] = 1, 0, 0, 0     # users 4-7: a single candidate
        n_test[8:10], outside[8:10] = 2, 3                                          # users 8-9: 5 admissible candidates
        n_test[10:12], outside[10:12] = 3, 7                                        # users 10-11: 10
        n_test[12:14], outside[12:14] = 4, 60                                       # users 12-13: 64, one wavefront
        n_test[14:16], outside[14:16] = 4, 61                                       # users 14-15: 65
        from_train[8:16], from_test[8:16] = (4, 4, 2, 2, 3, 3, 3, 3), 0
    train, test = _split(rng, n_users, n_items, n_train, n_test, graded)
    if not graded:
        test = test.tolil()
        for u in range(4):          # the test items of users 0-3 are two of their train items
            test[u, :] = 0
            test[u, train.indices[train.indptr[u]:train.indptr[u] + 2]] = 1.0
        test = sps.csr_matrix(test)
        test.eliminate_zeros()
    negative = _draw_negatives(rng, train, test, outside, from_train, from_test, explicit_zero)
    kwargs = {}
    if graded:
        test_items = np.unique(test.indices)
        kwargs = dict(min_ratings_per_user=2, exclude_seen=False,
                      ignore_items=np.sort(np.concatenate([rng.choice(test_items, 12, replace=False),
                                                           rng.choice(np.unique(negative.indices), 8, replace=False)])).tolist(),
                      ignore_users=sorted(rng.choice(n_users, 25, replace=False).tolist()))
        kwargs["ignore_items"] = sorted(set(kwargs["ignore_items"]))
    admissible = _admissible(train, test, negative, kwargs)
    if not graded:
        counts = admissible.sum(axis=1)
        assert not counts[:4].any() and np.all(counts[4:8] == 1)
        assert list(counts[8:16]) == [5, 5, 10, 10, 64, 64, 65, 65]
    X = train.toarray().astype(np.int64)
    models = {"mf": _factors(rng, n_users, n_items, 16, admissible, ALL, False),
              "mf_bias": _factors(rng, n_users, n_items, 16, admissible, ALL, True),
              "item": _item_similarity(rng, X, admissible, ALL, 0.35),
              "user": _user_similarity(rng, X, admissible, ALL, 0.35)}
    return dict(train=train, test=test, negative=negative, cutoffs=CUTOFFS, kwargs=kwargs, models=models)
