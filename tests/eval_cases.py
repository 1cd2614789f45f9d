"""Seeded inputs of the holdout-evaluator fixture (tests/golden/make_evaluator_fixture.py writes the reference's results for them,
tests/test_evaluation_*.py rebuild the same inputs): train / test split, evaluator arguments and the models whose lists are
evaluated.  The models are drawn, not stored, to keep the fixture small.

Every model value is an integer multiple of a power of two, small enough that each score is exact in float32 whatever the order
of its terms: the reference's host products, the device GEMM and the sparse scorer's LDS atomics all give the same bits, and no
list depends on rounding.  Ties among the scores that decide a list (the list width + 1 best admissible items) are removed by
nudging the model one unit at a time, so the reference's order is defined."""
import functools

import numpy as np
import scipy.sparse as sps

# 100 and 200 take the metric kernel past one 64-wide chunk, and 200 the pairwise DCG sum past one 128-entry leaf
CUTOFFS = [1, 5, 10, 100, 200]
CASES = ("binary", "graded", "wide")
MODELS = {"binary": ("mf", "mf_bias", "item", "user"), "graded": ("mf", "mf_bias", "item", "user"), "wide": ("mf",)}
MF_UNIT, SIM_UNIT = 2.0 ** -10, 2.0 ** -16          # factor entries |k| <= 600: 16-term dot products < 2^24 units of 2^-20


def _split(rng, n_users, n_items, train_per_user, test_per_user, graded):
    train = np.zeros((n_users, n_items), np.float32)
    test = np.zeros((n_users, n_items), np.float32)
    for u in range(n_users):
        perm = rng.permutation(n_items)
        nt, ns = train_per_user[u], test_per_user[u]
        train[u, perm[:nt]] = 1.0
        test[u, perm[nt:nt + ns]] = rng.integers(1, 6, ns) if graded else 1.0
    return sps.csr_matrix(train), sps.csr_matrix(test)


def _tied(S, admissible, width):
    """(user, item, other) triples to move apart: in each row, among the admissible scores at or above the (width + 1)-th largest,
    every item that shares its score with a lower item id (other)."""
    out = []
    for u in range(S.shape[0]):
        items = np.flatnonzero(admissible[u])
        vals = S[u, items]
        if len(vals) == 0:
            continue
        kth = np.sort(vals)[::-1][min(width, len(vals) - 1)]
        top = items[vals >= kth]
        v = S[u, top]
        order = np.lexsort((top, v))
        dup = np.flatnonzero(v[order][1:] == v[order][:-1])
        out += [(u, int(top[order][d + 1]), int(top[order][d])) for d in dup]
    return out


def _untie(score, bump, admissible, width):
    for _ in range(200):
        tied = _tied(score(), admissible, width)
        if not tied:
            return
        for u, j, other in tied:
            bump(u, j, other)
    raise AssertionError("could not separate tied scores")


def _factors(rng, n_users, n_items, k, admissible, width, use_bias):
    U = rng.integers(-600, 601, (n_users, k)).astype(np.int64)
    V = rng.integers(-600, 601, (n_items, k)).astype(np.int64)
    bu = rng.integers(-1 << 20, 1 << 20, n_users) if use_bias else np.zeros(n_users, np.int64)
    bi = rng.integers(-1 << 20, 1 << 20, n_items) if use_bias else np.zeros(n_items, np.int64)
    mu = 1 << 18 if use_bias else 0

    def bump(u, j, other):              # raise item j's score for user u by |U[u, t]| >= 1
        t = int(np.argmax(np.abs(U[u])))
        V[j, t] += 1 if U[u, t] > 0 else -1
    _untie(lambda: U @ V.T + bu[:, None] + bi[None, :] + mu, bump, admissible, width)
    f = lambda a, unit: (a * unit).astype(np.float32)
    model = dict(USER_factors=f(U, MF_UNIT), ITEM_factors=f(V, MF_UNIT))
    if use_bias:
        model.update(USER_bias=f(bu, MF_UNIT ** 2), ITEM_bias=f(bi, MF_UNIT ** 2), GLOBAL_bias=np.float32(mu * MF_UNIT ** 2))
    return model


def _item_similarity(rng, X, admissible, width, density):
    n = X.shape[1]
    K = np.where(rng.random((n, n)) < density, rng.integers(1, 1 << 16, (n, n)), 0).astype(np.int64)

    def bump(u, j, other):              # one more unit from a profile item that already reaches j
        profile = np.flatnonzero(X[u])
        K[profile[np.argmax(K[profile, j] > 0)], j] += 1
    _untie(lambda: X @ K, bump, admissible, width)
    return dict(W_sparse=sps.csr_matrix((K * SIM_UNIT).astype(np.float32)))


def _user_similarity(rng, X, admissible, width, density):
    n = X.shape[0]
    K = np.where(rng.random((n, n)) < density, rng.integers(1, 1 << 16, (n, n)), 0).astype(np.int64)

    def bump(u, j, other):              # one more unit from a neighbour who has seen j but not the item it ties with
        v = np.flatnonzero((X[:, j] > 0) & (X[:, other] == 0))
        K[u, v[np.argmax(K[u, v] > 0)]] += 1
    _untie(lambda: K @ X, bump, admissible, width)
    return dict(W_sparse=sps.csr_matrix((K * SIM_UNIT).astype(np.float32)))


@functools.lru_cache(maxsize=None)
def make_case(name):
    """dict(train, test, cutoffs, kwargs of the evaluator, models) -- models: name -> dict of the recommender attributes.  (Cached:
    callers copy what they keep -- recommenders and the evaluator copy their URMs, set_model copies the model.)"""
    rng = np.random.default_rng({"binary": 2026101601, "graded": 2026101602, "wide": 2026101603}[name])
    width = max(CUTOFFS)
    if name == "wide":
        n_users, n_items = 300, 40000
        train, test = _split(rng, n_users, n_items, rng.integers(5, 40, n_users), rng.integers(1, 12, n_users), False)
        admissible = train.toarray() == 0
        return dict(train=train, test=test, cutoffs=CUTOFFS, kwargs={},
                    models={"mf": _factors(rng, n_users, n_items, 8, admissible, width, False)})
    n_users, n_items = 400, 320
    n_train = rng.integers(10, 40, n_users)
    n_test = rng.integers(0, 25, n_users)
    n_test[:3] = 120                                    # more test items than cutoff 100
    n_test[3:6] = 230                                   # more test items than cutoff 200
    n_train[6:10] = n_items - 30                        # fewer admissible items than one chunk (exclude_seen)
    n_test[6:10] = 12
    n_train[10:14] = n_items - 150                      # lists of 150: three chunks, a pairwise DCG sum over two leaves
    n_test[10:14] = 20
    train, test = _split(rng, n_users, n_items, n_train, n_test, name == "graded")
    kwargs = {}
    if name == "graded":
        test_items = np.unique(test.indices)
        kwargs = dict(min_ratings_per_user=2, exclude_seen=False,
                      ignore_items=np.sort(np.concatenate([rng.choice(test_items, 12, replace=False),
                                                           rng.choice(n_items, 4, replace=False)])).tolist(),
                      ignore_users=sorted(rng.choice(n_users, 25, replace=False).tolist()))
    X = train.toarray().astype(np.int64)
    if kwargs.get("exclude_seen", True):
        admissible = X == 0
    else:
        admissible = np.ones(X.shape, bool)
    admissible[:, kwargs.get("ignore_items", [])] = False
    models = {"mf": _factors(rng, n_users, n_items, 16, admissible, width, False),
              "mf_bias": _factors(rng, n_users, n_items, 16, admissible, width, True),
              "item": _item_similarity(rng, X, admissible, width, 0.35),
              "user": _user_similarity(rng, X, admissible, width, 0.35)}
    return dict(train=train, test=test, cutoffs=CUTOFFS, kwargs=kwargs, models=models)


def set_model(rec, attrs):
    """Puts a case's model into a recommender of the matching base class."""
    for key, value in attrs.items():
        setattr(rec, key, value.copy() if hasattr(value, "copy") else value)
    if "USER_factors" in attrs:
        rec.use_bias = "USER_bias" in attrs
    return rec
