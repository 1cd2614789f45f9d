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

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "slim_elasticnet.npz")
RAND_R_MAX = 2 ** 31 - 1
M32 = 0xFFFFFFFF


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


def coordinate_sweep(state, n):
    """n draws of sklearn's our_rand_r % n (sklearn/utils/_random.pxd); returns (coordinates, state after)."""
    s = state or 1
    out = np.empty(n, np.int64)
    for k in range(n):
        s ^= (s << 13) & M32
        s ^= s >> 17
        s ^= (s << 5) & M32
        out[k] = (s & 0x7FFFFFFF) % n
    return out, s


def replay_target(G, d_all, j, seed, l1, l2, positive, max_iter=100, tol=1e-4):
    """Coordinate descent of target j in Gram form; returns (w, n_iter, converged)."""
    n = G.shape[0]
    q = G[:, j]
    yy = G[j, j]
    d = d_all.copy()
    d[j] = 0.0
    w = np.zeros(n)
    H = np.zeros(n)
    state = seed
    tol_j = tol * yy
    for it in range(max_iter):
        coords, state = coordinate_sweep(state, n)
        w_max = d_w_max = 0.0
        pos = 0
        while pos < n:
            ii = coords[pos:]
            dd = d[ii]
            live = dd != 0.0
            old = w[ii]
            t = q[ii] - H[ii] + dd * old
            new = np.sign(t) * np.maximum(np.abs(t) - l1, 0.0) / np.where(live, dd + l2, 1.0)
            if positive:
                new[t < 0.0] = 0.0
            changed = live & (new != old)
            acc = int(np.argmax(changed)) + 1 if changed.any() else len(ii)
            a_live = live[:acc]
            if a_live.any():
                w_max = max(w_max, np.abs(new[:acc][a_live]).max())
                d_w_max = max(d_w_max, np.abs(new[:acc] - old[:acc])[a_live].max())
            if changed.any():
                k = ii[acc - 1]
                H += (new[acc - 1] - w[k]) * G[:, k]
                w[k] = new[acc - 1]
            pos += acc
        if w_max == 0.0 or d_w_max / w_max < tol or it == max_iter - 1:
            XtA = q - H - l2 * w
            XtA[j] = 0.0
            dual = XtA.max() if positive else np.abs(XtA).max()
            Rn = yy - 2.0 * (w @ q) + w @ H
            if dual > l1:
                c = l1 / dual
                gap = 0.5 * Rn * (1.0 + c * c)
            else:
                c, gap = 1.0, Rn
            gap += l1 * np.abs(w).sum() - c * (yy - w @ q) + 0.5 * l2 * (1.0 + c * c) * (w @ w)
            if gap < tol_j:
                return w, it + 1, True
    return w, max_iter, False


def select(w, topK):
    """The reference's selection (SLIMElasticNetRecommender.py:107-111): min(nnz - 1, topK) largest values, lower index on ties."""
    nz = np.flatnonzero(w)
    k = min(len(nz) - 1, topK)
    if k <= 0:
        return nz[:0]
    order = np.lexsort((nz, -w[nz]))
    return nz[order[:k]]


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
        w, n_iter[j], _ = replay_target(G, d, j, int(seeds[j]), l1, l2, positive_only)
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
