"""Reference-generated fixture for SLIM ElasticNet (SLIM_ElasticNet/SLIMElasticNetRecommender.py:41-149): the REFERENCE's own
recommender, imported from the reference tree, fitted with the installed scikit-learn on small seeded URMs.  For every case it
records the hyper-parameters, the `np.random.seed` set before the fit, the reference's W_sparse, the number of sweeps of every
target's ElasticNet solve (`n_iter_`, captured by wrapping ElasticNet.fit) and one `np.random.rand()` drawn after the fit (the
fit draws one seed per item from NumPy's global state; the device fit must leave that state where the reference leaves it).
Writes tests/golden/slim_elasticnet.npz.  CPU only.  Run where the reference tree exists:
    python tests/golden/make_slim_elasticnet_fixture.py"""
import json
import os
import sys
import warnings

import numpy as np
import scipy.sparse as sps

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
from oracle import ref_loader                                                   # noqa: E402

Ref = ref_loader.load_python_reference("SLIM_ElasticNet.SLIMElasticNetRecommender", "SLIMElasticNetRecommender")
assert Ref is not None, "needs the reference tree"
import sklearn                                                                  # noqa: E402
from sklearn.linear_model import ElasticNet                                     # noqa: E402

_n_iter = []
_fit = ElasticNet.fit


def _recording_fit(self, *args, **kwargs):
    out = _fit(self, *args, **kwargs)
    _n_iter.append(int(np.max(self.n_iter_)))
    return out


ElasticNet.fit = _recording_fit


def urm(seed, n_users, n_items, valued, collinear=False):
    rng = np.random.default_rng(seed)
    pop = rng.random(n_items) ** 2 * 0.25 + 0.02
    act = rng.random(n_users) * 1.5 + 0.25
    dense = rng.random((n_users, n_items)) < np.clip(np.outer(act, pop), 0, 0.9)
    if collinear:                       # items 1..7 are near copies of item 0: the coordinate sequence decides the result
        for k in range(1, 8):
            dense[:, k] = dense[:, 0] ^ (rng.random(n_users) < 0.01)
    dense[:, 3 if not collinear else 40] = False        # an empty item
    dense[7, :] = False                                 # an empty user
    vals = rng.integers(1, 6, size=dense.shape) if valued else np.ones(dense.shape)
    X = sps.csr_matrix(np.where(dense, vals, 0).astype(np.float32))
    X.sort_indices()
    return X


URMS = {"binary": urm(11, 300, 120, False), "valued": urm(12, 260, 110, True), "collinear": urm(13, 300, 60, False, collinear=True)}
CASES = [
    dict(urm="binary", seed=3, l1_ratio=0.1, alpha=1e-3, positive_only=True, topK=10),
    dict(urm="binary", seed=4, l1_ratio=0.05, alpha=0.01, positive_only=True, topK=1),
    dict(urm="binary", seed=5, l1_ratio=0.5, alpha=0.02, positive_only=True, topK=1000),          # topK >= every nnz: the nnz-1 rule
    dict(urm="binary", seed=6, l1_ratio=1.0, alpha=5.0, positive_only=True, topK=50),             # W empty
    dict(urm="binary", seed=7, l1_ratio=0.1, alpha=0.003, positive_only=False, topK=20),
    dict(urm="binary", seed=8, l1_ratio=1.0, alpha=0.005, positive_only=True, topK=30),           # l2 = 0
    dict(urm="binary", seed=9, l1_ratio=1e-5, alpha=1.0, positive_only=True, topK=40),
    dict(urm="valued", seed=10, l1_ratio=0.1, alpha=0.2, positive_only=True, topK=15),
    dict(urm="valued", seed=11, l1_ratio=0.2, alpha=0.5, positive_only=False, topK=1000),
    dict(urm="valued", seed=12, l1_ratio=1e-3, alpha=0.8, positive_only=True, topK=5),
    dict(urm="collinear", seed=13, l1_ratio=0.05, alpha=3e-3, positive_only=True, topK=100),      # max_iter binds
    dict(urm="collinear", seed=14, l1_ratio=0.01, alpha=1e-3, positive_only=False, topK=100),  # ... for every target
]

out = {}
for name, X in URMS.items():
    out["X_%s_indptr" % name], out["X_%s_indices" % name] = X.indptr.astype(np.int32), X.indices.astype(np.int32)
    out["X_%s_data" % name], out["X_%s_shape" % name] = X.data.astype(np.float32), np.array(X.shape)
for n, case in enumerate(CASES):
    kw = {k: case[k] for k in ("l1_ratio", "alpha", "positive_only", "topK")}
    rec = Ref(URMS[case["urm"]].copy(), verbose=False)
    _n_iter.clear()
    np.random.seed(case["seed"])
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        rec.fit(**kw)
    W = sps.csr_matrix(rec.W_sparse, dtype=np.float32)
    out["after_%d" % n] = np.array(np.random.rand())
    out["W_%d_indptr" % n], out["W_%d_indices" % n] = W.indptr.astype(np.int32), W.indices.astype(np.int32)
    out["W_%d_data" % n], out["W_%d_shape" % n] = W.data, np.array(W.shape)
    out["n_iter_%d" % n] = np.array(_n_iter, np.int32)
    print("case %d %s: nnz %d, sweeps max %d, targets at max_iter %d" % (n, case, W.nnz, max(_n_iter), sum(i >= 100 for i in _n_iter)))
out["cases"] = np.array(json.dumps(CASES))
out["provenance"] = np.array("reference SLIMElasticNetRecommender.fit, scikit-learn %s, numpy %s" % (sklearn.__version__, np.__version__))
path = os.path.join(ROOT, "tests", "golden", "slim_elasticnet.npz")
np.savez_compressed(path, **out)
print("written", path, os.path.getsize(path), "bytes")
