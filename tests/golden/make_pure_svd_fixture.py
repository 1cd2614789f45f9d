"""Reference-generated fixture for PureSVD (MatrixFactorization/PureSVDRecommender.py): the REFERENCE's own PureSVDRecommender and
PureSVDItemRecommender, imported from the reference tree, fitted with the installed scikit-learn (randomized_svd) on the seeded URMs
of tests/pure_svd_cases.py.  Per case: the arguments, the singular values (column norms of USER_factors), USER_factors and
ITEM_factors -- or, where those would not fit the fixture, the score rows of 64 seeded users --, W_sparse for the item variant, and
for random_seed=None cases the `np.random.seed` set before the fit and one `np.random.rand()` drawn after it (the fit draws the
Gaussian block from NumPy's global state; the device fit must leave that state where the reference leaves it).
Writes tests/golden/pure_svd.npz.  CPU only.  Run where the reference tree exists:
    python tests/golden/make_pure_svd_fixture.py"""
import json
import os
import sys

import numpy as np
import scipy.sparse as sps

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from oracle import ref_loader                                                   # noqa: E402
import pure_svd_cases as P                                                      # noqa: E402

Ref = ref_loader.load_python_reference("MatrixFactorization.PureSVDRecommender", "PureSVDRecommender")
RefItem = ref_loader.load_python_reference("MatrixFactorization.PureSVDRecommender", "PureSVDItemRecommender")
assert Ref is not None and RefItem is not None, "needs the reference tree"
import sklearn                                                                  # noqa: E402

URMS = P.urms()
out = {}
for name in P.STORED_URMS:
    X = URMS[name]
    out["X_%s_indptr" % name], out["X_%s_indices" % name] = X.indptr.astype(np.int32), X.indices.astype(np.int32)
    out["X_%s_data" % name], out["X_%s_shape" % name] = X.data.astype(np.float32), np.array(X.shape)
out["zipf_checksum"] = np.array(P.urm_checksum(URMS["zipf"]), np.int64)

for n, case in enumerate(P.CASES):
    X = URMS[case["urm"]]
    rec = Ref(X.copy(), verbose=False)
    if case["seed"] is None:
        np.random.seed(case["np_seed"])
    rec.fit(num_factors=case["num_factors"], random_seed=case["seed"])
    if case["seed"] is None:
        out["after_%d" % n] = np.array(np.random.rand())
    U, V = np.asarray(rec.USER_factors), np.asarray(rec.ITEM_factors)
    out["s_%d" % n] = P.singular_values(U)
    if case["store"] == "factors":
        out["U_%d" % n], out["V_%d" % n] = U, V
    else:
        users = P.score_users(n, X.shape[0])
        out["users_%d" % n], out["scores_%d" % n] = users, (U[users] @ V.T).astype(np.float32)
        out["shapes_%d" % n] = np.array(U.shape + V.shape)
    print("case %d %s: USER_factors %s %s (%s), ITEM_factors %s %s, s[0] %.4g s[-1] %.4g" % (
        n, case, U.shape, U.dtype, type(rec.USER_factors).__name__, V.shape, V.dtype, out["s_%d" % n][0], out["s_%d" % n][-1]))

for n, case in enumerate(P.ITEM_CASES):
    X = URMS[case["urm"]]
    rec = RefItem(X.copy(), verbose=False)
    if case["seed"] is None:
        np.random.seed(case["np_seed"])
    rec.fit(num_factors=case["num_factors"], topK=case["topK"], random_seed=case["seed"])
    if case["seed"] is None:
        out["item_after_%d" % n] = np.array(np.random.rand())
    W = sps.csr_matrix(rec.W_sparse, dtype=np.float32)
    W.sort_indices()
    out["W_%d_indptr" % n], out["W_%d_indices" % n] = W.indptr.astype(np.int32), W.indices.astype(np.int32)
    out["W_%d_data" % n], out["W_%d_shape" % n] = W.data, np.array(W.shape)
    print("item case %d %s: W %s nnz %d" % (n, case, W.shape, W.nnz))

out["cases"], out["item_cases"] = np.array(json.dumps(P.CASES)), np.array(json.dumps(P.ITEM_CASES))
out["provenance"] = np.array("reference PureSVDRecommender / PureSVDItemRecommender.fit, scikit-learn %s, numpy %s" % (sklearn.__version__, np.__version__))
path = os.path.join(ROOT, "tests", "golden", "pure_svd.npz")
np.savez_compressed(path, **out)
print("written", path, os.path.getsize(path), "bytes")
