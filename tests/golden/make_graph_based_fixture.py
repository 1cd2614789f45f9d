"""Reference-generated fixture for P3alpha / RP3beta over the range their hyper-parameter search draws from: the REFERENCE's own
GraphBased/P3alphaRecommender.py and RP3betaRecommender.py, imported from the reference tree, on the URM and the cases of
tests/graph_cases.py (150 users x 90 items with cold items, empty users, a single-user item and a user who rated everything;
alpha 0.05 .. 2, beta 0 .. 2, topK 1 .. 1000, both normalisations, min_rating with implicit off and on).
Writes tests/golden/graph_based_search.npz: the URM and, per case, the reference's W_sparse as CSR arrays in its own dtype, plus the
JSON case list.  CPU only.  Run where the reference tree exists:
    python tests/golden/make_graph_based_fixture.py"""
import contextlib
import io
import json
import os
import sys

import numpy as np
import scipy.sparse as sps

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from oracle import ref_loader                                                   # noqa: E402
import graph_cases as G                                                         # noqa: E402

P3 = ref_loader.load_python_reference("GraphBased.P3alphaRecommender", "P3alphaRecommender")
RP3 = ref_loader.load_python_reference("GraphBased.RP3betaRecommender", "RP3betaRecommender")
assert P3 is not None and RP3 is not None, "needs the reference tree"

X = G.search_urm()
counts = np.bincount(X.indices, minlength=X.shape[1])
assert X.shape == (G.N_USERS, G.N_ITEMS) and (counts[list(G.COLD_ITEMS)] == 0).all() and counts[G.LONELY_ITEM] == 1
assert (np.diff(X.indptr)[list(G.EMPTY_USERS)] == 0).all() and np.diff(X.indptr)[G.FULL_USER] == G.N_ITEMS - len(G.COLD_ITEMS)
out = dict(X_data=X.data.astype(np.float32), X_indices=X.indices.astype(np.int32), X_indptr=X.indptr.astype(np.int32), X_shape=np.array(X.shape))
for n, case in enumerate(G.CASES):
    with contextlib.redirect_stdout(io.StringIO()):
        rec = (P3 if case["cls"] == "P3" else RP3)(X.copy(), verbose=False)
        rec.fit(**case["kw"])
    W = sps.csr_matrix(rec.W_sparse)
    W.sort_indices()
    out["W_%d_data" % n], out["W_%d_indices" % n], out["W_%d_indptr" % n] = W.data, W.indices.astype(np.int32), W.indptr.astype(np.int32)
    out["W_%d_shape" % n] = np.array(W.shape)
    print("case %2d %-3s %s: nnz %d, dtype %s" % (n, case["cls"], case["kw"], W.nnz, W.data.dtype))
out["cases"] = np.array(json.dumps(G.CASES))
out["provenance"] = np.array("reference P3alphaRecommender / RP3betaRecommender, numpy %s, scipy %s" % (np.__version__, __import__("scipy").__version__))
np.savez_compressed(G.GOLDEN, **out)
print("written", G.GOLDEN, os.path.getsize(G.GOLDEN), "bytes")
