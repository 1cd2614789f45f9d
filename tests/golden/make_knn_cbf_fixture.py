"""Reference-generated fixture for the content-based and CF+CBF hybrid KNN recommenders (KNN/ItemKNNCBFRecommender.py,
KNN/UserKNNCBFRecommender.py, KNN/ItemKNN_CFCBF_Hybrid_Recommender.py, KNN/UserKNN_CFCBF_Hybrid_Recommender.py): the REFERENCE's own
classes, imported from the reference tree, fitted on one small seeded URM with two item and two user content matrices.  For every
case it records the class, the content matrix, the fit arguments, the reference's W_sparse and its post-fit ICM_train / UCM_train
(re-weighted and, for the hybrids, stacked).

The fits run with use_implementation="python": the device follows Compute_Similarity_Python's top-K rule (the K largest cells of the
full column, zeros compete and are then dropped) where the Cython class pads with stale ids (tests/test_oracle_golden.py).

The matrices: 70 users x 60 items.  "icm_real" has real values and eleven items without features, items 5 and 17 among them (17 has
no interactions either, 30 has features and no interactions); "icm_all" is binary with feature 0 held by every item; "ucm_real" /
"ucm_all" likewise for users (users 3 and 11 are among those without features, 11 has no interactions).  With feature 0 everywhere
every column has 59 (69) positive neighbours; otherwise between none and a few dozen: topK 4 .. 12 cuts most columns, topK 100 none.
Writes tests/golden/knn_cbf.npz.  CPU only.  Run where the reference tree exists:
    python tests/golden/make_knn_cbf_fixture.py"""
import json
import os
import sys

import numpy as np
import scipy.sparse as sps

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
from oracle import ref_loader                                                   # noqa: E402

CLASSES = {
    "ItemKNNCBFRecommender": ref_loader.load_python_reference("KNN.ItemKNNCBFRecommender", "ItemKNNCBFRecommender"),
    "UserKNNCBFRecommender": ref_loader.load_python_reference("KNN.UserKNNCBFRecommender", "UserKNNCBFRecommender"),
    "ItemKNN_CFCBF_Hybrid_Recommender": ref_loader.load_python_reference("KNN.ItemKNN_CFCBF_Hybrid_Recommender",
                                                                         "ItemKNN_CFCBF_Hybrid_Recommender"),
    "UserKNN_CFCBF_Hybrid_Recommender": ref_loader.load_python_reference("KNN.UserKNN_CFCBF_Hybrid_Recommender",
                                                                         "UserKNN_CFCBF_Hybrid_Recommender"),
}
assert all(c is not None for c in CLASSES.values()), "needs the reference tree"

N_USERS, N_ITEMS = 70, 60


def content_matrix(seed, n_entities, n_features, real, empty, everywhere):
    rng = np.random.default_rng(seed)
    density = rng.random(n_features) * 0.25 + 0.05
    dense = rng.random((n_entities, n_features)) < density[None, :]
    if everywhere:
        dense[:, 0] = True
    dense[list(empty), :] = False
    vals = (rng.random(dense.shape) * 3 + 0.1) if real else np.ones(dense.shape)
    M = sps.csr_matrix(np.where(dense, vals, 0).astype(np.float32))
    M.sort_indices()
    return M


def interactions(seed):
    rng = np.random.default_rng(seed)
    pop = rng.random(N_ITEMS) ** 2 * 0.3 + 0.03
    act = rng.random(N_USERS) * 1.5 + 0.3
    dense = rng.random((N_USERS, N_ITEMS)) < np.clip(np.outer(act, pop), 0, 0.9)
    dense[:, [17, 30]] = False
    dense[11, :] = False
    X = sps.csr_matrix(np.where(dense, rng.integers(1, 6, size=dense.shape), 0).astype(np.float32))
    X.sort_indices()
    return X


URM = interactions(21)
MATRICES = {
    "icm_real": content_matrix(22, N_ITEMS, 12, True, (5, 17), False),
    "icm_all": content_matrix(23, N_ITEMS, 9, False, (), True),
    "ucm_real": content_matrix(24, N_USERS, 8, True, (3, 11), False),
    "ucm_all": content_matrix(25, N_USERS, 7, False, (), True),
}
CASES = [
    dict(cls="ItemKNNCBFRecommender", cm="icm_real", fit=dict(topK=10, shrink=0, similarity="cosine")),
    dict(cls="ItemKNNCBFRecommender", cm="icm_real", fit=dict(topK=5, shrink=2, similarity="pearson", feature_weighting="BM25")),
    dict(cls="ItemKNNCBFRecommender", cm="icm_all", fit=dict(topK=100, shrink=1, similarity="jaccard")),
    dict(cls="ItemKNNCBFRecommender", cm="icm_real", fit=dict(topK=8, shrink=3, similarity="asymmetric", asymmetric_alpha=0.3,
                                                              feature_weighting="TF-IDF")),
    dict(cls="ItemKNNCBFRecommender", cm="icm_all", fit=dict(topK=4, shrink=0, similarity="dice")),
    dict(cls="UserKNNCBFRecommender", cm="ucm_real", fit=dict(topK=10, shrink=5, similarity="cosine", feature_weighting="BM25")),
    dict(cls="UserKNNCBFRecommender", cm="ucm_all", fit=dict(topK=100, shrink=2, similarity="tversky", tversky_alpha=0.7, tversky_beta=1.2)),
    dict(cls="UserKNNCBFRecommender", cm="ucm_real", fit=dict(topK=6, shrink=1, similarity="adjusted", feature_weighting="TF-IDF")),
    dict(cls="ItemKNN_CFCBF_Hybrid_Recommender", cm="icm_real", weight=0.3, fit=dict(topK=10, shrink=5, similarity="cosine")),
    dict(cls="ItemKNN_CFCBF_Hybrid_Recommender", cm="icm_real", weight=2.5, fit=dict(topK=7, shrink=0, similarity="tanimoto")),
    dict(cls="ItemKNN_CFCBF_Hybrid_Recommender", cm="icm_all", weight=1.0, fit=dict(topK=100, shrink=10, similarity="cosine",
                                                                                     feature_weighting="TF-IDF")),
    dict(cls="ItemKNN_CFCBF_Hybrid_Recommender", cm="icm_real", weight=0.7, fit=dict(topK=5, shrink=2, similarity="pearson",
                                                                                      feature_weighting="BM25")),
    dict(cls="UserKNN_CFCBF_Hybrid_Recommender", cm="ucm_real", weight=0.4, fit=dict(topK=10, shrink=3, similarity="cosine")),
    dict(cls="UserKNN_CFCBF_Hybrid_Recommender", cm="ucm_all", weight=3.0, fit=dict(topK=100, shrink=0, similarity="dice")),
    dict(cls="UserKNN_CFCBF_Hybrid_Recommender", cm="ucm_real", weight=1.5, fit=dict(topK=5, shrink=4, similarity="asymmetric",
                                                                                      asymmetric_alpha=0.7, feature_weighting="BM25")),
    dict(cls="UserKNN_CFCBF_Hybrid_Recommender", cm="ucm_real", weight=0.6, fit=dict(topK=12, shrink=2, similarity="adjusted",
                                                                                      normalize=False)),
]


def pack(out, prefix, M):
    M = sps.csr_matrix(M)
    M.sort_indices()
    out[prefix + "_indptr"], out[prefix + "_indices"] = M.indptr.astype(np.int32), M.indices.astype(np.int32)
    out[prefix + "_data"], out[prefix + "_shape"] = M.data.astype(np.float32), np.array(M.shape)


out = {}
pack(out, "URM", URM)
for name, M in MATRICES.items():
    pack(out, name, M)
for n, case in enumerate(CASES):
    rec = CLASSES[case["cls"]](URM.copy(), MATRICES[case["cm"]].copy(), verbose=False)
    kw = dict(case["fit"], use_implementation="python")
    if "weight" in case:
        kw["ICM_weight" if case["cls"].startswith("Item") else "UCM_weight"] = case["weight"]
    rec.fit(**kw)
    after = rec.ICM_train if case["cls"].startswith("Item") else rec.UCM_train
    assert rec.W_sparse.dtype == np.float32         # (the reference's BM25 / TF-IDF return float64: stored as float32, the device's type)
    pack(out, "W_%d" % n, rec.W_sparse)
    pack(out, "CM_%d" % n, after)
    per_col = np.diff(sps.csc_matrix(rec.W_sparse).indptr)
    print("case %d %s: W nnz %d, neighbours per column %d .. %d, post-fit matrix %s nnz %d" % (
        n, case, rec.W_sparse.nnz, per_col.min(), per_col.max(), after.shape, after.nnz))
out["cases"] = np.array(json.dumps(CASES))
out["provenance"] = np.array("reference KNN CBF / CFCBF hybrid fits, use_implementation='python', numpy %s, scipy %s" % (
    np.__version__, __import__("scipy").__version__))
path = os.path.join(ROOT, "tests", "golden", "knn_cbf.npz")
np.savez_compressed(path, **out)
print("written", path, os.path.getsize(path), "bytes")
