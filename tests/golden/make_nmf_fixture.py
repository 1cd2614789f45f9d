"""Reference-generated fixture for NMF (MatrixFactorization/NMFRecommender.py): the REFERENCE's own NMFRecommender, imported from the
reference tree, fitted with the installed scikit-learn (sklearn.decomposition.NMF) on the seeded URMs of tests/nmf_cases.py.

Per case: the arguments; USER_factors and ITEM_factors, or -- where those would not fit the fixture -- the block of the score
matrix of 64 seeded users and 64 seeded items; n_iter of the fit and of the transform (sklearn does not keep the latter: it is read
off NMF._fit_transform, which this script wraps to look at its return value); the same two numbers of the reference's fit on a
float64 copy of the URM, and d = score_distance(W32 H32, W64 H64) over the WHOLE score matrix: how far the reference's float32 fit
is from its own float64 fit, the noise floor the device is measured against.  The float64 factors themselves are not stored:
with them the file would pass the size of the largest fixture several times over, and the tests use them through d only.  For
random_seed=None cases, the `np.random.seed` set before the fit and one `np.random.rand()` drawn after it.

Admission: a case enters the fixture only if both n_iter agree between the two precisions and d <= 1e-3 -- NMF with k near the
rank of the URM is ill-conditioned, the reference's own two precisions then end tens of iterations apart, and such a case says
nothing about a kernel.  Every case of nmf_cases.CASES must be admitted (asserted), except the full-size ml1m ones, which are
dropped with a message when they are not; every case of REJECTED below must fail (asserted), so that the list stays honest.

Writes tests/golden/nmf.npz.  CPU only.  Run where the reference tree exists:
    python tests/golden/make_nmf_fixture.py"""
import json
import os
import sys
import time
import warnings

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from oracle import ref_loader                                                   # noqa: E402
import nmf_cases as M                                                           # noqa: E402

Ref = ref_loader.load_python_reference("MatrixFactorization.NMFRecommender", "NMFRecommender")
assert Ref is not None, "needs the reference tree"
import sklearn                                                                  # noqa: E402
from sklearn.decomposition import NMF                                           # noqa: E402

warnings.filterwarnings("ignore")              # ConvergenceWarning at the cap of 500 iterations is part of several cases

_n_iter = []
_inner = NMF._fit_transform


def _recording(self, X, y=None, W=None, H=None, update_H=True):
    out = _inner(self, X, y=y, W=W, H=H, update_H=update_H)
    _n_iter.append(int(out[2]))
    return out


NMF._fit_transform = _recording

# outside the admission rule where the case table was drawn up (sklearn 1.7.2, seed 3)
REJECTED = (M._grid("clusters", 70, 3, [("cd", "nndsvda"), ("mu-fro", "random"), ("mu-fro", "nndsvda")], "scores")
            + M._grid("clusters", 130, 3, [p for p in M.ALL_SIX if p != ("cd", "random")], "scores")
            + M._grid("wide", 65, 3, [("mu-fro", "random"), ("mu-fro", "nndsvda")], "scores")
            + M._grid("tiny", 40, 3, [("mu-fro", "random")], "factors"))

URMS = M.urms()


def reference_fit(case, dtype):
    rec = Ref(URMS[case["urm"]].copy(), verbose=False)
    rec.URM_train = rec.URM_train.astype(dtype)          # the reference's constructor casts to float32
    solver, loss = M.SOLVERS[case["solver"]]
    if case["seed"] is None:
        np.random.seed(case["np_seed"])
    del _n_iter[:]
    rec.fit(num_factors=case["k"], solver=solver, init_type=case["init"], beta_loss=loss, random_seed=case["seed"])
    after = np.random.rand() if case["seed"] is None else None
    assert len(_n_iter) == 2
    return np.asarray(rec.USER_factors), np.asarray(rec.ITEM_factors), tuple(_n_iter), after


def run(case):
    U, V, n32, after = reference_fit(case, np.float32)
    U64, V64, n64, _ = reference_fit(case, np.float64)
    assert U.dtype == np.float32 and V.dtype == np.float32 and U64.dtype == np.float64
    d = M.score_distance(M.scores_of(U, V), M.scores_of(U64, V64))
    return U, V, n32, n64, d, after


out, admitted = {}, []
for name in M.REGENERATED:
    out["%s_checksum" % name] = np.array(M.urm_checksum(URMS[name]), np.int64)
for case in M.CASES:
    t = time.time()
    U, V, n32, n64, d, after = run(case)
    ok = n32 == n64 and d <= 1e-3
    print("%s: n_iter %s (float64 %s), d %.2e, %s, %.1f s" % (case, n32, n64, d, "admitted" if ok else "NOT ADMITTED", time.time() - t), flush=True)
    if not ok:
        assert case["urm"] == "ml1m", ("a case of the table fails the admission rule", case, n32, n64, d)
        continue                                      # a full-size case outside the rule is dropped, as the table allows
    n = len(admitted)
    admitted.append(case)
    out["n_iter_%d" % n], out["n_iter64_%d" % n], out["d_%d" % n] = np.array(n32), np.array(n64), np.array(d)
    if case["store"] == "factors":
        out["U_%d" % n], out["V_%d" % n] = U, V
    else:
        users, items = M.score_block(n, URMS[case["urm"]].shape)
        out["users_%d" % n], out["items_%d" % n] = users, items
        out["scores_%d" % n] = M.scores_of(U, V, users, items).astype(np.float32)
    if case["seed"] is None:
        out["after_%d" % n] = np.array(after)

for case in REJECTED:
    U, V, n32, n64, d, _ = run(case)
    print("rejected %s: n_iter %s (float64 %s), d %.2e" % (case, n32, n64, d), flush=True)
    assert n32 != n64 or d > 1e-3, ("a case listed as rejected passes the admission rule", case)
try:
    reference_fit(dict(urm="tiny", k=40, solver="cd", init="nndsvda", seed=3), np.float32)
    raise AssertionError("nndsvda with k > min(shape) must raise")
except ValueError as exc:
    out["nndsvda_error"] = np.array(str(exc))

out["cases"] = np.array(json.dumps(admitted))
out["provenance"] = np.array("reference NMFRecommender.fit, scikit-learn %s, numpy %s" % (sklearn.__version__, np.__version__))
path = os.path.join(ROOT, "tests", "golden", "nmf.npz")
np.savez_compressed(path, **out)
print("written", path, os.path.getsize(path), "bytes,", len(admitted), "cases")
