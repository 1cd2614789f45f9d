"""Reference-generated fixture for the non-personalized recommenders (Base/NonPersonalizedRecommender.py): the REFERENCE's own TopPop,
GlobalEffects and Random, imported from the reference tree, on three small seeded URMs.

Cases (about 300 users x 500 items, popularity-skewed so that TopPop's counts hold both ties and distinct values):
  binary    every stored value is 1
  ratings   1 .. 5 in half steps: every sum of them is exact in float64
  holes     ratings with a cold item (column 7), a cold user (row 11) and a stored explicit zero at (3, 5) in the matrix as passed
            (the recommenders' constructors drop it)
Per case: item_pop; mu, item_bias, user_bias at (lambda_user, lambda_item) = (10, 25) and (1, 2); the reference's recommend() lists
of TopPop and GlobalEffects (10, 25) for 40 users (the cold one among them) at cut-offs 5 and 20, with remove_seen_flag on and off,
without and with an items_to_compute subset; for Random(random_seed=7) the score blocks of two consecutive _compute_item_score calls
(3 users, then 2), the MT19937 state of np.random afterwards, and -- after a second fit(random_seed=7) -- its recommend() lists.
Writes tests/golden/non_personalized.npz (arrays and a JSON case list only).  CPU only.  Run where the reference tree exists:
    python tests/golden/make_non_personalized_fixture.py"""
import json
import os
import sys

import numpy as np
import scipy.sparse as sps

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
from oracle import ref_loader                                                   # noqa: E402

TopPop = ref_loader.load_python_reference("Base.NonPersonalizedRecommender", "TopPop")
GlobalEffects = ref_loader.load_python_reference("Base.NonPersonalizedRecommender", "GlobalEffects")
Random = ref_loader.load_python_reference("Base.NonPersonalizedRecommender", "Random")
assert TopPop is not None and GlobalEffects is not None and Random is not None, "needs the reference tree"

N_USERS, N_ITEMS = 300, 500
LAMBDAS = [(10, 25), (1, 2)]
CUTOFFS = [5, 20]
RANDOM_SEED, RANDOM_CUTOFF = 7, 10


def interactions(seed, values, holes=False):
    rng = np.random.default_rng(seed)
    pop = rng.random(N_ITEMS) ** 3 * 0.5 + 0.01
    act = rng.random(N_USERS) * 1.6 + 0.2
    dense = rng.random((N_USERS, N_ITEMS)) < np.clip(np.outer(act, pop), 0, 0.95)
    if holes:
        dense[:, 7] = False
        dense[11, :] = False
    ratings = np.ones(dense.shape) if values == "binary" else rng.integers(2, 11, size=dense.shape) / 2.0
    X = sps.csr_matrix(np.where(dense, ratings, 0).astype(np.float32))
    X.sort_indices()
    if holes:                                   # one stored zero, at a cell that holds nothing
        assert X[3, 5] == 0
        coo = X.tocoo()
        X = sps.csr_matrix((np.append(coo.data, np.float32(0)), (np.append(coo.row, 3), np.append(coo.col, 5))), shape=X.shape)
        X.sort_indices()
        assert X.nnz == coo.nnz + 1
    return X


CASES = [dict(name="binary", seed=31, values="binary", holes=False),
         dict(name="ratings", seed=32, values="ratings", holes=False),
         dict(name="holes", seed=33, values="ratings", holes=True)]


def padded(lists, width):
    table = np.full((len(lists), width), -1, np.int32)
    for r, items in enumerate(lists):
        table[r, :len(items)] = items
    return table


out = {}
for case in CASES:
    name = case["name"]
    URM = interactions(case["seed"], case["values"], case["holes"])
    out[name + "_indptr"], out[name + "_indices"] = URM.indptr.astype(np.int32), URM.indices.astype(np.int32)
    out[name + "_data"], out[name + "_shape"] = URM.data.astype(np.float32), np.array(URM.shape)
    rng = np.random.default_rng(case["seed"] + 100)
    users = np.sort(rng.choice(N_USERS, 40, replace=False)).astype(np.int32)
    if case["holes"] and 11 not in users:
        users[0] = 11
        users = np.sort(users)
    subset = np.sort(rng.choice(N_ITEMS, 120, replace=False)).astype(np.int32)
    out[name + "_users"], out[name + "_subset"] = users, subset

    top = TopPop(URM.copy())
    top.fit()
    out[name + "_item_pop"] = np.asarray(top.item_pop)
    models = {"toppop": top}
    for lu, li in LAMBDAS:
        ge = GlobalEffects(URM.copy())
        ge.fit(lambda_user=lu, lambda_item=li)
        tag = "%s_ge_%d_%d" % (name, lu, li)
        out[tag + "_mu"] = np.asarray(ge.mu)
        out[tag + "_item_bias"] = np.asarray(ge.item_bias, dtype=np.float64).ravel()
        out[tag + "_user_bias"] = np.asarray(ge.user_bias, dtype=np.float64).ravel()
        if (lu, li) == LAMBDAS[0]:
            models["ge"] = ge
    for model, rec in models.items():
        for cutoff in CUTOFFS:
            for seen in (1, 0):
                for sub in (0, 1):
                    lists = rec.recommend(users, cutoff=cutoff, remove_seen_flag=bool(seen), items_to_compute=subset if sub else None)
                    out["%s_%s_c%d_s%d_i%d" % (name, model, cutoff, seen, sub)] = padded(lists, cutoff)

    rnd = Random(URM.copy())
    rnd.fit(random_seed=RANDOM_SEED)
    out[name + "_random_block0"] = rnd._compute_item_score(users[:3])
    out[name + "_random_block1"] = rnd._compute_item_score(users[3:5], items_to_compute=subset)
    state = np.random.get_state()
    assert state[0] == "MT19937"
    out[name + "_random_state_keys"], out[name + "_random_state_pos"] = np.asarray(state[1], dtype=np.uint32), np.array(state[2])
    rnd.fit(random_seed=RANDOM_SEED)
    out[name + "_random_lists"] = padded(rnd.recommend(users, cutoff=RANDOM_CUTOFF), RANDOM_CUTOFF)
    print("case %s: nnz %d, item_pop %d .. %d (%d distinct), lists recorded: %d" % (
        name, URM.nnz, top.item_pop.min(), top.item_pop.max(), len(np.unique(top.item_pop)), 2 * len(CUTOFFS) * 4))

out["cases"] = np.array(json.dumps(dict(cases=[c["name"] for c in CASES], lambdas=LAMBDAS, cutoffs=CUTOFFS, random_seed=RANDOM_SEED,
                                        random_cutoff=RANDOM_CUTOFF)))
out["provenance"] = np.array("reference TopPop / GlobalEffects / Random, numpy %s, scipy %s" % (np.__version__, __import__("scipy").__version__))
path = os.path.join(ROOT, "tests", "golden", "non_personalized.npz")
np.savez_compressed(path, **out)
print("written", path, os.path.getsize(path), "bytes")
