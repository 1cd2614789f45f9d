"""Dense-weight scoring test helper (NumPy / SciPy only): the order contract of csrc/densescore.hip as a NumPy oracle and the small
models of tests/test_dense_score_spec.py (CPU) and tests/test_dense_score_gpu.py (device).

Contract: scores[u, j] is SciPy's `X[users] @ W` for a CSR X and a float32 ndarray W -- from +0.0, over the
stored cells of row u IN STORAGE ORDER, acc = acc + (x * W[i, j]) in float32 with the product rounded before the add.  The oracle
below restates that recurrence; test_dense_score_spec.py pins it to the SciPy that is installed, the device tests compare with the
SciPy product itself, with no tolerance.

Models: ratings 1..5, W ~ N(0, 0.01) with both signs (zero diagonal when square), every row of X with its indices in a random
order, profile lengths that pass any unroll or prefetch depth of the kernel, one explicitly stored zero.
"""
import functools
import os
import re

import numpy as np
import scipy.sparse as sps

import ranking_cases as RC

# profile length of user u (capped at n_mid): around the unroll depths, around a wavefront, and a long one
LENGTHS = (0, 1, 2, 3, 63, 64, 65, 700, 7, 8, 9, 17)
ZERO_USER = 10                  # the user whose first stored cell holds an explicit 0.0
EMPTY_USER = 0                  # profile of length 0: every score is +0.0, the list is all ties


def parse_tile(csrc=RC.CSRC):
    """DSCORE_TILE of densescore.hip: the columns of a workgroup's tile."""
    with open(os.path.join(csrc, "densescore.hip")) as f:
        found = re.findall(r"constexpr int DSCORE_TILE = (\d+);", f.read())
    assert len(found) == 1, found
    return int(found[0])


def first_wide_row():
    """The narrowest score row that no longer fits LDS at a small cutoff, not a multiple of 4."""
    n = 1
    while RC.fits_lds_rank(n, 10):
        n += 1
    assert n % 4 != 0
    return n


def shapes():
    """name -> (n_mid, n_out): tile boundaries (square), and a few rows of B under a score row on the wide ranking route."""
    T = parse_tile()
    out = {"n5": (5, 5), "tile_minus_1": (T - 1, T - 1), "tile": (T, T), "tile_plus_1": (T + 1, T + 1), "two_tiles_plus_3": (2 * T + 3, 2 * T + 3),
           "wide": (8, first_wide_row())}
    assert any(n % 4 for _, n in out.values())
    return out


def oracle(X, users, W):
    """The recurrence of the contract, one user at a time; float32 (len(users), n_out)."""
    X = sps.csr_matrix(X)
    W = np.asarray(W, dtype=np.float32)
    out = np.zeros((len(users), W.shape[1]), np.float32)
    for r, u in enumerate(users):
        acc = out[r]
        for q in range(X.indptr[u], X.indptr[u + 1]):
            product = np.float32(X.data[q]) * W[X.indices[q]]          # rounded to float32 ...
            acc += product                                             # ... before the add
    return out


def _unsorted_csr(rng, lengths, n_cols, values, explicit_zero=None):
    indptr = np.concatenate([[0], np.cumsum(lengths)]).astype(np.int32)
    indices = np.concatenate([rng.permutation(n_cols)[:n] for n in lengths] + [np.empty(0, np.int64)]).astype(np.int32)
    data = rng.choice(values, len(indices)).astype(np.float32)
    if explicit_zero is not None and lengths[explicit_zero]:
        data[indptr[explicit_zero]] = 0.0
    X = sps.csr_matrix((data, indices, indptr), shape=(len(lengths), n_cols))
    assert max(lengths) <= 3 or not X.has_sorted_indices             # (the order of a row is the order of the sum: keep it unsorted)
    return X


@functools.lru_cache(maxsize=None)
def model(name):
    """dict(X, W, seen, users): X n_users x n_mid (unsorted rows, ratings), W n_mid x n_out, seen n_users x n_out (X itself when
    square), users = every user."""
    n_mid, n_out = shapes()[name]
    rng = np.random.default_rng(20261019 + n_mid * 7 + n_out)
    lengths = [min(n, n_mid) for n in LENGTHS]
    X = _unsorted_csr(rng, lengths, n_mid, (1, 2, 3, 4, 5), explicit_zero=ZERO_USER)
    W = rng.normal(0.0, 0.01, (n_mid, n_out)).astype(np.float32)
    if n_mid == n_out:
        W[np.arange(n_mid), np.arange(n_mid)] = 0.0
        seen = X
    else:
        seen = _unsorted_csr(rng, [min(n, 40) for n in LENGTHS], n_out, (1,))
    assert (W > 0).any() and (W < 0).any()
    return dict(X=X, W=W, seen=seen, users=np.arange(len(lengths), dtype=np.int32))
