"""PureSVD on MI355X: host front-end of the svd_* entry points of libmi355rec.so.

Mirrors PureSVDRecommender / PureSVDItemRecommender (MatrixFactorization/PureSVDRecommender.py), which hand URM_train to sklearn's
`randomized_svd`.  With sklearn's defaults that is: a Gaussian block Q of `num_factors + 10` columns, `n_iter` (7 or 4) rounds of
`Q = L(M Q); Q = L(M^T Q)` with an LU factor as the normaliser L, an economic QR of `M Q`, and the SVD of the small `Q^T M`.  The
products run on the device (csrc/svd.hip); the normaliser is replaced by another basis of the same column space, Cholesky-QR: the
Gram matrix of the block comes from the device in float64, its Cholesky factor is inverted on the host (LAPACK on an r x r matrix)
and applied on the device.  The last step takes the Gram matrix of `M^T Q` (= B B^T), its eigen-decomposition on the host and two more
applies, so that between the upload of Q and the download of the factors nothing with n_users or n_items rows crosses PCIe.  A block
whose Gram matrix is numerically singular (r above the rank of the URM) is normalised on the host by a Householder QR instead, counted
in `fit_stats["host_fallbacks"]`.  Q is drawn from NumPy exactly as sklearn draws it, so `np.random` is left where
the reference's fit leaves it.
"""
import ctypes as C
import time

import numpy as np
import scipy.linalg as sla
import scipy.sparse as sps

from . import _native as N
from .block_steps import BlockPairSteps
from .recommender_base import BaseItemSimilarityMatrixRecommender, BaseMatrixFactorizationRecommender, check_matrix
from .scoring import GpuScoringMixin, GpuSimilarityScoringMixin, MI355XScorer

N_OVERSAMPLES = 10                # sklearn's randomized_svd default
# Cholesky-QR is trusted while the smallest squared pivot of the factor -- the squared length of what a column adds to the span of the
# columns before it -- stays above this fraction of trace(G).  The block is float32: a column whose new component is below
# eps32 = 6e-8 of the block's scale is rounding noise, i.e. 3.6e-15 of the trace; at 1e-11 the condition number of the block is
# about 3e5, where the float32 apply still leaves a basis that the second pass repairs (orthogonality loss ~ eps32 * cond = 0.02).
PIVOT_FLOOR = 1e-11
# the last step divides by the singular values of B: below this fraction of the largest one they are rank deficiency, not signal
SIGMA_FLOOR = 1e-4


def check_random_state(seed):
    """sklearn.utils.check_random_state: None is NumPy's global RandomState, an int seeds a new one."""
    if seed is None or seed is np.random:
        return np.random.mtrand._rand
    if isinstance(seed, (int, np.integer)):
        return np.random.RandomState(seed)
    if isinstance(seed, np.random.RandomState):
        return seed
    raise ValueError("%r cannot be used to seed a numpy.random.RandomState instance" % seed)


class PureSVD_MI355X_Steps(BlockPairSteps):
    """The URM in both layouts and two float32 blocks on the device: side 0 is (n_users, r), side 1 is (n_items, r)."""
    _PREFIX = "mi355rec_svd"
    _SIDE_NAMES = ("users", "items")
    r = property(lambda self: self.width)

    def product(self, dst_side):
        """dst_side 0: block[0] = URM . block[1]; dst_side 1: block[1] = URM^T . block[0]."""
        self._call("product", int(dst_side))

    def gram(self, side):
        G = np.empty((self.r, self.r), np.float64)
        self._call("gram", int(side), N.ptr(G))
        return G

    def apply(self, side, T):
        T = N.as_f32(T)
        if T.shape != (self.r, self.r):
            raise ValueError("the matrix of an apply must be %d x %d, got %r" % (self.r, self.r, T.shape))
        self._call("apply", int(side), N.ptr(T))

    def fit_info(self):
        ms = [C.c_double() for _ in range(3)]
        tail = self._fit_info_tail(*[C.byref(x) for x in ms])
        return dict({"product_ms": ms[0].value, "gram_ms": ms[1].value, "apply_ms": ms[2].value}, **tail)


def _inverse_cholesky_factor(G):
    """R^-1 for G = R^T R (float64), or None where the factorisation fails or a squared pivot falls below PIVOT_FLOOR * trace(G)."""
    trace = float(np.trace(G))
    if not np.isfinite(G).all() or not trace > 0.0:
        return None
    try:
        R = sla.cholesky(G, lower=False, check_finite=False)
    except sla.LinAlgError:
        return None
    pivots = np.diagonal(R)
    if not np.isfinite(pivots).all() or float(pivots.min()) ** 2 < PIVOT_FLOOR * trace:
        return None
    Rinv = sla.solve_triangular(R, np.eye(len(G)), lower=False, check_finite=False)
    return Rinv if np.isfinite(Rinv).all() else None


def normalise(steps, side, passes, counters):
    """block[side] <- a basis of its column space: Cholesky-QR `passes` times, a Householder QR on the host where that breaks down."""
    for _ in range(passes):
        Rinv = _inverse_cholesky_factor(steps.gram(side))
        counters["gram_apply_pairs"] += 1
        if Rinv is None:
            Q = sla.qr(steps.get_block(side), mode="economic", check_finite=False)[0]
            steps.set_block(side, np.nan_to_num(Q, nan=0.0, posinf=0.0, neginf=0.0))
            counters["host_fallbacks"] += 1
            return
        steps.apply(side, Rinv)


def randomized_svd_device(URM_train, num_factors, random_seed=None, power_passes=1):
    """(USER_factors = U diag(s), ITEM_factors = V, stats) of sklearn's randomized_svd(URM_train, num_factors, random_state=seed)."""
    t_start = time.perf_counter()
    A = check_matrix(URM_train, "csr", dtype=np.float32)
    n_users, n_items = A.shape
    num_factors = int(num_factors)
    if num_factors < 1:
        raise ValueError("num_factors must be at least 1, got %d" % num_factors)
    r = num_factors + N_OVERSAMPLES
    n_iter = 7 if num_factors < 0.1 * min(A.shape) else 4
    transpose = n_users < n_items
    # M = URM^T when transposed; `small` is the side of M's columns (the shorter one), `big` the side of its rows
    small, big = (0, 1) if transpose else (1, 0)
    n_small = A.shape[small]
    Q = check_random_state(random_seed).normal(size=(n_small, r)).astype(np.float32)
    # r above min(shape): the reference's LU factors shrink the block to n_small columns, a basis of the whole space; any
    # n_small independent columns span the same
    r_eff = min(r, n_small)
    counters = {"host_fallbacks": 0, "gram_apply_pairs": 0, "products": 0, "svd_on_host": 0}
    t_drawn = time.perf_counter()
    steps = PureSVD_MI355X_Steps(A, r_eff)
    try:
        t_created = time.perf_counter()
        steps.set_block(small, np.ascontiguousarray(Q[:, :r_eff]))
        for _ in range(n_iter):
            steps.product(big)
            normalise(steps, big, power_passes, counters)
            steps.product(small)
            normalise(steps, small, power_passes, counters)
            counters["products"] += 2
        steps.product(big)
        normalise(steps, big, 2, counters)                 # Q, orthonormal
        steps.product(small)                               # B^T = M^T Q
        counters["products"] += 2
        w, Uhat = sla.eigh(steps.gram(small), check_finite=False)          # B B^T = Uhat diag(s^2) Uhat^T
        w, Uhat = w[::-1], Uhat[:, ::-1]
        s = np.sqrt(np.maximum(w, 0.0))
        if np.isfinite(s).all() and s[0] > 0.0 and s[-1] > SIGMA_FLOOR * s[0]:
            # user side carries diag(s): U diag(s) when the users are M's rows, (V^T)^T diag(s) = B^T Uhat when they are its columns
            T_big = Uhat * s if not transpose else Uhat
            T_small = Uhat / s if not transpose else Uhat
            steps.apply(big, T_big)
            steps.apply(small, T_small)
            if not transpose:
                # V = B^T Uhat / s is orthonormal only to eps32 * s[0] / s[k]; one Cholesky-QR pass (R = I + a correction of that size)
                # makes it orthonormal to float32, as LAPACK's V is
                Rinv = _inverse_cholesky_factor(steps.gram(small))
                counters["gram_apply_pairs"] += 1
                if Rinv is not None:
                    steps.apply(small, Rinv)
            t_chain = time.perf_counter()
            USER_factors, ITEM_factors = steps.get_block(0), steps.get_block(1)
        else:
            # rank-deficient B: the reference's LAPACK SVD on the host, from the downloaded blocks
            counters["svd_on_host"] = 1
            t_chain = time.perf_counter()
            Qb, Bt = steps.get_block(big), steps.get_block(small)
            Uh, s, Vt = sla.svd(np.nan_to_num(Bt.T), full_matrices=False, lapack_driver="gesdd", check_finite=False)
            Ub, Vs = Qb @ Uh, Vt.T
            USER_factors, ITEM_factors = (Ub * s, Vs) if not transpose else (Vs * s, Ub)
        info = steps.fit_info()
        last_product = steps.stats()
    finally:
        steps.close()
    k = min(num_factors, r_eff)
    USER_factors = np.ascontiguousarray(USER_factors[:, :k], dtype=np.float32)
    ITEM_factors = np.ascontiguousarray(ITEM_factors[:, :k], dtype=np.float32)
    # svd_flip, decided on the user side in both branches: the entry of largest magnitude of every column becomes positive
    at = np.argmax(np.abs(USER_factors), axis=0)
    signs = np.sign(USER_factors[at, np.arange(k)]).astype(np.float32)
    USER_factors *= signs
    ITEM_factors *= signs
    stats = dict(counters, **info)
    # wall seconds: drawing Q, building the handle (both layouts, piece tables, upload), the chain of step-wise calls from the upload
    # of Q to the last apply (kernels, r x r copies and LAPACK calls together), the download of the factors with the sign flip
    stats.update(draw_s=t_drawn - t_start, create_s=t_created - t_drawn, chain_s=t_chain - t_created, download_s=time.perf_counter() - t_chain)
    stats.update(n_iter=n_iter, transpose=bool(transpose), r=r_eff, nnz=steps.nnz, singular_values=np.asarray(s[:k], np.float64),
                 product_algorithmic_bytes=last_product["algorithmic_bytes"], last_product_ms=last_product["kernel_ms"])
    return USER_factors, ITEM_factors, stats


def compute_W_sparse_from_item_latent_factors(ITEM_factors, topK=100):
    """W_sparse (float32 csr, W[neighbour, item]): per item the `topK` largest entries of V V^T, zeros dropped
    (PureSVDRecommender.py:53-109).  The device scorer ranks V V^T row by row; the kept values are recomputed from the chosen rows."""
    V = np.ascontiguousarray(ITEM_factors, dtype=np.float32)
    n_items, k = V.shape
    topK = int(topK)
    if topK < 1 or topK > n_items:
        raise ValueError("kth(={}) out of bounds ({})".format(topK - 1, n_items))       # the reference's argpartition fails the same way
    nothing_seen = sps.csr_matrix((n_items, n_items), dtype=np.float32)
    scorer = MI355XScorer(V, V, nothing_seen)
    rows, cols, values = [], [], []
    block = int(max(1, min(1024, (1 << 25) // max(1, topK * k))))
    try:
        for start in range(0, n_items, block):
            items = np.arange(start, min(n_items, start + block), dtype=np.int32)
            ranked, _ = scorer.recommend(items, topK, remove_seen=False)
            valid = ranked >= 0
            neighbours = np.where(valid, ranked, 0)
            w = np.einsum("ntk,nk->nt", V[neighbours], V[items]).astype(np.float32)
            keep = valid & (w != 0.0)
            rows.append(neighbours[keep])
            cols.append(np.broadcast_to(items[:, None], ranked.shape)[keep])
            values.append(w[keep])
    finally:
        scorer.close()
    W = sps.csr_matrix((np.concatenate(values), (np.concatenate(rows), np.concatenate(cols))), shape=(n_items, n_items), dtype=np.float32)
    W.sort_indices()
    return W


class _PureSVDLogic:
    """Drop-in for PureSVDRecommender: `fit(num_factors=100, random_seed=None)` sets float32 USER_factors = U diag(Sigma) and
    ITEM_factors = V of the randomized SVD of URM_train."""

    RECOMMENDER_NAME = "PureSVDRecommender"

    def __init__(self, URM_train, verbose=True):
        super(_PureSVDLogic, self).__init__(URM_train, verbose=verbose)

    def fit(self, num_factors=100, random_seed=None):
        self._print("Computing SVD decomposition...")
        self.USER_factors, self.ITEM_factors, self.fit_stats = randomized_svd_device(self.URM_train, num_factors, random_seed)
        self._print("Computing SVD decomposition... Done!")


class _PureSVDItemLogic:
    """Drop-in for PureSVDItemRecommender: `fit(num_factors=100, topK=None, random_seed=None)` sets W_sparse, the column-wise topK of
    V V^T (every item when topK is None)."""

    RECOMMENDER_NAME = "PureSVDItemRecommender"

    def __init__(self, URM_train, verbose=True):
        super(_PureSVDItemLogic, self).__init__(URM_train, verbose=verbose)

    def fit(self, num_factors=100, topK=None, random_seed=None):
        self._print("Computing SVD decomposition...")
        _, ITEM_factors, self.fit_stats = randomized_svd_device(self.URM_train, num_factors, random_seed)
        if topK is None:
            topK = self.n_items
        self.W_sparse = sps.csr_matrix(compute_W_sparse_from_item_latent_factors(ITEM_factors, topK=topK))
        self._print("Computing SVD decomposition... Done!")


class PureSVDRecommender(_PureSVDLogic, GpuScoringMixin, BaseMatrixFactorizationRecommender):
    pass


class PureSVDItemRecommender(_PureSVDItemLogic, GpuSimilarityScoringMixin, BaseItemSimilarityMatrixRecommender):
    pass
