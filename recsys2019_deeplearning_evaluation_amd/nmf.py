"""NMF on MI355X: host front-end of the nmf_* entry points of libmi355rec.so.

Mirrors NMFRecommender (MatrixFactorization/NMFRecommender.py), which hands URM_train to sklearn.decomposition.NMF (max_iter 500,
tol 1e-4, shuffle=True, no regularisation) and then calls its `transform`.  That is two solves: stage 1 for W (users x k) and H
(k x items) from the `random` or `nndsvda` initialisation, stage 2 for W alone with H fixed, started from zero (coordinate descent)
or from sqrt(mean / k) (multiplicative update).  The half-sweeps, multiplicative updates and divergences run on the device
(csrc/nmf.hip); the loop stays here because every iteration needs the stop statistic, and coordinate descent a fresh permutation,
on the host.  Every random number is drawn from NumPy exactly as sklearn draws it -- the initialisation (H before W), one
permutation per half-sweep, stage 2 from a fresh RandomState of the same integer seed -- so a fit with `random_seed=None` leaves
`np.random` where the reference's fit leaves it.  Between the upload of the initial blocks and the download of the factors only
permutations (4 k bytes) go to the device and one float64 per iteration comes back.
"""
import ctypes as C
import time

import numpy as np

from . import _native as N
from .block_steps import BlockPairSteps
from .pure_svd import check_random_state, randomized_svd_device
from .recommender_base import BaseMatrixFactorizationRecommender, check_matrix
from .scoring import GpuScoringMixin

MAX_ITER = 500                    # NMFRecommender.py:66
TOL = 1e-4                        # sklearn's default
LOSS_CODES = {"frobenius": 0, "kullback-leibler": 1}
PHASES = ("product_ms", "gemm_ms", "sweep_ms", "scale_ms", "sddmm_ms", "reduce_ms")


def check_permutation(permutation, k):
    """int32 copy of `permutation`; ValueError unless it holds every one of 0 .. k-1 once."""
    p = np.asarray(permutation)
    if p.shape != (k,) or not np.array_equal(np.sort(p), np.arange(k)):
        raise ValueError("not a permutation of 0 .. %d" % (k - 1))
    return N.as_i32(p)


class NMF_MI355X_Steps(BlockPairSteps):
    """The URM in both layouts and the two float32 blocks on the device: side 0 is W (n_users, k), side 1 is Ht = H^T (n_items, k)."""
    _PREFIX = "mi355rec_nmf"
    _SIDE_NAMES = ("W, users", "Ht, items")
    k = property(lambda self: self.width)

    def fill_block(self, side, value):
        self._call("fill_block", self._side(side), C.c_float(value))

    def cd_sweep(self, side, permutation, reuse=False, want_violation=True):
        """One half-sweep of block[side] in the order of `permutation`.  The violation is added to a total on the device; with
        want_violation that total is returned and reset, otherwise None (the W half of an iteration: the H half returns both)."""
        p = check_permutation(permutation, self.k)
        v = C.c_double()
        self._call("cd_sweep", self._side(side), N.ptr(p), int(bool(reuse)), C.byref(v) if want_violation else None)
        return v.value if want_violation else None

    def mu_step(self, side, loss, reuse=False):
        if loss not in LOSS_CODES:
            raise ValueError("loss %r: one of %s" % (loss, sorted(LOSS_CODES)))
        self._call("mu_step", self._side(side), LOSS_CODES[loss], int(bool(reuse)))

    def divergence(self, loss):
        if loss not in LOSS_CODES:
            raise ValueError("loss %r: one of %s" % (loss, sorted(LOSS_CODES)))
        d = C.c_double()
        self._call("divergence", LOSS_CODES[loss], C.byref(d))
        return d.value

    def error(self, loss):
        """sklearn's _beta_divergence(..., square_root=True): only the Kullback-Leibler sum is clipped at zero."""
        d = np.float64(self.divergence(loss))
        with np.errstate(invalid="ignore"):
            return np.sqrt(2 * d) if loss == "frobenius" else np.sqrt(2 * max(d, 0.0))

    def fit_info(self):
        ms = (C.c_double * len(PHASES))()
        tail = self._fit_info_tail(ms)
        return dict({name: ms[n] for n, name in enumerate(PHASES)}, **tail)


def _nndsvda(A, k, random_seed, stats):
    """sklearn's _initialize_nmf(init="nndsvda") (_nmf.py:316-361) with the device randomized SVD: S is recovered as the column norms
    of U diag(S); the sign of a component does not matter to the split below (x -> -x swaps the positive and the negative pair, and
    the larger product wins either way)."""
    US, V, svd_stats = randomized_svd_device(A, k, random_seed)
    stats["svd"] = {key: svd_stats[key] for key in ("create_bytes", "h2d_bytes", "d2h_bytes", "host_fallbacks", "svd_on_host", "products")}
    S = np.linalg.norm(US.astype(np.float64), axis=0).astype(np.float32)
    U = US / np.where(S > 0, S, np.float32(1))
    Vt = np.ascontiguousarray(V.T)
    W, H = np.zeros_like(U), np.zeros_like(Vt)
    W[:, 0] = np.sqrt(S[0]) * np.abs(U[:, 0])
    H[0, :] = np.sqrt(S[0]) * np.abs(Vt[0, :])

    def norm(x):
        return np.sqrt(np.dot(x, x))

    for j in range(1, k):
        x, y = U[:, j], Vt[j, :]
        x_p, y_p = np.maximum(x, 0), np.maximum(y, 0)
        x_n, y_n = np.abs(np.minimum(x, 0)), np.abs(np.minimum(y, 0))
        x_p_nrm, y_p_nrm, x_n_nrm, y_n_nrm = norm(x_p), norm(y_p), norm(x_n), norm(y_n)
        m_p, m_n = x_p_nrm * y_p_nrm, x_n_nrm * y_n_nrm
        with np.errstate(invalid="ignore", divide="ignore"):
            if m_p > m_n:
                u, v, sigma = x_p / x_p_nrm, y_p / y_p_nrm, m_p
            else:
                u, v, sigma = x_n / x_n_nrm, y_n / y_n_nrm, m_n
        lbd = np.sqrt(S[j] * sigma)
        W[:, j], H[j, :] = lbd * u, lbd * v
    W[W < 1e-6] = 0
    H[H < 1e-6] = 0
    avg = A.mean()
    W[W == 0] = avg
    H[H == 0] = avg
    return W, H


def nmf_device(URM_train, num_factors, solver="multiplicative_update", init_type="random", beta_loss="frobenius", random_seed=None):
    """(USER_factors = transform(URM), ITEM_factors = components_.T, stats) of the reference's NMF fit.  `solver` is "coordinate_descent"
    or "multiplicative_update", `init_type` "random" or "nndsvda", `beta_loss` "frobenius" or "kullback-leibler"."""
    t_start = time.perf_counter()
    A = check_matrix(URM_train, "csr", dtype=np.float32)
    n_users, n_items = A.shape
    k = int(num_factors)
    if k < 1:
        raise ValueError("num_factors must be at least 1, got %d" % k)
    if solver not in ("coordinate_descent", "multiplicative_update"):
        raise ValueError("solver %r: 'coordinate_descent' or 'multiplicative_update'" % (solver,))
    if init_type not in ("random", "nndsvda"):
        raise ValueError("init_type %r: 'random' or 'nndsvda'" % (init_type,))
    if beta_loss not in LOSS_CODES:
        raise ValueError("beta_loss %r: one of %s" % (beta_loss, sorted(LOSS_CODES)))
    cd = solver == "coordinate_descent"
    if cd and beta_loss != "frobenius":
        raise ValueError("Invalid beta_loss parameter: solver 'cd' does not handle beta_loss = %r" % (beta_loss,))
    if init_type != "random" and k > min(n_users, n_items):
        raise ValueError("init = '{}' can only be used when n_components <= min(n_samples, n_features)".format(init_type))
    if A.nnz and A.data.min() < 0:
        raise ValueError("Negative values in data passed to NMF (input X)")
    stats = {"draw_s": 0.0}

    def timed_draw(draw):
        t = time.perf_counter()
        out = draw()
        stats["draw_s"] += time.perf_counter() - t
        return out

    # ---- the initialisation, on the host --------------------------------------------------------------------------------------------
    mean = A.mean()                                    # float32, as sklearn computes it
    avg = np.sqrt(mean / k)
    if init_type == "random":
        rng = check_random_state(random_seed)
        H0 = timed_draw(lambda: avg * rng.standard_normal(size=(k, n_items)).astype(np.float32, copy=False))
        W0 = timed_draw(lambda: avg * rng.standard_normal(size=(n_users, k)).astype(np.float32, copy=False))
        np.abs(H0, out=H0)
        np.abs(W0, out=W0)
    else:
        W0, H0 = _nndsvda(A, k, random_seed, stats)
    t_init = time.perf_counter()

    steps = NMF_MI355X_Steps(A, k)
    try:
        t_created = time.perf_counter()
        steps.set_block(0, W0)
        steps.set_block(1, np.ascontiguousarray(H0.T))
        info0 = steps.fit_info()

        def solve(update_H):
            """One sklearn solve: (n_iter, trajectory of the stop statistic)."""
            trajectory = []
            if cd:
                rng = check_random_state(random_seed)
                violation_init = None
                for n_iter in range(1, MAX_ITER + 1):
                    p = timed_draw(lambda: rng.permutation(k))
                    violation = steps.cd_sweep(0, p, reuse=not update_H and n_iter > 1, want_violation=not update_H)
                    if update_H:
                        p = timed_draw(lambda: rng.permutation(k))
                        violation = steps.cd_sweep(1, p)
                    trajectory.append(violation)
                    if n_iter == 1:
                        violation_init = violation
                    if violation_init == 0 or violation / violation_init <= TOL:
                        break
                return n_iter, trajectory
            error_at_init = previous_error = steps.error(beta_loss)
            trajectory.append(float(error_at_init))
            for n_iter in range(1, MAX_ITER + 1):
                steps.mu_step(0, beta_loss, reuse=not update_H and n_iter > 1)
                if update_H:
                    steps.mu_step(1, beta_loss)
                if n_iter % 10 == 0:
                    error = steps.error(beta_loss)
                    trajectory.append(float(error))
                    with np.errstate(invalid="ignore", divide="ignore"):
                        if (previous_error - error) / error_at_init < TOL:
                            break
                    previous_error = error
            return n_iter, trajectory

        n_iter_fit, trajectory_fit = solve(True)
        info1 = steps.fit_info()
        t_fit = time.perf_counter()
        # stage 2, sklearn's transform: W alone, H fixed (_check_w_h, _nmf.py:1228-1233)
        steps.fill_block(0, 0.0 if cd else float(np.sqrt(mean / k)))
        n_iter_transform, trajectory_transform = solve(False)
        info2 = steps.fit_info()
        t_transform = time.perf_counter()
        USER_factors, ITEM_factors = steps.get_block(0), steps.get_block(1)
        info = steps.fit_info()
    finally:
        steps.close()
    stats.update(info)
    stats.update(n_iter_fit=n_iter_fit, n_iter_transform=n_iter_transform, trajectory_fit=trajectory_fit,
                 trajectory_transform=trajectory_transform, k=k, nnz=int(A.nnz),
                 fit_phase_ms={p: info1[p] - info0[p] for p in PHASES}, transform_phase_ms={p: info2[p] - info1[p] for p in PHASES},
                 init_block_bytes=4 * k * (n_users + n_items))
    # wall seconds: the initialisation (drawn or NNDSVD), building the handle, the two solves, the download
    stats.update(init_s=t_init - t_start, create_s=t_created - t_init, fit_s=t_fit - t_created, transform_s=t_transform - t_fit,
                 download_s=time.perf_counter() - t_transform)
    return USER_factors, ITEM_factors, stats


class _NMFLogic:
    """Drop-in for NMFRecommender: `fit(num_factors=100, l1_ratio=0.5, solver="multiplicative_update", init_type="random",
    beta_loss="frobenius", verbose=False, random_seed=None)` sets float32 USER_factors = NMF.transform(URM_train) and
    ITEM_factors = NMF.components_.T.  The reference passes no alpha_W, so l1_ratio has no numerical effect."""

    RECOMMENDER_NAME = "NMFRecommender"

    SOLVER_VALUES = {"coordinate_descent": "cd",
                     "multiplicative_update": "mu"}

    INIT_VALUES = ["random", "nndsvda"]

    BETA_LOSS_VALUES = ["frobenius", "kullback-leibler"]

    def __init__(self, URM_train, verbose=True):
        super(_NMFLogic, self).__init__(URM_train, verbose=verbose)

    def fit(self, num_factors=100, l1_ratio=0.5, solver="multiplicative_update", init_type="random", beta_loss="frobenius", verbose=False,
            random_seed=None):
        assert l1_ratio >= 0 and l1_ratio <= 1, "{}: l1_ratio must be between 0 and 1, provided value was {}".format(self.RECOMMENDER_NAME, l1_ratio)

        if solver not in self.SOLVER_VALUES:
            raise ValueError("Value for 'solver' not recognized. Acceptable values are {}, provided was '{}'".format(self.SOLVER_VALUES.keys(), solver))

        if init_type not in self.INIT_VALUES:
            raise ValueError("Value for 'init_type' not recognized. Acceptable values are {}, provided was '{}'".format(self.INIT_VALUES, init_type))

        if beta_loss not in self.BETA_LOSS_VALUES:
            raise ValueError("Value for 'beta_loss' not recognized. Acceptable values are {}, provided was '{}'".format(self.BETA_LOSS_VALUES, beta_loss))

        self._print("Computing NMF decomposition...")
        self.USER_factors, self.ITEM_factors, self.fit_stats = nmf_device(self.URM_train, num_factors, solver, init_type, beta_loss, random_seed)
        self._print("Computing NMF decomposition... Done!")


class NMFRecommender(_NMFLogic, GpuScoringMixin, BaseMatrixFactorizationRecommender):
    pass
