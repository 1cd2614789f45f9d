"""AsySVD's user factors estimated on the device (mi355rec_asy_user_factors, mi355rec_mf_asy_user_factors; asysvd_user_factors,
MatrixFactorization_MI355X_Epoch.estimate_user_factors, `user_factor_estimate = "device"`): the bytes of the host estimate -- SciPy's
URM.dot(Y) and NumPy's row division -- for every case and k, from a training handle that goes on training, and through a whole
early-stopping fit; test_asysvd_estimate_spec.py shows that another order, a fused multiply-add, float32 sums, a reciprocal or a float32
divisor would each change those bytes on the same inputs."""
import numpy as np
import pytest
import scipy.sparse as sps

from recsys2019_deeplearning_evaluation_amd import (MatrixFactorization_AsySVD_MI355X, MatrixFactorization_MI355X_Epoch, _native,
                                                    asysvd_user_factors)
from recsys2019_deeplearning_evaluation_amd import matrix_factorization as MF
from recsys2019_deeplearning_evaluation_amd import recommender_base as RB
from recsys2019_deeplearning_evaluation_amd.evaluation import EvaluatorHoldout_MI355X
from recsys2019_deeplearning_evaluation_amd.reference_binding import bind
from asysvd_estimate_cases import (CASES, EMPTY_ROWS, FULL_ROW, K_LIST, K_MAX, URM_ADVERSARIAL, URM_TRAIN_UNSORTED, draw_Y, host_estimate,
                                   reference)
from hand_off_cases import EMPTY_USER, N_ITEMS, N_USERS, URM_TEST, URM_TRAIN

pytestmark = pytest.mark.gpu


# ---- the stateless entry ------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("case", sorted(CASES))
@pytest.mark.parametrize("k", K_LIST)
def test_the_stateless_estimate_is_the_host_estimate_bit_for_bit(gpu, case, k):
    X = CASES[case]
    Y, want = reference(case, k)
    sorted_before = X.has_sorted_indices
    got = asysvd_user_factors(X, Y)
    assert got.dtype == np.float64 and got.shape == want.shape
    differ = np.flatnonzero((got.view(np.uint64) != want.view(np.uint64)).any(axis=1))
    print("%s k=%d: %d of %d rows differ%s" % (case, k, len(differ), len(got), "" if not len(differ) else ", the first is row %d, max |diff| %.3e"
                                               % (differ[0], np.abs(got - want).max())))
    assert got.tobytes() == want.tobytes()
    empty = got[EMPTY_ROWS[case]]
    assert not empty.any() and not np.signbit(empty).any()          # +0.0, not divided by 0
    assert X.has_sorted_indices == sorted_before                    # the caller's matrix is read, never sorted
    assert asysvd_user_factors(X, Y).tobytes() == got.tobytes()     # no atomics: a second call gives the same bytes


def test_the_stateless_estimate_follows_the_storage_order(gpu):
    """The unsorted cases are unsorted for a reason: summed in sorted order the bytes are others, on the host and on the device alike."""
    for X in (URM_ADVERSARIAL, URM_TRAIN_UNSORTED):
        Y = draw_Y(X.shape[1], 8)
        ordered = X.sorted_indices()
        assert not X.has_sorted_indices and ordered.has_sorted_indices
        as_stored, in_order = asysvd_user_factors(X, Y), asysvd_user_factors(ordered, Y)
        assert as_stored.tobytes() == host_estimate(X, Y).tobytes() and in_order.tobytes() == host_estimate(ordered, Y).tobytes()
        assert as_stored.tobytes() != in_order.tobytes()
    full = asysvd_user_factors(URM_ADVERSARIAL[FULL_ROW], draw_Y(URM_ADVERSARIAL.shape[1], 64))       # one row that holds every column
    assert full.tobytes() == host_estimate(URM_ADVERSARIAL[FULL_ROW], draw_Y(URM_ADVERSARIAL.shape[1], 64)).tobytes()


def test_the_stateless_estimate_takes_float64_ratings_that_float32_holds_and_refuses_the_others(gpu):
    Y = draw_Y(N_ITEMS, 8)
    wide = sps.csr_matrix(URM_TRAIN, dtype=np.float64)
    assert asysvd_user_factors(wide, Y).tobytes() == host_estimate(wide, Y).tobytes()
    wide.data[5] = 1.0 + 2.0 ** -40
    with pytest.raises(ValueError, match="float32 does not represent"):
        asysvd_user_factors(wide, Y)
    with pytest.raises(ValueError, match="ITEM_factors_Y has shape"):
        asysvd_user_factors(URM_TRAIN, Y[:-1])
    with pytest.raises(NotImplementedError, match="exceeds 256"):
        asysvd_user_factors(URM_TRAIN, np.zeros((N_ITEMS, K_MAX + 1)))


def test_bad_row_pointers_and_ids_are_refused_with_the_output_untouched(gpu):
    X, Y = URM_ADVERSARIAL, np.ascontiguousarray(draw_Y(URM_ADVERSARIAL.shape[1], 8))
    out = np.full((X.shape[0], 8), -3.5)
    divisor = np.sqrt(np.ediff1d(X.indptr)).astype(np.float64)
    p, lib = _native.ptr, _native.load()

    def call(indptr, indices):
        indptr, indices = np.ascontiguousarray(indptr, np.int32), np.ascontiguousarray(indices, np.int32)
        return lib.mi355rec_asy_user_factors(X.shape[0], X.shape[1], 8, p(indptr), p(indices), p(X.data), p(Y), p(divisor), p(out))

    late, back, high, low = X.indptr.copy(), X.indptr.copy(), X.indices.copy(), X.indices.copy()
    late[0], back[-1], high[100], low[0] = 2, back[-2] - 1, X.shape[1], -1
    for indptr, indices in ((late, X.indices), (back, X.indices), (X.indptr, high), (X.indptr, low)):
        assert call(indptr, indices) == _native.E_INVALID
        assert (out == -3.5).all()
    assert call(X.indptr, X.indices) == 0 and out.tobytes() == host_estimate(X, Y).tobytes()


# ---- the handle entry ---------------------------------------------------------------------------------------------------------------------

def _asy_epoch(k, use_bias, precision="auto", algorithm="ASY_SVD", seed=31):
    return MatrixFactorization_MI355X_Epoch(URM_TRAIN, n_factors=k, algorithm_name=algorithm, batch_size=1, learning_rate=0.01,
                                            use_bias=use_bias, sgd_mode="adagrad", user_reg=0.01, item_reg=0.01, bias_reg=0.01,
                                            random_seed=seed, precision=precision)


@pytest.mark.parametrize("use_bias", [True, False])
@pytest.mark.parametrize("k", [3, 24, 65, K_MAX])
def test_a_training_handle_estimates_its_user_factors_and_goes_on_training(gpu, k, use_bias):
    asy, plain = _asy_epoch(k, use_bias), _asy_epoch(k, use_bias)
    assert asy.precision == "fp64"
    for handle in (asy, plain):
        handle.epochIteration_Cython(2)
    Y = asy.get_USER_factors()
    assert Y.dtype == np.float64 and Y.shape == (N_ITEMS, k) and np.abs(Y).max() > 0
    want = host_estimate(URM_TRAIN, Y)
    got = asy.estimate_user_factors()
    st = asy.stats()
    assert got.dtype == np.float64 and got.tobytes() == want.tobytes()
    assert not got[EMPTY_USER].any() and not np.signbit(got[EMPTY_USER]).any()
    assert st["n_launches"] == 1 and 0 < st["kernel_ms"] <= st["call_ms"]
    assert st["algorithmic_bytes"] == URM_TRAIN.nnz * (8 * k + 8) + N_USERS * k * 8
    assert asy.estimate_user_factors().tobytes() == got.tobytes()
    # a divisor of the caller's: divided by it, and a 0 leaves the row as the product gives it
    divisor = np.arange(N_USERS, dtype=np.float64) % 5
    product = URM_TRAIN.dot(Y)
    product[divisor > 0] /= divisor[divisor > 0][:, None]
    assert asy.estimate_user_factors(divisor).tobytes() == product.tobytes()
    # training goes on as if nothing had been asked
    for handle in (asy, plain):
        handle.epochIteration_Cython()
    for a, b in zip(asy._download(use_bias), plain._download(use_bias)):
        assert (a is None and b is None) or a.tobytes() == b.tobytes()
    assert asy.get_USER_factors().tobytes() != Y.tobytes()
    asy.close()
    plain.close()


def test_other_handles_are_refused(gpu):
    divisor, out = np.ones(N_USERS), np.full((N_USERS, 8), 1.5)
    lib = _native.load()
    bpr = MatrixFactorization_MI355X_Epoch(URM_TRAIN, n_factors=8, algorithm_name="MF_BPR", batch_size=16, random_seed=1, sgd_mode="adagrad")
    asy32 = _asy_epoch(8, False, precision="fp32")
    for handle, match in ((bpr, "ASY_SVD"), (asy32, "fp64")):
        with pytest.raises(ValueError, match=match):
            handle.estimate_user_factors()
        assert lib.mi355rec_mf_asy_user_factors(handle._h, _native.ptr(divisor), _native.ptr(out)) == _native.E_UNSUPPORTED
        assert (out == 1.5).all()
        handle.close()
    asy = _asy_epoch(8, False)
    with pytest.raises(ValueError, match="row_divisor has shape"):
        asy.estimate_user_factors(np.ones(N_USERS + 1))
    asy.close()
    with pytest.raises(ValueError, match="closed"):
        asy.estimate_user_factors()


# ---- a device-mode fit is the host-mode fit -------------------------------------------------------------------------------------------------

FIT = dict(epochs=6, validation_every_n=1, stop_on_validation=True, lower_validations_allowed=2, validation_metric="MAP", num_factors=24,
           learning_rate=0.01, sgd_mode="adagrad", use_bias=True, item_reg=0.01, user_reg=0.01, bias_reg=0.01, random_seed=29)
MODEL_ATTRIBUTES = ("USER_factors", "ITEM_factors", "ITEM_factors_Y_best", "USER_bias", "ITEM_bias", "GLOBAL_bias")


def _bound_class():
    return bind(RB.BaseMatrixFactorizationRecommender, RB.BaseItemSimilarityMatrixRecommender, RB.BaseUserSimilarityMatrixRecommender,
                RB.Incremental_Training_Early_Stopping).MatrixFactorization_AsySVD_MI355X


class _Recording:
    """A thin wrapper around an evaluator: every result dict of a fit and the USER_factors each validation saw, in order."""

    def __init__(self, evaluator):
        self.evaluator, self.results, self.estimates = evaluator, [], []

    def evaluateRecommender(self, recommender):
        self.estimates.append(recommender.USER_factors.copy())
        results, string = self.evaluator.evaluateRecommender(recommender)
        self.results.append(results)
        return results, string


def _fit(cls, URM, mode):
    rec = cls(URM, verbose=False)
    if mode is not None:
        rec.user_factor_estimate = mode
    recording = _Recording(EvaluatorHoldout_MI355X(URM_TEST, [5, 10], verbose=False))
    rec.fit(evaluator_object=recording, **FIT)
    recording.evaluator.close()
    return rec, recording


def _assert_same_fit(a, b):
    (rec_a, seen_a), (rec_b, seen_b) = a, b
    assert len(seen_a.results) >= 2 and seen_a.results == seen_b.results
    assert rec_a.epochs_best == rec_b.epochs_best and rec_a.best_validation_metric == rec_b.best_validation_metric
    assert [e.tobytes() for e in seen_a.estimates] == [e.tobytes() for e in seen_b.estimates]
    for name in MODEL_ATTRIBUTES:
        x, y = np.asarray(getattr(rec_a, name)), np.asarray(getattr(rec_b, name))
        assert x.dtype == y.dtype and x.shape == y.shape and x.tobytes() == y.tobytes(), name


@pytest.fixture
def calls(monkeypatch):
    """How often either new entry is reached: the epoch object's method and the module function the logic class calls."""
    counts = {"handle": 0, "stateless": 0}
    original_method, original_function = MatrixFactorization_MI355X_Epoch.estimate_user_factors, MF.asysvd_user_factors

    def method(self, *args, **kwargs):
        counts["handle"] += 1
        return original_method(self, *args, **kwargs)

    def function(*args, **kwargs):
        counts["stateless"] += 1
        return original_function(*args, **kwargs)

    monkeypatch.setattr(MatrixFactorization_MI355X_Epoch, "estimate_user_factors", method)
    monkeypatch.setattr(MF, "asysvd_user_factors", function)
    return counts


@pytest.mark.parametrize("variant", ["package", "bound", "unsorted"])
def test_a_device_mode_fit_is_the_host_mode_fit(gpu, calls, variant):
    cls = _bound_class() if variant == "bound" else MatrixFactorization_AsySVD_MI355X
    URM = URM_TRAIN_UNSORTED if variant == "unsorted" else URM_TRAIN
    assert URM.has_sorted_indices == (variant != "unsorted")
    host = _fit(cls, URM, "host")
    assert host[0].URM_train.has_sorted_indices == (variant != "unsorted")     # the recommender's copy keeps the order
    _assert_same_fit(host, _fit(cls, URM, "host"))      # the premise: two host-mode fits with one seed are byte-equal
    assert calls == {"handle": 0, "stateless": 0}
    device = _fit(cls, URM, "device")
    validations = len(device[1].results) + 1            # (and the initial model, before training)
    assert calls == ({"handle": 0, "stateless": validations} if variant == "unsorted" else {"handle": validations, "stateless": 0})
    _assert_same_fit(device, host)
    assert device[0].USER_factors.dtype == np.float64
    assert len({e.tobytes() for e in device[1].estimates}) == len(device[1].estimates)      # every validation saw another model


def test_a_default_fit_reaches_neither_entry(gpu, calls):
    rec, recording = _fit(MatrixFactorization_AsySVD_MI355X, URM_TRAIN, None)
    assert rec.user_factor_estimate == "host" and len(recording.results) >= 2
    rec.set_URM_train(URM_TRAIN, estimate_item_similarity_for_cold_users=True)
    assert calls == {"handle": 0, "stateless": 0}


def test_the_cold_users_of_a_new_urm_get_the_host_modes_factors(gpu, calls):
    rng = np.random.default_rng(8)
    new = sps.csr_matrix(sps.random(N_USERS, N_ITEMS, density=0.03, format="csr", dtype=np.float32, random_state=np.random.RandomState(3)))
    new.data = rng.integers(1, 6, new.nnz).astype(np.float32)
    factors = {}
    for mode in ("host", "device"):
        rec, _ = _fit(MatrixFactorization_AsySVD_MI355X, URM_TRAIN, mode)
        before = dict(calls)
        rec.set_URM_train(new, estimate_item_similarity_for_cold_users=True)
        assert calls["stateless"] - before["stateless"] == (mode == "device") and calls["handle"] == before["handle"]
        factors[mode] = rec.USER_factors
        assert rec.USER_factors.tobytes() == host_estimate(rec.URM_train, rec.ITEM_factors_Y_best).tobytes()
    assert factors["device"].dtype == np.float64 and factors["device"].tobytes() == factors["host"].tobytes()
