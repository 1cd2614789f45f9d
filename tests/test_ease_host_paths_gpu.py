"""What the host side of the EASE_R handle reports around both eliminations (csrc/ease.hip, csrc/ease_pivot.hip, csrc/ease_plan.h):
the steps and launches of a shape, the figures of get_stats, the launches the weights and the top-K add, the refusals' exact text and
step, what stays readable after a refusal and that the handle takes a new matrix afterwards.  The numeric tests (test_ease_gpu.py,
test_ease_pivoted_gpu.py) would not notice a change in any of these.  Every matrix has at most 200 rows: a one-row matrix, a whole
tile, a tile and one row (for block 64: two blocks of the identity tail), a ragged last panel."""
import numpy as np
import pytest

from recsys2019_deeplearning_evaluation_amd import MI355XEase
import ease_cases as EC
import ease_pivoted_cases as PC

pytestmark = pytest.mark.gpu

SIZES = (1, 128, 129, 200)
NOT_SPD = "the matrix is not positive definite: a pivot <= 0 (or NaN) in elimination step %d of %d (block size %d)"
SINGULAR = "the matrix is singular: a pivot that is 0 (or NaN) in elimination step %d of %d (block size %d)"


def steps_of(n, block):
    return -(-n // 128) * 128 // block


def pivoted_launches(n, block, gathered):
    """init and widen; per step the six launches of the block step; per panel that holds rows of the matrix a load, a swap, a pick per
    column and an elimination after every column but the panel's last; the gather."""
    full, ragged = divmod(n, block)
    return 2 + 6 * steps_of(n, block) + full * (2 * block + 1) + (2 * ragged + 1 if ragged else 0) + (1 if gathered else 0)


@pytest.fixture(params=[(n, block) for n in SIZES for block in PC.BLOCKS], ids=lambda p: "n%d-block%d" % p)
def handle(request, gpu, monkeypatch):
    n, block = request.param
    monkeypatch.setenv("MI355REC_EASE_BLOCK", str(block))
    ease = MI355XEase(n)
    yield ease, n, block
    ease.close()


def check_stats(ease, n, block, launches, cell_bytes):
    steps = steps_of(n, block)
    st = ease.stats()
    assert st["n_units"] == steps and st["n_launches"] == launches and st["n_timed"] == 1
    assert st["algorithmic_flops"] == 2.0 * n ** 3 and st["algorithmic_bytes"] == 2.0 * cell_bytes * n * n * steps
    assert st["kernel_ms"] == st["call_ms"] == ease.fit_info()["invert_ms"] > 0


def test_unpivoted_inverse_reports_its_steps_and_launches(handle):
    ease, n, block = handle
    steps = steps_of(n, block)
    S = EC.random_spd(n)
    ease.set_matrix(S)
    ease.invert()
    info = ease.fit_info()
    assert (info["block"], info["steps"], info["failed_step"], info["launches"]) == (block, steps, -1, 4 * steps)
    check_stats(ease, n, block, 4 * steps, 4)
    with pytest.raises(ValueError, match="no pivoted inverse has run"):
        ease.pivot_info()
    P64 = np.linalg.inv(S.astype(np.float64))
    assert np.abs(ease.get_matrix() - P64).max() < EC.BAR * np.abs(P64).max()
    W = ease.get_dense()
    assert ease.fit_info()["launches"] == 4 * steps + 2 and ease.fit_info()["topk_ms"] > 0
    assert np.array_equal(ease.get_dense(), W) and ease.fit_info()["launches"] == 4 * steps + 2        # scaled once only
    idx, val = ease.get_topk(min(5, n))
    assert ease.fit_info()["launches"] == 4 * steps + 3
    assert idx.shape == val.shape == (n, min(5, n))


def test_pivoted_inverse_reports_its_steps_and_launches(handle):
    ease, n, block = handle
    steps = steps_of(n, block)
    G = PC.random_symmetric(n)
    ease.set_matrix(G)
    ease.invert(pivoted=True)
    info = ease.fit_info()
    launches = pivoted_launches(n, block, gathered=True)
    assert (info["block"], info["steps"], info["failed_step"], info["launches"]) == (block, steps, -1, launches)
    check_stats(ease, n, block, launches, 8)
    pivot = ease.pivot_info()
    assert 0 <= pivot["moved_rows"] <= n and 0 < pivot["min_pivot"] < np.inf and pivot["pivot_ms"] > 0 and pivot["update_ms"] > 0
    if n == 1:
        assert pivot["moved_rows"] == 0 and pivot["min_pivot"] == abs(float(G[0, 0]))
    assert np.isfinite(ease.get_matrix()).all()                     # (how close it is: test_ease_pivoted_gpu.py)
    ease.get_dense()
    assert ease.fit_info()["launches"] == launches + 2


@pytest.mark.parametrize("what", ["zero_last_row", "all_zero"])
def test_a_singular_matrix_is_refused_with_its_step_and_the_handle_recovers(handle, what):
    ease, n, block = handle
    steps = steps_of(n, block)
    G = PC.random_symmetric(n).copy()
    if what == "zero_last_row":
        G[n - 1, :] = 0.0
        step = (n - 1) // block
    else:
        G[:] = 0.0
        step = 0
    ease.set_matrix(G)
    with pytest.raises(FloatingPointError) as exc:
        ease.invert(pivoted=True)
    assert str(exc.value) == SINGULAR % (step, steps, block)
    info = ease.fit_info()
    launches = pivoted_launches(n, block, gathered=False)
    assert (info["failed_step"], info["launches"]) == (step, launches)
    check_stats(ease, n, block, launches, 8)
    pivot = ease.pivot_info()                                       # of the run that failed
    assert set(pivot) == {"moved_rows", "min_pivot", "pivot_ms", "update_ms"} and 0 <= pivot["moved_rows"] <= n
    for call in (ease.get_dense, ease.invert, lambda: ease.invert(pivoted=True)):
        with pytest.raises(ValueError):
            call()
    G = PC.random_symmetric(n)
    ease.set_matrix(G)
    with pytest.raises(ValueError):
        ease.pivot_info()                                           # (no pivoted inverse has run on the matrix that is set now)
    ease.invert(pivoted=True)
    assert ease.fit_info()["failed_step"] == -1 and ease.fit_info()["launches"] == pivoted_launches(n, block, gathered=True)
    assert np.isfinite(ease.get_matrix()).all()


def test_an_indefinite_matrix_is_refused_by_the_unpivoted_route_with_its_step_and_the_handle_recovers(handle):
    ease, n, block = handle
    steps = steps_of(n, block)
    S = EC.random_spd(n)
    G = S.copy()
    G[n - 1, n - 1] = -1.0              # every leading block before the last row is positive definite: the last pivot is the first <= 0
    ease.set_matrix(G)
    with pytest.raises(FloatingPointError) as exc:
        ease.invert()
    step = (n - 1) // block
    assert str(exc.value) == NOT_SPD % (step, steps, block)
    info = ease.fit_info()
    assert (info["failed_step"], info["launches"]) == (step, 4 * steps)
    check_stats(ease, n, block, 4 * steps, 4)
    for call in (ease.get_dense, ease.invert, lambda: ease.invert(pivoted=True), ease.pivot_info):
        with pytest.raises(ValueError):
            call()
    with pytest.raises(ValueError, match="^set_diagonal needs a matrix that has been set and not yet inverted$"):
        ease.set_diagonal(np.ones(n, np.float32))
    ease.set_matrix(S)
    ease.invert()
    assert ease.fit_info()["failed_step"] == -1
    P64 = np.linalg.inv(S.astype(np.float64))
    assert np.abs(ease.get_matrix() - P64).max() < EC.BAR * np.abs(P64).max()
    with pytest.raises(ValueError, match="^invert needs a matrix that has been set and not yet inverted$"):
        ease.invert()
    with pytest.raises(ValueError, match="^invert_pivoted needs a matrix that has been set and not yet inverted$"):
        ease.invert(pivoted=True)
