"""What the PureSVD and the NMF handle share (csrc/blocks.h), on the device, through both handle types: the block round trip, the
product against float64 NumPy, the traffic counters against the accounting of csrc/blocks_plan.h, and the refusals that need a live
handle.  The URM is 5 x 1100 with rows of 0, 1, 512, 513 and 1025 cells -- empty, one piece, exactly one piece, two and three pieces
of 512 -- and its transpose (1100 short rows); the widths sit on both sides of each lane-group width (16 | 32 | 64) and of the 64-wide
Gram tile."""
import numpy as np
import pytest
import scipy.sparse as sps

import test_blocks_plan as BP
from recsys2019_deeplearning_evaluation_amd.nmf import NMF_MI355X_Steps
from recsys2019_deeplearning_evaluation_amd.pure_svd import PureSVD_MI355X_Steps
from test_pure_svd_gpu import U32

pytestmark = pytest.mark.gpu

ROW_LENGTHS = (0, 1, 512, 513, 1025)
N_COLS = 1100
WIDTHS = (1, 16, 17, 33, 65)
HANDLES = {"svd": PureSVD_MI355X_Steps, "nmf": NMF_MI355X_Steps}
_URMS = {}


def urm(transposed, values):
    """(the URM, rows of more than one piece in its CSR and in its CSC layout); made once per kind"""
    if (transposed, values) not in _URMS:
        rng = np.random.default_rng(11)
        rows = np.repeat(np.arange(len(ROW_LENGTHS)), ROW_LENGTHS)
        cols = np.concatenate([np.sort(rng.choice(N_COLS, n, replace=False)) for n in ROW_LENGTHS])
        data = np.ones(len(rows), np.float32) if values == "ones" else rng.uniform(0.5, 2.0, len(rows)).astype(np.float32)
        X = sps.csr_matrix((data, (rows, cols)), shape=(len(ROW_LENGTHS), N_COLS), dtype=np.float32)
        X = sps.csr_matrix(X.T) if transposed else X
        X.sort_indices()
        long_rows = [int((np.diff(M.indptr) > BP.SPLIT).sum()) for M in (X, sps.csc_matrix(X))]
        _URMS[(transposed, values)] = (X, long_rows)
    return _URMS[(transposed, values)]


@pytest.fixture(scope="module")
def plan(tmp_path_factory):
    return BP.build_shim(tmp_path_factory.mktemp("block_pair"))


def blocks_for(X, width, seed):
    rng = np.random.default_rng(seed)
    return [np.abs(rng.normal(size=(n, width))).astype(np.float32) + np.float32(0.25) for n in X.shape]


def counters(steps):
    info = steps.fit_info()
    return {name: info[name] for name in ("launches", "h2d_bytes", "d2h_bytes", "calls")}


@pytest.mark.parametrize("values", ["ones", "real"])
@pytest.mark.parametrize("width", WIDTHS)
@pytest.mark.parametrize("transposed", [False, True])
@pytest.mark.parametrize("kind", sorted(HANDLES))
def test_block_round_trip_is_bit_exact(gpu, kind, transposed, width, values):
    X, _ = urm(transposed, values)
    steps = HANDLES[kind](X, width)
    try:
        assert steps.fit_info()["all_ones"] == (values == "ones")
        blocks = blocks_for(X, width, width)
        for side in (0, 1):
            assert (steps.get_block(side) == 0).all()          # as create leaves it
            steps.set_block(side, blocks[side])
        for side in (1, 0):
            got = steps.get_block(side)
            assert got.shape == blocks[side].shape and got.tobytes() == blocks[side].tobytes(), (kind, side)
    finally:
        steps.close()


@pytest.mark.parametrize("values", ["ones", "real"])
@pytest.mark.parametrize("width", WIDTHS)
@pytest.mark.parametrize("transposed", [False, True])
def test_svd_product_against_float64_and_its_counters(gpu, plan, transposed, width, values):
    """Every cell within the float32 summation bound of its row, (length + 2) * 2^-24 * sum |s| |x| (as test_product_kernels_alone has
    it); a second call gives the same bits; fit_info counts what blocks_plan.h predicts, the second launch of long rows included."""
    X, long_rows = urm(transposed, values)
    want_counts, want_figures, _, _ = BP.accounting_of(plan, X.shape[0], X.shape[1], X.nnz, width, *long_rows)
    steps = PureSVD_MI355X_Steps(X, width)
    try:
        blocks = blocks_for(X, width, 100 + width)
        expect = dict(launches=0, h2d_bytes=0, d2h_bytes=0, calls=0)
        assert counters(steps) == expect
        for dst in (0, 1):
            S = sps.csr_matrix(X if dst == 0 else X.T, dtype=np.float64)
            B = blocks[1 - dst]
            steps.set_block(1 - dst, B)
            steps.product(dst)
            stats = steps.stats()
            got = steps.get_block(dst)
            want = S @ B.astype(np.float64)
            bound = (np.diff(S.indptr)[:, None] + 2) * U32 * (abs(S) @ np.abs(B).astype(np.float64))
            assert (np.abs(got - want) <= bound).all(), (width, values, dst, float((np.abs(got - want) - bound).max()))
            assert (got[np.diff(S.indptr) == 0] == 0).all()
            steps.product(dst)
            assert steps.get_block(dst).tobytes() == got.tobytes()
            assert want_counts["product_%d" % dst] == (2 if long_rows[dst] else 1)
            assert (stats["algorithmic_bytes"], stats["algorithmic_flops"], stats["n_units"]) == tuple(want_figures["product"]) + (X.nnz,)
            expect["launches"] += 2 * want_counts["product_%d" % dst]
            expect["h2d_bytes"] += want_counts["set_block_bytes_%d" % (1 - dst)]
            expect["d2h_bytes"] += 2 * want_counts["set_block_bytes_%d" % dst]
            expect["calls"] += 5
            assert counters(steps) == expect, (dst, long_rows)
        steps.gram(1)
        steps.apply(1, np.eye(width, dtype=np.float32))
        expect["launches"] += want_counts["gram"] + want_counts["apply"]
        expect["d2h_bytes"] += want_counts["gram_d2h_bytes"]
        expect["h2d_bytes"] += want_counts["apply_h2d_bytes"]
        expect["calls"] += 2
        assert counters(steps) == expect
    finally:
        steps.close()
    assert sorted(long_rows) == [0, 2]


@pytest.mark.parametrize("values", ["ones", "real"])
@pytest.mark.parametrize("width", WIDTHS)
@pytest.mark.parametrize("transposed", [False, True])
def test_nmf_calls_count_what_the_plan_predicts(gpu, plan, transposed, width, values):
    X, long_rows = urm(transposed, values)
    want, figures, _, _ = BP.accounting_of(plan, X.shape[0], X.shape[1], X.nnz, width, *long_rows)
    steps = NMF_MI355X_Steps(X, width)
    try:
        blocks = blocks_for(X, width, 200 + width)
        steps.set_block(0, blocks[0])
        steps.set_block(1, blocks[1])
        expect = dict(launches=0, h2d_bytes=want["set_block_bytes_0"] + want["set_block_bytes_1"], d2h_bytes=0, calls=2)
        assert counters(steps) == expect

        def called(launches, h2d=0, d2h=0):
            expect.update(launches=expect["launches"] + (want[launches] if launches else 0), h2d_bytes=expect["h2d_bytes"] + h2d, d2h_bytes=expect["d2h_bytes"] + d2h,
                          calls=expect["calls"] + 1)
            assert counters(steps) == expect, launches

        assert np.isfinite(steps.divergence("frobenius"))       # the product of the users' layout, into a buffer of its own
        called("divergence_loss0", d2h=want["scalar_bytes"])
        assert (steps.stats()["algorithmic_bytes"], steps.stats()["algorithmic_flops"]) == tuple(figures["divergence"])
        for side in (0, 1):
            steps.mu_step(side, "frobenius")
            called("mu_loss0_reuse0_side%d" % side)
            assert (steps.stats()["algorithmic_bytes"], steps.stats()["algorithmic_flops"]) == tuple(figures["mu_frobenius_%d" % side])
        steps.mu_step(1, "frobenius", reuse=True)
        called("mu_loss0_reuse1_side1")
        for side in (0, 1):
            steps.mu_step(side, "kullback-leibler")
            called("mu_loss1_reuse0_side%d" % side)
            assert (steps.stats()["algorithmic_bytes"], steps.stats()["algorithmic_flops"]) == tuple(figures["mu_kl"])
        assert np.isfinite(steps.divergence("kullback-leibler"))
        called("divergence_loss1", d2h=want["scalar_bytes"])
        for side in (0, 1):
            assert steps.cd_sweep(side, np.arange(width)[::-1]) >= 0.0
            called("sweep_reuse0_side%d" % side, h2d=want["permutation_bytes"], d2h=want["scalar_bytes"])
        assert steps.cd_sweep(1, np.arange(width), reuse=True, want_violation=False) is None
        called("sweep_reuse1_side1", h2d=want["permutation_bytes"])
        steps.fill_block(0, 0.5)
        called("fill")
        for side in (0, 1):
            B = steps.get_block(side)
            assert np.isfinite(B).all() and (B >= 0).all()
            called(None, d2h=want["set_block_bytes_%d" % side])
    finally:
        steps.close()


def test_refusals_that_need_a_live_handle(gpu):
    from recsys2019_deeplearning_evaluation_amd import _native as N
    X, _ = urm(False, "real")
    lib = N.load()

    def refused(rc, text):
        assert rc == N.E_INVALID and lib.mi355rec_last_error().decode() == text, (rc, lib.mi355rec_last_error().decode())

    svd = PureSVD_MI355X_Steps(X, 3)
    try:
        B, G = np.zeros((N_COLS, 3), np.float32), np.zeros((3, 3), np.float64)
        block_side = "side 2: 0 (users x r) or 1 (items x r)"
        refused(lib.mi355rec_svd_set_block(svd._h, 2, N.ptr(B)), block_side)
        refused(lib.mi355rec_svd_get_block(svd._h, 2, N.ptr(B)), block_side)
        refused(lib.mi355rec_svd_gram(svd._h, 2, N.ptr(G)), block_side)
        refused(lib.mi355rec_svd_apply(svd._h, 2, N.ptr(B)), block_side)
        refused(lib.mi355rec_svd_product(svd._h, 2), "side 2: 0 (users = URM . items) or 1 (items = URM^T . users)")
        refused(lib.mi355rec_svd_product(svd._h, -1), "side -1: 0 (users = URM . items) or 1 (items = URM^T . users)")
        # the NULL check comes first in the PureSVD entry points
        refused(lib.mi355rec_svd_product(None, 2), "NULL argument")
        assert counters(svd) == dict(launches=0, h2d_bytes=0, d2h_bytes=0, calls=0)
    finally:
        svd.close()
    nmf = NMF_MI355X_Steps(X, 3)
    try:
        perm = N.as_i32(np.arange(3))
        refused(lib.mi355rec_nmf_cd_sweep(nmf._h, 0, N.ptr(perm), 1, None), "reuse: no frobenius products of side 0 are held")
        refused(lib.mi355rec_nmf_mu_step(nmf._h, 1, 1, 1), "reuse: nothing of side 1 and loss 1 is held")
        nmf.set_block(0, np.ones((X.shape[0], 3), np.float32))
        nmf.set_block(1, np.ones((X.shape[1], 3), np.float32))
        nmf.mu_step(0, "frobenius")
        refused(lib.mi355rec_nmf_mu_step(nmf._h, 1, 0, 1), "reuse: nothing of side 1 and loss 0 is held")          # another side
        refused(lib.mi355rec_nmf_mu_step(nmf._h, 0, 1, 1), "reuse: nothing of side 0 and loss 1 is held")          # another loss
        nmf.mu_step(0, "frobenius", reuse=True)
        nmf.set_block(1, np.ones((X.shape[1], 3), np.float32))                                                        # what was held is stale
        refused(lib.mi355rec_nmf_cd_sweep(nmf._h, 0, N.ptr(perm), 1, None), "reuse: no frobenius products of side 0 are held")
        refused(lib.mi355rec_nmf_cd_sweep(nmf._h, 0, N.ptr(N.as_i32([0, 2, 2])), 0, None), "not a permutation of 0 .. 2: entry 2 is 2")
        refused(lib.mi355rec_nmf_fill_block(nmf._h, 0, -1.0), "fill value -1 is negative")
    finally:
        nmf.close()
