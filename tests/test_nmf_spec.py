"""NMF without a device: the NumPy restatement of tests/nmf_cases.py against the reference's own fits (tests/golden/nmf.npz, made by
tests/golden/make_nmf_fixture.py with scikit-learn's NMF), the package's surface, the argument checks and the build-level check of
the two hot kernels.

d of a case = score_distance(W32 H32, W64 H64) of the REFERENCE's fit on the float32 URM and on a float64 copy of it: how far the
reference's own rounding puts it from the exact iteration.  A case is in the fixture only if both runs stop after the same number
of iterations and d <= 1e-3.  The restatement must stop where the reference stops and land within max(4 d, 1e-6) of it: a factor
two for a second, independent rounding of the same size and another two for the summation order of another BLAS."""
import inspect
import os
import subprocess

import numpy as np
import pytest
import scipy.sparse as sps

import nmf_cases as M
import test_native_abi as abi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = "/opt/rocm/bin/hipcc"
FLOOR = 1e-6


def _replay(case, dtype=np.float32):
    if case["seed"] is None:
        np.random.seed(case["np_seed"])
    return M.replay(case["X"], case["k"], case["solver_name"], case["init"], case["loss"], case["seed"], dtype)


def test_replay_reproduces_the_reference_fixture_within_its_noise_floor():
    state = np.random.get_state()
    try:
        lines = []
        for case in M.load_cases():
            assert 0.0 <= case["d"] <= 1e-3, M.label(case)
            r = _replay(case)
            e = M.distance_to_reference(case, r["U"], r["V"])
            lines.append((M.label(case), r["n_iter_fit"], r["n_iter_transform"], case["n_iter_fit"], case["n_iter_transform"], case["d"], e))
            print("%s: n_iter %d / %d (reference %d / %d), d %.2e, replay(float32) against the fixture %.2e" % lines[-1])
        for line in lines:
            assert line[1:3] == line[3:5], line
            assert line[6] <= max(4 * line[5], FLOOR), line
    finally:
        np.random.set_state(state)


def test_replay_leaves_numpy_random_state_where_the_reference_leaves_it():
    state = np.random.get_state()
    try:
        seen = set()
        for case in M.load_cases():
            if case["seed"] is not None:
                continue
            _replay(case)
            assert np.random.rand() == case["after"], M.label(case)
            seen.add(case["solver"])
        assert seen == {"cd", "mu-kl"}
    finally:
        np.random.set_state(state)


def test_fixture_holds_the_cases_of_the_table():
    cases = M.load_cases()
    have = {(c["urm"], c["k"], c["solver"], c["init"], c["seed"]) for c in cases}
    for c in M.CASES:
        if c["urm"] != "ml1m":                          # a full-size case outside the admission rule may be dropped by the generator
            assert (c["urm"], c["k"], c["solver"], c["init"], c["seed"]) in have, c
    assert {c["solver"] for c in cases} == {"cd", "mu-fro", "mu-kl"} and {c["init"] for c in cases} == {"random", "nndsvda"}
    assert any(c["X"].shape[0] < c["X"].shape[1] for c in cases) and any(c["k"] > c["X"].shape[1] for c in cases)
    assert any((c["X"].data != 1.0).any() and (np.diff(c["X"].indptr) == 0).any() for c in cases), "real values and an empty user"
    assert {c["k"] for c in cases} >= {5, 8, 12, 33, 65, 70, 130}
    assert max(max(c["n_iter_fit"], c["n_iter_transform"]) for c in cases) == M.MAX_ITER, "a case at the cap"
    assert os.path.getsize(M.GOLDEN) <= 640 * 1024


def test_single_steps_float32_against_float64():
    """The single-step restatements that the device tests compare with: in float32 they sit within 1e-4 of their float64 selves."""
    rng = np.random.default_rng(4)
    X = sps.csr_matrix(M.clusters_urm(31, 90, 50, 4, valued=True))
    W, H = np.abs(rng.normal(size=(90, 7))), np.abs(rng.normal(size=(7, 50)))
    W[rng.random(W.shape) < 0.2] = 0.0
    perm = rng.permutation(7)
    for step in ("cd", "mu-fro", "mu-kl"):
        out = []
        for dtype in (np.float32, np.float64):
            Xd, Wd, Hd = sps.csr_matrix(X, dtype=dtype), W.astype(dtype), H.astype(dtype)
            if step == "cd":
                Ht = np.ascontiguousarray(Hd.T)
                v = M.cd_half_sweep(Xd, Wd, Ht, perm)
                assert v > 0
            else:
                loss = "frobenius" if step == "mu-fro" else "kullback-leibler"
                M.mu_w(Xd, Wd, Hd, loss)
                M.mu_h(Xd, Wd, Hd, loss)
                assert M.divergence(Xd, Wd, Hd, loss) > 0
            assert Wd.dtype == dtype and (Wd >= 0).all()
            out.append(Wd.astype(np.float64))
        assert np.abs(out[0] - out[1]).max() <= 1e-4 * np.abs(out[1]).max(), step


# ---- the package's surface ----------------------------------------------------------------------------------------------------------
def test_package_exports_and_binds_the_class():
    import recsys2019_deeplearning_evaluation_amd as pkg
    from recsys2019_deeplearning_evaluation_amd import recommender_base as RB
    from recsys2019_deeplearning_evaluation_amd.reference_binding import bind
    from recsys2019_deeplearning_evaluation_amd.scoring import GpuScoringMixin
    assert "NMFRecommender" in pkg.__all__
    assert issubclass(pkg.NMFRecommender, (GpuScoringMixin, RB.BaseMatrixFactorizationRecommender))
    assert list(inspect.signature(pkg.NMFRecommender.fit).parameters) == ["self", "num_factors", "l1_ratio", "solver", "init_type", "beta_loss",
                                                                        "verbose", "random_seed"]
    defaults = {n: p.default for n, p in inspect.signature(pkg.NMFRecommender.fit).parameters.items() if n != "self"}
    assert defaults == dict(num_factors=100, l1_ratio=0.5, solver="multiplicative_update", init_type="random", beta_loss="frobenius",
                            verbose=False, random_seed=None)

    class MF(RB.BaseMatrixFactorizationRecommender):
        pass

    class ItemSim(RB.BaseItemSimilarityMatrixRecommender):
        pass

    class UserSim(RB.BaseUserSimilarityMatrixRecommender):
        pass

    R = bind(MF, ItemSim, UserSim, RB.Incremental_Training_Early_Stopping)
    assert issubclass(R.NMFRecommender, MF) and issubclass(R.NMFRecommender, GpuScoringMixin)
    assert R.NMFRecommender.RECOMMENDER_NAME == "NMFRecommender"


def test_header_declares_the_nmf_group():
    names = abi.declared_symbols()
    for entry in ("create", "set_block", "get_block", "fill_block", "cd_sweep", "mu_step", "divergence", "get_stats", "fit_info", "destroy"):
        assert "mi355rec_nmf_" + entry in names, entry
    abi.test_library_exports_every_declared_symbol()
    abi.test_binding_covers_header_exactly()


def test_fit_argument_errors_have_the_reference_wording():
    from recsys2019_deeplearning_evaluation_amd import NMFRecommender
    X = M.clusters_urm(25, 60, 25, 3)
    rec = NMFRecommender(X, verbose=False)
    with pytest.raises(AssertionError, match="NMFRecommender: l1_ratio must be between 0 and 1, provided value was 1.5"):
        rec.fit(num_factors=4, l1_ratio=1.5)
    with pytest.raises(ValueError, match="Value for 'solver' not recognized. Acceptable values are .*, provided was 'als'"):
        rec.fit(num_factors=4, solver="als")
    with pytest.raises(ValueError, match="Value for 'init_type' not recognized. Acceptable values are .*, provided was 'nndsvd'"):
        rec.fit(num_factors=4, init_type="nndsvd")
    with pytest.raises(ValueError, match="Value for 'beta_loss' not recognized. Acceptable values are .*, provided was 'itakura-saito'"):
        rec.fit(num_factors=4, beta_loss="itakura-saito")
    # sklearn's own refusals, raised before any device call (without a device that call would be a NativeLibraryError)
    z = np.load(M.GOLDEN, allow_pickle=False)
    with pytest.raises(ValueError) as info:
        rec.fit(num_factors=40, solver="coordinate_descent", init_type="nndsvda", random_seed=3)
    assert str(info.value) == str(z["nndsvda_error"])
    with pytest.raises(ValueError, match="solver 'cd' does not handle beta_loss = 'kullback-leibler'"):
        rec.fit(num_factors=4, solver="coordinate_descent", beta_loss="kullback-leibler")
    assert not hasattr(rec, "USER_factors")


def test_bad_abi_arguments_are_refused_before_touching_the_device():
    import ctypes as C
    from recsys2019_deeplearning_evaluation_amd import _native as N
    from recsys2019_deeplearning_evaluation_amd.nmf import NMF_MI355X_Steps, check_permutation
    X = sps.random(20, 10, 0.3, format="csr", dtype=np.float32, random_state=0)
    for k in (0, -3, 4097):
        with pytest.raises(ValueError, match="outside \\[1, 4096\\]"):
            NMF_MI355X_Steps(X, k)
    neg = X.copy()
    neg.data[0] = -1.0
    with pytest.raises(ValueError, match="negative value"):
        NMF_MI355X_Steps(neg, 4)
    bad = X.copy()
    bad.indices = bad.indices.copy()
    bad.indices[0] = 10                       # a column outside the matrix
    with pytest.raises(ValueError):
        NMF_MI355X_Steps(bad, 4)
    # every refusal of create, word for word: the ones both handle types share, the width with NMF's noun, the negative value
    from _util import block_pair_create_refusals
    assert len(block_pair_create_refusals("nmf", "number of components k", nmf=True)) == 20
    # side and loss are looked at before the handle is: a wrong one is reported as such even on a NULL handle
    lib = N.load()
    perm = N.as_i32(np.arange(4))
    v = C.c_double()
    for call, what in ((lambda: lib.mi355rec_nmf_cd_sweep(None, 2, N.ptr(perm), 0, C.byref(v)), "side 2"),
                       (lambda: lib.mi355rec_nmf_mu_step(None, -1, 0, 0), "side -1"),
                       (lambda: lib.mi355rec_nmf_mu_step(None, 0, 2, 0), "loss 2"),
                       (lambda: lib.mi355rec_nmf_divergence(None, 7, C.byref(v)), "loss 7"),
                       (lambda: lib.mi355rec_nmf_fill_block(None, 3, 0.0), "side 3")):
        assert call() == N.E_INVALID
        assert lib.mi355rec_last_error().decode().startswith(what), what
    for p in ([0, 1, 1, 3], [0, 1, 2, 4], [0, 1, 2], [[0, 1, 2, 3]]):
        with pytest.raises(ValueError, match="not a permutation"):
            check_permutation(p, 4)
    assert check_permutation([3, 1, 0, 2], 4).dtype == np.int32


def test_no_cpu_fallback_without_device():
    from recsys2019_deeplearning_evaluation_amd import NMFRecommender, _native
    if _native.device_count() > 0:
        pytest.skip("a device is present")
    X = sps.random(40, 30, 0.3, format="csr", dtype=np.float32, random_state=0)
    for solver, init in (("coordinate_descent", "random"), ("multiplicative_update", "nndsvda")):
        with pytest.raises(_native.NativeLibraryError):
            NMFRecommender(X, verbose=False).fit(num_factors=4, solver=solver, init_type=init, random_seed=1)


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not installed")
def test_sweep_and_sddmm_kernels_use_no_scratch_memory(tmp_path):
    from test_kernel_spills import _resource
    asm = str(tmp_path / "nmf.s")
    src = os.path.join(ROOT, "recsys2019_deeplearning_evaluation_amd", "csrc", "nmf.hip")
    subprocess.run([HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-munsafe-fp-atomics", "-S", "--cuda-device-only",
                    src, "-o", asm], check=True, stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)
    for kernel in ("nmf_cd_sweep_kernel", "nmf_sddmm_kernelILb0EE", "nmf_sddmm_kernelILb1EE"):
        assert _resource(asm, kernel, "ScratchSize") == 0, kernel
        assert _resource(asm, kernel, "Occupancy") >= 4, kernel          # at least four workgroups of 256 threads per CU
