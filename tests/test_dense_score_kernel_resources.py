"""Build-level check behind DESIGN section 16: csrc/densescore.hip compiles for gfx950 (hipcc cross-compiles without a GPU), its
kernels keep everything in registers, and no multiply of a score is fused with its add -- the order contract rounds the product
first, hipcc's default for device code would contract the two."""
import os
import subprocess

import pytest

from test_kernel_spills import HIPCC, ROOT, _kernel_text, _resource

KERNELS = ("dscore_rows_kernelILi4EE", "dscore_rows_kernelILi8EE", "dscore_cand_kernelILi256EE")
FUSED = ("v_fma", "v_fmac", "v_pk_fma")


@pytest.fixture(scope="module")
def asm(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("densescore") / "densescore.s")
    src = os.path.join(ROOT, "recsys2019_deeplearning_evaluation_amd", "csrc", "densescore.hip")
    subprocess.run([HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-munsafe-fp-atomics", "-S", "--cuda-device-only",
                    src, "-o", out], check=True, stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)
    return out


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not installed")
@pytest.mark.parametrize("name", KERNELS)
def test_kernel_keeps_to_registers_and_does_not_contract(asm, name):
    assert _resource(asm, name, "ScratchSize") == 0
    body = _kernel_text(asm, name)
    assert not [t for t in body if t.startswith(FUSED)], name
    assert any(t.startswith(("v_mul_f32", "v_pk_mul_f32")) for t in body), name
    assert any(t.startswith(("v_add_f32", "v_pk_add_f32")) for t in body), name


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not installed")
def test_rows_kernel_streams_b_in_16_byte_loads_and_leaves_room_for_eight_waves(asm):
    for name in KERNELS[:2]:
        body = _kernel_text(asm, name)
        assert any(t.startswith("global_load_dwordx4") for t in body), name
        assert _resource(asm, name, "Occupancy") == 8, name
