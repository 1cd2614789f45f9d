"""Build-level check behind DESIGN section 13: the update kernel of the EASE_R elimination (csrc/ease.hip) keeps everything in
registers, multiplies on the matrix cores and leaves room for four workgroups per CU.  Compiles ease.hip to assembly for gfx950
(hipcc cross-compiles without a GPU)."""
import os
import subprocess

import pytest

from test_kernel_spills import HIPCC, ROOT, _kernel_text, _resource


@pytest.fixture(scope="module")
def asm(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("ease") / "ease.s")
    src = os.path.join(ROOT, "recsys2019_deeplearning_evaluation_amd", "csrc", "ease.hip")
    subprocess.run([HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-munsafe-fp-atomics", "-S", "--cuda-device-only",
                    src, "-o", out], check=True, stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)
    return out


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not installed")
@pytest.mark.parametrize("block", [64, 128])
def test_update_kernel_resources(asm, block):
    name = "ease_update_kernelILi%dEE" % block
    assert _resource(asm, name, "ScratchSize") == 0
    body = _kernel_text(asm, name)
    # 4 accumulators x 2 MFMAs per K pair, the K chunk of 32 unrolled four pairs at a time
    assert sum(1 for t in body if t.startswith("v_mfma_f32_32x32x2")) >= 16
    # four 256-thread workgroups per CU = 4 wavefronts per SIMD, i.e. at most 128 registers per lane (vector and
    # accumulation registers together) and a quarter of the LDS
    assert _resource(asm, name, "NumVgprs") + _resource(asm, name, "NumAgprs") <= 128
    assert _resource(asm, name, "Occupancy") >= 4
