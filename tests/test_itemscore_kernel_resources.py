"""Build-level check behind DESIGN section 15: csrc/itemscore.hip compiles for gfx950 (hipcc cross-compiles without a GPU) and its
ranking kernels -- both shapes of the windowed kernel and the candidate-row kernel -- keep everything in registers; the windowed
kernel's LDS is the bitmap and a few words, whatever the catalogue."""
import os
import subprocess

import pytest

from test_kernel_spills import HIPCC, ROOT, _kernel_text, _resource


@pytest.fixture(scope="module")
def asm(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("itemscore") / "itemscore.s")
    src = os.path.join(ROOT, "recsys2019_deeplearning_evaluation_amd", "csrc", "itemscore.hip")
    subprocess.run([HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-munsafe-fp-atomics", "-S", "--cuda-device-only",
                    src, "-o", out], check=True, stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)
    return out


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not installed")
@pytest.mark.parametrize("threads", [64, 256])
def test_windowed_rank_kernel_resources(asm, threads):
    name = "itemscore_rank_kernelILi%dEE" % threads
    assert _resource(asm, name, "ScratchSize") == 0
    assert _resource(asm, name, "LDSByteSize") <= 4 * threads + 64          # the bitmap (a word per lane) and the wavefront totals
    body = _kernel_text(asm, name)
    assert any(t.startswith("ds_or_b32") for t in body)                      # the bitmap is marked in LDS ...
    assert not any(t.startswith(("global_atomic", "flat_atomic")) for t in body)    # ... and nothing is counted in global memory
    assert any(t.startswith("v_bcnt_u32_b32") or t.startswith("s_bcnt1") for t in body)     # popcounts of the bitmap words


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not installed")
def test_candidate_kernel_resources(asm):
    assert _resource(asm, "itemscore_cand_kernelILi256EE", "ScratchSize") == 0
