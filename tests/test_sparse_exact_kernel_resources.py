"""Build-level check behind DESIGN section 17: csrc/spexact.hip compiles for gfx950 (hipcc cross-compiles without a GPU), its kernels
keep everything in registers, no multiply of a score is fused with its add -- the order contract rounds the product first, hipcc's
default for device code would contract the two -- and no float atomic is left anywhere: the order of a cell's adds is the profile's."""
import os
import subprocess

import pytest

from test_kernel_spills import HIPCC, ROOT, _kernel_text, _resource

SCORE_KERNEL = "spexact_rows_kernel"
KERNELS = (SCORE_KERNEL, "spexact_cand_kernelILi256EE", "spexact_check_kernel", "spexact_cuts_kernel")
FUSED = ("v_fma", "v_fmac", "v_pk_fma")
FLOAT_ATOMICS = ("ds_add_f32", "ds_add_rtn_f32", "global_atomic_add_f32")


@pytest.fixture(scope="module")
def asm(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("spexact") / "spexact.s")
    src = os.path.join(ROOT, "recsys2019_deeplearning_evaluation_amd", "csrc", "spexact.hip")
    subprocess.run([HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-munsafe-fp-atomics", "-S", "--cuda-device-only",
                    src, "-o", out], check=True, stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)
    return out


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not installed")
@pytest.mark.parametrize("name", KERNELS)
def test_kernel_keeps_to_registers_does_not_contract_and_has_no_float_atomic(asm, name):
    assert _resource(asm, name, "ScratchSize") == 0
    body = _kernel_text(asm, name)
    assert body, name
    assert not [t for t in body if t.startswith(FUSED)], name
    assert not [t for t in body if t.startswith(FLOAT_ATOMICS)], name


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not installed")
def test_the_score_path_multiplies_then_adds_in_lds(asm):
    body = _kernel_text(asm, SCORE_KERNEL)
    assert any(t.startswith("v_mul_f32") for t in body)
    assert any(t.startswith("v_add_f32") for t in body)
    assert any(t.startswith("ds_read_b32") or t.startswith("ds_load_b32") for t in body)
    assert any(t.startswith("ds_write_b32") or t.startswith("ds_store_b32") for t in body)


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not installed")
def test_the_whole_translation_unit_has_no_float_atomic(asm):
    with open(asm) as f:
        text = f.read()
    for word in FLOAT_ATOMICS + ("global_atomic_pk_add", "flat_atomic_add_f32", "ds_pk_add"):
        assert word not in text, word
