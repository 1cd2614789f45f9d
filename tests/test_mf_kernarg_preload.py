"""Build-level check behind the mini-batch kernel's prologue: compiled with the flags csrc/Makefile gives mf.hip, every
mf_batch_kernel instance has its leading arguments -- what a task header's address is made of -- preloaded into scalar registers
(a non-zero .amdhsa_user_sgpr_kernarg_preload_length in its kernel descriptor) and uses no scratch memory.  Compiles mf.hip to
assembly for gfx950 (hipcc cross-compiles without a GPU, under a minute)."""
import os
import re
import shlex
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "recsys2019_deeplearning_evaluation_amd", "csrc")
HIPCC = "/opt/rocm/bin/hipcc"


def _makefile_compile_command():
    """The command `make` would run for build/mf.o (dry run, forced), as a list of arguments."""
    out = subprocess.run(["make", "-C", CSRC, "-n", "-B", "build/mf.o"], check=True, capture_output=True, text=True).stdout
    lines = [ln for ln in out.split("\n") if " -c mf.hip " in ln]
    assert len(lines) == 1, out
    return shlex.split(lines[0])


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not installed")
def test_mini_batch_kernels_preload_their_leading_arguments(tmp_path):
    cmd = _makefile_compile_command()
    assert cmd[-4:] == ["-c", "mf.hip", "-o", "build/mf.o"], cmd
    asm = str(tmp_path / "mf.s")
    subprocess.run(cmd[:-4] + ["-S", "--cuda-device-only", "mf.hip", "-o", asm], check=True, cwd=CSRC, stdout=subprocess.DEVNULL,
                   stderr=subprocess.DEVNULL)
    text = open(asm).read()
    seen = 0
    for block in text.split(".amdhsa_kernel ")[1:]:
        name, block = block.split("\n", 1)
        if "15mf_batch_kernelI" not in name:
            continue
        block = block[:block.index(".end_amdhsa_kernel")]
        preload = re.search(r"\.amdhsa_user_sgpr_kernarg_preload_length\s+(\d+)", block)
        scratch = re.search(r"\.amdhsa_private_segment_fixed_size\s+(\d+)", block)
        assert preload and int(preload.group(1)) > 0, name
        assert scratch and int(scratch.group(1)) == 0, name
        seen += 1
    assert seen == 32, seen          # BPR and FunkSVD x float and double x four row widths x plain sgd and the other optimisers
