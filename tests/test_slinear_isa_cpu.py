"""Compiler-output checks of csrc/slinear.hip that need no GPU: its gfx950 assembly holds no back-to-back pair of
different matrix-core opcodes chained through SrcC (tools/mfma_pairs.py, tests/test_isa_cpu.py), uses the bf16 matrix
instruction and no other matrix opcode, and no kernel of it needs scratch memory."""
import os
import re
import shutil
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import mfma_pairs  # noqa: E402

HIPCC = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
SRC = os.path.join(ROOT, "binary-networks-pytorch_amd", "csrc", "slinear.hip")


@pytest.fixture(scope="module")
def asm(tmp_path_factory):
    if not os.path.exists(HIPCC):
        pytest.skip("hipcc not installed")
    out = tmp_path_factory.mktemp("slinear") / "k.s"
    subprocess.run([HIPCC, "-O3", "-std=c++17", "--offload-arch=gfx950", "--cuda-device-only", "-S", SRC, "-o", str(out)],
                   check=True, capture_output=True, timeout=600)
    return out.read_text()


def test_no_back_to_back_mixed_mfma_chain(asm):
    assert mfma_pairs.dependent_pairs(asm) == []


def test_the_only_matrix_opcode_is_the_bf16_one(asm):
    ops = set(re.findall(r"^\s*(v_(?:mfma|smfmac)\w+)", asm, re.M))
    assert ops == {"v_mfma_f32_16x16x32_bf16"}, ops


def test_no_kernel_spills(asm):
    """Scratch use would mean the accumulators or the weight fragments of a K block left the register file."""
    sizes = [int(v) for v in re.findall(r"\.private_segment_fixed_size:\s*(\d+)", asm)]
    assert len(sizes) == 3 and not any(sizes), sizes               # both blockings of the GEMM and the mask kernel
