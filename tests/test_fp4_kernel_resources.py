"""Register spills and scratch of the MXFP4 kernels (csrc/gemm_fp4.hip), from the compiler's own resource report (device code only,
no GPU needed) - the way tests/test_kernel_resources.py holds gemm_fp8.hip to zero spills.  One compile feeds every assertion."""
import os
import re
import shutil
import subprocess

import pytest

from test_kernel_resources import CSRC, HIPCC, ROOT

SRC = "gemm_fp4.hip"
KERNELS = ("gemm_mxfp4_kernel", "quantize_mxfp4_kernel", "linear_decode_mxfp4_kernel", "linear_decode_mxfp4_mfma_kernel")
FIELDS = {"vgpr_spill": r"VGPRs Spill: (\d+)", "sgpr_spill": r"SGPRs Spill: (\d+)", "scratch": r"ScratchSize \[bytes/lane\]: (\d+)"}


@pytest.fixture(scope="module")
def usage():
    """{kernel name: {vgpr_spill, sgpr_spill, scratch}} of every kernel in the file"""
    if not shutil.which(HIPCC):
        pytest.skip("hipcc not available")
    assert os.path.exists(os.path.join(CSRC, SRC)), "csrc/gemm_fp4.hip is missing"
    cmd = [HIPCC, "-O3", "-std=c++17", "--offload-arch=gfx950", "-I" + os.path.join(ROOT, "include"), "-I" + CSRC, "-S", "--cuda-device-only",
           os.path.join(CSRC, SRC), "-o", os.devnull, "-Rpass-analysis=kernel-resource-usage"]
    out = subprocess.run(cmd, capture_output=True, text=True, timeout=900)
    assert out.returncode == 0, out.stderr[-2000:]
    table, name = {}, None
    for line in out.stderr.splitlines():
        m = re.search(r"Function Name: (\S+)", line)
        if m:
            name = m.group(1)
            table[name] = {}
        for field, pat in FIELDS.items():
            m = re.search(pat, line)
            if m and name:
                table[name][field] = int(m.group(1))
    return table


def test_every_fp4_kernel_is_reported(usage):
    for k in KERNELS:
        assert any(k in name for name in usage), f"no {k} instance in {SRC}"
    # prefill: 2 dtypes x 4 epilogues; decode: 2 dtypes x 4 epilogues x (4 row counts | 2 row blocks); quantiser: 2 dtypes
    assert len(usage) >= 8 + 32 + 16 + 2
    assert all(set(v) == set(FIELDS) for v in usage.values())


def test_fp4_kernels_do_not_spill(usage):
    bad = {k: v for k, v in usage.items() if v["vgpr_spill"] or v["sgpr_spill"]}
    assert not bad, bad


def test_fp4_kernels_use_no_scratch(usage):
    bad = {k: v["scratch"] for k, v in usage.items() if v["scratch"]}
    assert not bad, bad
