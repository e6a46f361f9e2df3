"""Register spills of gemm_layout_kernel (hipcc -Rpass-analysis=kernel-resource-usage on gemm.hip, device code only, no GPU needed):
every instantiation - 2 dtypes x 2 epilogues (NONE, RES) x 3 layouts (NN, TN, TK) x 2 tile forms = 24 - reports 0 spilled VGPRs."""
import shutil

import pytest

from test_kernel_resources import HIPCC, _report


def test_layout_kernels_do_not_spill():
    if not shutil.which(HIPCC):
        pytest.skip("hipcc not available")
    spills = {k: v for k, v in _report("gemm.hip").items() if "gemm_layout_kernel" in k}
    assert len(spills) == 24, sorted(spills)
    assert all(v == 0 for v in spills.values()), {k: v for k, v in spills.items() if v}
    for dt in ("6bf16_t", "5f16_t"):
        for epi in ("Li0E", "Li5E"):
            for flags in ("Lb0ELb1E", "Lb1ELb1E", "Lb1ELb0E"):
                for big in ("Lb0E", "Lb1E"):
                    assert any(dt + "E" + epi + flags + big in k or dt + epi + flags + big in k for k in spills), (dt, epi, flags, big)
