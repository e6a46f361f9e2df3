"""csrc/pe_mlp.hip compiles for gfx950 without register spills (hipcc -Rpass-analysis=kernel-resource-usage, device code only, no GPU
needed), in the manner of tests/test_pe_points_kernel_resources.py: the hidden kernel keeps a lane's 24 first-layer weights, its bias and
LayerNorm vectors and a row of eight values in registers over the rows of its wave, and the weight-gradient kernel 24 f32 sums per lane -
scratch traffic in either would be paid per row."""
import shutil

import pytest

from test_kernel_resources import HIPCC, _report


def test_pe_mlp_kernels_do_not_spill():
    if not shutil.which(HIPCC):
        pytest.skip("hipcc not available")
    spills = _report("pe_mlp.hip", ("-ffp-contract=off",))
    names = " ".join(spills)
    for kernel in ("pe_mlp_hidden_kernel", "visual_tokens_rows_kernel", "pe_rows_grad_kernel", "pe_mlp_wgrad_partial_kernel",
                   "pe_mlp_wgrad_final_kernel"):
        assert kernel in names, (kernel, sorted(spills))
    assert all(v == 0 for v in spills.values()), {k: v for k, v in spills.items() if v}
