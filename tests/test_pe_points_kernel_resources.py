"""csrc/pe_points.hip compiles for gfx950 without register spills (hipcc -Rpass-analysis=kernel-resource-usage, device code only, no GPU
needed), in the manner of tests/test_sample_kernel_resources.py: the min/max kernel folds 27 16-byte vectors per lane in registers and the
fused kernel's on-the-fly form evaluates eight double-precision sines per lane - scratch traffic in either would be paid per token."""
import shutil

import pytest

from test_kernel_resources import HIPCC, _report


def test_pe_points_kernels_do_not_spill():
    if not shutil.which(HIPCC):
        pytest.skip("hipcc not available")
    spills = _report("pe_points.hip", ("-ffp-contract=off",))
    names = " ".join(spills)
    for kernel in ("coord_sample_kernel", "coord_minmax_kernel", "sin3d_table_points_kernel", "sin3d_pe_points_kernel",
                   "visual_tokens_points_kernel"):
        assert kernel in names, (kernel, sorted(spills))
    assert all(v == 0 for v in spills.values()), {k: v for k, v in spills.items() if v}
