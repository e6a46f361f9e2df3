"""csrc/sample.hip compiles for gfx950 without register spills (hipcc -Rpass-analysis=kernel-resource-usage, device code only, no GPU needed),
in the manner of tests/test_beam_kernel_resources.py: the threshold kernel runs up to 34 passes over a row at 1024 threads per workgroup
(at most 128 VGPRs each) and the draw kernel carries ten Philox rounds and two logarithms per token - scratch traffic in either loop would
be paid per token."""
import shutil

import pytest

from test_kernel_resources import HIPCC, _report


def test_sample_kernels_do_not_spill():
    if not shutil.which(HIPCC):
        pytest.skip("hipcc not available")
    spills = _report("sample.hip", ("-ffp-contract=off",))
    names = " ".join(spills)
    for kernel in ("sample_threshold_kernel", "sample_draw_kernel", "sample_merge_kernel"):
        assert kernel in names, (kernel, sorted(spills))
    assert all(v == 0 for v in spills.values()), {k: v for k, v in spills.items() if v}
