"""csrc/beam.hip compiles for gfx950 without register spills (hipcc -Rpass-analysis=kernel-resource-usage, device code only, no GPU needed),
in the manner of tests/test_kernel_resources.py: the top-K rounds keep 17 64-bit keys per thread in registers and index them with
compile-time indices only - a spill there would put scratch traffic into every one of up to 64 rounds."""
import shutil

import pytest

from test_kernel_resources import HIPCC, _report


def test_beam_kernels_do_not_spill():
    if not shutil.which(HIPCC):
        pytest.skip("hipcc not available")
    spills = _report("beam.hip")
    names = " ".join(spills)
    for kernel in ("beam_lse_part_kernel", "beam_topk_part_kernel", "beam_topk_merge_kernel", "beam_step_kernel", "beam_kv_gather_kernel"):
        assert kernel in names, (kernel, sorted(spills))
    assert all(v == 0 for v in spills.values()), {k: v for k, v in spills.items() if v}
