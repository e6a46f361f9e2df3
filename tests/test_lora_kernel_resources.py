"""csrc/lora.hip compiles for gfx950 without register spills (hipcc -Rpass-analysis=kernel-resource-usage, device code only, no GPU
needed), in the manner of tests/test_sample_kernel_resources.py: the wgrad kernel keeps up to 24 accumulator tiles per wave and the down
kernel up to 12 beside the next K step's prefetched operands - scratch traffic in either loop would be paid per 32 rows."""
import shutil

import pytest

from test_kernel_resources import HIPCC, _report


def test_lora_kernels_do_not_spill():
    if not shutil.which(HIPCC):
        pytest.skip("hipcc not available")
    spills = _report("lora.hip")
    names = " ".join(spills)
    for kernel in ("lora_down_kernel", "lora_wgrad_partial_kernel", "lora_wgrad_sum_kernel"):
        assert kernel in names, (kernel, sorted(spills))
    assert sum("lora_down_kernel" in k for k in spills) == 10              # 5 rank buckets x 2 dtypes
    assert sum("lora_wgrad_partial_kernel" in k for k in spills) == 10
    assert sum("lora_wgrad_sum_kernel" in k for k in spills) == 3          # f32, f16, bf16 outputs
    assert all(v == 0 for v in spills.values()), {k: v for k, v in spills.items() if v}
