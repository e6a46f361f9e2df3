"""CPU checks of the 'mlp' / 'score' grounding-head training (no GPU): the new C-ABI entries are declared, exported and bound, the
host rule behind the BCE targets (llava_qwen.py:313-322), the heads' reference keys and optimizer groups, and the compiler's
register report of csrc/ground_heads.hip."""
import os
import shutil

import pytest
import torch

from v3d import _native, train
from v3d.train_module import ground_key_map

from test_abi_host import declared_symbols
from test_kernel_resources import HIPCC, _report

NEW = ("v3d_ground_rowdot_bce", "v3d_mul_rows_grad")


def test_new_entries_are_declared_exported_and_bound():
    lib = _native.lib()
    names = declared_symbols()
    for n in NEW:
        assert n in names and hasattr(lib, n) and n in _native.SIGNATURES, n
    assert len(_native.SIGNATURES["v3d_ground_rowdot_bce"][1]) == 17 and len(_native.SIGNATURES["v3d_mul_rows_grad"][1]) == 12
    assert lib.v3d_abi_version() == 7                          # entries added, none changed


def test_new_entries_reject_bad_arguments_without_a_device():
    lib = _native.lib()
    assert lib.v3d_ground_rowdot_bce(None, 8, 1, None, 8, None, 0, None, 1.0, None, None, None, 8, None, None, 2, None) == -1
    assert b"null pointer" in lib.v3d_last_error()
    p = 256                                                    # any non-null value: the shape is checked before anything is read
    assert lib.v3d_ground_rowdot_bce(p, 8, 1025, p, 8, None, 0, p, 1.0, p, None, p + 4096, 8, p, None, 2, None) == -1
    assert b"1 to 1024 rows" in lib.v3d_last_error()
    assert lib.v3d_ground_rowdot_bce(p, 3592, 4, p, 3592, None, 0, p, 1.0, p, None, p + 4096, 3592, p, None, 2, None) == -1
    assert lib.v3d_mul_rows_grad(p, 12, p, 12, p, 3, 12, p, 12, p, 2, None) == -1
    assert b"multiple of 8" in lib.v3d_last_error()


def test_bce_targets_follow_the_reference_rule():
    pos, w = train.ground_bce_targets([], 7)                   # P = 0: all targets 0, all weights 1
    assert pos.dtype == torch.uint8 and pos.tolist() == [0] * 7 and w == 1.0
    pos, w = train.ground_bce_targets([2], 7)
    assert pos.tolist() == [0, 0, 1, 0, 0, 0, 0] and w == 6.0
    pos, w = train.ground_bce_targets([1, 4, 4], 7)            # duplicates: counted in P, the target set once
    assert pos.tolist() == [0, 1, 0, 0, 1, 0, 0] and w == (7 - 3) / 3
    pos, w = train.ground_bce_targets(list(range(5)), 5)       # P = n: every weight 0
    assert pos.tolist() == [1] * 5 and w == 0.0
    with pytest.raises(_native.V3DError):
        train.ground_bce_targets([7], 7)


def test_head_key_maps_and_no_decay_groups():
    m = ground_key_map("mlp")
    assert m["ground_head.0.weight"] == ("head", "w0") and m["ground_head.2.bias"] == ("head", "ln_b") and len(m) == 6
    s = ground_key_map("score")
    assert s["ground_head_obj.1.weight"] == ("obj", "ln_w") and s["ground_head_score.3.weight"] == ("score", "w3") and len(s) == 18
    i = ground_key_map("infonce")
    assert i["ground_head_query.2.weight"] == ("query", "ln_w") and i["ground_head_zero_target"] == (None, "zero_target")
    with pytest.raises(_native.V3DError):
        ground_key_map("cosine")
    z = lambda *shape: torch.zeros(*shape)                     # noqa: E731
    head = lambda o, out: {"w0": z(o, 8), "b0": z(o), "ln_w": z(o), "ln_b": z(o), "w3": z(out, o), "b3": z(out)}      # noqa: E731
    tree = {"llm": {"norm": z(8)}, "ground": {"obj": head(16, 16), "query": head(16, 16), "score": head(16, 1)}}
    groups = dict(zip(train._paths(tree), train.param_groups(tree, 1e-5, weight_decay=0.1)))
    for mod in ("obj", "query", "score"):
        for leaf in ("b0", "ln_w", "ln_b", "b3"):
            assert groups[f"ground.{mod}.{leaf}"] == (1e-5, 0.0), (mod, leaf)      # LayerNorm parameters and biases: not decayed
        for leaf in ("w0", "w3"):
            assert groups[f"ground.{mod}.{leaf}"] == (1e-5, 0.1), (mod, leaf)


def test_ground_heads_kernels_do_not_spill():
    if not shutil.which(HIPCC) and not os.path.exists(HIPCC):
        pytest.skip("hipcc not available")
    spills = _report("ground_heads.hip")
    assert len(spills) >= 6 and any("ground_rowdot_bce" in k for k in spills) and any("mul_rows_grad" in k for k in spills)
    assert all(v == 0 for v in spills.values()), spills
