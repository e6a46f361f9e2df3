"""The CPU restatement of the P-point position encodings (tests/pe_points_check.py) against the reference's own outputs
(tests/golden/pe_points.npz, written by tools/gen_pe_points_golden.py), and the type-string parser."""
import numpy as np
import pytest
import torch

import pe_points_check as PC


def _same(got, want_bits, kind):
    """equal values with NaN positions equal (-0 and +0 compare equal: the rule compares values, not zero signs)."""
    want = PC.from_bits(want_bits, kind).float().numpy()
    got = got.float().numpy()
    assert got.shape == want.shape, (got.shape, want.shape)
    assert np.array_equal(np.isnan(got), np.isnan(want))
    assert np.array_equal(np.nan_to_num(got, nan=0.0), np.nan_to_num(want, nan=0.0))


@pytest.mark.parametrize("kind", ["f32", "f16", "bf16"])
@pytest.mark.parametrize("mode", list(PC.MODES))
def test_coordinates_and_ids_bit_for_bit(golden, mode, kind):
    g = golden("pe_points")
    pts = PC.aggregate(PC.seeded_coords(kind), mode)
    _same(pts, g[f"{mode}_pts_{kind}"], kind)
    vox = PC.discrete(pts)
    _same(vox, g[f"{mode}_vox_{kind}"], kind)
    ids = torch.nan_to_num(vox.float(), nan=-1.0).to(torch.int16).numpy()
    assert np.array_equal(ids, g[f"{mode}_ids_{kind}"])
    assert np.isnan(pts.float().numpy()).any(), "the seeded input must reach every mode with a NaN"
    v = vox.float().numpy()
    assert np.nanmin(v) == 0 and np.nanmax(v) == 300, "the seeded input must reach both clamps"


def test_sample_modes_nest(golden):
    nine = PC.sample_points(PC.seeded_coords("f32"), 9)
    assert torch.equal(torch.nan_to_num(PC.sample_points(PC.seeded_coords("f32"), 5)), torch.nan_to_num(nine[:, :, :, [0, 2, 4, 6, 8]]))
    assert torch.equal(torch.nan_to_num(PC.sample_points(PC.seeded_coords("f32"), 1)), torch.nan_to_num(nine[:, :, :, 4]))


@pytest.mark.parametrize("continuous", [False, True])
@pytest.mark.parametrize("E,P", PC.PE_CASES)
def test_pe_reproduces_the_reference(golden, E, P, continuous):
    g = golden("pe_points")
    src = "cont" if continuous else "ids"
    if E == 256:        # f32: same operations in the same order -> at most 1 f32 ulp (values in [-1, 1]: 2^-23 covers it)
        got = PC.pe(PC.pe_inputs(E, P, "f32", continuous), E, P).numpy()
        want = g[f"pe_E{E}_P{P}_{src}_f32"]
        assert np.abs(got - want).max() <= 2.0 ** -23
        nf = E // (3 * P)
        assert np.all(want[:, 3 * P * nf:] == 0) and np.all(got[:, 3 * P * nf:] == 0)
    for kind in ("f16", "bf16"):
        got = PC.pe(PC.pe_inputs(E, P, kind, continuous), E, P)
        _same(got, g[f"pe_E{E}_P{P}_{src}_{kind}"], kind)


def test_correctly_rounded_trig_stays_inside_the_gpu_tests_caps():
    """What the issue measured: the kernels' rule (f64 trig rounded once) against torch's f32 trig differs by at most one 16-bit ulp in a
    share of elements far below the GPU tests' 2e-3 cap."""
    for E, P in PC.PE_CASES:
        for kind in ("f16", "bf16"):
            for cont in (False, True):
                x = PC.pe_inputs(E, P, kind, cont)
                a, b = PC.bits(PC.pe(x, E, P)).astype(np.int32), PC.bits(PC.pe_f64(x, E, P)).astype(np.int32)
                assert np.abs(a - b).max() <= 1 and (a != b).mean() < 2e-4, (E, P, kind, cont)


def test_type_string_parser():
    from v3d._native import V3DError
    from v3d.loader import parse_position_type
    table = {"avg": ("avg", 1), "sample9": ("sample9", 9), "sample5": ("sample5", 5), "sample1": ("sample1", 1), "minmax": ("minmax", 2)}
    for word, (agg, P) in table.items():
        assert parse_position_type(f"{word}-discrete-sin3d") == (agg, P, True)
        assert parse_position_type(f"{word}-sin3d") == (agg, P, False)
    assert parse_position_type("avg-discrete-sin3d") == ("avg", 1, True)
    for bad in ("avg-discrete-mlp", "sample9-discrete-mlp", "avg-discrete-sin3d-mrope", "mrope", "discrete-sin3d", "sin3d", "avg-discrete"):
        with pytest.raises(V3DError):
            parse_position_type(bad)


def test_engine_config_carries_the_type():
    import types
    from v3d import loader
    from v3d._native import V3DError
    sd = {loader.VIT_PREFIX + "embeddings.patch_embedding.weight": torch.zeros(144, 3, 14, 14),
          loader.VIT_PREFIX + "embeddings.position_embedding.weight": torch.zeros(729, 144),
          loader.VIT_PREFIX + "encoder.layers.0.mlp.fc1.weight": torch.zeros(272, 144), "lm_head.weight": torch.zeros(320, 256)}
    hf = types.SimpleNamespace(hidden_size=256, intermediate_size=384, num_hidden_layers=1, num_attention_heads=2, num_key_value_heads=1,
                               rms_norm_eps=1e-6, rope_theta=1e6, world_position_embedding_type="minmax-sin3d")
    cfg = loader.engine_config(hf, sd)
    assert (cfg.aggregation, cfg.n_points, cfg.discrete) == ("minmax", 2, False)
    del hf.world_position_embedding_type
    cfg = loader.engine_config(hf, sd)
    assert (cfg.aggregation, cfg.n_points, cfg.discrete) == ("avg", 1, True)
    hf.world_position_embedding_type = "avg-discrete-mlp"
    with pytest.raises(V3DError):
        loader.engine_config(hf, sd)
