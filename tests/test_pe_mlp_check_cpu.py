"""The CPU restatement of the learned MLP position encoding (tests/pe_mlp_check.py) against the reference module's own outputs
(tests/golden/pe_mlp.npz and, stage by stage with the weights as drawn, tests/golden/pe_mlp_stages.npz; both written by
tools/gen_pe_mlp_golden.py), the hidden kernel's bounds against an f32 emulation of its arithmetic
(and against four wrong kernels), and the type-string parser and engine_config for the `mlp` types."""
import types

import numpy as np
import pytest
import torch

import pe_mlp_check as MC
import rowwise_check as RC

WORST = {}


@pytest.mark.parametrize("E,kind,src", MC.MODULE_CASES)
def test_restatement_reproduces_the_reference_module(golden, E, kind, src):
    """At most 1 % of the elements of a case may differ, none by more than one ulp of the output: any more means the rule is wrong."""
    want = golden("pe_mlp")[f"pe_E{E}_{src}_{kind}"]
    p, x = MC.seeded_mlp(E, kind), MC.seeded_inputs(kind, src, MC.ROWS[E])
    share, worst = MC.ulp_shares(MC.restate(x, p), want)
    print(f"E={E} {kind} {src}: {100 * share:.3f} % of {want.size} elements differ, at most {worst} ulp")
    assert tuple(want.shape) == (MC.ROWS[E], E)
    assert share <= 0.01 and worst <= 1
    xf = x.float()
    if src == "ids":
        assert bool((xf == xf.round()).all()) and xf.max() > 256, "integer-valued inputs, ids above 256 included"
    else:
        assert xf.min() < 0 and bool((xf != xf.round()).any()), "continuous inputs, negative ones included"


def _ulps(got, want_bits):
    return np.abs(MC.ordered(MC.bits(got)) - MC.ordered(want_bits))


@pytest.mark.parametrize("kind,src", MC.STAGE_CASES)
def test_restatement_stage_by_stage_with_the_weights_as_drawn(golden, kind, src):
    """The reference module's own z, h and pe (tests/golden/pe_mlp_stages.npz; no b3 offset, so outputs that cancel to near zero are in).
    Each stage of the restatement: at most 1 % of the elements differ, and every element is within one ulp of the reference OR within
    what the reference's own f32 arithmetic of that stage may be off by (rowwise_check.layernorm's bound for h, last_linear_slack for pe -
    a unit in the last place of a near-zero output is far below either).  The last Linear is restated from the reference's own h, so that
    its bound is not charged with an upstream flip; the whole chain is held to the 1 % share."""
    g = golden("pe_mlp_stages")
    dt = MC.DT[kind]
    for E in (256, 3584):
        p, x = MC.seeded_mlp(E, kind, b3_offset=0.0), MC.seeded_inputs(kind, src, MC.STAGE_ROWS[E])
        z, h, pe = MC.restate(x, p, stages=True)
        want_pe = g[f"pe_E{E}_{src}_{kind}"]
        assert float((_ulps(pe, want_pe) != 0).mean()) <= 0.01
        assert float(np.abs(MC.from_bits(want_pe, kind).float().numpy()).min()) < 2.0 ** -6, "the case must hold outputs near zero"
        ref_h = MC.from_bits(g[f"h_{src}_{kind}"] if E == 256 else g[f"h_E{E}_{src}_{kind}"], kind)
        last = MC._round(ref_h.double() @ p["w3"].double().T + p["b3"].double(), dt).to(dt)
        d = _ulps(last, want_pe)
        err = (last.double() - MC.from_bits(want_pe, kind).double()).abs().numpy()
        ok = (d <= 1) | (err <= MC.last_linear_slack(ref_h, p).numpy())
        print(f"{kind} {src} E={E}: pe from the reference's h: {100 * (d != 0).mean():.3f} % differ, at most {d.max()} ulp, worst err / slack "
              f"{(err / MC.last_linear_slack(ref_h, p).numpy()).max():.3f}")
        assert (d != 0).mean() <= 0.01 and ok.all()
        if E != 256:
            continue
        dz = _ulps(z, g[f"z_{src}_{kind}"])
        assert (dz != 0).mean() <= 0.01 and dz.max() <= 1
        ref_z = MC.from_bits(g[f"z_{src}_{kind}"], kind)
        hr = torch.relu(MC._round(RC.layernorm(ref_z, p["ln_w"], p["ln_b"], MC.EPS)[0], dt)).to(dt)      # from the reference's own z
        dh = _ulps(hr, g[f"h_{src}_{kind}"])
        errh = (hr.double() - ref_h.double()).abs()
        okh = torch.from_numpy(dh <= 1) | (errh <= RC.layernorm(ref_z, p["ln_w"], p["ln_b"], MC.EPS)[1])
        print(f"{kind} {src}: z {100 * (dz != 0).mean():.3f} % / {dz.max()} ulp;  h {100 * (dh != 0).mean():.3f} % / {dh.max()} ulp")
        assert (dh != 0).mean() <= 0.01 and bool(okh.all())
        assert float((_ulps(h, g[f"h_{src}_{kind}"]) != 0).mean()) <= 0.01


@pytest.mark.parametrize("kind", ["f16", "bf16"])
def test_restatement_is_sensitive_to_the_rounding_points(golden, kind):
    """Dropping the rounding of z or of the LayerNorm output - another rule - moves far more than 1 % of the elements."""
    E, src = 256, "cont"
    want = golden("pe_mlp")[f"pe_E{E}_{src}_{kind}"]
    p, x = MC.seeded_mlp(E, kind), MC.seeded_inputs(kind, src, MC.ROWS[E])
    pd = {k: v.double() for k, v in p.items()}
    z = x.double() @ pd["w0"].T + pd["b0"]                                           # z NOT rounded
    y = torch.nn.functional.layer_norm(z, (MC.HIDDEN,), pd["ln_w"], pd["ln_b"], MC.EPS)   # nor the LayerNorm's output
    pe = MC._round(torch.relu(y) @ pd["w3"].T + pd["b3"], x.dtype).to(x.dtype)
    share, _ = MC.ulp_shares(pe, want)
    assert share > 0.01, share


@pytest.mark.parametrize("kind", ["f16", "bf16"])
@pytest.mark.parametrize("src", ["ids", "cont"])
def test_emulated_kernel_is_inside_the_bounds(kind, src):
    """An f32 emulation of v3d_pe_mlp_hidden (three fused multiply-adds, f32 row statistics in the kernel's order) against the bounds the
    GPU test holds the kernel to; the worst ratio is recorded."""
    p, x = MC.seeded_mlp(256, kind), MC.seeded_inputs(kind, src, 393)
    z, h = MC.emulate_hidden(x, p)
    rz, rh = RC.ratio(z, MC.z_reference(x, p)), RC.ratio(h, MC.h_reference(z, p))
    WORST[(kind, src)] = (rz, rh)
    print(f"{kind} {src}: worst ratio z {rz:.3f}, h {rh:.3f}")
    assert rz <= 1.0 and rh <= 1.0
    # the emulation follows the rule: its stages are the restatement's up to rounding flips
    sz, sh, _ = MC.restate(x, p, stages=True)
    for got, want in ((z, sz), (h, sh)):
        share, worst = MC.ulp_shares(got, MC.bits(want))
        assert share < 0.01 and worst <= 1, (share, worst)


def test_worst_ratios_of_the_emulated_kernel():
    """Runs after the cases above (file order): the worst |err| / bound per dtype and input kind, printed (-s) and held below 1 - and
    above 0.5, so that a bound loosened by a factor of two would show here."""
    assert set(WORST) == {(k, s) for k in ("f16", "bf16") for s in ("ids", "cont")}, "run the whole file"
    for key, (rz, rh) in sorted(WORST.items()):
        print(f"{key[0]:5s} {key[1]:5s} z {rz:.3f}  h {rh:.3f}")
    assert max(r for pair in WORST.values() for r in pair) <= 1.0
    assert max(rz for rz, _ in WORST.values()) > 0.5 and max(rh for _, rh in WORST.values()) > 0.5


@pytest.mark.parametrize("kind", ["f16", "bf16"])
@pytest.mark.parametrize("mutate", MC.MUTATIONS)
def test_bounds_reject_wrong_kernels(kind, mutate):
    """b0 dropped, g and beta swapped, the unbiased variance, ReLU before the LayerNorm: each is outside the bounds."""
    p, x = MC.seeded_mlp(256, kind), MC.seeded_inputs(kind, "cont", 393)
    z, h = MC.emulate_hidden(x, p, mutate=mutate)
    rz = RC.ratio(z, MC.z_reference(x, p))
    rh = RC.ratio(h, MC.h_reference(z, p))          # centred on the mutated kernel's own z, as the GPU test does
    print(f"{kind} {mutate}: ratio z {rz:.3g}, h {rh:.3g}")
    assert max(rz, rh) > 1.0
    if mutate == "no_b0":
        assert rz > 1.0
    else:
        assert rz <= 1.0 and rh > 1.0


def test_wgrad_bound_is_exact_on_integers():
    """Integer-valued dz and x: every product and partial sum is exact in f32, so the f64 reference is the bit-exact answer and a dropped
    row or partial moves it by an integer."""
    g = torch.Generator().manual_seed(3)
    dz = torch.randint(-3, 4, (400, MC.HIDDEN), generator=g).to(torch.bfloat16)
    x = torch.randint(0, 8, (400, 3), generator=g).to(torch.bfloat16)
    dw, bound = MC.wgrad_reference(dz, x, torch.float32)
    assert bool((dw == dw.round()).all()) and dw.abs().max() < 2 ** 24
    assert float(bound.max()) < 0.5          # so any wrong integer is outside


def test_encoder_parser():
    from v3d._native import V3DError
    from v3d.loader import parse_mlp_position_type, parse_position_encoder, parse_position_type
    for wtype, want in (("avg-discrete-mlp", ("avg", 1, True)), ("avg-mlp", ("avg", 1, False)), ("sample1-discrete-mlp", ("sample1", 1, True)),
                        ("sample1-mlp", ("sample1", 1, False))):
        assert parse_position_encoder(wtype) == "mlp"
        assert parse_mlp_position_type(wtype) == want
        with pytest.raises(V3DError):
            parse_position_type(wtype)                                   # the sin3d parser keeps its contract
    assert parse_position_encoder("avg-discrete-sin3d-mlp") == "mlp"     # `mlp` wins over `sin3d` (llava_arch.py:60-63)
    for wtype in ("avg-discrete-sin3d", "sample9-sin3d", "minmax-discrete-sin3d"):
        assert parse_position_encoder(wtype) == "sin3d"
        with pytest.raises(V3DError):
            parse_mlp_position_type(wtype)
    for bad, why in (("sample9-discrete-mlp", "num_feats"), ("sample5-mlp", "num_feats"), ("minmax-mlp", "num_feats"),
                     ("avg-discrete-mlp-mrope", "mrope"), ("mrope", "mrope"), ("avg-discrete-sin3d-mrope", "mrope"), ("mlp", "names none")):
        with pytest.raises(V3DError, match="world_position_embedding_type") as e:
            parse_position_encoder(bad)
        assert why in str(e.value), (bad, str(e.value))


def _tiny_sd():
    from v3d import loader
    return {loader.VIT_PREFIX + "embeddings.patch_embedding.weight": torch.zeros(144, 3, 14, 14),
            loader.VIT_PREFIX + "embeddings.position_embedding.weight": torch.zeros(729, 144),
            loader.VIT_PREFIX + "encoder.layers.0.mlp.fc1.weight": torch.zeros(272, 144), "lm_head.weight": torch.zeros(320, 256)}


def test_engine_config_takes_an_mlp_type_with_its_tensors():
    from v3d import loader
    from v3d._native import V3DError
    from v3d.engine import EngineConfig
    assert EngineConfig().pe_kind == "sin3d"
    hf = types.SimpleNamespace(hidden_size=256, intermediate_size=384, num_hidden_layers=1, num_attention_heads=2, num_key_value_heads=1,
                               rms_norm_eps=1e-6, rope_theta=1e6, world_position_embedding_type="avg-discrete-mlp")
    sd = _tiny_sd()
    with pytest.raises(V3DError, match="world_position_embedding_type.*model.world_position_embedding.mlp.0.weight"):
        loader.engine_config(hf, sd)
    mlp = {MC.SD_PREFIX + MC.REF_KEYS[k]: v for k, v in MC.seeded_mlp(256, "bf16").items()}
    part = dict(sd, **mlp)
    del part[MC.SD_PREFIX + "mlp.3.bias"]
    with pytest.raises(V3DError, match="mlp.3.bias"):
        loader.engine_config(hf, part)
    cfg = loader.engine_config(hf, dict(sd, **mlp))
    assert (cfg.pe_kind, cfg.aggregation, cfg.n_points, cfg.discrete) == ("mlp", "avg", 1, True)
    hf.world_position_embedding_type = "sample1-mlp"
    cfg = loader.engine_config(hf, dict(sd, **mlp))
    assert (cfg.pe_kind, cfg.aggregation, cfg.n_points, cfg.discrete) == ("mlp", "sample1", 1, False)
    for bad in ("sample9-discrete-mlp", "minmax-mlp", "avg-discrete-mlp-mrope"):
        hf.world_position_embedding_type = bad
        with pytest.raises(V3DError, match="world_position_embedding_type"):
            loader.engine_config(hf, dict(sd, **mlp))
    # MLP tensors under a sin3d type are ignored
    hf.world_position_embedding_type = "avg-discrete-sin3d"
    cfg = loader.engine_config(hf, dict(sd, **mlp))
    assert (cfg.pe_kind, cfg.aggregation, cfg.n_points, cfg.discrete) == ("sin3d", "avg", 1, True)


def test_trainable_module_accepts_the_mlp_types_and_refuses_the_rest():
    from v3d._native import V3DError
    from v3d.train_module import _training_position_type
    assert _training_position_type("avg-discrete-sin3d") == ("sin3d", "avg", True)
    assert _training_position_type("avg-discrete-mlp") == ("mlp", "avg", True)
    assert _training_position_type("sample1-mlp") == ("mlp", "sample1", False)
    for bad in ("sample9-discrete-sin3d", "avg-sin3d", "minmax-sin3d"):
        with pytest.raises(V3DError, match="training supports"):
            _training_position_type(bad)
    for bad in ("sample9-discrete-mlp", "mrope"):
        with pytest.raises(V3DError, match="world_position_embedding_type"):
            _training_position_type(bad)


def test_training_steps_name_missing_centres():
    """pe_mlp without the centres it has to encode is refused by name, before anything runs."""
    from v3d import train
    from v3d._native import V3DError
    rows, mask = torch.tensor([3, 5]), torch.zeros((6, 4), dtype=torch.uint8)
    with pytest.raises(V3DError, match="pe_centres"):
        train.sample_forward_backward({}, None, None, None, None, None, None, None, 2, 4, 2, 128, coord_rows=rows, pe_mlp={}, pe_centres=None)
    with pytest.raises(V3DError, match="pe_centres"):
        train.ground_sample_forward_backward({}, None, None, None, None, None, 7, mask, None, None, None, 2, 4, 2, 128, pe_mlp={}, pe_centres=None)
    with pytest.raises(V3DError, match=r"pe_centres \[6, 3\]"):
        train.ground_sample_forward_backward({}, None, None, None, None, None, 7, mask, None, None, None, 2, 4, 2, 128, pe_mlp={},
                                             pe_centres=torch.zeros((5, 3)))
