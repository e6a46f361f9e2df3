"""The engine under the learned MLP position encoding against the REFERENCE's own whole model (tests/golden/tiny_model_pe_mlp.npz, written
by tools/gen_pe_mlp_golden.py: the tiny LlavaQwenForCausalLM of tests/golden/tiny_model.npz - same weights, same F2 inputs - with an `mlp`
world_position_embedding_type and six seeded MLP tensors), after tests/test_gpu_pe_variants_model.py and with its tolerances; the overlay
building the module, scene reuse under it, the trainable module's checkpoint round trip, and the shipped type left as it was."""
import dataclasses

import pytest
import torch

import pe_mlp_check as MC
import tiny_model_fixture as TM
from test_gpu_pe_variants_model import SCORE_TOL, TOL, _assert_tokens_or_near_tie, rel_err

pytestmark = pytest.mark.gpu

CASES = [("avg-discrete-mlp", "f16"), ("avg-discrete-mlp", "bf16"), ("avg-mlp", "f16"), ("sample1-discrete-mlp", "f16")]


@pytest.fixture(scope="module")
def g():
    return TM.load()


@pytest.fixture(scope="module")
def gm(golden):
    return golden("tiny_model_pe_mlp")


def mlp_tensors(gm):
    """the six seeded tensors (bf16 bits) under their reference keys, as f32."""
    return {MC.SD_PREFIX + MC.REF_KEYS[k]: MC.from_bits(gm["mlp." + k], "bf16").float() for k in MC.KEYS}


def state_dict(g, gm, zero_pe=False):
    sd = dict(TM.state_dict(g), **mlp_tensors(gm))
    if zero_pe:
        for k in ("mlp.3.weight", "mlp.3.bias"):
            sd[MC.SD_PREFIX + k] = torch.zeros_like(sd[MC.SD_PREFIX + k])
    return sd


def _engine(g, gm, wtype, dt, zero_pe=False, **kw):
    from v3d.engine import Engine
    from v3d.loader import parse_mlp_position_type
    aggregation, n_points, discrete = parse_mlp_position_type(wtype)
    cfg = dataclasses.replace(TM.engine_config(), aggregation=aggregation, n_points=n_points, discrete=discrete, pe_kind="mlp")
    return Engine(cfg, state_dict(g, gm, zero_pe), dtype=dt, device="cuda", max_frames=2, **kw)


def _want(gm, wtype, kind, name):
    return MC.from_bits(gm[f"{wtype.replace('-', '_')}_{name}_{kind}"], kind).float()


@pytest.mark.parametrize("wtype,kind", CASES)
def test_engine_matches_reference_model(g, gm, wtype, kind):
    dt, tol = TM.DT[kind], TOL[kind]
    tag = wtype.replace("-", "_")
    inp = TM.case_inputs(g, "F2")
    eng = _engine(g, gm, wtype, dt)
    assert eng.pe_kind == "mlp" and eng.pe_table is None and set(eng.pe_mlp) == set(MC.KEYS)
    feats = eng.encode_images(inp["images"].cuda())
    vox = eng.voxel_ids(inp["world_coords"].to(dt).cuda())
    assert vox.dtype == dt and tuple(vox.shape) == (2, 14, 14, 3)           # the dtype-valued coordinates, not int32 ids
    if "discrete" in wtype:
        assert bool((vox.float() == vox.float().round()).all())
    x = eng.build_inputs_embeds(inp["ids"], feats, vox)
    from v3d import ops
    assert torch.equal(eng.ws.pe_rows[:392], ops.pe_mlp(vox, eng.pe_mlp))       # the PE rows lie in the engine's own scratch
    want = _want(gm, wtype, kind, "embeds")
    assert tuple(x.shape) == tuple(want.shape) == (11 + 420, 256)
    err = rel_err(x, want)
    print(f"{wtype} {kind}: inputs_embeds rel L2 {err:.2e}")
    assert err < tol
    # the encoding itself must be what the bound sees: with the PE zeroed the embeds are outside it by more than 10 x
    zero = _engine(g, gm, wtype, dt, zero_pe=True)
    zx = zero.build_inputs_embeds(inp["ids"], zero.encode_images(inp["images"].cuda()), zero.voxel_ids(inp["world_coords"].to(dt).cuda()))
    assert rel_err(zx, want) > 10 * tol
    logits = eng.llm_forward(x, 0)
    want_logits = torch.from_numpy(gm[f"{tag}_logits_{kind}"])
    assert rel_err(logits, want_logits) < 3 * tol
    toks = eng.generate(inp["ids"], inp["images"].cuda(), inp["world_coords"].cuda(), max_new_tokens=4).tolist()
    steps = [want_logits] + list(torch.from_numpy(gm[f"{tag}_step_logits_{kind}"]))
    _assert_tokens_or_near_tie(toks, gm[f"{tag}_tokens_{kind}"].tolist(), steps)


@pytest.mark.parametrize("kind", ["f16", "bf16"])
def test_coord_rows_and_grounding_scores(g, gm, kind):
    """Scan2Cap's <coord> rows (the box centre voxelised and encoded by the same module: llava_arch.py:416-418, 697-700) and the infonce
    grounding scores (object centres likewise, :420, :499-501), with the bounds of tests/test_gpu_pe_variants_model.py:86-112."""
    wtype, dt, tol = "avg-discrete-mlp", TM.DT[kind], TOL[kind]
    inp = TM.case_inputs(g, "F2")
    cids, box = torch.from_numpy(g["F2_cids"]), torch.from_numpy(g["F2_box_in"])
    eng = _engine(g, gm, wtype, dt)
    feats = eng.encode_images(inp["images"].cuda())
    vox = eng.voxel_ids(inp["world_coords"].to(dt).cuda())
    x = eng.build_inputs_embeds(cids, feats, vox, box_input=box, coord_token_id=317)
    want = _want(gm, wtype, kind, "coord_rows")
    got = x[[8 + 420 - 1, 11 + 420 - 1]].float().cpu()
    ulp = 2.0 ** (-7 if kind == "bf16" else -10)
    assert bool(((got - want).abs() <= ulp * (want.abs() + 1.0)).all())
    logits = eng.llm_forward(x, 0)
    assert rel_err(logits, torch.from_numpy(gm[f"avg_discrete_mlp_coord_logits_{kind}"])) < 3 * tol
    at = cids.tolist().index(-200)
    eng.use(eng.new_context())
    eng.prefill_scene(cids[: at + 1], inp["images"].cuda(), inp["world_coords"].cuda())
    a = eng.answer(cids[at + 1:], max_new_tokens=3, box_input=box, coord_token_id=317)
    b = eng.answer_group([cids[at + 1:]], max_new_tokens=3, box_inputs=[box], coord_token_id=317)[0]
    assert torch.equal(a.cpu(), b.cpu()[: len(a)])
    gi = int((inp["glabels"] == TM.GROUND_TOKEN).nonzero()[0])
    scores = eng.ground_scores(inp["gids"], gi, inp["images"].cuda(), inp["world_coords"].cuda(), inp["boxes"])
    assert scores.shape == (6,)
    assert float((scores.float().cpu() - _want(gm, wtype, kind, "scores")).abs().max()) < SCORE_TOL[kind]


def test_scene_reuse(g, gm):
    """prefill_scene + answer / answer_group give the tokens generate gives for each question alone, under the margin rule of
    tests/test_gpu_scene_reuse.py:47-58."""
    from test_gpu_scene_reuse import _assert_flips_are_near_ties
    inp = TM.case_inputs(g, "F2")
    eng = _engine(g, gm, "avg-discrete-mlp", torch.float16)
    gen = torch.Generator().manual_seed(5)
    images, coords = inp["images"].cuda(), inp["world_coords"].cuda()
    prefix = torch.cat([torch.randint(0, 300, (9,), generator=gen), torch.tensor([-200])])
    questions = [torch.randint(0, 300, (n,), generator=gen) for n in (12, 3, 20)]
    steps = 4
    alone = [eng.generate(torch.cat([prefix, q]), images, coords, max_new_tokens=steps).clone().cpu() for q in questions]
    eng.use(eng.new_context())
    assert eng.prefill_scene(prefix, images, coords) == 9 + 420
    rows = [t.cpu() for t in eng.answer_group(questions, max_new_tokens=steps)]
    assert all(len(r) == steps for r in rows)
    _assert_flips_are_near_ties(eng, questions, alone, rows, steps)
    one = eng.answer(questions[0], max_new_tokens=steps).cpu()
    _assert_flips_are_near_ties(eng, questions[:1], alone[:1], [one], steps)


def test_overlay_builds_the_module_and_generates_what_the_engine_generates(g, gm):
    from llava.model.language_model.llava_qwen import LlavaQwenConfig, LlavaQwenForCausalLM
    from llava.model.position_encoding import PositionEmbeddingMLP
    from v3d import ops
    inp = TM.case_inputs(g, "F2")
    hf = LlavaQwenConfig(vocab_size=320, hidden_size=256, intermediate_size=384, num_hidden_layers=2, num_attention_heads=2,
                         num_key_value_heads=1, max_position_embeddings=2048, rms_norm_eps=1e-6, rope_theta=1000000.0)
    hf.rope_theta, hf.ground_head_type, hf.world_position_embedding_type = 1000000.0, "infonce", "avg-discrete-mlp"
    hf.min_xyz_range, hf.max_xyz_range, hf.voxel_size = [-15, -15, -5], [15, 15, 5], 0.1
    model = LlavaQwenForCausalLM(hf, state_dict(g, gm), dtype=torch.float16, device="cuda")
    mod = model.get_model().world_position_embedding
    assert isinstance(mod, PositionEmbeddingMLP) and mod.hidden_size == 512
    assert sorted(k for k, _ in mod.named_parameters()) == sorted(MC.REF_KEYS.values())
    vd = {"world_coords": inp["world_coords"][None].half().cuda(), "box_input": torch.Tensor([]), "objects": inp["boxes"][None].half().cuda()}
    out = model.generate(inp["ids"][None].cuda(), images=inp["images"][None].half().cuda(), modalities="video", do_sample=False, num_beams=1,
                         max_new_tokens=4, use_cache=True, video_dict=vd)
    eng = _engine(g, gm, "avg-discrete-mlp", torch.float16)
    toks = eng.generate(inp["ids"], inp["images"].cuda(), inp["world_coords"].cuda(), max_new_tokens=4)
    assert out[0].tolist()[: len(toks)] == toks.tolist()
    # the module's call contract: [B, N, 3] -> [B, N, E], the engine's own rows
    xyz = MC.seeded_inputs("f16", "ids", 50)[None].cuda()
    pe = mod(xyz)
    assert tuple(pe.shape) == (1, 50, 256) and torch.equal(pe[0], ops.pe_mlp(xyz[0], eng.pe_mlp))
    assert torch.equal(pe[0], ops.pe_mlp(xyz[0], model.engine.pe_mlp))
    assert torch.equal(eng.centre_pe(xyz[0].contiguous()), ops.pe_mlp(ops.discrete_coords(xyz[0].contiguous()), eng.pe_mlp))     # voxelised first
    # a stand-alone module with loaded weights computes the same
    alone = PositionEmbeddingMLP(256)
    alone.load_state_dict({k[len(MC.SD_PREFIX):]: v for k, v in mlp_tensors(gm).items()}, strict=True)
    assert torch.equal(alone.to(device="cuda", dtype=torch.float16)(xyz), pe)
    with pytest.raises(NotImplementedError):
        PositionEmbeddingMLP(256, n_points=9)


def test_shipped_type_is_what_it_was(g, gm):
    """The shipped type keeps its table and its kernels; MLP tensors in the state dict under a sin3d type are ignored."""
    import types

    from v3d import loader
    from v3d.engine import Engine
    inp = TM.case_inputs(g, "F2")
    eng = Engine(TM.engine_config(), TM.state_dict(g), dtype=torch.bfloat16, device="cuda", max_frames=2)
    assert eng.pe_kind == "sin3d" and eng.pe_table is not None and eng.pe_mlp is None
    hf = types.SimpleNamespace(**TM.HF_CONFIG)
    cfg = loader.engine_config(hf, state_dict(g, gm))
    assert cfg.pe_kind == "sin3d"
    both = Engine(dataclasses.replace(TM.engine_config(), pe_kind=cfg.pe_kind), state_dict(g, gm), dtype=torch.bfloat16, device="cuda", max_frames=2)
    assert both.pe_kind == "sin3d" and both.pe_table is not None and both.pe_mlp is None
    xs = []
    for e in (eng, both):
        feats = e.encode_images(inp["images"].cuda())
        vox = e.voxel_ids(inp["world_coords"].to(torch.bfloat16).cuda())
        assert vox.dtype == torch.int32
        xs.append(e.build_inputs_embeds(inp["ids"], feats, vox).clone())
    assert torch.equal(xs[0], xs[1])
    assert rel_err(xs[0], TM.expected(g, "F2", "bf16")["embeds"]) < TOL["bf16"]
    hf.world_position_embedding_type = "avg-discrete-mlp"
    assert loader.engine_config(hf, state_dict(g, gm)).pe_kind == "mlp"


def test_trainable_module_round_trips_the_six_tensors(g, gm):
    from v3d._native import V3DError
    from v3d.train_module import LlavaQwenTrainable
    sd = {k: v.to(torch.bfloat16) for k, v in state_dict(g, gm).items()}
    m = LlavaQwenTrainable.from_reference_state_dict(sd, n_q=2, n_kv=1, vit_heads=2, dtype=torch.bfloat16, device="cuda",
                                                     world_position_embedding_type="avg-discrete-mlp")
    assert m.pe_kind == "mlp" and m.pe_table is None
    assert sorted(n for n in m.names if n.startswith("pe_mlp.")) == sorted("pe_mlp." + k for k in MC.KEYS)
    back = m.reference_state_dict()
    assert set(back) == set(sd)
    for k in mlp_tensors(gm):
        assert back[k].dtype == torch.bfloat16 and torch.equal(back[k].cpu(), sd[k]), k
    # under the shipped type the same tensors are carried through unmodelled, bit for bit
    shipped = LlavaQwenTrainable.from_reference_state_dict(sd, n_q=2, n_kv=1, vit_heads=2, dtype=torch.bfloat16, device="cuda")
    assert shipped.pe_kind == "sin3d" and not any(n.startswith("pe_mlp.") for n in shipped.names)
    back = shipped.reference_state_dict()
    for k in mlp_tensors(gm):
        assert torch.equal(back[k].cpu(), sd[k]), k
    with pytest.raises(V3DError, match="model.world_position_embedding.mlp.0.weight"):
        LlavaQwenTrainable.from_reference_state_dict({k: v.to(torch.bfloat16) for k, v in TM.state_dict(g).items()}, n_q=2, n_kv=1, vit_heads=2,
                                                     dtype=torch.bfloat16, device="cuda", world_position_embedding_type="avg-discrete-mlp")
