"""The engine under the other sin3d position encodings against the REFERENCE's own whole model
(tests/golden/tiny_model_pe_variants.npz, written by tools/gen_pe_points_golden.py: the tiny LlavaQwenForCausalLM of
tests/golden/tiny_model.npz - same weights, same F2 inputs - with another world_position_embedding_type), the overlay taking the
type, scene reuse under it, and the refusals."""
import dataclasses

import pytest
import torch

import pe_points_check as PC
import tiny_model_fixture as TM

pytestmark = pytest.mark.gpu

CASES = [("sample9-discrete-sin3d", "f16"), ("sample9-discrete-sin3d", "bf16"), ("minmax-discrete-sin3d", "f16"), ("sample5-sin3d", "f16"),
         ("sample1-discrete-sin3d", "f16")]
# relative L2 of inputs_embeds: tests/test_gpu_model_golden.py:30 (2e-2 bf16, 3e-3 f16), x3 on the logits (:45)
TOL = {"bf16": 2e-2, "f16": 3e-3}
# grounding scores, absolute: tests/test_gpu_model_golden.py:58
SCORE_TOL = {"bf16": 4e-2, "f16": 6e-3}


def rel_err(got, want):
    got, want = got.float().cpu(), want.float()
    return ((got - want).norm() / want.norm().clamp_min(1e-9)).item()


@pytest.fixture(scope="module")
def g():
    return TM.load()


@pytest.fixture(scope="module")
def gv(golden):
    return golden("tiny_model_pe_variants")


def _engine(g, wtype, dt, **kw):
    from v3d.engine import Engine
    from v3d.loader import parse_position_type
    aggregation, n_points, discrete = parse_position_type(wtype)
    cfg = dataclasses.replace(TM.engine_config(), aggregation=aggregation, n_points=n_points, discrete=discrete)
    return Engine(cfg, TM.state_dict(g), dtype=dt, device="cuda", max_frames=2, **kw)


def _want(gv, wtype, kind, name):
    return PC.from_bits(gv[f"{wtype.replace('-', '_')}_{name}_{kind}"], kind).float()


def _assert_tokens_or_near_tie(toks, want_tokens, ref_steps):
    """the margin rule of tests/test_gpu_model_golden.py:49-55 / tests/test_gpu_engine.py:71-76: a differing token's top-2 logit margin in
    the reference is below 0.05 of its largest |logit|."""
    for i, (a, b) in enumerate(zip(toks, want_tokens)):
        if a != b:
            top2 = torch.topk(ref_steps[i], 2).values
            assert (top2[0] - top2[1]).item() < 0.05 * ref_steps[i].abs().max().item(), f"token {i}: {a} != {b}"
            return
    assert list(toks) == list(want_tokens)


@pytest.mark.parametrize("wtype,kind", CASES)
def test_engine_matches_reference_model(g, gv, wtype, kind):
    dt, tol = TM.DT[kind], TOL[kind]
    inp = TM.case_inputs(g, "F2")
    eng = _engine(g, wtype, dt)
    assert (eng.pe_table is None) == ("discrete" not in wtype)
    feats = eng.encode_images(inp["images"].cuda())
    vox = eng.voxel_ids(inp["world_coords"].to(dt).cuda())
    x = eng.build_inputs_embeds(inp["ids"], feats, vox)
    want = _want(gv, wtype, kind, "embeds")
    assert tuple(x.shape) == tuple(want.shape) == (11 + 420, 256)
    err = rel_err(x, want)
    print(f"{wtype} {kind}: inputs_embeds rel L2 {err:.2e}")
    assert err < tol
    # the encoding itself must be what separates the cases: the shipped type's embeds are far outside the bound
    assert rel_err(TM.expected(g, "F2", kind)["embeds"], want) > 10 * tol
    logits = eng.llm_forward(x, 0)
    want_logits = torch.from_numpy(gv[f"{wtype.replace('-', '_')}_logits_{kind}"])
    assert rel_err(logits, want_logits) < 3 * tol
    toks = eng.generate(inp["ids"], inp["images"].cuda(), inp["world_coords"].cuda(), max_new_tokens=4).tolist()
    steps = [want_logits] + list(torch.from_numpy(gv[f"{wtype.replace('-', '_')}_step_logits_{kind}"]))
    _assert_tokens_or_near_tie(toks, gv[f"{wtype.replace('-', '_')}_tokens_{kind}"].tolist(), steps)


@pytest.mark.parametrize("kind", ["f16", "bf16"])
def test_coord_rows_and_grounding_scores_sample9(g, gv, kind):
    """Scan2Cap's <coord> rows (the box centre repeated 9 times, voxelised, encoded: llava_arch.py:409-418, 697-700) and the infonce
    grounding scores (object centres likewise, :413, :420, :500), with the bounds of tests/test_gpu_model_golden.py:58-85."""
    wtype, dt, tol = "sample9-discrete-sin3d", TM.DT[kind], TOL[kind]
    inp = TM.case_inputs(g, "F2")
    cids, box = torch.from_numpy(g["F2_cids"]), torch.from_numpy(g["F2_box_in"])
    eng = _engine(g, wtype, dt)
    feats = eng.encode_images(inp["images"].cuda())
    vox = eng.voxel_ids(inp["world_coords"].to(dt).cuda())
    x = eng.build_inputs_embeds(cids, feats, vox, box_input=box, coord_token_id=317)
    want = _want(gv, wtype, kind, "coord_rows")
    got = x[[8 + 420 - 1, 11 + 420 - 1]].float().cpu()
    ulp = 2.0 ** (-7 if kind == "bf16" else -10)
    assert bool(((got - want).abs() <= ulp * (want.abs() + 1.0)).all())          # PE within 1 ulp16, one rounded add
    logits = eng.llm_forward(x, 0)
    assert rel_err(logits, torch.from_numpy(gv[f"sample9_discrete_sin3d_coord_logits_{kind}"])) < 3 * tol
    # the same prompt through prefill_scene + answer (the fourth place a box centre is encoded) gives generate's tokens
    at = cids.tolist().index(-200)
    eng.use(eng.new_context())
    eng.prefill_scene(cids[: at + 1], inp["images"].cuda(), inp["world_coords"].cuda())
    a = eng.answer(cids[at + 1:], max_new_tokens=3, box_input=box, coord_token_id=317)
    b = eng.answer_group([cids[at + 1:]], max_new_tokens=3, box_inputs=[box], coord_token_id=317)[0]
    assert torch.equal(a.cpu(), b.cpu()[: len(a)])
    gi = int((inp["glabels"] == TM.GROUND_TOKEN).nonzero()[0])
    scores = eng.ground_scores(inp["gids"], gi, inp["images"].cuda(), inp["world_coords"].cuda(), inp["boxes"])
    assert scores.shape == (6,)
    assert float((scores.float().cpu() - _want(gv, wtype, kind, "scores")).abs().max()) < SCORE_TOL[kind]


def test_overlay_takes_the_type(g):
    """LlavaQwenForCausalLM with hf.world_position_embedding_type = 'sample9-discrete-sin3d' generates what the engine call generates, and
    its world_position_embedding module is built for 9 points."""
    from llava.model.language_model.llava_qwen import LlavaQwenConfig, LlavaQwenForCausalLM
    from llava.model.position_encoding import PositionEmbeddingSine3D
    from v3d import ops
    inp = TM.case_inputs(g, "F2")
    hf = LlavaQwenConfig(vocab_size=320, hidden_size=256, intermediate_size=384, num_hidden_layers=2, num_attention_heads=2,
                         num_key_value_heads=1, max_position_embeddings=2048, rms_norm_eps=1e-6, rope_theta=1000000.0)
    hf.rope_theta, hf.ground_head_type, hf.world_position_embedding_type = 1000000.0, "infonce", "sample9-discrete-sin3d"
    hf.min_xyz_range, hf.max_xyz_range, hf.voxel_size = [-15, -15, -5], [15, 15, 5], 0.1
    model = LlavaQwenForCausalLM(hf, TM.state_dict(g), dtype=torch.float16, device="cuda")
    assert model.get_model().world_position_embedding.n_points == 9
    vd = {"world_coords": inp["world_coords"][None].half().cuda(), "box_input": torch.Tensor([]), "objects": inp["boxes"][None].half().cuda()}
    out = model.generate(inp["ids"][None].cuda(), images=inp["images"][None].half().cuda(), modalities="video", do_sample=False, num_beams=1,
                         max_new_tokens=4, use_cache=True, video_dict=vd)
    eng = _engine(g, "sample9-discrete-sin3d", torch.float16)
    toks = eng.generate(inp["ids"], inp["images"].cuda(), inp["world_coords"].cuda(), max_new_tokens=4)
    assert out[0].tolist()[: len(toks)] == toks.tolist()
    # the mixin's aggregation methods, with the reference's names and shapes
    x = PC.seeded_coords("f16").cuda()
    assert tuple(model.sample_n_points(x, n_points=9).shape) == (2, 14, 14, 9, 3)
    assert tuple(model.sample_n_points(x, n_points=1).shape) == (2, 14, 14, 3)
    assert tuple(model.minmax_coordinate_in_patch(x).shape) == (2, 14, 14, 2, 3)
    pe = PositionEmbeddingSine3D(256, n_points=9)
    xyz = PC.pe_inputs(256, 9, "f16", True)[None].cuda()
    assert torch.equal(pe(xyz), ops.sin3d_pe(xyz, 256, n_points=9))


def test_scene_reuse_under_minmax(g):
    """prefill_scene + answer_group of 3 questions give the tokens generate gives for each question alone, under the margin rule
    (tests/test_gpu_scene_reuse.py:47-58: a flip only where answer()'s own top-2 margin is below 0.02 of the largest |logit|)."""
    from test_gpu_scene_reuse import _assert_flips_are_near_ties
    inp = TM.case_inputs(g, "F2")
    eng = _engine(g, "minmax-discrete-sin3d", torch.float16)
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


def test_refusals(g):
    import types
    from v3d import loader
    from v3d._native import V3DError
    from v3d.train_module import LlavaQwenTrainable
    hf = types.SimpleNamespace(**TM.HF_CONFIG)
    for bad in ("avg-discrete-mlp", "avg-discrete-sin3d-mrope", "mrope", "discrete-sin3d"):
        hf.world_position_embedding_type = bad
        with pytest.raises(V3DError, match="world_position_embedding_type"):
            loader.engine_config(hf, TM.state_dict(g))
    hf.world_position_embedding_type = "minmax-sin3d"
    cfg = loader.engine_config(hf, TM.state_dict(g))
    assert (cfg.aggregation, cfg.n_points, cfg.discrete) == ("minmax", 2, False)
    with pytest.raises(V3DError, match="training supports"):
        LlavaQwenTrainable({"newline": torch.zeros(256, device="cuda")}, 2, 1, world_position_embedding_type="sample9-discrete-sin3d")
    from v3d.engine import Engine
    with pytest.raises(V3DError, match="n_points"):      # a hand-made config whose fields contradict each other
        Engine(dataclasses.replace(TM.engine_config(), aggregation="minmax", n_points=9), TM.state_dict(g), dtype=torch.float16,
               device="cuda", max_frames=2)
