"""Engine.beam_search end to end on the two-layer test engine of tests/test_gpu_scene_reuse.py (bf16 and f16): every step's candidates against
an f64 decoder under tests/beam_check.py's check_topk, the state against BeamRef fed with the engine's own candidates, the result's
independence of how the prompt's K/V got there, and the public surface (generate / answer keywords, the overlay's generate_beam, the eval
runner's --num_beams).

Trace check.  The engine's trace (the K candidates of every executed step) is replayed on the host: BeamRef.step on the engine's candidates
gives the running sequences and scores before every step; the f64 decoder of tests/answer_check.py is teacher-forced with those sequences
behind the prompt; candidate (b, v) then has the f64 score running[b] (the engine's own f32 value, so nothing accumulates in the check) +
f64 log_softmax(f64 logits of beam b)[v].  bound = 2 e_ref[logits] max|logit| of the beam's row, e_ref[logits] as answer_check defines it
(the 16-bit oracle against f64 on the same rows, the maximum over all checked rows).  The prompt has 457 rows: not a multiple of 64.
MEASURED on one MI355X (-s prints them): e_ref[logits] 1.0e-2 .. 1.3e-2 (bf16) / 1.2e-3 .. 1.8e-3 (f16); worst |score - f64| 2.9e-2 .. 3.9e-2 (bf16) /
1.9e-3 .. 4.3e-3 (f16) against smallest bounds of 8.4e-2 / 1.0e-2: at most 0.40 of the bound.  The test model's greedy continuation settles on
one token after the first, so the searches with EOS ids end after 2 - 4 steps; the two cases without EOS run all 8 steps (the gather moves 1 .. 7 rows)."""
import json
import os

import pytest
import torch

import answer_check as ac
import beam_check as bc
from oracle import pipeline_oracle as PO
from v3d._native import V3DError

pytestmark = pytest.mark.gpu

OCFG = dict(layers=2, heads=2, kv_heads=1, rope_theta=1e6, eps=1e-6)
VOCAB, NEW = 320, 8
N_PRE, N_Q = 14, 23
S = N_PRE + 2 * 210 + N_Q


class _Box:
    pass


@pytest.fixture(scope="module", params=["bf16", "f16"])
def world(request):
    from v3d.engine import Engine, EngineConfig, LlmConfig, VitConfig, random_state_dict
    w = _Box()
    w.name, w.dt = request.param, {"bf16": torch.bfloat16, "f16": torch.float16}[request.param]
    cfg = EngineConfig(vit=VitConfig(hidden=144, inter=272, layers=2, heads=2),
                       llm=LlmConfig(hidden=256, inter=384, layers=2, heads=2, kv_heads=1, vocab=VOCAB, max_pos=1024))
    sd = random_state_dict(cfg, torch.float32, "cpu", seed=31, std=0.08)
    w.eng = Engine(cfg, sd, dtype=w.dt, device="cuda", max_frames=2)
    w.ref = ac.Reference(sd, w.dt, OCFG, "cuda")
    g = torch.Generator().manual_seed(32)
    w.images = torch.randn(2, 3, 384, 384, generator=g).cuda()
    w.coords = ((torch.rand(2, 384, 384, 3, generator=g) - 0.5) * 20).cuda()
    w.prefix = torch.cat([torch.randint(0, VOCAB, (N_PRE,), generator=g), torch.tensor([PO.IMAGE_TOKEN_INDEX])])
    w.question = torch.randint(0, VOCAB, (N_Q,), generator=g)
    w.prompt = torch.cat([w.prefix, w.question])
    assert S % 64 != 0
    # the prompt's rows as the engine embeds them, and both references' K/V and last-row logits of the prompt (computed once, shared)
    feats = w.eng.encode_images(w.images)
    x16 = w.eng.build_inputs_embeds(w.prompt, feats, w.eng.voxel_ids(w.coords.to(w.dt))).clone()
    assert x16.shape[0] == S
    kv64, _, lg64 = w.ref.forward64(x16.double()[None], 0)
    kv16, _, lg16 = w.ref.forward16(x16[None], 0)
    w.past64, w.past16, w.logits64_0, w.logits16_0 = kv64, kv16, lg64[0, -1:].clone(), lg16[0, -1:].double().clone()
    w.greedy = w.eng.generate(w.prompt, w.images, w.coords, max_new_tokens=NEW).cpu()
    yield w
    w.__dict__.clear()
    import gc
    gc.collect()
    torch.cuda.empty_cache()


def _step_logits(w, seqs):
    """f64 and 16-bit-oracle logits [B, V] of the next token behind [prompt | seqs[b]] (all of one length >= 1)"""
    ids = torch.tensor(seqs, dtype=torch.int64)
    x16 = w.ref.embed(ids)
    _, _, l64 = w.ref.forward64(x16.double(), S, w.past64)
    _, _, l16 = w.ref.forward16(x16, S, w.past16)
    return l64[:, -1], l16[:, -1].double()


def _replay(w, trace, B, eos, lp, label):
    """The module docstring's trace check.  -> (BeamRef after the last executed step, e_ref[logits], worst |score - f64|, smallest bound)"""
    K = trace["K"]
    ref = bc.BeamRef(B, VOCAB, NEW, eos, lp)
    assert ref.K == K and trace["cand_score"].shape == (trace["steps"], K)
    per_step = []
    for t in range(trace["steps"]):
        l64, l16 = (w.logits64_0, w.logits16_0) if t == 0 else _step_logits(w, ref.run_seq)
        per_step.append((ref.run_score.clone(), l64.cpu(), l16.cpu()))
        ref.step(trace["cand_score"][t], trace["cand_flat"][t])
    e_ref = max(ac._logit_err(l16, l64).max().item() for _, l64, l16 in per_step)
    worst, tight = 0.0, float("inf")
    for t, (running, l64, _) in enumerate(per_step):
        M = l64.shape[0]
        alive = running[:M] > bc.NEG
        s64 = torch.where(alive[:, None], running[:M, None].double() + torch.log_softmax(l64, -1), torch.tensor(float("-inf"), dtype=torch.float64))
        row_bound = 2.0 * e_ref * l64.abs().amax(-1)
        parents = (trace["cand_flat"][t].long() // VOCAB).clamp(0, M - 1)
        bound = row_bound[parents]
        worst = max(worst, bc.check_topk(trace["cand_score"][t], trace["cand_flat"][t], s64, bound, label=f"{label} step {t}"))
        tight = min(tight, bound.min().item())
    return ref, e_ref, worst, tight


@pytest.mark.parametrize("B,n_eos,lp", [(2, 1, 1.0), (4, 2, 0.6), (5, 1, 1.0), (4, 0, 1.0), (5, 0, 0.6)])
def test_trace_against_the_f64_decoder(world, B, n_eos, lp):
    """EOS ids: the last distinct tokens of the greedy continuation (late ones, so that the searches run for several steps and the K/V
    gather moves several rows); n_eos = 0: no EOS, all 8 steps run and the gather moves up to 7 rows."""
    w = world
    distinct = list(dict.fromkeys(w.greedy.tolist()))
    eos = tuple(distinct[-n_eos:]) if n_eos else None
    assert n_eos == 0 or len(eos) == n_eos
    toks, trace = w.eng.generate(w.prompt, w.images, w.coords, max_new_tokens=NEW, eos_token_id=eos, num_beams=B, length_penalty=lp, return_trace=True)
    ref, e_ref, worst, tight = _replay(w, trace, B, eos or (), lp, f"{w.name} B={B}")
    print(f"\n[beam search {w.name} B={B} K={trace['K']} greedy={w.greedy.tolist()} eos={eos} lp={lp}] steps {trace['steps']} (queued {trace['queued_steps']}), e_ref[logits] {e_ref:.2e}, "
          f"worst |score - f64| {worst:.2e}, smallest bound {tight:.2e}, result {toks.tolist()} score {trace['score']:.4f}")
    assert ref.done and ref.steps == trace["steps"] and trace["state"]["done"] == 1
    assert bc.views_snapshot(trace["state"]) == ref.snapshot(), "the engine's final state differs from BeamRef on the engine's own candidates"
    want, score, n = ref.result()
    assert toks.tolist() == want and trace["length"] == n and torch.tensor(trace["score"], dtype=torch.float32) == torch.tensor(score, dtype=torch.float32)
    assert toks.is_cuda and toks.dtype == torch.int64
    if not n_eos:
        assert trace["steps"] == NEW and toks.numel() == NEW


def test_result_does_not_depend_on_how_the_prompt_was_prefilled(world):
    w = world
    B, eos = 4, (int(w.greedy[4]),)
    kw = dict(max_new_tokens=NEW, eos_token_id=eos, num_beams=B, return_trace=True)
    full, tr_full = w.eng.generate(w.prompt, w.images, w.coords, **kw)
    again, tr_again = w.eng.generate(w.prompt, w.images, w.coords, **kw)
    assert torch.equal(full, again) and torch.equal(tr_full["cand_flat"], tr_again["cand_flat"])
    assert torch.equal(tr_full["cand_score"].view(torch.int32), tr_again["cand_score"].view(torch.int32)), "two identical calls must be bit-identical"
    keep = w.eng.ctx
    scene = w.eng.use(w.eng.new_context())
    try:
        P = w.eng.prefill_scene(w.prefix, w.images, w.coords)
        questions = [w.question, w.question[:9], torch.flip(w.question, [0])]
        before = w.eng.answer_group(questions, max_new_tokens=NEW)
        prefix_rows = [c[:P].clone() for c in scene.kv]
        cached, tr_cached = w.eng.answer(w.question, **kw)
        # a question of 23 rows runs through the prefill kernels the uncached pass used: the same K/V bits, so normally the same search
        if not torch.equal(cached, full):
            steps = min(tr_full["steps"], tr_cached["steps"])
            t = next(i for i in range(steps) if not torch.equal(tr_full["cand_flat"][i], tr_cached["cand_flat"][i]))
            _, e_ref, _, _ = _replay(w, tr_full, B, eos, 1.0, "uncached")
            ref = bc.BeamRef(B, VOCAB, NEW, eos, 1.0)
            for i in range(t):                             # the part both searches share
                ref.step(tr_full["cand_score"][i], tr_full["cand_flat"][i])
            l64 = (w.logits64_0 if t == 0 else _step_logits(w, ref.run_seq)[0]).cpu()
            s64 = (ref.run_score[: l64.shape[0], None].double() + torch.log_softmax(l64, -1)).reshape(-1)
            k = next(i for i in range(tr_full["K"]) if tr_full["cand_flat"][t][i] != tr_cached["cand_flat"][t][i])
            a, b = int(tr_full["cand_flat"][t][k]), int(tr_cached["cand_flat"][t][k])
            margin, bound = abs(s64[a] - s64[b]).item(), 2.0 * e_ref * l64.abs().max().item()
            print(f"\n[beam search {w.name}] cached and uncached searches part at step {t} rank {k}: f64 margin {margin:.3e}, bound {bound:.3e}")
            assert margin <= 2.0 * bound, (t, k, a, b, margin, bound)
        for a, b in zip(scene.kv, prefix_rows):
            assert torch.equal(a[:P], b), "a beam search disturbed the scene's prefix rows"
        after = w.eng.answer_group(questions, max_new_tokens=NEW)
        assert all(torch.equal(a, b) for a, b in zip(before, after)), "answer_group after a beam run differs from before it"
        assert w.eng.ctx is scene
    finally:
        w.eng.use(keep)


def test_surface(world):
    w = world
    eng = w.eng
    assert torch.equal(eng.generate(w.prompt, w.images, w.coords, max_new_tokens=NEW, num_beams=1).cpu(), w.greedy)
    with pytest.raises(V3DError):
        eng.generate(w.prompt, w.images, w.coords, max_new_tokens=4, num_beams=17)
    with pytest.raises(V3DError):
        eng.generate(w.prompt, w.images, w.coords, max_new_tokens=4, num_beams=16, eos_token_id=(1, 2, 3, 4))       # K = 5 * 16 > 64
    with pytest.raises(V3DError):
        eng.generate(w.prompt, w.images, w.coords, max_new_tokens=4, num_beams=2, stopping=lambda t: False)
    with pytest.raises(V3DError):
        eng.generate(w.prompt, w.images, w.coords, max_new_tokens=4, num_beams=0)
    # 16 beams, no EOS: every step runs, the result has max_new_tokens tokens
    wide = eng.generate(w.prompt, w.images, w.coords, max_new_tokens=5, num_beams=16)
    assert wide.shape == (5,) and int(wide.max()) < VOCAB


def test_overlay_generate_beam():
    from llava.model.language_model.llava_qwen import LlavaQwenConfig, LlavaQwenForCausalLM
    from v3d.engine import EngineConfig, LlmConfig, VitConfig, random_state_dict
    cfg = EngineConfig(vit=VitConfig(hidden=144, inter=272, layers=1, heads=2),
                       llm=LlmConfig(hidden=256, inter=384, layers=1, heads=2, kv_heads=1, vocab=320, max_pos=1024))
    sd = random_state_dict(cfg, torch.float32, "cpu", seed=9, std=0.05)
    hf = LlavaQwenConfig(vocab_size=320, hidden_size=256, intermediate_size=384, num_hidden_layers=1, num_attention_heads=2,
                         num_key_value_heads=1, max_position_embeddings=1024, rms_norm_eps=1e-6, rope_theta=1000000.0)
    hf.rope_theta, hf.world_position_embedding_type = 1000000.0, "avg-discrete-sin3d"
    model = LlavaQwenForCausalLM(hf, sd, dtype=torch.float16, device="cuda")
    g = torch.Generator().manual_seed(10)
    images = torch.randn(1, 2, 3, 384, 384, generator=g).half().cuda()
    vd = {"world_coords": ((torch.rand(1, 2, 384, 384, 3, generator=g) - 0.5) * 10).half().cuda(), "box_input": torch.Tensor([])}
    t = torch.randint(0, 300, (1, 16), generator=g)
    input_ids = torch.cat([t[:, :6], torch.tensor([[-200]]), t[:, 6:]], 1).cuda()
    greedy = model.generate(input_ids, images=images, modalities="video", do_sample=False, num_beams=1, max_new_tokens=6, use_cache=True, video_dict=vd)
    eos = int(greedy[0, 3])
    out = model.generate_beam(input_ids, images=images, modalities="video", video_dict=vd, num_beams=4, max_new_tokens=6, length_penalty=0.8, eos_token_id=eos)
    want = model.engine.generate(input_ids[0].cpu(), images[0], vd["world_coords"][0], max_new_tokens=6, eos_token_id=eos, num_beams=4, length_penalty=0.8)
    assert out.dim() == 2 and out.shape[0] == 1 and out.dtype == torch.int64 and torch.equal(out[0], want)
    assert torch.equal(model.generate_beam(input_ids, images=images, modalities="video", video_dict=vd, num_beams=1, max_new_tokens=6), greedy)
    with pytest.raises(NotImplementedError, match="generate_beam"):
        model.generate(input_ids, images=images, video_dict=vd, num_beams=4)
    with pytest.raises(TypeError):
        model.generate_beam(input_ids, images=images, video_dict=vd, num_beams=2, early_stopping=True)


def test_runner_num_beams(tmp_path):
    """eval_3d --task scan2cap --num_beams 2 on the synthetic scene files: the plain loop and --reuse-scenes write the same records."""
    import tiny_model_fixture as TM
    from test_gpu_eval_harness import _argv, _dataset
    from v3d import eval_3d as E3
    root = str(tmp_path)
    qs = _dataset(root)
    ckpt = TM.write_checkpoint(os.path.join(root, "llava_qwen_tiny"), TM.load())
    caps = []
    for i, q in enumerate(qs[:5]):
        c = dict(q, id=f"c{i}", box_input=None if i == 2 else [0.3 * i, -0.2 * i, 0.5, 1, 1, 1], annotations=[f"t{50 + i}"])
        c["conversations"] = [{"from": "human", "value": q["conversations"][0]["value"] + " t317 t9"}, q["conversations"][1]]
        caps.append(c)
    json.dump(caps, open(os.path.join(root, "caps.json"), "w"))
    assert E3.main(_argv(root, ckpt, "caps.json", "beam_plain.jsonl", "--task", "scan2cap", "--num_beams", "2")) == 0
    assert E3.main(_argv(root, ckpt, "caps.json", "beam_reuse.jsonl", "--task", "scan2cap", "--num_beams", "2", "--reuse-scenes")) == 0
    plain = [json.loads(l) for l in open(os.path.join(root, "out", "beam_plain.jsonl"))]
    reuse = [json.loads(l) for l in open(os.path.join(root, "out", "beam_reuse.jsonl"))]
    assert [r["sample_id"] for r in plain] == [c["id"] for c in caps] and plain[2]["pred_response"] == ""
    assert all(list(r) == ["dataset", "sample_id", "prompt", "pred_response", "gt_response", "model_id", "question_type", "scene"] for r in plain)
    assert plain == reuse
