"""Sampling through the engine, the overlay model and the eval runners (do_sample): the degenerate forms equal greedy decoding token for
token; with return_logits every token of generate, answer and answer_group passes tests/sample_check.py's check_draws against the very
logits it was drawn from, at the step and on the stream the rule prescribes (what catches a step counter or a stream wired wrongly);
seeds reproduce; model.generate_sample returns generate's shape, honours torch.manual_seed and falls back to generation_config; the
refusals stay; eval_scanqa --temperature writes the same records with and without --reuse-scenes, and temperature 0 the bytes of a run
without the flags."""
import json
import os

import pytest
import torch

import sample_check as sc
from oracle import pipeline_oracle as PO
from v3d._native import V3DError

pytestmark = pytest.mark.gpu

VOCAB, NEW = 320, 8
SETTING = dict(temperature=0.8, top_k=40, top_p=0.95)


class _Box:
    pass


@pytest.fixture(scope="module", params=["bf16", "f16"])
def world(request):
    from v3d.engine import Engine, EngineConfig, LlmConfig, VitConfig, random_state_dict
    w = _Box()
    w.name, w.dt = request.param, {"bf16": torch.bfloat16, "f16": torch.float16}[request.param]
    cfg = EngineConfig(vit=VitConfig(hidden=144, inter=272, layers=2, heads=2),
                       llm=LlmConfig(hidden=256, inter=384, layers=2, heads=2, kv_heads=1, vocab=VOCAB, max_pos=1024))
    sd = random_state_dict(cfg, torch.float32, "cpu", seed=41, std=0.08)
    w.eng = Engine(cfg, sd, dtype=w.dt, device="cuda", max_frames=2)
    g = torch.Generator().manual_seed(42)
    w.images = torch.randn(2, 3, 384, 384, generator=g).cuda()
    w.coords = ((torch.rand(2, 384, 384, 3, generator=g) - 0.5) * 20).cuda()
    w.prefix = torch.cat([torch.randint(0, VOCAB, (14,), generator=g), torch.tensor([PO.IMAGE_TOKEN_INDEX])])
    w.questions = [torch.randint(0, VOCAB, (n,), generator=g) for n in (23, 9, 17, 5, 23, 12)]
    w.prompt = torch.cat([w.prefix, w.questions[0]])
    w.greedy = w.eng.generate(w.prompt, w.images, w.coords, max_new_tokens=NEW).cpu()
    yield w
    w.__dict__.clear()
    import gc
    gc.collect()
    torch.cuda.empty_cache()


def _args(seed, streams):
    return dict(T=SETTING["temperature"], top_k=SETTING["top_k"], top_p=SETTING["top_p"], seed=seed, streams=streams)


def test_degenerate_forms_are_greedy(world):
    w = world
    for kw in (dict(top_k=1), dict(top_p=1e-6), dict(top_k=1, temperature=0.3, seed=9, stream=4)):
        got = w.eng.generate(w.prompt, w.images, w.coords, max_new_tokens=NEW, do_sample=True, **kw)
        assert got.is_cuda and got.dtype == torch.int64 and torch.equal(got.cpu(), w.greedy), kw
    # do_sample=False runs the greedy code whatever the other arguments say
    assert torch.equal(w.eng.generate(w.prompt, w.images, w.coords, max_new_tokens=NEW, do_sample=False, temperature=5.0, top_k=3, seed=1).cpu(), w.greedy)


def test_every_token_is_the_rules_draw_from_its_own_logits(world):
    w = world
    eng = w.eng
    toks, logits = eng.generate(w.prompt, w.images, w.coords, max_new_tokens=NEW, do_sample=True, seed=123, stream=7, return_logits=True, **SETTING)
    assert toks.shape == (NEW,) and logits.shape == (NEW, 1, VOCAB) and logits.dtype == w.dt
    sc.check_draws(toks.cpu()[:, None], None, logits.cpu(), _args(123, [7]), what=f"{w.name} generate")
    again = eng.generate(w.prompt, w.images, w.coords, max_new_tokens=NEW, do_sample=True, seed=123, stream=7, **SETTING)
    assert torch.equal(again, toks), "the same seed and stream must give the same tokens"
    others = [eng.generate(w.prompt, w.images, w.coords, max_new_tokens=NEW, do_sample=True, seed=s, stream=t, **SETTING) for s, t in ((124, 7), (123, 8))]
    assert not all(torch.equal(o, toks) for o in others), "neither another seed nor another stream changed a token"
    keep = eng.ctx
    scene = eng.use(eng.new_context())
    try:
        eng.prefill_scene(w.prefix, w.images, w.coords)
        one, l1 = eng.answer(w.questions[1], max_new_tokens=NEW, do_sample=True, seed=5, stream=3, return_logits=True, **SETTING)
        assert one.shape == (NEW,) and l1.shape == (NEW, 1, VOCAB)
        sc.check_draws(one.cpu()[:, None], None, l1.cpu(), _args(5, [3]), what=f"{w.name} answer")
        streams = list(range(10, 16))
        answers, lg = eng.answer_group(w.questions, max_new_tokens=NEW, do_sample=True, seed=5, streams=streams, return_logits=True, **SETTING)
        assert len(answers) == 6 and all(a.shape == (NEW,) for a in answers) and lg.shape == (NEW, 6, VOCAB)
        sc.check_draws(torch.stack([a.cpu() for a in answers], 1), None, lg.cpu(), _args(5, streams), what=f"{w.name} answer_group")
        twice = eng.answer_group(w.questions, max_new_tokens=NEW, do_sample=True, seed=5, streams=streams, **SETTING)
        assert all(torch.equal(a, b) for a, b in zip(answers, twice))
        default = eng.answer_group(w.questions[:3], max_new_tokens=NEW, do_sample=True, seed=5, return_logits=True, **SETTING)
        sc.check_draws(torch.stack([a.cpu() for a in default[0]], 1), None, default[1].cpu(), _args(5, [0, 1, 2]), what=f"{w.name} answer_group, default streams")
        assert eng.ctx is scene
    finally:
        eng.use(keep)
    samples = [(torch.cat([w.prefix, q]), w.images, w.coords) for q in w.questions[:3]]
    grp, lg = eng.generate_group(samples, max_new_tokens=NEW, do_sample=True, seed=77, streams=[4, 2, 9], return_logits=True, **SETTING)
    sc.check_draws(torch.stack([a.cpu() for a in grp], 1), None, lg.cpu(), _args(77, [4, 2, 9]), what=f"{w.name} generate_group")


def test_refusals(world):
    w = world
    kw = dict(max_new_tokens=4, do_sample=True)
    with pytest.raises(V3DError, match="num_beams"):
        w.eng.generate(w.prompt, w.images, w.coords, num_beams=2, **kw)
    for bad in (dict(temperature=0.0), dict(temperature=float("nan")), dict(top_p=0.0), dict(top_p=1.5), dict(top_k=-1), dict(stream=-1)):
        with pytest.raises(V3DError):
            w.eng.generate(w.prompt, w.images, w.coords, **kw, **bad)
    with pytest.raises(V3DError):
        w.eng.generate(w.prompt, w.images, w.coords, max_new_tokens=4, return_logits=True)
    with pytest.raises(V3DError):
        w.eng.generate_group([(w.prompt, w.images, w.coords)] * 2, streams=[1], **kw)


def test_overlay_generate_sample():
    from llava.model.language_model.llava_qwen import LlavaQwenConfig, LlavaQwenForCausalLM
    from v3d.engine import EngineConfig, LlmConfig, VitConfig, random_state_dict
    import types
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
    kw = dict(images=images, modalities="video", video_dict=vd, max_new_tokens=6, use_cache=True)
    out = model.generate_sample(input_ids, temperature=0.7, top_p=0.9, top_k=30, seed=11, **kw)
    want = model.engine.generate(input_ids[0].cpu(), images[0], vd["world_coords"][0], max_new_tokens=6, do_sample=True, temperature=0.7, top_p=0.9,
                                 top_k=30, seed=11)
    assert out.dim() == 2 and out.shape == (1, 6) and out.dtype == torch.int64 and torch.equal(out[0], want)
    # seed=None: one 63-bit seed from torch's default CPU generator
    torch.manual_seed(1234)
    a = model.generate_sample(input_ids, temperature=0.7, top_p=0.9, **kw)
    torch.manual_seed(1234)
    seed = int(torch.randint(0, 2 ** 63 - 1, (1,), dtype=torch.int64).item())
    torch.manual_seed(1234)
    b = model.generate_sample(input_ids, temperature=0.7, top_p=0.9, **kw)
    assert torch.equal(a, b) and torch.equal(a, model.generate_sample(input_ids, temperature=0.7, top_p=0.9, seed=seed, **kw))
    drawn = {tuple(model.generate_sample(input_ids, temperature=0.7, top_p=0.9, **kw)[0].tolist()) for _ in range(4)}
    assert len(drawn) > 1, "four runs on the advancing generator drew the same six tokens"
    # None falls back to generation_config
    model.generation_config = types.SimpleNamespace(temperature=0.6, top_k=20, top_p=0.8, do_sample=True)
    assert torch.equal(model.generate_sample(input_ids, seed=3, **kw), model.generate_sample(input_ids, temperature=0.6, top_k=20, top_p=0.8, seed=3, **kw))
    model.generation_config = types.SimpleNamespace(temperature=None)
    assert torch.equal(model.generate_sample(input_ids, seed=3, **kw), model.generate_sample(input_ids, temperature=1.0, top_k=0, top_p=1.0, seed=3, **kw))
    greedy = model.generate(input_ids, do_sample=False, num_beams=1, **kw)
    assert torch.equal(model.generate_sample(input_ids, top_k=1, seed=3, **kw), greedy)
    with pytest.raises(NotImplementedError, match="generate_beam") as e:
        model.generate(input_ids, images=images, video_dict=vd, do_sample=True, temperature=0.7)
    assert "generate_sample" in str(e.value)
    with pytest.raises(NotImplementedError):
        model.generate_sample(input_ids, num_beams=2, **kw)
    with pytest.raises(TypeError):
        model.generate_sample(input_ids, repetition_penalty=1.1, **kw)


def test_runner_temperature(tmp_path):
    """eval_scanqa --temperature 0.7 --seed 3 on the synthetic scene files: the plain loop and --reuse-scenes write the same records (each
    question draws from the stream of its index in the question file; asserted outright, which asks more than the margin rule would), another
    seed writes others, and temperature 0 writes the bytes of a run without the sampling flags."""
    import tiny_model_fixture as TM
    from test_gpu_eval_harness import _argv, _dataset
    from v3d import eval_scanqa as E
    root = str(tmp_path)
    qs = _dataset(root)
    ckpt = TM.write_checkpoint(os.path.join(root, "llava_qwen_tiny"), TM.load())
    draw = ("--temperature", "0.7", "--top_p", "0.95", "--top_k", "60", "--seed", "3")
    assert E.main(_argv(root, ckpt, "questions.json", "s_plain.jsonl", *draw)) == 0
    assert E.main(_argv(root, ckpt, "questions.json", "s_reuse.jsonl", "--reuse-scenes", *draw)) == 0
    assert E.main(_argv(root, ckpt, "questions.json", "s_other.jsonl", "--temperature", "0.7", "--top_p", "0.95", "--top_k", "60", "--seed", "4")) == 0
    read = lambda name: [json.loads(l) for l in open(os.path.join(root, "out", name))]       # noqa: E731
    plain, reuse, other = read("s_plain.jsonl"), read("s_reuse.jsonl"), read("s_other.jsonl")
    assert [r["sample_id"] for r in plain] == [q["id"] for q in qs]
    assert plain == reuse, [(a["pred_response"], b["pred_response"]) for a, b in zip(plain, reuse)]
    assert plain != other
    assert E.main(_argv(root, ckpt, "questions.json", "g_flags.jsonl", "--no-pipeline", "--temperature", "0", "--top_p", "0.9", "--seed", "5")) == 0
    assert E.main(_argv(root, ckpt, "questions.json", "g_plain.jsonl", "--no-pipeline")) == 0
    assert open(os.path.join(root, "out", "g_flags.jsonl"), "rb").read() == open(os.path.join(root, "out", "g_plain.jsonl"), "rb").read()
    with pytest.raises(SystemExit):
        E.main(_argv(root, ckpt, "questions.json", "never.jsonl", "--temperature", "0.7", "--num_beams", "2"))
    assert not os.path.exists(os.path.join(root, "out", "never.jsonl"))
