"""The logits processors through the engine, the overlay model and the eval runners: with return_logits every token of generate, answer and
answer_group is the first maximum of tests/logits_check.py's processed row, replayed from the RAW logits the call returns, for each control
and for all three; no_repeat_ngram_size = 1 gives distinct tokens and = 2 no repeated bigram; min_new_tokens holds an early EOS back;
sampled tokens pass sample_check.check_draws on the processed logits; neutral values give today's tokens; a question's answer in
answer_group does not depend on its companions; beams and bad values are refused by name; model.generate / generate_sample honour
generation_config, and beams never read it; eval_scanqa writes the same records with and without --reuse-scenes under the flags, neutral
flags write the bytes of a run without them, and a checkpoint that ships processors in generation_config.json changes no runner record."""
import json
import os
import types

import pytest
import torch

import logits_check as lc
import sample_check as sc
from oracle import pipeline_oracle as PO
from v3d._native import V3DError
from v3d.generation import GenerationRule

pytestmark = pytest.mark.gpu

VOCAB, NEW, SEED = 320, 24, 41
SAMPLING = dict(temperature=0.8, top_k=40, top_p=0.95)


class _Box:
    pass


@pytest.fixture(scope="module", params=["bf16", "f16"])
def world(request):
    from v3d.engine import Engine, EngineConfig, LlmConfig, VitConfig, random_state_dict
    w = _Box()
    w.name, w.dt = request.param, {"bf16": torch.bfloat16, "f16": torch.float16}[request.param]
    cfg = EngineConfig(vit=VitConfig(hidden=144, inter=272, layers=2, heads=2),
                       llm=LlmConfig(hidden=256, inter=384, layers=2, heads=2, kv_heads=1, vocab=VOCAB, max_pos=1024))
    sd = random_state_dict(cfg, torch.float32, "cpu", seed=SEED, std=0.08)
    w.eng = Engine(cfg, sd, dtype=w.dt, device="cuda", max_frames=2)
    g = torch.Generator().manual_seed(42)
    w.images = torch.randn(2, 3, 384, 384, generator=g).cuda()
    w.coords = ((torch.rand(2, 384, 384, 3, generator=g) - 0.5) * 20).cuda()
    w.prefix = torch.cat([torch.randint(0, VOCAB, (14,), generator=g), torch.tensor([PO.IMAGE_TOKEN_INDEX])])
    w.questions = [torch.randint(0, VOCAB, (n,), generator=g) for n in (23, 9, 17, 5, 23, 12)]
    w.prompt = torch.cat([w.prefix, w.questions[0]])
    w.greedy = w.eng.generate(w.prompt, w.images, w.coords, max_new_tokens=NEW).cpu()
    w.eos = int(w.greedy[3])                                 # an id the plain run emits within its first four tokens
    yield w
    w.__dict__.clear()
    import gc
    gc.collect()
    torch.cuda.empty_cache()


def _kw(settings):
    return dict(repetition_penalty=settings.get("p", 1.0), no_repeat_ngram_size=settings.get("n", 0), min_new_tokens=settings.get("k", 0))


def _settings(w):
    return [dict(p=1.3), dict(n=2), dict(n=1), dict(k=10, eos=(w.eos,)), dict(p=1.3, n=2, k=10, eos=(w.eos,)), dict(p=0.8, n=3, k=24, eos=(w.eos, 7, 300))]


def _bigrams(t):
    return list(zip(t, t[1:]))


def test_fixture_greedy_run_repeats_a_token_and_a_bigram(world):
    t = world.greedy.tolist()
    assert len(t) == NEW
    assert len(set(t)) < len(t) and len(set(_bigrams(t))) < len(_bigrams(t)), \
        f"the FIXTURE is at fault, not the engine: the plain greedy run of seed {SEED} repeats no token or no bigram in {NEW} tokens ({t}); pick another SEED"


def test_every_choice_is_the_first_maximum_of_its_processed_row(world):
    w, eng = world, world.eng
    keep = eng.ctx
    for settings in _settings(w):
        eos = settings.get("eos")
        what = f"{w.name} {settings}"
        toks, raw = eng.generate(w.prompt, w.images, w.coords, max_new_tokens=NEW, eos_token_id=eos, return_logits=True, **_kw(settings))
        assert raw.shape == (toks.numel(), 1, VOCAB) and raw.dtype == w.dt and bool(torch.isfinite(raw.float()).all()), "the returned logits are the raw ones"
        assert lc.check_choice([toks.cpu()], raw, settings, what=what + " generate") == toks.numel()
        again = eng.generate(w.prompt, w.images, w.coords, max_new_tokens=NEW, eos_token_id=eos, **_kw(settings))
        assert torch.equal(again, toks)
        scene = eng.use(eng.new_context())
        try:
            eng.prefill_scene(w.prefix, w.images, w.coords)
            one, r1 = eng.answer(w.questions[1], max_new_tokens=NEW, eos_token_id=eos, return_logits=True, **_kw(settings))
            lc.check_choice([one.cpu()], r1, settings, what=what + " answer")
            answers, rg = eng.answer_group(w.questions, max_new_tokens=NEW, eos_token_id=eos, return_logits=True, **_kw(settings))
            assert len(answers) == 6 and rg.shape[1:] == (6, VOCAB) and bool(torch.isfinite(rg.float()).all())
            lc.check_choice([a.cpu() for a in answers], rg, settings, what=what + " answer_group")
            # a question's answer does not depend on the rows it is batched with (tests/test_gpu_scene_reuse.py's form of "answer_group equals
            # answering alone"): the same six questions in other row positions give the same answers, exactly - a row's history is its own
            # column of the token buffer.  Token equality with answer() / a group of one is NOT asserted: their question rows and one-row decode
            # linears sum in another order, the raw logits differ in the last bits (measured here, bf16, n = 2, question 2, step 17: the
            # processed top-2 is 3.109375 / 3.078125 in the batch and 3.078125 / 3.078125 alone), and once a ban leaves low-ranked tokens on
            # top such a near-tie turns; those runs are checked against their OWN logits instead.
            for order in (list(reversed(range(6))), [3, 4, 5, 0, 1, 2]):
                moved = eng.answer_group([w.questions[i] for i in order], max_new_tokens=NEW, eos_token_id=eos, **_kw(settings))
                for pos, i in enumerate(order):
                    assert torch.equal(moved[pos], answers[i]), (what, order, i, moved[pos].tolist(), answers[i].tolist())
            alone, ra = eng.answer_group([w.questions[2]], max_new_tokens=NEW, eos_token_id=eos, return_logits=True, **_kw(settings))
            lc.check_choice([alone[0].cpu()], ra, settings, what=what + " answer_group of one")
            for q in w.questions[2:4]:
                t, r = eng.answer(q, max_new_tokens=NEW, eos_token_id=eos, return_logits=True, **_kw(settings))
                lc.check_choice([t.cpu()], r, settings, what=what + " answer")
            assert eng.ctx is scene
        finally:
            eng.use(keep)
    samples = [(torch.cat([w.prefix, q]), w.images, w.coords) for q in w.questions[:3]]
    settings = dict(p=1.3, n=2)
    grp, rg = eng.generate_group(samples, max_new_tokens=NEW, return_logits=True, **_kw(settings))
    lc.check_choice([a.cpu() for a in grp], rg, settings, what=f"{w.name} generate_group")


def test_ngram_bans_and_min_new_tokens_show_in_the_tokens(world):
    w, eng = world, world.eng
    t1 = eng.generate(w.prompt, w.images, w.coords, max_new_tokens=NEW, no_repeat_ngram_size=1).tolist()
    assert len(t1) == NEW and len(set(t1)) == NEW, t1
    t2 = eng.generate(w.prompt, w.images, w.coords, max_new_tokens=NEW, no_repeat_ngram_size=2).tolist()
    assert len(set(_bigrams(t2))) == len(_bigrams(t2)) and t2 != w.greedy.tolist(), t2
    keep = eng.ctx
    eng.use(eng.new_context())
    try:
        eng.prefill_scene(w.prefix, w.images, w.coords)
        for n in (1, 2):
            for a in eng.answer_group(w.questions, max_new_tokens=NEW, no_repeat_ngram_size=n):
                a = a.tolist()
                units = a if n == 1 else _bigrams(a)
                assert len(set(units)) == len(units), (n, a)
    finally:
        eng.use(keep)
    plain = eng.generate(w.prompt, w.images, w.coords, max_new_tokens=NEW, eos_token_id=w.eos).tolist()
    assert len(plain) <= 4 and plain[-1] == w.eos
    held = eng.generate(w.prompt, w.images, w.coords, max_new_tokens=NEW, eos_token_id=w.eos, min_new_tokens=10).tolist()
    assert len(held) >= 10 and w.eos not in held[:10] and held[:len(plain) - 1] == plain[:-1], (plain, held)


def test_sampling_draws_from_the_processed_logits(world):
    w, eng = world, world.eng
    settings = dict(p=1.3, n=2, k=10, eos=(w.eos,))
    toks, raw = eng.generate(w.prompt, w.images, w.coords, max_new_tokens=NEW, eos_token_id=w.eos, do_sample=True, seed=123, stream=7, return_logits=True,
                             **SAMPLING, **_kw(settings))
    assert toks.numel() >= 10 and raw.shape == (toks.numel(), 1, VOCAB) and bool(torch.isfinite(raw.float()).all())
    done = lc.processed_logits([toks.cpu()], raw.cpu(), settings)
    args = dict(T=SAMPLING["temperature"], top_k=SAMPLING["top_k"], top_p=SAMPLING["top_p"], seed=123, streams=[7])
    sc.check_draws(toks.cpu()[:, None], None, done, args, what=f"{w.name} generate, sampled under the processors")
    assert len(set(_bigrams(toks.tolist()))) == len(_bigrams(toks.tolist()))
    keep = eng.ctx
    eng.use(eng.new_context())
    try:
        eng.prefill_scene(w.prefix, w.images, w.coords)
        settings = dict(p=1.3, n=2)
        streams = list(range(10, 16))
        answers, rg = eng.answer_group(w.questions, max_new_tokens=NEW, do_sample=True, seed=5, streams=streams, return_logits=True, **SAMPLING, **_kw(settings))
        done = lc.processed_logits([a.cpu() for a in answers], rg.cpu(), settings)
        sc.check_draws(torch.stack([a.cpu() for a in answers], 1), None, done, dict(args, seed=5, streams=streams), what=f"{w.name} answer_group, sampled")
    finally:
        eng.use(keep)


def test_neutral_values_give_todays_tokens(world):
    w, eng = world, world.eng
    got = eng.generate(w.prompt, w.images, w.coords, max_new_tokens=NEW, repetition_penalty=1.0, no_repeat_ngram_size=0, min_new_tokens=0)
    assert torch.equal(got.cpu(), w.greedy)
    off = dict(repetition_penalty=1, no_repeat_ngram_size=0, min_new_tokens=0)
    assert eng._choice(GenerationRule(**dict(off, repetition_penalty=1.0)), None) is None and eng._choice(GenerationRule(num_beams=3, **off), 5, 4) is None
    with pytest.raises(V3DError):                          # nothing to return the logits of: plain greedy decoding keeps no copy
        eng.generate(w.prompt, w.images, w.coords, max_new_tokens=4, return_logits=True)


def test_refusals(world):
    w, eng = world, world.eng
    call = lambda **kw: eng.generate(w.prompt, w.images, w.coords, max_new_tokens=8, **kw)          # noqa: E731
    for kw in (dict(repetition_penalty=1.2), dict(no_repeat_ngram_size=2), dict(min_new_tokens=2, eos_token_id=5)):
        with pytest.raises(V3DError, match="num_beams"):
            call(num_beams=2, **kw)
    for bad, field in ((dict(repetition_penalty=0.0), "repetition_penalty"), (dict(repetition_penalty=-1.0), "repetition_penalty"),
                       (dict(repetition_penalty=float("nan")), "repetition_penalty"), (dict(repetition_penalty=float("inf")), "repetition_penalty"),
                       (dict(no_repeat_ngram_size=-1), "no_repeat_ngram_size"), (dict(no_repeat_ngram_size=1.5), "no_repeat_ngram_size"),
                       (dict(min_new_tokens=-1, eos_token_id=5), "min_new_tokens"), (dict(min_new_tokens=9, eos_token_id=5), "max_new_tokens"),
                       (dict(min_new_tokens=2), "eos_token_id")):
        with pytest.raises(V3DError, match=field):
            call(**bad)
    keep = eng.ctx
    eng.use(eng.new_context())
    try:
        eng.prefill_scene(w.prefix, w.images, w.coords)
        with pytest.raises(V3DError, match="num_beams"):
            eng.answer(w.questions[0], max_new_tokens=8, num_beams=2, no_repeat_ngram_size=2)
        with pytest.raises(V3DError, match="repetition_penalty"):
            eng.answer_group(w.questions, max_new_tokens=8, repetition_penalty=0)
    finally:
        eng.use(keep)


def test_overlay_generate_honours_generation_config():
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
    kw = dict(images=images, modalities="video", video_dict=vd, max_new_tokens=12, use_cache=True)
    eng_args = (input_ids[0].cpu(), images[0], vd["world_coords"][0])
    plain = model.generate(input_ids, do_sample=False, num_beams=1, **kw)
    want = model.engine.generate(*eng_args, max_new_tokens=12, no_repeat_ngram_size=1, repetition_penalty=1.3)
    assert len(set(want.tolist())) == 12
    model.generation_config = types.SimpleNamespace(no_repeat_ngram_size=1, repetition_penalty=1.3, min_new_tokens=None)
    out = model.generate(input_ids, do_sample=False, num_beams=1, **kw)
    assert out.dim() == 2 and out.shape == (1, 12) and out.dtype == torch.int64 and torch.equal(out[0], want) and not torch.equal(out, plain)
    assert torch.equal(model.generate(input_ids, processors={}, **kw), plain), "processors given outright override generation_config"
    drawn = model.generate_sample(input_ids, temperature=0.7, top_p=0.9, seed=11, **kw)
    assert drawn.shape == (1, 12) and len(set(drawn[0].tolist())) == 12
    assert torch.equal(drawn[0], model.engine.generate(*eng_args, max_new_tokens=12, do_sample=True, temperature=0.7, top_p=0.9, seed=11, no_repeat_ngram_size=1,
                                                       repetition_penalty=1.3))
    # beams never read generation_config's processors (a checkpoint that ships them searches as it always has); given outright they are refused
    beam = model.generate_beam(input_ids, num_beams=2, **kw)
    with pytest.raises(NotImplementedError, match="beams"):
        model.generate_beam(input_ids, num_beams=2, processors=dict(no_repeat_ngram_size=2), **kw)
    assert torch.equal(model.generate_beam(input_ids, num_beams=2, processors={}, **kw), beam)
    assert torch.equal(model.generate_beam(input_ids, num_beams=1, **kw), out), "num_beams=1 is generate()"
    model.generation_config = None
    assert torch.equal(model.generate_beam(input_ids, num_beams=2, **kw), beam)
    assert torch.equal(model.generate(input_ids, **kw), plain)
    assert torch.equal(model.generate(input_ids, processors=dict(no_repeat_ngram_size=1, repetition_penalty=1.3), **kw)[0], want)
    with pytest.raises(TypeError, match="generation_config"):
        model.generate(input_ids, no_repeat_ngram_size=2, **kw)


def test_runner_flags(tmp_path):
    """eval_scanqa --repetition_penalty 1.3 --no_repeat_ngram_size 1 --min_new_tokens 4 on the synthetic scene files: the one-question loop and
    --reuse-scenes write the same records (a row's history is its own tokens, whatever it is batched with), the pipelined --reuse-scenes run
    writes them too, no answer repeats a word on any path (the cross-scene pipeline included), and neutral flags write the bytes of a run without the flags."""
    import tiny_model_fixture as TM
    from test_gpu_eval_harness import _argv, _dataset
    from v3d import eval_scanqa as E
    root = str(tmp_path)
    qs = _dataset(root)
    ckpt = TM.write_checkpoint(os.path.join(root, "llava_qwen_tiny"), TM.load())
    flags = ("--max-new-tokens", "12", "--repetition_penalty", "1.3", "--no_repeat_ngram_size", "1", "--min_new_tokens", "4")
    assert E.main(_argv(root, ckpt, "questions.json", "p_plain.jsonl", "--no-pipeline", *flags)) == 0
    assert E.main(_argv(root, ckpt, "questions.json", "p_reuse.jsonl", "--no-pipeline", "--reuse-scenes", *flags)) == 0
    assert E.main(_argv(root, ckpt, "questions.json", "p_reuse_pipe.jsonl", "--reuse-scenes", *flags)) == 0
    assert E.main(_argv(root, ckpt, "questions.json", "p_pipe.jsonl", *flags)) == 0
    assert E.main(_argv(root, ckpt, "questions.json", "p_pipe_one.jsonl", "--max-new-tokens", "12", "--no_repeat_ngram_size", "1")) == 0      # one control alone
    assert E.main(_argv(root, ckpt, "questions.json", "g_long.jsonl", "--no-pipeline", "--max-new-tokens", "12")) == 0
    read = lambda name: [json.loads(l) for l in open(os.path.join(root, "out", name))]       # noqa: E731
    plain, reuse, reuse_pipe, pipe, unflagged = read("p_plain.jsonl"), read("p_reuse.jsonl"), read("p_reuse_pipe.jsonl"), read("p_pipe.jsonl"), read("g_long.jsonl")
    assert [r["sample_id"] for r in plain] == [q["id"] for q in qs]
    assert plain == reuse, [(a["pred_response"], b["pred_response"]) for a, b in zip(plain, reuse)]
    assert reuse_pipe == reuse
    assert plain != unflagged
    for records in (plain, reuse, reuse_pipe, pipe, read("p_pipe_one.jsonl")):
        for r in records:
            words = r["pred_response"].split()
            assert len(words) == len(set(words)), r["pred_response"]
    assert E.main(_argv(root, ckpt, "questions.json", "g_flags.jsonl", "--no-pipeline", "--repetition_penalty", "1.0", "--no_repeat_ngram_size", "0",
                        "--min_new_tokens", "0")) == 0
    assert E.main(_argv(root, ckpt, "questions.json", "g_plain.jsonl", "--no-pipeline")) == 0
    assert open(os.path.join(root, "out", "g_flags.jsonl"), "rb").read() == open(os.path.join(root, "out", "g_plain.jsonl"), "rb").read()
    # a checkpoint whose generation_config.json ships a processor: the runners pass their flags outright, so without the flags - beams,
    # the plain loop and --reuse-scenes alike - the records are those of the checkpoint without the file
    assert E.main(_argv(root, ckpt, "questions.json", "b_plain.jsonl", "--num_beams", "2")) == 0
    assert E.main(_argv(root, ckpt, "questions.json", "b_plain_reuse.jsonl", "--num_beams", "2", "--reuse-scenes")) == 0
    with open(os.path.join(ckpt, "generation_config.json"), "w") as f:
        json.dump({"repetition_penalty": 1.05, "no_repeat_ngram_size": 2}, f)
    assert E.main(_argv(root, ckpt, "questions.json", "b_shipped.jsonl", "--num_beams", "2")) == 0
    assert E.main(_argv(root, ckpt, "questions.json", "b_shipped_reuse.jsonl", "--num_beams", "2", "--reuse-scenes")) == 0
    assert E.main(_argv(root, ckpt, "questions.json", "g_shipped.jsonl", "--no-pipeline")) == 0
    raw = lambda name: open(os.path.join(root, "out", name), "rb").read()       # noqa: E731
    assert raw("b_shipped.jsonl") == raw("b_plain.jsonl") and raw("g_shipped.jsonl") == raw("g_plain.jsonl")
    assert raw("b_shipped_reuse.jsonl") == raw("b_plain_reuse.jsonl") and len(read("b_shipped.jsonl")) == len(qs)
    for bad in (("--no_repeat_ngram_size", "2", "--num_beams", "2"), ("--repetition_penalty", "0"), ("--min_new_tokens", "99")):
        with pytest.raises(SystemExit):
            E.main(_argv(root, ckpt, "questions.json", "never.jsonl", *bad))
    assert not os.path.exists(os.path.join(root, "out", "never.jsonl"))
