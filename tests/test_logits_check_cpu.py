"""tests/logits_check.py, the logits processors' rule, checked on the CPU: the restatement against transformers' own
RepetitionPenaltyLogitsProcessor, NoRepeatNGramLogitsProcessor and MinNewTokensLengthLogitsProcessor (round16 of their f32 result, bit for
bit); the scope of the history and the order of application pinned end to end against transformers' generate on a tiny random Qwen2; and
the library's host twin against the restatement on the kernel's case list.  Every comparison is exact."""
import math

import pytest
import torch

import logits_check as lc
from v3d import ops
from v3d._native import V3DError

DTYPES = {"bf16": torch.bfloat16, "f16": torch.float16}


def _hf(scores32, ids, p, n, k, eos):
    """transformers' three processors in _get_logits_processor's order over f32 scores [M, V] and input_ids [M, L] (the generated tokens)"""
    from transformers.generation.logits_process import (MinNewTokensLengthLogitsProcessor, NoRepeatNGramLogitsProcessor,
                                                        RepetitionPenaltyLogitsProcessor)
    s = scores32.clone()
    if p != 1.0:
        s = RepetitionPenaltyLogitsProcessor(penalty=p)(ids, s)
    if n > 0:
        s = NoRepeatNGramLogitsProcessor(n)(ids, s)
    if k > 0:
        s = MinNewTokensLengthLogitsProcessor(0, k, list(eos), device="cpu")(ids, s)
    return s


@pytest.mark.parametrize("name", sorted(DTYPES))
def test_restatement_is_round16_of_transformers(name):
    dt = DTYPES[name]
    g = torch.Generator().manual_seed(5)
    M, V = 6, 500
    n_checked = 0
    for L in (0, 1, 2, 3, 5, 40, 300):
        x = (torch.randn(M, V, generator=g) * 4.0).to(dt)
        ids = torch.randint(0, 9, (M, L), generator=g) * 7 + 3            # nine ids: every n-gram size below finds repeats
        if L:
            x[0, ids[0, 0]] = 0.0
            x[1, ids[1, 0]] = -math.inf
            x[2, ids[2, 0]] = 6.5e4 if dt == torch.float16 else 3.0e38     # the division stays finite, a product would not
            x[3, ids[3, 0]] = -6.0e4 if dt == torch.float16 else -3.0e38   # f32 * 1.3 rounds to -inf in 16 bits
            x[4, ids[4, 0]] = 6.0e-8 if dt == torch.float16 else 1e-38     # the smallest magnitudes: subnormal results
        for p, n, k, eos in ((1.3, 0, 0, ()), (0.8, 0, 0, ()), (1.0, 1, 0, ()), (1.0, 2, 0, ()), (1.0, 3, 0, ()), (1.0, 0, 4, (3, 10)), (1.0, 0, 2, (499,)),
                             (1.3, 2, 4, (3, 17, 24)), (1.05, 3, 301, (10,))):
            want = _hf(x.float(), ids, p, n, k, eos).to(dt)
            got = lc.process_rows(x, ids.t().contiguous(), L, p, n, k, eos)
            assert torch.equal(lc.bits(got), lc.bits(want)), (name, L, p, n, k, eos)
            twin = ops.logits_process_rows_host(x.float(), dt, ids.t().contiguous() if L else None, L, p, n, k, eos)      # the library's arithmetic, directly
            assert torch.equal(lc.bits(twin), lc.bits(want.float())), ("host twin", name, L, p, n, k, eos)
            n_checked += int((lc.bits(got) != lc.bits(x)).sum())
    assert n_checked > 500, "the settings above changed almost nothing: the comparison shows little"


def test_generate_pins_history_scope_and_order():
    """transformers' generate(inputs_embeds=...) - what the reference's generate calls (llava_qwen.py:226) - starts its input_ids empty, so the
    processors see the generated tokens only, and it applies penalty, n-gram ban, min-new-tokens in that order: its tokens are those of the
    restated loop driven by the same model."""
    from transformers import Qwen2Config, Qwen2ForCausalLM
    torch.manual_seed(3)
    cfg = Qwen2Config(vocab_size=64, hidden_size=32, intermediate_size=48, num_hidden_layers=2, num_attention_heads=2, num_key_value_heads=1,
                      max_position_embeddings=128, tie_word_embeddings=False)
    model = Qwen2ForCausalLM(cfg).float().eval()
    NEW = 16
    # the prompt is made of tokens the generation would repeat: a processor that looked at the prompt would give other tokens
    prompt = torch.randint(0, 64, (1, 9), generator=torch.Generator().manual_seed(4))
    embeds = model.get_input_embeddings()(prompt).detach()

    def loop(settings):
        with torch.no_grad():
            out = model(inputs_embeds=embeds, use_cache=True)
            toks = []
            for _ in range(NEW):
                x = lc.process(out.logits[0, -1], toks, settings.get("p", 1.0), settings.get("n", 0), settings.get("k", 0), settings.get("eos", ()))
                tok = int((x == x.max()).nonzero()[0])
                # the library's twin on this step's logits at 16 bits and this history: the restatement's bits
                x16 = out.logits[0, -1].to(torch.bfloat16)
                hist = torch.tensor(toks, dtype=torch.int64) if toks else None
                twin = ops.logits_process_rows_host(x16.float()[None], torch.bfloat16, hist, len(toks), settings.get("p", 1.0), settings.get("n", 0),
                                                    settings.get("k", 0), settings.get("eos", ()))[0]
                want16 = lc.process(x16, toks, settings.get("p", 1.0), settings.get("n", 0), settings.get("k", 0), settings.get("eos", ()))
                assert torch.equal(lc.bits(twin), lc.bits(want16.float())), (settings, toks)
                toks.append(tok)
                if tok in settings.get("eos", ()):
                    break
                out = model(input_ids=torch.tensor([[tok]]), past_key_values=out.past_key_values, use_cache=True)
        return toks

    plain = loop({})
    eos = plain[2]                                                           # the plain run would stop after three tokens
    settings = dict(p=1.3, n=2, k=6, eos=(eos,))
    want = loop(settings)
    with torch.no_grad():
        got = model.generate(inputs_embeds=embeds, do_sample=False, repetition_penalty=1.3, no_repeat_ngram_size=2, min_new_tokens=6,
                             eos_token_id=eos, pad_token_id=0, max_new_tokens=NEW)[0].tolist()
    assert got == want, (got, want)
    assert len(want) >= 6 and want != plain[: len(want)], "the controls changed nothing on this model: the pin shows little"
    # had the prompt been part of the history, the tokens would differ
    with_prompt = []
    with torch.no_grad():
        out = model(inputs_embeds=embeds, use_cache=True)
        for _ in range(len(want)):
            x = lc.process(out.logits[0, -1], prompt[0].tolist() + with_prompt, 1.3, 2, 6 + prompt.shape[1], (eos,))
            with_prompt.append(int((x == x.max()).nonzero()[0]))
            out = model(input_ids=torch.tensor([[with_prompt[-1]]]), past_key_values=out.past_key_values, use_cache=True)
    assert with_prompt != want, "a history that includes the prompt gives the same tokens here: the scope is not pinned"
    lc.check_choice([torch.tensor(want)], torch.stack([_raw for _raw in _raw_logits(model, embeds, want)])[:, None], settings, what="restated loop")


def _raw_logits(model, embeds, toks):
    with torch.no_grad():
        out = model(inputs_embeds=embeds, use_cache=True)
        for tok in toks:
            yield out.logits[0, -1].clone()
            out = model(input_ids=torch.tensor([[tok]]), past_key_values=out.past_key_values, use_cache=True)


@pytest.mark.parametrize("name", sorted(DTYPES))
def test_host_twin_is_the_restatement_on_the_kernel_cases(name):
    dt = DTYPES[name]
    changed = 0
    for case in lc.kernel_cases(dt):
        want, count = lc.expected(case)
        x = case["logits"].float()
        ops.logits_process_rows_host(x, dt, case["history"], case["L"], case["p"], case["n"], case["k"], case["eos"], V=case["V"])
        assert torch.equal(lc.bits(x), lc.bits(want.float())), case["name"]
        assert torch.equal(x[:, case["V"]:], torch.full_like(x[:, case["V"]:], lc.SENTINEL)), case["name"]
        if lc.must_change(case):
            assert int(count[0]) > 0, f"{case['name']}: the restatement changes nothing in row 0"
        changed += int(count.sum())
    assert changed > 5000


def test_host_twin_penalises_a_repeated_id_once():
    case = lc.make_case("repeat", torch.bfloat16, 2, 1100, p=1.3)
    x = case["logits"].float()
    ops.logits_process_rows_host(x, torch.bfloat16, case["history"], 1100, 1.3, V=case["V"])
    once = (torch.tensor(3.0) / torch.tensor(1.3)).to(torch.bfloat16).float()
    assert float(x[0, lc.REPEAT_ID]) == float(once) and float(x[1, lc.REPEAT_ID]) == float(once)


def test_host_twin_refuses_bad_arguments():
    x = torch.zeros(2, 16)
    h = torch.zeros(4, 2, dtype=torch.int64)
    for kw in (dict(repetition_penalty=0.0), dict(repetition_penalty=-1.0), dict(repetition_penalty=float("nan")), dict(no_repeat_ngram_size=-1),
               dict(min_new_tokens=-1)):
        with pytest.raises(V3DError):
            ops.logits_process_rows_host(x, torch.float16, h, 4, **kw)
    with pytest.raises(V3DError):
        ops.logits_process_rows_host(x, torch.float16, h, 5)                  # more steps than the history holds
    with pytest.raises(V3DError, match="LOGITS_MAX_HISTORY"):
        ops.logits_process_rows_host(x, torch.float16, torch.zeros(ops.LOGITS_MAX_HISTORY + 1, 2, dtype=torch.int64), ops.LOGITS_MAX_HISTORY + 1)
    with pytest.raises(V3DError):
        ops.logits_process_rows_host(x, torch.float16, h.to(torch.int32), 4)
    ops.logits_process_rows_host(x, torch.float16, torch.zeros(ops.LOGITS_MAX_HISTORY, 2, dtype=torch.int64), ops.LOGITS_MAX_HISTORY, 1.5, 2)


def test_python_limits_are_the_headers():
    """ops.LOGITS_MAX_M / LOGITS_MAX_HISTORY restate csrc/logits_rule.h's constants: read from the header, and the built library refuses
    exactly one past each"""
    import os
    import re
    src = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "video-3d-llm_amd", "csrc", "logits_rule.h")).read()
    val = lambda name: int(re.search(r"constexpr int %s = (\d+);" % name, src).group(1))          # noqa: E731
    assert ops.LOGITS_MAX_M == val("LOGITS_MAX_M") and ops.LOGITS_MAX_HISTORY == val("LOGITS_MAX_HISTORY")
    M = ops.LOGITS_MAX_M
    ops.logits_process_rows_host(torch.zeros(M, 8), torch.float16, torch.zeros(2, M, dtype=torch.int64), 2, 1.5)
    with pytest.raises(V3DError):
        ops.logits_process_rows_host(torch.zeros(M + 1, 8), torch.float16, torch.zeros(2, M + 1, dtype=torch.int64), 2, 1.5)
