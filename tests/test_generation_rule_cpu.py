"""v3d.generation on the host: the rule's checks, its off table, fit() and the drivers' flag helpers.  No GPU, no native library."""
import argparse
import dataclasses
import math

import pytest

from v3d._native import V3DError
from v3d.generation import OFF, GenerationRule, add_arguments, processors_on, rule_from_flags, rule_of

R = GenerationRule
CONTROLS = (dict(do_sample=True), dict(repetition_penalty=1.2), dict(no_repeat_ngram_size=2), dict(min_new_tokens=2))


def test_the_default_rule_is_plain_greedy_decoding():
    r = R()
    assert (r.num_beams, r.length_penalty, r.return_trace) == (1, 1.0, False)
    assert (r.do_sample, r.temperature, r.top_k, r.top_p, r.seed) == (False, 1.0, 0, 1.0, 0)
    assert (r.repetition_penalty, r.no_repeat_ngram_size, r.min_new_tokens, r.return_logits) == (1.0, 0, 0, False)
    assert r.plain and r.processors == {} and r.check(None, 16, None) is r
    assert {f.name for f in dataclasses.fields(R)} == {"num_beams", "length_penalty", "return_trace", "do_sample", "temperature", "top_k", "top_p", "seed",
                                                       "repetition_penalty", "no_repeat_ngram_size", "min_new_tokens", "return_logits"}


@pytest.mark.parametrize("bad, field", [
    (dict(repetition_penalty=0.0), "repetition_penalty"), (dict(repetition_penalty=-1.0), "repetition_penalty"),
    (dict(repetition_penalty=float("nan")), "repetition_penalty"), (dict(repetition_penalty=float("inf")), "repetition_penalty"),
    (dict(repetition_penalty="x"), "repetition_penalty"), (dict(repetition_penalty=None), "repetition_penalty"),
    (dict(no_repeat_ngram_size=-1), "no_repeat_ngram_size"), (dict(no_repeat_ngram_size=1.5), "no_repeat_ngram_size"),
    (dict(no_repeat_ngram_size=True), "no_repeat_ngram_size"), (dict(min_new_tokens=-1), "min_new_tokens"), (dict(min_new_tokens=2.0), "min_new_tokens"),
    (dict(do_sample=True, temperature=0.0), "temperature"), (dict(do_sample=True, temperature=-0.5), "temperature"),
    (dict(do_sample=True, temperature=float("nan")), "temperature"), (dict(do_sample=True, temperature=float("inf")), "temperature"),
    (dict(do_sample=True, top_p=0.0), "top_p"), (dict(do_sample=True, top_p=1.5), "top_p"), (dict(do_sample=True, top_p=float("nan")), "top_p"),
    (dict(do_sample=True, top_k=-1), "top_k"), (dict(do_sample=True, top_k=2.5), "top_k"),
    (dict(num_beams=0), "num_beams"), (dict(num_beams=2.0), "num_beams"),
])
def test_values_out_of_range_are_refused_by_name(bad, field):
    with pytest.raises(V3DError, match=field):
        R(**bad)


def test_sampling_values_are_read_only_when_sampling():
    assert R(temperature=5.0, top_k=3, seed=1).plain
    assert R(do_sample=True, temperature=0.3, top_k=1, top_p=1e-6, seed=2 ** 64 + 5).do_sample


def test_call_dependent_refusals():
    with pytest.raises(V3DError, match="eos_token_id"):
        R(min_new_tokens=2).check(None, 8)
    with pytest.raises(V3DError, match="eos_token_id"):
        R(min_new_tokens=2).check((), 8)
    with pytest.raises(V3DError, match="max_new_tokens"):
        R(min_new_tokens=9).check(5, 8)
    assert R(min_new_tokens=8).check(5, 8).min_new_tokens == 8 and R(min_new_tokens=8).check([5, 7], None).min_new_tokens == 8
    with pytest.raises(V3DError, match="max_new_tokens"):                   # (flag parsing: the EOS ids are not known yet)
        R(min_new_tokens=9).check(max_new_tokens=8)
    assert R(min_new_tokens=3).check(max_new_tokens=8).min_new_tokens == 3
    with pytest.raises(V3DError, match="num_beams"):
        R(num_beams=2).check(5, 8, stopping=lambda toks: False)
    assert R().check(5, 8, stopping=lambda toks: False).plain and R(num_beams=2).check(5, 8).num_beams == 2
    assert R().check(None, -1).plain and R(no_repeat_ngram_size=2).check(None, 0).min_new_tokens == 0      # the length itself is the engine's to refuse


def test_beams_exclude_every_other_control():
    for kw in CONTROLS:
        with pytest.raises(V3DError, match="num_beams"):
            R(num_beams=2, **kw)
    with pytest.raises(V3DError, match="num_beams"):
        R(num_beams=2, return_logits=True)
    with pytest.raises(V3DError, match="return_trace"):
        R(return_trace=True)
    beams = R(num_beams=3, length_penalty=0.5, return_trace=True, repetition_penalty=1, no_repeat_ngram_size=0, min_new_tokens=0)
    assert beams.plain and beams.check(5, 4).processors == {}


def test_who_keeps_the_logits():
    with pytest.raises(V3DError, match="return_logits"):
        R(return_logits=True)
    with pytest.raises(V3DError, match="return_logits"):
        R(return_logits=True, repetition_penalty=1.0, no_repeat_ngram_size=0, min_new_tokens=0, temperature=0.7)
    for kw in CONTROLS:
        assert R(return_logits=True, **kw).return_logits and not R(return_logits=True, **kw).plain
    assert R(return_logits=True, do_sample=True, no_repeat_ngram_size=2).return_logits


def test_the_off_table():
    assert OFF == {"repetition_penalty": 1.0, "no_repeat_ngram_size": 0, "min_new_tokens": 0}
    assert R(repetition_penalty=1.0, no_repeat_ngram_size=0, min_new_tokens=0).processors == {} and R(repetition_penalty=1).plain
    assert R(repetition_penalty=1.3, min_new_tokens=4).processors == {"repetition_penalty": 1.3, "min_new_tokens": 4}
    assert not R(no_repeat_ngram_size=1).plain and not R(do_sample=True).plain and R(do_sample=True).processors == {}
    assert processors_on({}) == {} and processors_on(dict(repetition_penalty=None, no_repeat_ngram_size=0, min_new_tokens=3)) == {"min_new_tokens": 3}
    shipped = argparse.Namespace(repetition_penalty=1.05, no_repeat_ngram_size=2.0, min_new_tokens=None, temperature=0.6)
    on = processors_on(shipped)
    assert on == {"repetition_penalty": 1.05, "no_repeat_ngram_size": 2} and isinstance(on["no_repeat_ngram_size"], int)
    assert processors_on(None) == {}
    with pytest.raises(KeyError):
        processors_on(dict(top_k=3))


def test_fit_cuts_min_new_tokens_and_nothing_else():
    r = R(do_sample=True, temperature=0.7, top_k=5, top_p=0.9, seed=3, repetition_penalty=1.3, no_repeat_ngram_size=2, min_new_tokens=10, return_logits=True)
    assert r.fit(10) is r and r.fit(512) is r
    cut = r.fit(4)
    assert cut.min_new_tokens == 4 and dataclasses.replace(cut, min_new_tokens=10) == r
    assert r.fit(0).min_new_tokens == 0 and r.fit(-3).min_new_tokens == 0 and dataclasses.replace(r.fit(-3), min_new_tokens=10) == r
    assert R().fit(0) == R() and R(num_beams=2).fit(1).num_beams == 2


def test_rule_of_takes_a_rule_or_keywords():
    r = R(no_repeat_ngram_size=2)
    assert rule_of(r, {}) is r and rule_of(None, {}) == R() and rule_of(None, dict(no_repeat_ngram_size=2)) == r
    with pytest.raises(TypeError):
        rule_of(None, dict(no_repeat_ngram=2))
    with pytest.raises(TypeError):
        rule_of(r, dict(top_k=3))
    for beam_kw in (dict(num_beams=1), dict(length_penalty=0.5), dict(return_trace=False)):      # a call without beams does not know these keywords
        with pytest.raises(TypeError):
            rule_of(None, beam_kw, beams=False)
    assert rule_of(None, dict(no_repeat_ngram_size=2), beams=False) == r and rule_of(None, dict(num_beams=2)).num_beams == 2
    with pytest.raises(V3DError, match="repetition_penalty"):
        rule_of(None, dict(repetition_penalty=0))


def _parse(*flags):
    ap = argparse.ArgumentParser()
    ap.add_argument("--max-new-tokens", type=int, default=512)
    add_arguments(ap)
    return rule_from_flags(ap, ap.parse_args(list(flags)))


def test_flags_round_trip():
    assert _parse() == R()
    assert _parse("--temperature", "0", "--top_p", "0.9", "--seed", "5") == R()
    assert _parse("--repetition_penalty", "1.0", "--no_repeat_ngram_size", "0", "--min_new_tokens", "0") == R()
    assert _parse("--num_beams", "4", "--length_penalty", "0.8") == R(num_beams=4, length_penalty=0.8)
    assert _parse("--temperature", "0.7", "--top_p", "0.95", "--top_k", "60", "--seed", "3") == R(do_sample=True, temperature=0.7, top_p=0.95, top_k=60, seed=3)
    got = _parse("--max-new-tokens", "12", "--repetition_penalty", "1.3", "--no_repeat_ngram_size", "1", "--min_new_tokens", "4", "--temperature", "0.5")
    assert got == R(repetition_penalty=1.3, no_repeat_ngram_size=1, min_new_tokens=4, do_sample=True, temperature=0.5)
    assert math.isclose(got.processors["repetition_penalty"], 1.3) and _parse("--max-new-tokens", "12", "--min_new_tokens", "12").min_new_tokens == 12


@pytest.mark.parametrize("bad", [
    ("--no_repeat_ngram_size", "2", "--num_beams", "2"), ("--repetition_penalty", "0"), ("--max-new-tokens", "12", "--min_new_tokens", "99"),
    ("--temperature", "0.7", "--num_beams", "2"), ("--temperature", "-1"), ("--temperature", "0.7", "--top_p", "1.5"), ("--temperature", "0.7", "--top_k", "-1"),
    ("--repetition_penalty", "inf"), ("--no_repeat_ngram_size", "-1"), ("--min_new_tokens", "-1"), ("--num_beams", "0"),
    ("--min_new_tokens", "2", "--num_beams", "2"), ("--repetition_penalty", "1.2", "--num_beams", "3"),
    ("--top_p", "1.5"), ("--top_p", "0"), ("--top_k", "-1"), ("--temperature", "nan"), ("--temperature", "inf"),      # range-checked at temperature 0 too
])
def test_flags_the_rule_refuses_exit(bad, capsys):
    with pytest.raises(SystemExit):
        _parse(*bad)
    assert "error" in capsys.readouterr().err
