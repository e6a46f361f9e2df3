"""The generation controls, stated once: a GenerationRule is what a caller asks of one generation call, checked in one place and carried
whole from the drivers' flags to the engine's token loops.  Host code only: Engine._choice turns a rule into device state.
A new control is a field here with its check, its device state in Engine._choice / TokenChoice, and its flag in add_arguments."""
import dataclasses
import math

from ._native import V3DError

OFF = {"repetition_penalty": 1.0, "no_repeat_ngram_size": 0, "min_new_tokens": 0}          # the processor values that mean "off"
UNKNOWN = object()          # check(eos_token_id=UNKNOWN): the EOS ids are not known yet (flag parsing, before the model is loaded)


def eos_ids(eos_token_id):
    """eos_token_id (None, an int or a collection of ints) -> tuple of ints"""
    ids = () if eos_token_id is None else (eos_token_id,) if isinstance(eos_token_id, int) else eos_token_id
    return tuple(int(e) for e in ids)


def processors_on(src):
    """The processor controls that are on in `src`: a dict given outright (its values as they are), or an object with such attributes
    (a generation_config: values cast as transformers reads them); a missing or None entry is off."""
    if isinstance(src, dict):
        return {k: v for k, v in src.items() if v is not None and v != OFF[k]}
    return {k: type(off)(v) for k, off in OFF.items() for v in (getattr(src, k, None),) if v is not None and v != off}


@dataclasses.dataclass(frozen=True)
class GenerationRule:
    """How the tokens of one generation call are chosen; GenerationRule() is plain greedy decoding.  A rule that exists is in range and
    free of contradictions (V3DError otherwise); check() adds what only the call knows.  DESIGN section 2 states what each computes.
    num_beams > 1: beam search (Engine.beam_search) with length_penalty and, with return_trace, its trace.  Excludes all that follows.
    do_sample: every token is drawn on the device from softmax(logits / temperature) after top_k and top_p, seeded by `seed` and the
    row's stream id (which belongs to the row, not to the rule).
    repetition_penalty / no_repeat_ngram_size / min_new_tokens: the logits processors, applied on the device to the logits every token
    is chosen from, greedy or sampled, each row over its own generated tokens; OFF holds their neutral values.
    return_logits: the call also returns the RAW logits of the executed steps [n_steps, rows, V] - what a sampled call drew from, or
    the copy a greedy call takes before its processors change them; plain greedy decoding keeps no copy and is refused."""
    num_beams: int = 1
    length_penalty: float = 1.0
    return_trace: bool = False
    do_sample: bool = False
    temperature: float = 1.0
    top_k: int = 0
    top_p: float = 1.0
    seed: int = 0
    repetition_penalty: float = OFF["repetition_penalty"]
    no_repeat_ngram_size: int = OFF["no_repeat_ngram_size"]
    min_new_tokens: int = OFF["min_new_tokens"]
    return_logits: bool = False

    def __post_init__(self):
        B = self.num_beams
        if not isinstance(B, int) or B < 1:
            raise V3DError(f"num_beams must be a positive integer (got {B!r})")
        if B == 1 and self.return_trace:
            raise V3DError("return_trace belongs to beam search (num_beams > 1)")
        try:
            p = float(self.repetition_penalty)
        except (TypeError, ValueError):
            p = float("nan")
        if not (p > 0.0 and math.isfinite(p)):
            raise V3DError(f"repetition_penalty must be a finite float > 0 (got {self.repetition_penalty!r}; 1.0 is off)")
        for name in ("no_repeat_ngram_size", "min_new_tokens"):
            v = getattr(self, name)
            if isinstance(v, bool) or not isinstance(v, int) or v < 0:
                raise V3DError(f"{name} must be an integer >= 0 (got {v!r}; 0 is off)")
        if self.do_sample:
            T, tp, tk = float(self.temperature), float(self.top_p), self.top_k
            if not (T > 0.0 and math.isfinite(T)) or not (0.0 < tp <= 1.0) or int(tk) != tk or tk < 0:
                raise V3DError(f"do_sample needs a finite temperature > 0, top_k >= 0 and 0 < top_p <= 1 (got {self.temperature!r}, {tk!r}, {self.top_p!r})")
        if B > 1 and self.processors:
            raise V3DError("repetition_penalty / no_repeat_ngram_size / min_new_tokens cannot be combined with num_beams > 1: transformers applies "
                           "them to the log-softmax scores inside its beam search, v3d_beam_topk forms those scores inside the kernel and a beam's "
                           "history follows its parent - processors under beams are not built")
        if B > 1 and self.do_sample:
            raise V3DError("do_sample cannot be combined with num_beams > 1: beam-sample is not built")
        if self.return_logits and self.plain:
            raise V3DError("return_logits belongs to do_sample=True or a logits processor (num_beams = 1): plain greedy decoding and beam "
                           "search keep no copy of the logits")

    @property
    def processors(self):
        """the processor controls that are on, as a dict ({}: none)"""
        return processors_on(self)

    @property
    def plain(self):
        """nothing touches the logits between the LM head and the argmax (greedy decoding, or beams): the loops run untouched"""
        return not (self.do_sample or self.processors)

    def check(self, eos_token_id=UNKNOWN, max_new_tokens=None, stopping=None):
        """What a rule cannot know by itself: the call's EOS ids, its length and its stopping callback.  Returns the rule."""
        if self.num_beams > 1 and stopping is not None:
            raise V3DError("a stopping callback cannot be combined with num_beams > 1: beams stop by EOS ids and max_new_tokens only")
        k = self.min_new_tokens
        if k > 0 and eos_token_id is not UNKNOWN and not eos_ids(eos_token_id):
            raise V3DError(f"min_new_tokens = {k} needs an eos_token_id: it bans the EOS ids, and none is given")
        if k > 0 and max_new_tokens is not None and k > max_new_tokens:
            raise V3DError(f"min_new_tokens = {k} exceeds max_new_tokens = {max_new_tokens}")
        return self

    def fit(self, max_new_tokens):
        """The rule with min_new_tokens bounded by the max_new_tokens a call actually runs (a long prompt cuts it to the engine's room)."""
        return dataclasses.replace(self, min_new_tokens=max(int(max_new_tokens), 0)) if self.min_new_tokens > max_new_tokens else self


def rule_of(rule, controls, beams=True):
    """The rule of a call that takes its controls as rule= or as the fields' keywords; unknown ones, or beams where there are none: TypeError"""
    if not beams and {"num_beams", "length_penalty", "return_trace"} & set(controls):
        raise TypeError(f"got an unexpected keyword argument among {sorted(controls)}: this call has no beams")
    if rule is None:
        return GenerationRule(**controls)
    if controls:
        raise TypeError(f"the generation controls come as rule= or as keywords, not both (got rule= and {sorted(controls)})")
    return rule


# ---------------------------------------------------------------------- the drivers' flags
def add_arguments(ap):
    """--num_beams / --length_penalty, --temperature / --top_p / --top_k / --seed and the three processor flags of the eval drivers"""
    ap.add_argument("--num_beams", type=int, default=1,
                    help="the reference drivers' flag (model_scanqa.py:173-185): beams per question for the generation tasks; N > 1 runs one question "
                         "at a time (with --reuse-scenes: one scene prefill, then one beam search per question) - the cross-scene decode group "
                         "is greedy and is not used with beams")
    ap.add_argument("--length_penalty", type=float, default=1.0, help="beam search: a finished hypothesis scores sum(log p) / n ** length_penalty")
    ap.add_argument("--temperature", type=float, default=0.0,
                    help="the reference drivers' flag: 0 (default) decodes greedily; > 0 draws every token on the device from softmax(logits / "
                         "temperature) after --top_k and --top_p.  Each question draws from the random stream of its index in the question file, so the "
                         "records do not depend on batching, --reuse-scenes or the number of ranks; sampling runs one question (or scene batch) at a time")
    ap.add_argument("--top_p", type=float, default=1.0, help="sampling: keep the most probable tokens whose mass before them is below top_p (1: off)")
    ap.add_argument("--top_k", type=int, default=0, help="sampling: keep the top_k most probable tokens (0: off)")
    ap.add_argument("--seed", type=int, default=0, help="sampling: the 64-bit seed of the run")
    ap.add_argument("--repetition_penalty", type=float, default=OFF["repetition_penalty"],
                    help="the logits of every token generated so far are divided (positive) or multiplied (negative) by this (transformers' "
                         "repetition_penalty; 1: off)")
    ap.add_argument("--no_repeat_ngram_size", type=int, default=OFF["no_repeat_ngram_size"],
                    help="no n-gram of this size occurs twice in an answer (the reference drivers' commented-out no_repeat_ngram_size=3; 0: off)")
    ap.add_argument("--min_new_tokens", type=int, default=OFF["min_new_tokens"], help="the EOS ids cannot be chosen before this many tokens (0: off)")


def rule_from_flags(ap, a):
    """The rule of the parsed flags `a` (add_arguments, plus the drivers' --max-new-tokens); what the rule refuses is ap.error.
    --temperature 0 is greedy decoding; the sampling flags are range-checked all the same."""
    draw = dict(do_sample=True, temperature=a.temperature or 1.0, top_k=a.top_k, top_p=a.top_p, seed=a.seed)
    try:
        GenerationRule(**draw)
        return GenerationRule(num_beams=a.num_beams, length_penalty=a.length_penalty, repetition_penalty=a.repetition_penalty,
                              no_repeat_ngram_size=a.no_repeat_ngram_size, min_new_tokens=a.min_new_tokens, **(draw if a.temperature != 0 else {})).check(max_new_tokens=a.max_new_tokens)
    except V3DError as e:
        ap.error(str(e))
