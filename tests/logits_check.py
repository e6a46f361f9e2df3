"""The logits processors' rule ("Logits processors, stated once") restated in plain torch, the rule every choice of a
run is checked against, and the inputs of the kernel tests.

process(logits, history, p, n, k, eos)   one row.  The history is the tokens generated so far (never the prompt), L = len(history):
    repetition_penalty p   every distinct id v of the history: x[v] = x[v] < 0 ? x[v] * p : x[v] / p, in f32 from the unpenalised value,
                           rounded once (to nearest even) into the row's dtype;
    no_repeat_ngram_size n if L + 1 >= n: every i in [0, L - n] with h[i .. i+n-1) == h[L-n+1 .. L) sets x[h[i+n-1]] = -inf;
    min_new_tokens k       while L < k every EOS id is set to -inf;
in that order, ids outside [0, V) skipped, nothing else written (columns [V, ld) of a padded row included).
check_choice(tokens, raw_logits, settings)   replays a run from the raw logits of its steps: every token is the argmax (the lowest index on
ties) of its processed row."""
import math

import torch


def process(logits, history, p=1.0, n=0, k=0, eos=(), V=None):
    """logits: one row ([ld], any float dtype; the result has its dtype) -> the processed row (a new tensor).  history: the generated
    tokens so far (ints); V: the columns that are vocabulary (default: all)."""
    x = logits.clone()
    V = x.numel() if V is None else int(V)
    h = [int(t) for t in history]
    L = len(h)
    ok = lambda v: 0 <= v < V                                                  # noqa: E731
    if p != 1.0:
        ids = sorted({v for v in h if ok(v)})
        if ids:
            idx = torch.tensor(ids, dtype=torch.int64)
            s = logits[idx].float()                                           # gather: the unpenalised values
            pen = torch.tensor(p, dtype=torch.float32)
            x[idx] = torch.where(s < 0, s * pen, s / pen).to(x.dtype)         # scatter: one rounding
    if n > 0 and L + 1 >= n:
        tail = h[L - n + 1:]
        for i in range(0, L - n + 1):
            if h[i: i + n - 1] == tail and ok(h[i + n - 1]):
                x[h[i + n - 1]] = -math.inf
    if L < k:
        for e in eos:
            if ok(int(e)):
                x[int(e)] = -math.inf
    return x


def process_rows(logits, history, n_prev, p=1.0, n=0, k=0, eos=(), V=None):
    """logits [M, ld], history [>= n_prev, >= M] (row m's tokens are history[:n_prev, m]) -> the processed rows"""
    return torch.stack([process(logits[m], history[:n_prev, m].tolist() if n_prev else [], p, n, k, eos, V) for m in range(logits.shape[0])])


def bits(x):
    """the raw 16-bit (or 32-bit) patterns, so that -0 / +0 and the pad columns compare exactly"""
    return x.contiguous().view(torch.int16 if x.element_size() == 2 else torch.int32)


def processed_logits(tokens, raw_logits, settings):
    """raw_logits [n_steps, M, V] and the rows' tokens (a list of M 1-D tensors, row m of length <= n_steps) -> the logits every token was
    chosen from, [n_steps, M, V]; steps past a row's end keep its raw logits."""
    out = raw_logits.clone()
    for m, row in enumerate(tokens):
        row = [int(t) for t in row]
        for t in range(len(row)):
            out[t, m] = process(raw_logits[t, m], row[:t], settings.get("p", 1.0), settings.get("n", 0), settings.get("k", 0), settings.get("eos", ()))
    return out


def check_choice(tokens, raw_logits, settings, what=""):
    """tokens: a list of M 1-D token tensors (a row may end early, after its EOS); raw_logits [>= len, M, V]: the unprocessed logits of the
    steps; settings = dict(p, n, k, eos).  Asserts that token t of row m is the first maximum of process(raw_logits[t, m], tokens[m][:t])."""
    raw_logits = raw_logits.detach().cpu()
    assert raw_logits.dim() == 3 and raw_logits.shape[1] == len(tokens), (what, tuple(raw_logits.shape), len(tokens))
    n = 0
    for m, row in enumerate(tokens):
        row = [int(t) for t in row]
        assert len(row) <= raw_logits.shape[0], f"{what}: row {m} has {len(row)} tokens for {raw_logits.shape[0]} steps of logits"
        for t, tok in enumerate(row):
            x = process(raw_logits[t, m], row[:t], settings.get("p", 1.0), settings.get("n", 0), settings.get("k", 0), settings.get("eos", ())).float()
            best = float(x.max())
            first = int((x == best).nonzero()[0])
            assert tok == first, (f"{what}: row {m} step {t}: token {tok} (processed logit {float(x[tok])}, raw {float(raw_logits[t, m, tok])}) is not the "
                                  f"first maximum {first} ({best}) after history {row[:t]}")
            n += 1
    return n


# ---------------------------------------------------------------- the kernel cases (tests/test_logits_check_cpu.py: the host twin;
# tests/test_gpu_logits_process.py: the kernel)

SENTINEL = 123.0          # the pad columns [V, ld): must survive
REPEAT_ID = 777           # the id planted at history positions 3, 3 + 256 and 1030


def _history(gen, kind, steps, V):
    """one row's tokens.  'few': six ids, so n-grams repeat and overlap; 'run': one id throughout (every window matches, all overlapping);
    'wide': ids over the whole vocabulary, so a 3-gram does not recur in a short history - with ids outside [0, V) planted; 'period': a
    period-7 pattern with one id == V (the first id out of range)."""
    if kind == "few":
        h = torch.randint(40, 46, (steps,), generator=gen)
    elif kind == "run":
        h = torch.full((steps,), 51, dtype=torch.int64)
    elif kind == "wide":
        h = torch.randint(0, V, (steps,), generator=gen)
        for at, v in ((1, V + 5), (4, -3), (6, 1 << 40)):
            if at < steps:
                h[at] = v
    else:
        h = (torch.arange(steps) % 7) * 11 + 100
        if steps > 9:
            h[9] = V
    return h.to(torch.int64)


KINDS = ("few", "wide", "run", "period")


def extremes(dtype):
    """logits whose penalised value overflows to +-inf or lands among the subnormals of the 16-bit format (and, for bf16, of f32): the
    largest and the smallest magnitudes of `dtype`, both signs"""
    big, tiny = (6.5e4, 6.0e-8) if dtype == torch.float16 else (3.0e38, 1.0e-38)
    return (big, -big, tiny, -tiny, big * 0.9, -big * 0.9, tiny * 3, -tiny * 3)


def make_case(name, dtype, M, L, p=1.0, n=0, k=0, eos=(), V=1000, ld=1024, seed=0, extreme=False):
    """logits [M, ld] of `dtype` (N(0, 3^2), the pad columns = SENTINEL; a positive and a negative value, zero and -inf planted on history
    ids - with extreme=True the format's largest and smallest magnitudes as well), history [L + 2, M + 3] int64 (the step stride exceeds
    M; rows of different kinds; the two steps past L and the three spare columns hold ids the rule must not see)."""
    gen = torch.Generator().manual_seed(1000 + seed)
    x = (torch.randn(M, ld, generator=gen) * 3.0).to(dtype)
    x[:, V:] = SENTINEL
    steps, stride = L + 2, M + 3
    hist = torch.full((steps, stride), 7, dtype=torch.int64)
    for m in range(M):
        hist[:, m] = _history(gen, KINDS[m % 4], steps, V)
        if L >= 1100:
            hist[3, m] = hist[3 + 256, m] = hist[1030, m] = REPEAT_ID
            x[m, REPEAT_ID] = 3.0
        d = sorted({int(v) for v in hist[:L, m].tolist() if 0 <= v < V and v != REPEAT_ID})
        for v, val in zip(d, (2.5, -2.5, 0.0, -math.inf) + (extremes(dtype) if extreme else ())):
            x[m, v] = val
    return dict(name=name, M=M, V=V, ld=ld, L=L, p=p, n=n, k=k, eos=tuple(eos), logits=x, history=hist)


def kernel_cases(dtype):
    """The case list of the issue: V = 1000 of ld 1024 and one case at V = 152064; M in {1, 5, 32}; history lengths {0, 1, n-2, n-1, n, 2n,
    300, 1100}; each control alone and all three together; one and three EOS ids at L = k - 1 and L = k."""
    cases = []
    add = lambda *a, **kw: cases.append(make_case(*a, seed=len(cases), **kw))          # noqa: E731
    for L in (0, 1, 2, 300, 1100):
        add(f"penalty-L{L}", dtype, 5, L, p=1.3)
    add("penalty-below-one-L300", dtype, 5, 300, p=0.75)
    for n in (1, 2, 3):
        for L in sorted({0, 1, max(n - 2, 0), n - 1, n, 2 * n, 300, 1100}):
            add(f"ngram{n}-L{L}", dtype, 5, L, n=n)
    for eos in ((17,), (17, 999, 3)):
        for L in (4, 5):                                                               # k = 5: L = k - 1 bans, L = k does not
            add(f"min-new-eos{len(eos)}-L{L}", dtype, 5, L, k=5, eos=eos)
    add("min-new-eos-out-of-range", dtype, 5, 2, k=5, eos=(1000, -1, 12))
    for M in (1, 5, 32):
        for L in (0, 1, 2, 6, 300, 1100):
            add(f"all-M{M}-L{L}", dtype, M, L, p=1.3, n=3 if L == 6 else 2, k=L + 1 if L % 2 == 0 else L, eos=(17, 40, 51))
    add("all-V152064", dtype, 5, 300, p=1.3, n=2, k=512, eos=(151645, 151643), V=152064, ld=152064)
    add("all-V152064-M32-L1100", dtype, 32, 1100, p=1.2, n=3, k=4, eos=(151645,), V=152064, ld=152064)
    for p in (1.3, 0.8, 1.0e-3, 1.0e3):                                                # overflow to +-inf, results among the subnormals
        add(f"penalty-extremes-p{p:g}", dtype, 5, 300, p=p, extreme=True)
    return cases


def expected(case):
    """(the processed rows, the number of changed 16-bit entries per row)"""
    want = process_rows(case["logits"], case["history"], case["L"], case["p"], case["n"], case["k"], case["eos"], case["V"])
    return want, (bits(want) != bits(case["logits"])).sum(1)


def must_change(case):
    """cases in which the rule certainly rewrites an entry of row 0 (a 'few' row): a kernel that writes nothing cannot pass them"""
    L = case["L"]
    return (case["p"] != 1.0 and L > 0) or (case["n"] == 1 and L >= 1) or (case["n"] > 1 and L >= 300) or (L < case["k"] and any(0 <= e < case["V"] for e in case["eos"]))
