"""Sampling (v3d_sample_rows, its host twin, Engine's do_sample paths) against its specification.  A helper, not a test:
tests/test_sample_check_cpu.py proves that SampleRef's kept set is what transformers' three warpers keep, that the host twin passes
check_draws and the chi-square rule, that the inputs of the GPU tests are usable, and that the rules below reject eight planted faults;
tests/test_gpu_sample_kernels.py and tests/test_gpu_sampling.py apply them.

The rule ("Sampling, stated once").  Per row: logits x[V] (16-bit, or f32 for the twin), T > 0, top_k (0 = off,
otherwise clamped to V), 0 < top_p <= 1 (1 = off, as transformers builds no warper then), a 64-bit seed, a step, a 32-bit stream id.
Token i comes before j when x_i > x_j, or x_i == x_j and i < j; r_i = tokens before i.  z_i = f32(x_i) / f32(T).  Top-k keeps r_i <
top_k.  p = softmax(z) over those, m_i = the sum of p_j over survivors before i; top-p keeps m_i < top_p or r_i == 0.  Draw: u_i =
((w >> 8) + 0.5) * 2^-24 with w = word i & 3 of Philox4x32-10 at counter (i >> 2, step, stream, 0), key (seed low, seed high); g_i =
-log(-log(u_i)); the token is the kept i with the largest z_i + g_i, the lower index on equal keys.  SampleRef states it in f64 torch
(z is the f32 quotient, widened), with Philox restated here in Python.

check_draws.  A draw passes only if the token is in range, is not surely removed (r_i >= top_k, or m_i >= top_p + bound_m), and its
f64 key is at least the largest f64 key over the surely kept tokens (r_i < top_k and m_i < top_p - bound_m, or r_i == 0) minus 2 *
bound_key.  bound_key = 4 * e_key, e_key = max |torch-CPU f32 evaluation of z + g - f64| on the test's inputs; bound_m = 4 * e_m, e_m
likewise for the f32 softmax and its descending cumulative sum: the project's 4 x e_ref convention (tests/answer_check.py).  No bound
comes from the code under test.  A draw whose token is not the f64 winner is "excused"; at most 1 draw in 200 of a case may be, and
each is printed with its margin."""
import math

import torch

M0, M1, W0, W1 = 0xD2511F53, 0xCD9E8D57, 0x9E3779B9, 0xBB67AE85
MASK = 0xFFFFFFFF

# (temperature, top_k, top_p): the five settings every test sweeps
SETTINGS = [(1.0, 0, 1.0), (0.7, 50, 1.0), (0.2, 0, 0.9), (1.3, 40, 0.95), (1.0, 0, 1e-6)]

PHILOX_KNOWN = [
    ((0, 0, 0, 0), (0, 0), (0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8)),
    ((MASK,) * 4, (MASK,) * 2, (0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd)),
    ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0), (0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1)),
]


def philox4x32_10(counter, key):
    """Philox4x32-10 over Python ints."""
    c0, c1, c2, c3 = [int(c) & MASK for c in counter]
    k0, k1 = [int(k) & MASK for k in key]
    for _ in range(10):
        p0, p1 = M0 * c0, M1 * c2
        c0, c1, c2, c3 = (p1 >> 32) ^ c1 ^ k0, p1 & MASK, (p0 >> 32) ^ c3 ^ k1, p0 & MASK
        k0, k1 = (k0 + W0) & MASK, (k1 + W1) & MASK
    return (c0, c1, c2, c3)


def token_words(idx, step, stream, seed):
    """The Philox word of every token: idx int64 tensor of token indices, stream an int64 tensor that broadcasts against it (or an int)
    -> int64 tensor of 32-bit words.  int64 products wrap modulo 2^64, which keeps every bit that is read."""
    idx = torch.as_tensor(idx, dtype=torch.int64)
    c0 = idx >> 2
    c2 = torch.as_tensor(stream, dtype=torch.int64) & MASK
    c0, c2 = torch.broadcast_tensors(c0, c2)
    c1 = torch.full_like(c0, int(step) & MASK)
    c3 = torch.zeros_like(c0)
    k0, k1 = int(seed) & MASK, (int(seed) >> 32) & MASK
    for _ in range(10):
        p0, p1 = c0 * M0, c2 * M1
        c0, c1, c2, c3 = ((p1 >> 32) & MASK) ^ c1 ^ k0, p1 & MASK, ((p0 >> 32) & MASK) ^ c3 ^ k1, p0 & MASK
        k0, k1 = (k0 + W0) & MASK, (k1 + W1) & MASK
    lane = torch.broadcast_to(idx & 3, c0.shape)
    return torch.where(lane == 0, c0, torch.where(lane == 1, c1, torch.where(lane == 2, c2, c3)))


def row_words(V, step, streams, seed):
    """The words of tokens 0 .. V-1 for every stream id: [len(streams), V].  One Philox call per four tokens."""
    G = (V + 3) // 4
    c0 = torch.arange(G, dtype=torch.int64)[None, :]
    c2 = (torch.as_tensor(streams, dtype=torch.int64) & MASK)[:, None]
    c0, c2 = [t.contiguous() for t in torch.broadcast_tensors(c0, c2)]
    c1 = torch.full_like(c0, int(step) & MASK)
    c3 = torch.zeros_like(c0)
    k0, k1 = int(seed) & MASK, (int(seed) >> 32) & MASK
    for _ in range(10):
        p0, p1 = c0 * M0, c2 * M1
        c0, c1, c2, c3 = ((p1 >> 32) & MASK) ^ c1 ^ k0, p1 & MASK, ((p0 >> 32) & MASK) ^ c3 ^ k1, p0 & MASK
        k0, k1 = (k0 + W0) & MASK, (k1 + W1) & MASK
    return torch.stack([c0, c1, c2, c3], dim=-1).reshape(c0.shape[0], 4 * G)[:, :V]


def gumbel64(words):
    u = ((words >> 8).double() + 0.5) * 2.0 ** -24
    return -torch.log(-torch.log(u))


def gumbel32(words):
    """g in torch-CPU f32.  n + 0.5 needs 25 bits once n >= 2^23, so the upper half goes through 1 - u (exact in f32 there) and log1p."""
    n = words >> 8
    small = n < (1 << 23)
    a_lo = -torch.log((torch.where(small, n, 0).float() + 0.5) * 2.0 ** -24)
    a_hi = -torch.log1p(-((torch.where(small, 1, (1 << 24) - n).float() - 0.5) * 2.0 ** -24))
    return -torch.log(torch.where(small, a_lo, a_hi))


class SampleRef:
    """The specification over the rows x [M, V] (bf16 / f16 / f32 host tensor).  In token order: rank (r_i), m (f64, +inf outside the
    top-k survivors), kept (bool), kept_count [M]; e_m = max |f32 softmax + cumulative sum - f64| over the survivors.
    mutant: one of the planted faults of tests/test_sample_check_cpu.py (None = the rule)."""

    def __init__(self, x, T, top_k, top_p, mutant=None):
        x = x.detach().cpu()
        self.M, self.V = x.shape
        self.T, self.top_p, self.mutant = float(T), float(top_p), mutant
        self.k = self.V if (top_k <= 0 or top_k > self.V) else int(top_k)
        z32 = x.float() / torch.tensor(1.0 if mutant == "no_temperature" else T, dtype=torch.float32)
        self.z32, self.z = z32, z32.double()
        xs = x.double()
        if mutant == "ties_high":
            order = (self.V - 1) - torch.sort(xs.flip(1), dim=1, descending=True, stable=True).indices
        else:
            order = torch.sort(xs, dim=1, descending=True, stable=True).indices
        pos = torch.arange(self.V).expand(self.M, -1)
        self.order = order
        self.rank = torch.empty_like(order).scatter_(1, order, pos)
        surv = pos < self.k
        if mutant == "p_before_k":
            surv_p = torch.ones_like(surv)
        else:
            surv_p = surv
        zs = self.z.gather(1, order)
        zs_m = torch.where(surv_p, zs, torch.full_like(zs, -math.inf))
        p = torch.softmax(zs_m, dim=1)
        m = torch.cumsum(p, dim=1) - p
        p32 = torch.softmax(zs_m.float(), dim=1)
        m32 = torch.cumsum(p32, dim=1) - p32
        self.e_m = float((m32.double() - m)[surv_p].abs().max())
        if self.top_p < 1.0:
            inside = (m <= self.top_p) if mutant == "p_inclusive" else (m < self.top_p)
            keep = surv & (inside | (pos == 0))
        else:
            keep = surv
        m = torch.where(surv, m, torch.full_like(m, math.inf))
        self.p_sorted, self.keep_sorted = p, keep
        self.m = torch.empty_like(m).scatter_(1, order, m)
        self.kept = torch.empty_like(keep).scatter_(1, order, keep)
        self.kept_count = keep.sum(1)

    def probabilities(self):
        """The warped distribution [M, V] (f64): softmax(z) over the kept set."""
        zk = torch.where(self.kept, self.z, torch.full_like(self.z, -math.inf))
        return torch.softmax(zk, dim=1)

    def words(self, step, streams, seed):
        st = torch.as_tensor(streams, dtype=torch.int64)
        if self.mutant == "no_stream":
            st = torch.zeros_like(st)
        if self.mutant == "no_step":
            step = 0
        w = row_words(self.V, step, st, seed)
        if self.mutant == "shared_u":
            w = w[:, :1].expand(-1, self.V)
        return w

    def keys(self, step, streams, seed):
        """(f64 keys, f32 keys) [M, V] of every token."""
        w = self.words(step, streams, seed)
        if self.mutant == "no_outer_log":
            u = ((w >> 8).double() + 0.5) * 2.0 ** -24
            return self.z + torch.log(u), None
        return self.z + gumbel64(w), self.z32 + gumbel32(w)

    @staticmethod
    def winner(keys, mask):
        """argmax of keys over mask per row, the lower index on equal keys (torch.argmax returns the first maximum)."""
        return torch.argmax(torch.where(mask, keys, torch.full_like(keys, -math.inf)), dim=1)

    def draw(self, step, streams, seed):
        return self.winner(self.keys(step, streams, seed)[0], self.kept)


def _as_list(v, n, what):
    v = list(v)
    assert len(v) == n, (what, len(v), n)
    return [int(i) for i in v]


def check_draws(tokens, kept_counts, x, args, what="", ref=None):
    """tokens [n_steps, M] drawn from x ([M, V]: the same logits at every step, or [n_steps, M, V]) with args = dict(T, top_k, top_p,
    seed, steps (one per row of tokens; default 0, 1, ...), streams (one per column; default 0 .. M-1)); kept_counts ([n_steps, M] or
    None) are compared with SampleRef's exactly.  Optional args bound_key / bound_m replace the bounds computed from these inputs.
    Returns dict(n, excused=[(step, row, token, winner, margin)], e_key, e_m, bound_key, bound_m); raises AssertionError otherwise."""
    tokens = torch.as_tensor(tokens).detach().cpu().to(torch.int64)
    n_steps, M = tokens.shape
    per_step = x.dim() == 3
    V = x.shape[-1]
    steps = _as_list(args.get("steps", range(n_steps)), n_steps, "steps")
    streams = _as_list(args.get("streams", range(M)), M, "streams")
    T, top_k, top_p, seed = args["T"], args["top_k"], args["top_p"], args["seed"]
    assert bool(((tokens >= 0) & (tokens < V)).all()), f"{what}: a token outside [0, {V})"
    if kept_counts is not None:
        kept_counts = torch.as_tensor(kept_counts).detach().cpu().to(torch.int64)
    refs = [ref if ref is not None else SampleRef(x, T, top_k, top_p)] if not per_step else [SampleRef(x[t], T, top_k, top_p) for t in range(n_steps)]
    e_m = max(r.e_m for r in refs)
    bound_m = float(args.get("bound_m", 4.0 * e_m))
    rows = torch.arange(M)
    e_key, found = 0.0, []
    for t in range(n_steps):
        r = refs[t if per_step else 0]
        tok = tokens[t]
        if kept_counts is not None:
            assert torch.equal(kept_counts[t], r.kept_count), f"{what}: step {steps[t]}: kept {kept_counts[t].tolist()} != {r.kept_count.tolist()}"
        rank, m = r.rank[rows, tok], r.m[rows, tok]
        gone = (rank >= r.k) | ((top_p < 1.0) & (rank > 0) & (m >= top_p + bound_m))
        assert not bool(gone.any()), f"{what}: step {steps[t]}: rows {rows[gone].tolist()} drew a removed token {tok[gone].tolist()}"
        k64, k32 = r.keys(steps[t], streams, seed)
        e_key = max(e_key, float((k32.double() - k64).abs().max()))
        sure = (r.rank < r.k) & ((r.m < top_p - bound_m) | (r.rank == 0)) if top_p < 1.0 else (r.rank < r.k)
        best = torch.where(sure, k64, torch.full_like(k64, -math.inf)).max(dim=1).values
        win = r.winner(k64, r.kept)
        found.append((tok, k64[rows, tok], best, win, k64[rows, win]))
    bound_key = float(args.get("bound_key", 4.0 * e_key))
    excused = []
    for t, (tok, mine, best, win, top) in enumerate(found):
        low = mine < best - 2.0 * bound_key
        assert not bool(low.any()), (f"{what}: step {steps[t]}: rows {rows[low].tolist()} drew {tok[low].tolist()} whose keys are "
                                     f"{(best - mine)[low].tolist()} below the best kept key (bound {2.0 * bound_key:.3g})")
        for b in rows[win != tok].tolist():
            excused.append((steps[t], b, int(tok[b]), int(win[b]), float(top[b] - mine[b])))
    for e in excused:
        print(f"{what}: excused: step {e[0]} row {e[1]} drew {e[2]}, the f64 winner is {e[3]} (key margin {e[4]:.3g}, bound_key {bound_key:.3g})")
    n = n_steps * M
    assert len(excused) * 200 <= n, f"{what}: {len(excused)} of {n} draws are not the f64 winner (at most 1 in 200)"
    return dict(n=n, excused=excused, e_key=e_key, e_m=e_m, bound_key=bound_key, bound_m=bound_m)


# ---------------------------------------------------------------- the chi-square rule

def chi2_quantile_upper(df, q=1e-6):
    """The upper-q quantile of chi-square(df) by Wilson-Hilferty."""
    from statistics import NormalDist
    zq = NormalDist().inv_cdf(1.0 - q)
    return df * (1.0 - 2.0 / (9.0 * df) + zq * math.sqrt(2.0 / (9.0 * df))) ** 3


def chi2_check(tokens, probs, q=1e-6):
    """Pearson chi-square of the drawn tokens (1-D) against the distribution probs [V] (f64): bins of descending probability pooled until
    each expects >= 5 draws.  Returns (statistic, bound, degrees of freedom); the rule is statistic < bound."""
    tokens = torch.as_tensor(tokens).reshape(-1).cpu().to(torch.int64)
    n = tokens.numel()
    V = probs.numel()
    counts = torch.bincount(tokens, minlength=V).double()
    if bool((counts[probs <= 0.0] > 0).any()):         # a token of probability zero was drawn: no pooling may hide that
        return math.inf, 1.0, 0
    order = torch.argsort(probs, descending=True, stable=True)
    exp, obs = (probs[order] * n).tolist(), counts[order].tolist()
    bins, e_acc, o_acc = [], 0.0, 0.0
    for e, o in zip(exp, obs):
        e_acc += e
        o_acc += o
        if e_acc >= 5.0:
            bins.append([e_acc, o_acc])
            e_acc = o_acc = 0.0
    if e_acc > 0.0 or o_acc > 0.0:                     # the tail joins the last bin
        if bins:
            bins[-1][0] += e_acc
            bins[-1][1] += o_acc
        else:
            bins.append([e_acc, o_acc])
    df = len(bins) - 1
    if df < 1:                                         # one bin: nothing to compare
        return 0.0, 1.0, 0
    stat = sum((o - e) ** 2 / e for e, o in bins)
    return stat, chi2_quantile_upper(df, q), df


# ---------------------------------------------------------------- the inputs of the GPU kernel tests

GPU_SHAPES = [(1000, 1024), (4099, 4099), (70000, 70000)]          # (V, ldx)
GPU_SEED = 0x5EEDC0DE12345
GPU_STEPS = 64


def gpu_logits(V, dtype, rows=32, seed=11):
    """The rows of the kernel tests: N(0, 2.5^2) logits rounded to dtype (many equal 16-bit values at V = 70000), fixed seed.  The tests with
    fewer rows take the first ones."""
    g = torch.Generator().manual_seed(seed * 1000003 + V)
    return (torch.randn(rows, V, generator=g) * 2.5).to(dtype)


def margin_to_top_p(ref):
    """min |m_i - top_p| over the top-k survivors of every row (inf when top-p is off): kept counts can be compared exactly when it is
    above 2 * bound_m."""
    if ref.top_p >= 1.0:
        return math.inf
    m = ref.m[torch.isfinite(ref.m) & (ref.rank > 0)]             # (the first token is kept whatever its m)
    return float((m - ref.top_p).abs().min()) if m.numel() else math.inf
