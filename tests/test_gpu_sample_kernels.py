"""The sampler's kernels on their own (csrc/sample.hip, v3d_sample_rows) under tests/sample_check.py: every draw against the f64 statement of
the rule (check_draws; kept counts exactly), the degenerate forms against v3d_argmax_rows, a planted winner at every cut the launch plan
makes in a row, top-k and exact ties at the cut, drawn frequencies under the chi-square rule, independence of M / row position / ldx, and the
argument check.  The inputs are sample_check.gpu_logits (fixed seeds; tests/test_sample_check_cpu.py shows them usable: no token's mass
within 2 * bound_m of top_p, the f32 evaluation under the excused cap).  One reference pass per case serves the 1-, 5- and 32-row calls: a
row's draw does not depend on the rows beside it, so they are the first rows of the same logits on the same streams."""
import ctypes
import math

import pytest
import torch

import sample_check as sc
from v3d import ops
from v3d._native import V3DError, lib

pytestmark = pytest.mark.gpu


def _padded(x, ldx):
    """x [M, V] behind a leading dimension ldx; the columns behind V hold a huge logit that must never be read."""
    M, V = x.shape
    buf = torch.full((M, ldx), 60.0, dtype=x.dtype)
    buf[:, :V] = x
    return buf.cuda()[:, :V] if ldx > V else x.cuda()


def _draw(xd, setting, seed, steps, streams=None):
    """xd [M, V] device rows (any row stride) -> (tokens [n_steps, M], kept [n_steps, M]) on the host: one call per step, one sync."""
    T, k, p = setting
    M, V = xd.shape
    ws = ops.sample_workspace(M, V)
    toks = torch.full((len(steps), M), -7, dtype=torch.int64, device="cuda")
    kept = torch.full((len(steps), M), -7, dtype=torch.int32, device="cuda")
    st = None if streams is None else torch.tensor(streams, dtype=torch.int32, device="cuda")
    for j, step in enumerate(steps):
        ops.sample_rows(xd, toks[j], ws, T, k, p, seed, step, st, kept=kept[j])
    torch.cuda.synchronize()
    return toks.cpu(), kept.cpu()


@pytest.mark.parametrize("setting", sc.SETTINGS, ids=lambda s: "T%g-k%d-p%g" % s)
@pytest.mark.parametrize("V,ldx", sc.GPU_SHAPES)
@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16], ids=["bf16", "f16"])
def test_draws_against_f64(dtype, V, ldx, setting):
    T, k, p = setting
    x = sc.gpu_logits(V, dtype)
    assert int(lib().v3d_sample_workspace_bytes(32, V)) > 0
    got = {M: _draw(_padded(x[:M], ldx), setting, sc.GPU_SEED, range(sc.GPU_STEPS)) for M in (1, 5, 32)}
    toks, kept = got[32]
    for M in (1, 5):                                            # the smaller calls are the first rows of the larger one, bit for bit
        assert torch.equal(got[M][0], toks[:, :M]) and torch.equal(got[M][1], kept[:, :M]), f"{M} rows differ from the first rows of 32"
    r = sc.check_draws(toks, kept, x, dict(T=T, top_k=k, top_p=p, seed=sc.GPU_SEED), what=f"{dtype} V={V} {setting}")
    print(f"{dtype} V={V} ldx={ldx} {setting}: {r['n']} draws, {len(r['excused'])} excused, e_key {r['e_key']:.3g}, e_m {r['e_m']:.3g}")


@pytest.mark.parametrize("setting", [(1.0, 0, 1.0), (0.7, 50, 0.9)], ids=lambda s: "T%g-k%d-p%g" % s)
def test_draws_at_the_models_vocabulary(setting):
    T, k, p = setting
    V = 152064
    x = sc.gpu_logits(V, torch.bfloat16)
    toks, kept = _draw(x.cuda(), setting, sc.GPU_SEED, range(8))
    r = sc.check_draws(toks, kept, x, dict(T=T, top_k=k, top_p=p, seed=sc.GPU_SEED), what=f"V={V} {setting}")
    print(f"V={V} {setting}: {r['n']} draws, {len(r['excused'])} excused, e_key {r['e_key']:.3g}, e_m {r['e_m']:.3g}")


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16], ids=["bf16", "f16"])
def test_degenerate_forms_are_argmax(dtype):
    """top_k = 1 and top_p = 1e-6 keep the first token of the order alone: v3d_argmax_rows' answer, ties included."""
    V = 4099
    x = sc.gpu_logits(V, dtype, rows=8, seed=5)
    top = x.float().max(dim=1).values
    g = torch.Generator().manual_seed(9)
    for m in range(1, 8):                                       # rows 1..7: the maximum two to eight times, at scattered columns
        cols = torch.randperm(V, generator=g)[: m + 1]
        x[m, cols] = top[m].to(dtype)
    x[7, 0] = x[7, V - 1] = top[7].to(dtype)
    xd = x.cuda()
    want = torch.empty(8, dtype=torch.int64, device="cuda")
    ops.argmax_rows(xd, want, torch.empty(256 * 8, dtype=torch.float32, device="cuda"))
    assert torch.equal(want.cpu(), torch.argmax(x.float(), dim=1))
    for setting in ((1.0, 1, 1.0), (0.3, 1, 0.5), (1.0, 0, 1e-6), (2.0, 7, 1e-6)):
        toks, kept = _draw(xd, setting, 77, range(6))
        assert torch.equal(toks, want.cpu()[None].expand(6, -1)), setting
        assert bool((kept == 1).all()), setting


def test_planted_winner_at_every_cut():
    """One logit 40 above the rest (every other token together has probability below 1e-12): every draw returns it, wherever the launch plan
    cuts the row - index 0, V - 1, the first and last index of every chunk of the draw."""
    V, M = 3 * 4096 + 5, 32
    chunk = ops.sample_chunk(M, V)
    assert 0 < chunk < V and chunk % 4 == 0
    cols = {0, V - 1}
    for lo in range(0, V, chunk):
        cols |= {lo, min(lo + chunk, V) - 1}
    cols = sorted(cols)
    assert len(cols) >= 6
    x = sc.gpu_logits(V, torch.bfloat16, rows=len(cols), seed=3).float().clamp(-4, 4)
    for m, c in enumerate(cols):
        x[m, c] = 44.0
    x = x.to(torch.bfloat16)
    for setting in ((1.0, 0, 1.0), (0.7, 50, 0.9), (1.0, 3, 1.0)):
        toks, _ = _draw(x.cuda(), setting, 2024, range(8))
        assert torch.equal(toks, torch.tensor(cols)[None].expand(8, -1)), setting


def _binomial_interval(n, p, q=1e-6):
    """[lo, hi] with P(X < lo) <= q / 2 and P(X > hi) <= q / 2 for X ~ Binomial(n, p)."""
    logpmf = [math.lgamma(n + 1) - math.lgamma(i + 1) - math.lgamma(n - i + 1) + i * math.log(p) + (n - i) * math.log1p(-p) for i in range(n + 1)]
    pmf = [math.exp(v) for v in logpmf]
    lo, acc = 0, 0.0
    while acc + pmf[lo] <= q / 2:
        acc += pmf[lo]
        lo += 1
    hi, acc = n, 0.0
    while acc + pmf[hi] <= q / 2:
        acc += pmf[hi]
        hi -= 1
    return lo, hi


def test_top_k_keeps_exactly_the_top_two():
    """top_k = 2 with every other logit 2^-7 below the second: 4096 draws return the two only, split as their two-way softmax."""
    V, a, b = 5000, 1234, 4321
    row = torch.full((V,), 1.0 - 2.0 ** -7)
    row[a], row[b] = 2.0, 1.0
    x = row.to(torch.bfloat16)[None].expand(32, -1).contiguous()
    assert float(x[0, 0]) == 1.0 - 2.0 ** -7
    toks, kept = _draw(x.cuda(), (1.0, 2, 1.0), 31337, range(128))
    assert bool(((toks == a) | (toks == b)).all()) and bool((kept == 2).all())
    n = toks.numel()
    lo, hi = _binomial_interval(n, math.e / (1.0 + math.e))
    got = int((toks == a).sum())
    print(f"top-2 split: {got} of {n} (the 1e-6 interval is [{lo}, {hi}])")
    assert lo <= got <= hi


def test_exact_ties_at_the_cut_keep_the_lowest_indices():
    """300 equal bf16 values, the largest of the row, straddle top_k = 4: the four lowest indices stay, and each is drawn."""
    V = 9000
    g = torch.Generator().manual_seed(21)
    row = torch.randn(V, generator=g).clamp(-3, 0.5) - 8.0
    cols = torch.randperm(V, generator=g)[:300].sort().values
    row[cols] = 1.0
    x = row.to(torch.bfloat16)[None].expand(8, -1).contiguous()
    for setting in ((1.0, 4, 1.0), (0.5, 4, 0.999)):
        toks, kept = _draw(x.cuda(), setting, 5, range(50))
        assert bool((kept == 4).all()), setting
        assert sorted(set(toks.reshape(-1).tolist())) == cols[:4].tolist(), setting
    # the mass cut inside the tied value: the 300 equal tokens carry nearly all the mass, top_p = 0.1 keeps about a tenth of them
    ref = sc.SampleRef(x[:1], 1.0, 0, 0.1)
    n = int(ref.kept_count[0])
    assert 4 < n < 300 and sc.margin_to_top_p(ref) > 1e-4
    toks, kept = _draw(x.cuda(), (1.0, 0, 0.1), 6, range(50))
    assert bool((kept == n).all())
    assert set(toks.reshape(-1).tolist()) <= set(cols[:n].tolist())


@pytest.mark.parametrize("setting", [(0.7, 50, 1.0), (1.0, 0, 0.9)], ids=lambda s: "T%g-k%d-p%g" % s)
def test_drawn_frequencies(setting):
    """8192 draws (32 streams x 256 steps) of one row of 1000 logits under the chi-square rule of sample_check."""
    T, k, p = setting
    x = sc.gpu_logits(1000, torch.bfloat16, rows=1, seed=17)
    ref = sc.SampleRef(x, T, k, p)
    assert sc.margin_to_top_p(ref) > 2 * 4 * ref.e_m
    toks, kept = _draw(x.expand(32, -1).contiguous().cuda(), setting, 424242, range(256))
    assert bool((kept == int(ref.kept_count[0])).all())
    stat, bound, df = sc.chi2_check(toks, ref.probabilities()[0])
    print(f"{setting}: chi-square {stat:.1f} on {df} degrees of freedom (bound {bound:.1f})")
    assert stat < bound


def test_a_rows_draw_depends_on_its_logits_seed_step_and_stream_only():
    V = 4099
    x = sc.gpu_logits(V, torch.bfloat16, seed=8)
    setting, seed, steps = (0.9, 200, 0.95), 99, [0, 1, 7]
    xd = x.cuda()
    toks, kept = _draw(xd, setting, seed, steps)
    again, _ = _draw(xd, setting, seed, steps)
    assert torch.equal(toks, again)
    wide = _padded(x, 4200)
    for m in (0, 3, 31):
        one, k1 = _draw(xd[m: m + 1], setting, seed, steps, streams=[m])
        assert torch.equal(one[:, 0], toks[:, m]) and torch.equal(k1[:, 0], kept[:, m])
        other, _ = _draw(wide[m: m + 1], setting, seed, steps, streams=[m])
        assert torch.equal(other[:, 0], toks[:, m])
    rev, _ = _draw(xd.flip(0).contiguous(), setting, seed, steps, streams=list(range(31, -1, -1)))       # another row position
    assert torch.equal(rev.flip(1), toks)
    assert not torch.equal(_draw(xd, setting, seed + 1, steps)[0], toks)
    assert not torch.equal(_draw(xd, setting, seed, [s + 100 for s in steps])[0], toks)
    assert not torch.equal(_draw(xd, setting, seed, steps, streams=list(range(32, 64)))[0], toks)


def test_bad_arguments_are_refused_before_any_launch():
    V = 1000
    x = sc.gpu_logits(V, torch.bfloat16).cuda()
    out = torch.full((33,), -7, dtype=torch.int64, device="cuda")
    need = int(lib().v3d_sample_workspace_bytes(32, V))
    assert need > 0 and int(lib().v3d_sample_workspace_bytes(33, V)) == 0 and int(lib().v3d_sample_workspace_bytes(32, 1 << 27)) == 0
    ws = torch.empty(need, dtype=torch.uint8, device="cuda")
    p = lambda t: ctypes.c_void_p(t.data_ptr())       # noqa: E731

    def call(M=32, T=1.0, k=0, top_p=1.0, bytes_=need, dtype=ops.BF16):
        return lib().v3d_sample_rows(p(x), x.stride(0), M, V, dtype, T, k, top_p, 1, 0, None, p(out), None, p(ws), bytes_, None)

    for kw in (dict(T=0.0), dict(T=float("nan")), dict(T=float("inf")), dict(T=-1.0), dict(top_p=0.0), dict(top_p=1.5), dict(top_p=float("nan")),
               dict(k=-1), dict(M=33), dict(M=0), dict(bytes_=need - 1), dict(dtype=ops.F32)):
        assert call(**kw) < 0, kw
        assert len(lib().v3d_last_error()) > 0, kw
    torch.cuda.synchronize()
    assert bool((out == -7).all())                     # nothing ran
    with pytest.raises(V3DError):
        ops.sample_rows(x, out, ws, temperature=0.0)
    assert call() == 0
    torch.cuda.synchronize()
    assert bool(((out[:32] >= 0) & (out[:32] < V)).all()) and int(out[32]) == -7
