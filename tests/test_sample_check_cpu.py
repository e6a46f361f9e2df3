"""tests/sample_check.py, the sampler's specification and rules, checked on the CPU: Philox4x32-10's known answers (the Python restatement and
the library's), SampleRef's kept set against transformers' three warpers, the host twin under check_draws and under the chi-square rule, the
inputs of the GPU kernel tests shown usable, and eight planted faults that the rules must reject.

Against transformers.  TemperatureLogitsWarper, TopKLogitsWarper and TopPLogitsWarper(min_tokens_to_keep=1) are applied to f64 scores, in
that order, a warper left out where generate would not build it (top_k == 0, top_p == 1).  On tie-free rows the kept sets are equal.  With
equal values at the cut transformers leaves the choice open (TopK keeps every token equal to the k-th value, TopP an unstable sort's pick):
there the kept COUNT is compared for the top-p-only settings, and SampleRef's kept tokens of the cut value must be its lowest indices."""
import math

import pytest
import torch

import sample_check as sc
from v3d import ops
from v3d._native import V3DError


def test_philox_known_answers():
    for counter, key, want in sc.PHILOX_KNOWN:
        assert sc.philox4x32_10(counter, key) == want
        assert tuple(ops.philox4x32_10_host(counter, key)) == want
    seed = 0x0123456789ABCDEF
    w = sc.row_words(41, 3, [5, 0x7FFFFFFF], seed)
    assert torch.equal(w, sc.token_words(torch.arange(41), 3, torch.tensor([[5], [0x7FFFFFFF]]), seed))
    for b, s in enumerate((5, 0x7FFFFFFF)):
        for i in (0, 1, 2, 3, 4, 39, 40):
            assert int(w[b, i]) == sc.philox4x32_10((i >> 2, 3, s, 0), (seed & sc.MASK, seed >> 32))[i & 3]
            assert int(w[b, i]) == ops.philox4x32_10_host((i >> 2, 3, s, 0), (seed & sc.MASK, seed >> 32))[i & 3]
    # the two branches of the f32 Gumbel meet the f64 one: the ends of the 24-bit grid and its middle
    n = torch.tensor([0, 1, (1 << 23) - 1, 1 << 23, (1 << 24) - 2, (1 << 24) - 1]) << 8
    assert float((sc.gumbel32(n).double() - sc.gumbel64(n)).abs().max()) < 4e-6 and bool(torch.isfinite(sc.gumbel32(n)).all())


def _hf_kept(x, T, k, p):
    from transformers.generation.logits_process import TemperatureLogitsWarper, TopKLogitsWarper, TopPLogitsWarper
    s = x.double()
    s = TemperatureLogitsWarper(float(T))(None, s)
    if k > 0:
        s = TopKLogitsWarper(top_k=int(k))(None, s)
    if p < 1.0:
        s = TopPLogitsWarper(top_p=float(p), min_tokens_to_keep=1)(None, s)
    return torch.isfinite(s)


@pytest.mark.parametrize("setting", sc.SETTINGS, ids=lambda s: "T%g-k%d-p%g" % s)
def test_kept_set_is_what_transformers_warpers_keep(setting):
    T, k, p = setting
    g = torch.Generator().manual_seed(100)
    x = torch.randn(6, 700, generator=g) * 2.0
    assert all(x[m].unique().numel() == 700 for m in range(6))                 # tie-free
    ref = sc.SampleRef(x, T, k, p)
    assert torch.equal(ref.kept, _hf_kept(x, T, k, p))
    assert bool((ref.kept_count >= 1).all()) and (k == 0 or bool((ref.kept_count <= k).all()))
    # equal values at the cut: rows of whole numbers whose largest value, 2, is shared by about a sixth of the tokens
    xt = (torch.randn(6, 700, generator=g) * 2.0).round_().clamp_(max=2.0)
    assert all(int((xt[m] == 2.0).sum()) > 60 for m in range(6))
    ref = sc.SampleRef(xt, T, k, p)
    if k == 0:
        assert torch.equal(ref.kept_count, _hf_kept(xt, T, k, p).sum(1))
    ties_cut = 0
    for m in range(6):
        cut = xt[m][ref.kept[m]].min()
        same = (xt[m] == cut).nonzero()[:, 0]
        n = int(ref.kept[m][same].sum())
        assert ref.kept[m][same[:n]].all() and not ref.kept[m][same[n:]].any()   # the lowest indices of the cut value
        ties_cut += int(n < same.numel())
        assert bool(ref.kept[m][xt[m] > cut].all()) and not bool(ref.kept[m][xt[m] < cut].any())
    assert ties_cut > 0 or (k == 0 and p == 1.0), "no row had its cut inside a run of equal values"


@pytest.mark.parametrize("setting", sc.SETTINGS, ids=lambda s: "T%g-k%d-p%g" % s)
def test_twin_passes_check_draws(setting):
    T, k, p = setting
    for V, dtype in ((1000, torch.bfloat16), (4099, torch.float16)):
        x = sc.gpu_logits(V, dtype, rows=5)
        streams = [0, 1, 2, 70000, 4]
        got = [ops.sample_rows_host(x.float(), T, k, p, sc.GPU_SEED, step, streams) for step in range(sc.GPU_STEPS)]
        toks, kept = torch.stack([g[0] for g in got]), torch.stack([g[1] for g in got])
        r = sc.check_draws(toks, kept, x, dict(T=T, top_k=k, top_p=p, seed=sc.GPU_SEED, streams=streams), what=f"twin V={V} {setting}")
        assert len(r["excused"]) * 200 <= r["n"]
    with pytest.raises(V3DError):
        ops.sample_rows_host(x.float(), 0.0, k, p)
    with pytest.raises(V3DError):
        ops.sample_rows_host(x.float(), T, -1, p)


def _usable(V, dtypes, steps, rows=32):
    """The GPU inputs at vocabulary V: no token's mass within 2 * bound_m of top_p, and the torch-f32 evaluation of the rule (f32 keys, the f64
    kept set) names the f64 winner in all but 1 draw of 200.  The Philox words of a step are formed once for every dtype and setting."""
    cases = []
    for dtype in dtypes:
        x = sc.gpu_logits(V, dtype, rows=rows)
        for T, k, p in sc.SETTINGS:
            ref = sc.SampleRef(x, T, k, p)
            margin = sc.margin_to_top_p(ref)
            assert margin > 2 * 4 * ref.e_m, (dtype, V, (T, k, p), margin, ref.e_m)
            cases.append([(dtype, (T, k, p)), ref.z, ref.z32, ref.kept, 0])
            del ref
    for step in range(steps):
        w = sc.row_words(V, step, range(rows), sc.GPU_SEED)
        g64, g32 = sc.gumbel64(w), sc.gumbel32(w)
        for c in cases:
            _, z, z32, kept, _ = c
            c[4] += int((sc.SampleRef.winner(z + g64, kept) != sc.SampleRef.winner((z32 + g32).double(), kept)).sum())
    for name, _, _, _, missed in cases:
        assert missed * 200 <= steps * rows, (V, name, missed)


@pytest.mark.parametrize("V", [v for v, _ in sc.GPU_SHAPES])
def test_gpu_inputs_are_usable(V):
    _usable(V, (torch.bfloat16, torch.float16), sc.GPU_STEPS)


def test_gpu_inputs_at_the_models_vocabulary_are_usable():
    V = 152064
    x = sc.gpu_logits(V, torch.bfloat16)
    for T, k, p in ((1.0, 0, 1.0), (0.7, 50, 0.9)):
        ref = sc.SampleRef(x, T, k, p)
        assert sc.margin_to_top_p(ref) > 2 * 4 * ref.e_m
        missed = 0
        for step in range(8):
            k64, k32 = ref.keys(step, range(32), sc.GPU_SEED)
            missed += int((ref.winner(k64, ref.kept) != ref.winner(k32.double(), ref.kept)).sum())
        assert missed * 200 <= 8 * 32


CHI_SETTINGS = [(1.0, 0, 1.0), (0.7, 20, 1.0), (1.3, 0, 0.9)]


def _chi_row():
    g = torch.Generator().manual_seed(64)
    return (torch.randn(1, 64, generator=g) * 1.5).to(torch.bfloat16)


def _many_draws(x, setting, n, draw):
    """n draws of the one row x as 32 streams x n / 32 steps; draw(rows [32, V], step, streams) -> tokens [32]"""
    rows = x.expand(32, -1).contiguous()
    return torch.stack([draw(rows, step, list(range(32))) for step in range(n // 32)])


@pytest.mark.parametrize("setting", CHI_SETTINGS, ids=lambda s: "T%g-k%d-p%g" % s)
def test_twin_draws_follow_the_warped_softmax(setting):
    """200 000 draws of the twin at V = 64 against the f64 warped softmax: Pearson chi-square, bins pooled to an expectation of 5, below the
    upper 1e-6 quantile."""
    T, k, p = setting
    x = _chi_row()
    ref = sc.SampleRef(x, T, k, p)
    assert sc.margin_to_top_p(ref) > 2 * 4 * ref.e_m
    toks = _many_draws(x, setting, 200000, lambda rows, step, streams: ops.sample_rows_host(rows.float(), T, k, p, 2718281828, step, streams)[0])
    stat, bound, df = sc.chi2_check(toks, ref.probabilities()[0])
    print(f"{setting}: chi-square {stat:.1f} on {df} degrees of freedom (bound {bound:.1f})")
    assert df >= 5 and stat < bound


def test_chi_square_quantile():
    """Wilson-Hilferty against the exact upper 1e-6 quantiles of chi-square (10 df 46.863, 50 df 112.608, 200 df 309.838): within 2.5 %,
    0.5 % from 50 degrees of freedom on."""
    for df, want, tol in ((10, 46.863, 0.025), (50, 112.608, 0.005), (200, 309.838, 0.005)):
        assert abs(sc.chi2_quantile_upper(df) - want) / want < tol


FAULTS = ["no_temperature", "p_before_k", "p_inclusive", "shared_u", "no_stream", "no_step", "no_outer_log", "ties_high"]


@pytest.mark.parametrize("fault", FAULTS)
def test_planted_faults_are_rejected(fault):
    """Each fault is planted in a copy of the rule (SampleRef(mutant=...)); check_draws or the chi-square rule must refuse its draws, and
    pass the draws of the rule itself on the same inputs."""
    V, T, k, p, seed = 64, 0.6, 12, 0.8, 99
    g = torch.Generator().manual_seed(7)
    if fault == "ties_high":                                   # equal values across the top-k cut
        x = (torch.randn(1, V, generator=g) * 1.5).to(torch.bfloat16).float().round_().to(torch.bfloat16)
    elif fault == "p_inclusive":                               # two equal halves: m_1 = 0.5 = top_p exactly
        x = torch.full((1, V), -300.0)
        x[0, 5] = x[0, 40] = 2.0
        x, T, k, p = x.to(torch.bfloat16), 1.0, 0, 0.5
    else:
        x = (torch.randn(1, V, generator=g) * 1.5).to(torch.bfloat16)
    rows = x.expand(32, -1).contiguous()
    streams = list(range(32))
    good, bad = sc.SampleRef(rows, T, k, p), sc.SampleRef(rows, T, k, p, mutant=fault)
    args = dict(T=T, top_k=k, top_p=p, seed=seed)

    def verdict(ref):
        toks = torch.stack([ref.draw(step, streams, seed) for step in range(128)])           # 4096 draws
        try:
            sc.check_draws(toks, None, rows, args, what=fault, ref=good)
        except AssertionError:
            return False
        stat, bound, _ = sc.chi2_check(toks, good.probabilities()[0])
        return stat < bound

    assert verdict(good), "the rule's own draws were refused"
    assert not verdict(bad), f"the planted fault {fault!r} went unnoticed"


def test_chi2_check_pools_and_refuses():
    probs = torch.tensor([0.5, 0.3, 0.15, 0.04, 0.0095, 0.0005], dtype=torch.float64)
    g = torch.Generator().manual_seed(1)
    toks = torch.multinomial(probs, 5000, replacement=True, generator=g)
    stat, bound, df = sc.chi2_check(toks, probs)
    assert df == 4 and stat < bound                                              # the last token expects 2.5 draws: it joins the bin before it
    stat, bound, _ = sc.chi2_check(torch.multinomial(torch.tensor([0.4, 0.4, 0.15, 0.04, 0.0095, 0.0005]), 5000, replacement=True, generator=g), probs)
    assert stat > bound
    assert math.isinf(sc.chi2_check(torch.tensor([0, 0, 1]), torch.tensor([1.0, 0.0], dtype=torch.float64))[0])
