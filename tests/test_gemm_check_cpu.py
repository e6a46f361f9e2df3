"""The GEMM checker (tests/gemm_check.py) is neither loose nor wrong: an f32 emulation of the kernels' arithmetic passes it, and
emulations with one thing wrong fail it - under the bound on random inputs, or bit for bit on exact ones - where the rule it replaces
(err <= tol |want| + tol scale against an f32 torch chain) let the rounding and GELU mutants through.  No GPU: -m "not gpu".

The emulation follows gemm.hip: k in 32-wide blocks (one 16 x 16 x 32 MFMA each), one f32 add per block, optionally 2 .. 4 K-chunks
summed in f32 (the split-K tail); acc + bias rounded to 16 bit once; each epilogue on 16-bit inputs in f32, rounded once more.

Worst |err| / bound of the emulation over 64 x 256 outputs and all eight epilogues (the constants C_ACC = 2, C0 = 32 were settled here):
    K         64     320    3584   18944
    bf16    0.992   0.980   0.920   0.670
    f16     0.977   0.946   0.708   0.245
The exact family (bit-for-bit / interval check) rejects every mutant at every K in both dtypes.  The bound on random inputs also
rejects the structural ones everywhere (worst ratios from 10 at K = 18 944 to 1e5), and the rounding ones where the accumulation term
is smaller than one rounding: double rounding 62 / 7.4 / 0.97 (bf16, K = 320 / 3584 / 18 944) and 13.7 / 1.17 / 0.27 (f16), 16-bit
partials 92 / 7.4 / 1.30 and 11 / 1.27 / 0.21, truncation 1.94 / 1.85 / 1.13 and 1.92 / 1.30 / 0.30.  The GELU swap (0.4 .. 1.0) and
the unrounded silu (0.1 .. 0.6) are inside the bound at every K - each is within one rounding of the truth - and are carried by the
exact family alone.
"""
import pytest
import torch

import gemm_check as gc
from gemm_check import (EPI_BIAS, EPI_BIAS_GELU_ERF, EPI_BIAS_GELU_TANH, EPI_BIAS_RELU, EPI_BIAS_RES, EPI_NONE, EPI_RES, EPI_SWIGLU)

DT = {"bf16": torch.bfloat16, "f16": torch.float16}
M, N = 64, 256
KS = (64, 320, 3584, 18944)
RES_MOD = 5


def trunc16(x, dt):
    """f32 -> 16 bit by truncation (toward zero) -> f32."""
    r = x.to(dt)
    over = r.float().abs() > x.abs()
    return torch.where(over, torch.nextafter(r, torch.zeros_like(r)), r).float()


def f_gelu_erf(x):
    return 0.5 * x * (1.0 + torch.erf(x * 0.70710678118654752440))


def f_gelu_tanh(x):
    k = -2.0 * 0.7978845608028654 * 1.4426950408889634
    z = x * (k * 0.044715 * (x * x) + k)
    return x / (1.0 + torch.exp2(z))


def f_silu(x):
    return x / (1.0 + torch.exp2(-1.4426950408889634 * x))


def emulate(a, w, bias, res, epi, res_mod=0, mut=None, split=1):
    """Kernel arithmetic in f32 on the CPU -> [M, n_out] 16 bit.  mut names the one thing done wrong."""
    dt = a.dtype
    af, wf = a.float().clone(), w.float().clone()
    Mm, K = af.shape
    if mut == "drop_k":                       # one k term missing
        af[:, K // 2 + 5] = 0
    elif mut == "drop_frag":                  # one 8-wide fragment missing
        af[:, K // 2 + 8: K // 2 + 16] = 0
    elif mut == "kstep_twice":                # K-step 0 read again in place of K-step 1 (a stale ring slot)
        af[:, 64:128] = af[:, 0:64]
        wf[:, 64:128] = wf[:, 0:64]
    nb = K // 32
    cuts = [32 * (c * nb // split) for c in range(split + 1)]
    parts = []
    for c in range(split):
        acc = torch.zeros(Mm, wf.shape[0])
        for k in range(cuts[c], cuts[c + 1], 32):
            acc = acc + af[:, k:k + 32] @ wf[:, k:k + 32].T
        parts.append(acc.to(dt).float() if mut == "partials16" else acc)
    acc = parts[0]
    for p in parts[1:]:
        acc = acc + p
    to16 = (lambda x: trunc16(x, dt)) if mut == "trunc" else (lambda x: x.to(dt).float())
    b = bias.float() if epi in gc.HAS_BIAS else torch.zeros(wf.shape[0])
    if mut == "bias_n1":
        b = torch.roll(b, -1)
    yr = to16(to16(acc) + b) if mut == "double_round" else to16(acc + b)
    if epi in (EPI_NONE, EPI_BIAS):
        out = yr
    elif epi in (EPI_BIAS_RES, EPI_RES):
        idx = torch.arange(Mm)
        idx = (idx + (1 if mut == "res_mod_off" else 0)) % res_mod if res_mod > 0 else idx
        out = to16(yr + res.float()[idx])
    elif epi == EPI_BIAS_RELU:
        out = yr if mut == "no_relu" else yr.clamp_min(0)
    elif epi in (EPI_BIAS_GELU_ERF, EPI_BIAS_GELU_TANH):
        erf = (epi == EPI_BIAS_GELU_ERF) != (mut == "gelu_swap")
        out = to16(f_gelu_erf(yr) if erf else f_gelu_tanh(yr))
    else:
        g, u = gc.split_gate_up(yr)
        if mut == "gate_up_swapped":
            g, u = u, g
        s = f_silu(g)
        out = to16((s if mut == "silu_unrounded" else to16(s)) * u)
    return out.to(dt)


def inputs(family, K, dt, epi, seed=0):
    if family == "random":
        a, w, b, r = gc.random_inputs(M, N, K, dt, seed=seed + K, res_rows=RES_MOD)
    else:
        target = 2.0 if epi in (EPI_BIAS_GELU_ERF, EPI_BIAS_GELU_TANH, EPI_SWIGLU) else None
        a, w, b, r = gc.exact_inputs(M, N, K, dt, seed=seed + K, target=target, res_rows=RES_MOD)
    return a, w, b, r


def verdict(out, a, w, b, r, epi, family):
    c = gc.compare(out, a, w, b, r, epi, RES_MOD, exact=family == "exact")
    return c, (c["ratio"] > 1.0 if family == "random" else c["outside"] > 0)


@pytest.mark.parametrize("kind", ["bf16", "f16"])
@pytest.mark.parametrize("K", KS)
def test_emulation_is_inside_the_bound_and_exact_on_exact_inputs(kind, K):
    dt = DT[kind]
    worst = 0.0
    for epi in range(8):
        for split in ((1, 3) if K >= 320 else (1,)):
            a, w, b, r = inputs("random", K, dt, epi)
            c, rejected = verdict(emulate(a, w, b, r, epi, RES_MOD, split=split), a, w, b, r, epi, "random")
            assert not rejected, f"{gc.EPI_NAMES[epi]} split {split}: ratio {c['ratio']}"
            worst = max(worst, c["ratio"])
            a, w, b, r = inputs("exact", K, dt, epi)
            c, rejected = verdict(emulate(a, w, b, r, epi, RES_MOD, split=split), a, w, b, r, epi, "exact")
            assert not rejected and c["ratio"] <= 1.0, f"exact {gc.EPI_NAMES[epi]} split {split}: {c}"
            if epi in gc.EXACT_EPIS:
                assert c["unequal"] == 0
    print(f"emulation {kind} K={K}: worst ratio {worst:.3f}")
    assert worst > 0.1 or K > 4000, "the bound is far from the emulation: loose"


# mutant -> (epilogue it is applied to, K-chunks, smallest K it applies to)
MUTANTS = {
    "drop_k": (EPI_BIAS, 1, 64),
    "drop_frag": (EPI_BIAS, 1, 64),
    "kstep_twice": (EPI_NONE, 1, 128),
    "double_round": (EPI_BIAS, 1, 64),
    "partials16": (EPI_BIAS, 3, 320),
    "trunc": (EPI_BIAS, 1, 64),
    "gelu_swap": (EPI_BIAS_GELU_ERF, 1, 64),
    "gelu_swap_tanh": (EPI_BIAS_GELU_TANH, 1, 64),
    "silu_unrounded": (EPI_SWIGLU, 1, 64),
    "no_relu": (EPI_BIAS_RELU, 1, 64),
    "res_mod_off": (EPI_BIAS_RES, 1, 64),
    "gate_up_swapped": (EPI_SWIGLU, 1, 64),
    "bias_n1": (EPI_BIAS, 1, 64),
}
# The families that must reject each mutant at every K it applies to (so no mutant goes unrejected anywhere).
CARRIER = {
    "drop_k": "random+exact", "drop_frag": "random+exact", "kstep_twice": "random+exact", "no_relu": "random+exact",
    "res_mod_off": "random+exact", "gate_up_swapped": "random+exact", "bias_n1": "random+exact",
    "double_round": "exact", "partials16": "exact", "trunc": "exact", "gelu_swap": "exact", "gelu_swap_tanh": "exact", "silu_unrounded": "exact",
}


@pytest.mark.parametrize("kind", ["bf16", "f16"])
@pytest.mark.parametrize("K", KS)
def test_every_mutant_is_rejected_by_the_family_named_for_it(kind, K):
    dt = DT[kind]
    for name, (epi, split, kmin) in MUTANTS.items():
        if K < kmin:
            continue
        mut = "gelu_swap" if name == "gelu_swap_tanh" else name
        hit = {}
        for family in ("random", "exact"):
            a, w, b, r = inputs(family, K, dt, epi)
            c, hit[family] = verdict(emulate(a, w, b, r, epi, RES_MOD, mut=mut, split=split), a, w, b, r, epi, family)
            print(f"{name} {kind} K={K} {family}: ratio {c['ratio']:.2f} outside {c['outside']} rejected {hit[family]}")
        want = CARRIER[name]
        for family in want.split("+"):
            assert hit[family], f"{name} at K = {K} ({kind}) is not rejected by the {family} family"


@pytest.mark.parametrize("kind", ["bf16", "f16"])
def test_the_old_rule_accepts_the_rounding_and_gelu_mutants(kind):
    """What tests/test_gpu_gemm.py's rule let through on its own inputs (M x 256 x K, randn * 0.5 and * 0.05 / 0.08): documents what
    the new checks replace."""
    dt = DT[kind]
    for K in (320, 3584):
        for name in ("double_round", "partials16", "trunc", "gelu_swap", "gelu_swap_tanh", "silu_unrounded"):
            epi, split, _ = MUTANTS[name]
            a, w, b, r = gc.random_inputs(M, N, K, dt, seed=K, res_rows=RES_MOD)
            lin = (a.float() @ w.float().T + (b.float() if epi in gc.HAS_BIAS else 0.0)).to(dt).float()
            if epi == EPI_BIAS_GELU_ERF:
                want = torch.nn.functional.gelu(lin).to(dt)
            elif epi == EPI_BIAS_GELU_TANH:
                want = torch.nn.functional.gelu(lin, approximate="tanh").to(dt)
            elif epi == EPI_SWIGLU:
                g, u = gc.split_gate_up(lin)
                want = (torch.nn.functional.silu(g).to(dt).float() * u).to(dt)
            else:
                want = lin.to(dt)
            scale = None if epi == EPI_BIAS else (0.5 if epi == EPI_SWIGLU else 1.0)
            out = emulate(a, w, b, r, epi, RES_MOD, mut="gelu_swap" if name == "gelu_swap_tanh" else name, split=split)
            assert gc.old_rule_ok(out, want, dt, scale), f"{name} K = {K}: the old rule rejected it after all"


@pytest.mark.parametrize("kind", ["bf16", "f16"])
def test_gather_names_the_k_that_was_read(kind):
    dt = DT[kind]
    for transposed in (False, True):
        a, w, want = gc.gather_inputs(200, 128, 192, dt, stride=5, shift=3, transposed=transposed)
        out = emulate(a, w, None, None, EPI_NONE)
        assert torch.equal(out, want)                                     # an honest kernel returns the selected values bit for bit
        a2 = a.clone()
        a2[:, 64:128] = a[:, 0:64]                                         # K-step 1 reads K-step 0's A image
        bad = emulate(a2, w, None, None, EPI_NONE)
        assert not torch.equal(bad, want)
        text = gc.gather_explain(bad, a, w, want, transposed)
        assert "outputs differ" in text and "k = " in text
    k0 = gc.gather_k0(192, 192, stride=5, shift=3)
    assert k0.unique().numel() == 192                                     # M >= K with an odd stride: every k is addressed by some row
