"""The decode-linear checker (tests/decode_check.py) is neither loose nor wrong: an f32 emulation of each kernel form's arithmetic, with
its real grouping, passes it, and emulations with one thing wrong fail it on the exact or the gather family.  No GPU: -m "not gpu".

Emulations (decode.hip), all in f32 on 16-bit inputs (a product of two 16-bit numbers is exact in f32, so s + a * b is the fma):
  valu      thread t sums the 8-element chunks t, t + 256, ... in order, 8 fmas per chunk; xor butterfly 32 .. 1 inside each wave; the
            four wave sums added in order
  mfma      128-element tile s goes to wave s % 8, a wave adds its tiles in ascending order (four 32-wide MFMAs each: one f32 add per
            MFMA, the 32 products inside it taken as an f32 dot product); the eight slices are added in order 0 .. 7.  The r04,
            persistent and streaming kernels all promise this order.
  split     K cut into C chunks of hi or hi - 1 tiles (dc.split_plan), each summed like `mfma` from its own tile 0; the f32 chunk sums
            are added in ascending order (decode_combine_kernel)
  fp8_valu  16-element chunks, 16 fmas per chunk, otherwise `valu`;  fp8_mfma: 256-element tiles of eight MFMAs, otherwise `mfma`;
            both multiply the f32 sum by sw[n] once, then add the bias
then acc (+ bias) rounded to 16 bit once; + res rounded once more; SwiGLU round(round(silu(gate16)) * up16).

Worst |err| / bound of the emulation on the random family (M = 4 rows for the VALU forms, 20 for the others, 128 weight rows, all four
epilogues; the K-split at K = 4224 and 18944, e4m3 matrix core at K = 18944 only - the forms' own shape rules):
    K            64     1152    4224    18944
    bf16       0.990   0.965   0.906    0.661
    f16        0.957   0.829   0.592    0.218
and the exact family comes back bit for bit (interval for SwiGLU) everywhere.

Mutants, each rejected by the exact family at every K it applies to (E), by the gather family (G), and what the rule these checks replace
(tests/test_gpu_llm_ops.py: |err| <= 2^-7 |ref| + 2^-8 rms(ref), SwiGLU 2^-6 and 2^-6, on randn x, randn * 0.05 weights, bf16) says to
the same emulation at K = 1152 / 4224 / 18944 (A = accepted, r = rejected, - = does not apply at that K):
    mutant                                          new     old rule
    last_tile        a wave's last tile dropped      E G     r r r
    chunk256         the tid + 256 chunk dropped     E G     - r r
    split_early      K-split boundary a tile early   E G     - r r
    bias_late        bias after the output rounding  E       A A A
    res_early        residual before it              E       A A A
    swiglu_unrounded gate / up not rounded           E       A A A
    gate_up_swapped                                  E       r r r
    row0             row m answered from row 0       E G     r r r
    partial16        16-bit K-split partial          E       - A r
    scale_n1         e4m3 scale of row n + 1         E G     r r r
    scale_late       e4m3 scale after the bias       E       r r r
(G is asserted only where the one-hot element can meet the fault: the structural mutants.)  The old rule accepts the rounding-point
mutants bias_late, res_early and swiglu_unrounded at every K and the 16-bit partial at K = 4224; it rejects the structural ones here
because a whole tile or chunk is missing - a single dropped k element (one product of about 0.05 against an rms term of 0.027 at
K = 18944) is what it lets through, and what the gather family names.
"""
import pytest
import torch

import decode_check as dc
import gemm_check as gc
from decode_check import DEC_BIAS, DEC_NONE, DEC_RES, DEC_SWIGLU

DT = {"bf16": torch.bfloat16, "f16": torch.float16}
KS = (64, 1152, 4224, 18944)
N = 128
CUS = 256
WORST = {}


def f_silu(x):
    return x / (1.0 + torch.exp(-x))


def _valu_sum(xf, wf, chunk, mut):
    """[M, N] f32: the VALU form's sum (chunk = 8 elements for 16-bit weights, 16 for e4m3)."""
    M, K = xf.shape
    span = 256 * chunk
    rounds = -(-K // span)
    pad = rounds * span - K
    x = torch.nn.functional.pad(xf, (0, pad)).reshape(M, 1, rounds, 256, chunk)
    w = torch.nn.functional.pad(wf, (0, pad)).reshape(1, wf.shape[0], rounds, 256, chunk)
    s = torch.zeros(M, wf.shape[0], 256)
    for i in range(rounds):
        if mut == "chunk256" and i == 1:
            continue
        for j in range(chunk):
            s = s + x[:, :, i, :, j] * w[:, :, i, :, j]
    s = s.reshape(M, wf.shape[0], 4, 64)
    lane = torch.arange(64)
    for off in (32, 16, 8, 4, 2, 1):
        s = s + s[..., lane ^ off]
    r = s[..., 0]
    return ((r[..., 0] + r[..., 1]) + r[..., 2]) + r[..., 3]


def _mfma_sum(xf, wf, tile, mut=None):
    """[M, N] f32: tile s -> wave s % 8 ascending, 32-wide MFMAs, eight slices in order."""
    M, K = xf.shape
    tiles = K // tile
    part = [torch.zeros(M, wf.shape[0]) for _ in range(8)]
    for s in range(tiles):
        if mut == "last_tile" and s == tiles - 1:
            continue
        for k in range(s * tile, (s + 1) * tile, 32):
            part[s % 8] = part[s % 8] + xf[:, k:k + 32] @ wf[:, k:k + 32].T
    v = torch.zeros(M, wf.shape[0])
    for p in part:
        v = v + p
    return v


def _split_sum(xf, wf, dt, mut):
    K = xf.shape[1]
    C, hi, n_hi, _ = dc.split_plan(K // 128, N // 16, CUS)
    y = torch.zeros(xf.shape[0], wf.shape[0])
    for c in range(C):
        t0 = c * hi if c < n_hi else n_hi * hi + (c - n_hi) * (hi - 1)
        ct = hi if c < n_hi else hi - 1
        if mut == "split_early" and c == 1:
            t0 -= 1                          # tile t0 - 1 summed twice, the chunk's last tile missed
        p = _mfma_sum(xf[:, 128 * t0:128 * (t0 + ct)], wf[:, 128 * t0:128 * (t0 + ct)], 128, "last_tile" if mut == "last_tile" and c == C - 1 else None)
        y = y + (p.to(dt).float() if mut == "partial16" else p)
    return y


def emulate(form, x, w, bias, res, epi, mut=None, sw=None):
    """Kernel arithmetic in f32 on the CPU -> [M, n_out] 16 bit.  w: 16-bit weights, or the e4m3 codes' values as f32 with sw [N]."""
    dt = x.dtype
    xf, wf = x.float(), w.float()
    if form in ("valu", "fp8_valu"):
        acc = _valu_sum(xf, wf, 8 if form == "valu" else 16, mut)
    elif form in ("mfma", "fp8_mfma"):
        acc = _mfma_sum(xf, wf, 128 if form == "mfma" else 256, mut)
    else:
        acc = _split_sum(xf, wf, dt, mut)
    to16 = lambda t: t.to(dt).float()                                   # noqa: E731
    b = bias.float() if epi == DEC_BIAS else torch.zeros(wf.shape[0])
    if sw is not None:
        s = torch.roll(sw, -1) if mut == "scale_n1" else sw
        acc = (acc + b) * s if mut == "scale_late" else acc * s + b
    else:
        acc = acc + (0.0 if mut == "bias_late" else b)
    if mut == "row0":
        acc[-1] = acc[0]
    if epi == DEC_SWIGLU:
        g, u = gc.split_gate_up(acc if mut == "swiglu_unrounded" else to16(acc))
        if mut == "gate_up_swapped":
            g, u = u, g
        return (to16(f_silu(g)) * u).to(dt)
    if epi == DEC_RES:
        return (to16(acc + res.float()) if mut == "res_early" else to16(to16(acc) + res.float())).to(dt)
    if mut == "bias_late":
        return to16(to16(acc) + b).to(dt)
    return acc.to(dt)


def applies(form, K):
    if form in ("valu", "fp8_valu"):
        return True
    if form == "mfma":
        return K % 128 == 0
    if form == "fp8_mfma":
        return K % 256 == 0
    return K % 128 == 0 and K // 128 > 32                           # split


def rows(form):
    return 4 if form.endswith("valu") else 20


def make(form, family, K, dt, epi, seed=0):
    """-> x, w (values as the emulation multiplies them), bias, res, sw or None, and the reference's weights (f64 for e4m3)."""
    M = rows(form)
    target = 2.0 if epi == DEC_SWIGLU else None
    if form.startswith("fp8"):
        if family == "exact":
            x, q, sw, b, r = dc.exact_inputs_fp8(M, N, K, dt, seed=seed + K, target=target)
        else:
            x, q, sw, b, r = dc.random_inputs_fp8(M, N, K, dt, seed=seed + K)
        return x, q.view(torch.float8_e4m3fn).float(), b, r, sw, dc.dequant(q, sw)
    if family == "exact":
        x, w, b, r = gc.exact_inputs(M, N, K, dt, seed=seed + K, target=target)
    else:
        x, w, b, r = gc.random_inputs(M, N, K, dt, seed=seed + K)
    return x, w, b, r, None, w


def verdict(out, x, wref, b, r, epi, family, fp8):
    c = gc.compare(out, x, wref, b, r, dc.GEMM_EPI[epi], exact=family == "exact", lin_rel=dc.FP8_LIN_REL if fp8 else 0.0)
    return c, (c["ratio"] > 1.0 if family == "random" else c["outside"] > 0)


FORMS = ("valu", "mfma", "split", "fp8_valu", "fp8_mfma")


@pytest.mark.parametrize("kind", ["bf16", "f16"])
@pytest.mark.parametrize("K", KS)
def test_emulation_is_inside_the_bound_and_exact_on_exact_inputs(kind, K):
    dt = DT[kind]
    worst = 0.0
    for form in FORMS:
        if not applies(form, K):
            continue
        for epi in (DEC_NONE, DEC_BIAS, DEC_RES, DEC_SWIGLU):
            if form == "split" and epi == DEC_SWIGLU:
                continue
            fp8 = form.startswith("fp8")
            x, w, b, r, sw, wref = make(form, "random", K, dt, epi)
            c, rejected = verdict(emulate(form, x, w, b, r, epi, sw=sw), x, wref, b, r, epi, "random", fp8)
            assert not rejected and c["ratio"] < 1.0, f"{form} {dc.DEC_NAMES[epi]}: ratio {c['ratio']}"
            worst = max(worst, c["ratio"])
            x, w, b, r, sw, wref = make(form, "exact", K, dt, epi)
            c, rejected = verdict(emulate(form, x, w, b, r, epi, sw=sw), x, wref, b, r, epi, "exact", fp8)
            assert not rejected and c["ratio"] <= 1.0, f"exact {form} {dc.DEC_NAMES[epi]}: {c}"
            if epi != DEC_SWIGLU:
                assert c["unequal"] == 0, f"exact {form} {dc.DEC_NAMES[epi]}: {c}"
    print(f"DECODECHK emulation {kind} K={K}: worst ratio {worst:.3f}")
    assert worst > 0.1, "the bound is far from the emulation: loose"


# mutant -> (form, epilogue, applies at K, the gather family must reject it too)
MUTANTS = {
    "last_tile": ("mfma", DEC_NONE, lambda K: K % 128 == 0, True),
    "chunk256": ("valu", DEC_NONE, lambda K: K > 2048, True),
    "split_early": ("split", DEC_NONE, lambda K: applies("split", K), True),
    "bias_late": ("mfma", DEC_BIAS, lambda K: K % 128 == 0, False),
    "res_early": ("mfma", DEC_RES, lambda K: K % 128 == 0, False),
    "swiglu_unrounded": ("mfma", DEC_SWIGLU, lambda K: K % 128 == 0, False),
    "gate_up_swapped": ("mfma", DEC_SWIGLU, lambda K: K % 128 == 0, False),
    "row0": ("mfma", DEC_NONE, lambda K: K % 128 == 0, True),
    "partial16": ("split", DEC_BIAS, lambda K: applies("split", K), False),
    "scale_n1": ("fp8_valu", DEC_NONE, lambda K: True, True),
    "scale_late": ("fp8_valu", DEC_BIAS, lambda K: True, False),
}
# the VALU mutants of the rounding points run on the VALU emulation where K is no multiple of 128
VALU_AT_64 = ("bias_late", "res_early", "swiglu_unrounded", "gate_up_swapped", "row0")


def gather_rejects(form, K, dt, mut):
    """Both orientations with the one-hot element placed where the mutant bites (the last tile / the second chunk round / the tile the early
    boundary misses; rows 0 and M - 1 select different k) -> True if either orientation differs from the selected values."""
    M = rows(form)
    if mut == "split_early":
        C, hi, n_hi, _ = dc.split_plan(K // 128, N // 16, CUS)
        shift = 128 * (hi + (hi if 1 < n_hi else hi - 1) - 1) + 5      # chunk 1's last tile
    elif mut == "chunk256":
        shift = 2048 + 5
    else:
        shift = K - 60
    hit = False
    for transposed in (False, True):
        if form.startswith("fp8"):
            x, q, sw, want, _ = dc.gather_inputs_fp8(M, N, K, dt, stride=1, shift=shift, transposed=transposed)
            out = emulate(form, x, q.view(torch.float8_e4m3fn).float(), None, None, DEC_NONE, mut=mut, sw=sw)
            good = emulate(form, x, q.view(torch.float8_e4m3fn).float(), None, None, DEC_NONE, sw=sw)
        else:
            x, w, want = gc.gather_inputs(M, N, K, dt, stride=1, shift=shift, transposed=transposed)
            out = emulate(form, x, w, None, None, DEC_NONE, mut=mut)
            good = emulate(form, x, w, None, None, DEC_NONE)
        assert torch.equal(good, want), f"{form}: the honest emulation does not return the selected values ({'transposed' if transposed else 'plain'})"
        hit = hit or not torch.equal(out, want)
    return hit


@pytest.mark.parametrize("kind", ["bf16", "f16"])
@pytest.mark.parametrize("K", KS)
def test_every_mutant_is_rejected_by_the_exact_family(kind, K):
    dt = DT[kind]
    for name, (form, epi, ok, gather) in MUTANTS.items():
        if not ok(K):
            if not (name in VALU_AT_64 and K % 128):
                continue
            form = "valu"
        fp8 = form.startswith("fp8")
        x, w, b, r, sw, wref = make(form, "exact", K, dt, epi)
        c, rejected = verdict(emulate(form, x, w, b, r, epi, mut=name, sw=sw), x, wref, b, r, epi, "exact", fp8)
        print(f"DECODECHK {name} {form} {kind} K={K} exact: unequal {c['unequal']} outside {c['outside']} ratio {c['ratio']:.2f}")
        assert rejected, f"{name} at K = {K} ({kind}, {form}) is not rejected by the exact family"
        if gather:
            assert gather_rejects(form, K, dt, name), f"{name} at K = {K} ({kind}, {form}) is not rejected by the gather family"


def old_rule_ok(got, x, w, b, r, epi, dt):
    """The rule of tests/test_gpu_llm_ops.py::test_linear_decode_rows(_k_split): f64 reference, 2^-7 |ref| + 2^-8 rms(ref); SwiGLU against
    the rounded torch chain with 2^-6 and 2^-6."""
    ref = x.double() @ w.double().T
    if epi == DEC_SWIGLU:
        g, u = gc.split_gate_up(ref.to(dt).float())
        want = (torch.nn.functional.silu(g).to(dt).float() * u).double()
        return bool(((got.double() - want).abs() <= 2.0 ** -6 * want.abs() + 2.0 ** -6 * want.pow(2).mean().sqrt()).all())
    if epi == DEC_BIAS:
        ref = ref + b.double()
    if epi == DEC_RES:
        ref = ref.to(dt).double() + r.double()
    return bool(((got.double() - ref).abs() <= 2.0 ** -7 * ref.abs() + 2.0 ** -8 * ref.pow(2).mean().sqrt()).all())


OLD_RULE_ACCEPTS = ("bias_late", "res_early", "swiglu_unrounded")


def test_the_old_rule_and_the_mutants():
    """The old rule on its own inputs (bf16, randn and randn * 0.05) against every mutant: prints the table of the docstring and asserts
    the part of it that is the reason for this checker - the rounding-point mutants pass the old rule at every K."""
    dt = torch.bfloat16
    table = {}
    for K in KS[1:]:
        for name, (form, epi, ok, _) in MUTANTS.items():
            if not ok(K):
                table.setdefault(name, []).append("-")
                continue
            M = rows(form)
            g = torch.Generator().manual_seed(K)
            x = torch.randn(M, K, generator=g).to(dt)
            w = (torch.randn(N, K, generator=g) * 0.05).to(dt)
            b = torch.randn(N, generator=g).to(dt)
            r = torch.randn(M, N, generator=g).to(dt)
            sw, wv = None, w
            if form.startswith("fp8"):
                sw = w.float().abs().amax(1) / 448.0
                q = (w.float() / sw[:, None]).to(torch.float8_e4m3fn)
                wv, w = q.float(), q.double() * sw.double()[:, None]
            out = emulate(form, x, wv, b, r, epi, mut=name, sw=sw)
            accepted = old_rule_ok(out, x, w, b, r, epi, dt)
            table.setdefault(name, []).append("A" if accepted else "r")
    for name, v in table.items():
        print(f"DECODECHK old rule {name:18s} {' '.join(v)}")
    for name in OLD_RULE_ACCEPTS:
        assert "r" not in table[name], f"the old rule rejects {name} after all: {table[name]}"


def test_gather_names_the_k_that_was_read():
    for dt in DT.values():
        x, w, want = gc.gather_inputs(20, N, 1152, dt, stride=5, shift=1100)
        bad = emulate("mfma", x, w, None, None, DEC_NONE, mut="last_tile")
        text = gc.gather_explain(bad, x, w, want)
        assert "outputs differ" in text and "k = " in text
        x, q, sw, want, w16 = dc.gather_inputs_fp8(4, N, 400, dt, stride=3, shift=7)
        bad = emulate("fp8_valu", x, q.view(torch.float8_e4m3fn).float(), None, None, DEC_NONE, mut="scale_n1", sw=sw)
        assert "outputs differ" in gc.gather_explain(bad, x, w16, want)


def test_expected_form_on_known_shapes():
    """The dispatcher's rule as decode.hip's comments and the existing tests state it."""
    f = dc.expected_form
    assert f(1, 4608, 3584, DEC_BIAS, True, 1, CUS).kernel == "valu"
    assert f(32, 4608, 3584, DEC_BIAS, True, 1, CUS)[:7] == ("mfma2", 2, 1, 0, 4, True, True)
    assert f(32, 4608, 3584, DEC_BIAS, False, 1, CUS).grid == (144, 1)                # 288 groups: 144 x 2
    assert f(32, 3584, 18944, DEC_RES, False, 1, CUS).kernel == "split"
    assert f(32, 37888, 18944 // 2 * 2, DEC_SWIGLU, False, 1, CUS).kernel == "mfma"   # SwiGLU over a long K: no K-split
    assert f(32, 3584, 18944, DEC_RES, False, 3, CUS).kernel == "stream"
    assert f(32, 3584, 18944, DEC_RES, False, 0, CUS).kernel == "mfma"
    assert f(16, 1024, 1024, DEC_NONE, False, 2, CUS).kernel == "stream"               # 8 tiles: below the persistent form's 9
    assert f(16, 1024, 896, DEC_NONE, False, 3, CUS).kernel == "mfma"                  # 7 tiles: a wave without one
    assert (f(2, 4096, 1152, DEC_NONE, False, 0, CUS).OG, f(16, 8192, 1152, DEC_NONE, False, 0, CUS).OG, f(17, 8192, 1152, DEC_NONE, False, 0, CUS).OG) == (2, 1, 2)
    assert f(32, 8192, 1152, DEC_SWIGLU, False, 0, CUS).UN == 1 and f(32, 8192, 1152, DEC_RES, False, 0, CUS).UN == 2
    assert f(3, 512, 400, DEC_NONE, False, 1, CUS, fp8=True).kernel == "fp8_valu" and f(3, 512, 512, DEC_NONE, False, 1, CUS, fp8=True).kernel == "fp8_mfma"
    with pytest.raises(ValueError):
        f(5, 36, 520, DEC_NONE, False, 1, CUS)
    with pytest.raises(ValueError):
        f(16, 512, 3584, DEC_RES, True, 1, CUS)                                        # no fused norm with a residual: VALU form, 4 rows


def test_cases_cover_every_instantiation():
    """Through expected_form with cus = 256: every case runs the kernel it is listed under, and the table reaches every instantiation the
    dispatcher can launch for the 16-bit linears, workgroups that walk 1, 2 and 3 groups, and both K-split chunk lengths."""
    seen = set()
    walks = set()
    split_both = False
    for c in dc.CASES:
        fm = dc.form_of(c, CUS)
        assert fm.kernel == c.form, (c, fm)
        seen.add((fm.kernel, c.epi, fm.MB, fm.OG, fm.UN, fm.NT, fm.short, fm.NORM))
        if fm.kernel == "mfma2":
            walks |= set(fm.groups)
        if fm.kernel == "split":
            C, hi, n_hi = fm.split
            split_both = split_both or 0 < n_hi < C
    E4 = range(4)
    want = set()
    want |= {("valu", e, m, 0, 0, 0, False, nrm) for e in E4 for m in (1, 2, 3, 4) for nrm in (False, True)}
    want |= {("mfma", e, mb, og, 1 if (2 if e == DEC_SWIGLU else 1) * og * mb >= 8 else 2, 0, False, False) for e in E4 for mb in (1, 2) for og in (1, 2)}
    want |= {("mfma2", e, mb, 1, 0, nt, short, nrm) for e in E4 for mb in (1, 2) for nt in (2, 3, 4) for short in (False, True)
             for nrm in (False, True) if not (nrm and e == DEC_RES)}
    missing = want - seen
    assert not missing, sorted(missing)
    assert {(k[1], k[2]) for k in seen if k[0] == "stream"} == {(e, mb) for e in E4 for mb in (1, 2)}
    assert {k[6] for k in seen if k[0] == "stream"} == {False, True}               # waves with equal and with unequal tile counts
    # the K-split pair: both row-block counts with every tiles-per-wave instantiation, every epilogue of the combine kernel
    split_seen = {(k[2], k[5]) for k in seen if k[0] == "split"}
    assert split_seen == {(mb, nt) for mb in (1, 2) for nt in (2, 3, 4)}, split_seen
    assert {k[1] for k in seen if k[0] == "split"} == {DEC_NONE, DEC_BIAS, DEC_RES}
    assert split_both, "no K-split case with n_hi < C"
    assert {1, 2, 3} <= walks, walks
    # the e4m3 forms: every epilogue, every row count of the VALU form, both row-block counts of the matrix-core form
    assert {(k[1], k[2]) for k in seen if k[0] == "fp8_valu"} == {(e, m) for e in E4 for m in (1, 2, 3, 4)}
    assert {(k[1], k[2]) for k in seen if k[0] == "fp8_mfma"} == {(e, mb) for e in E4 for mb in (1, 2)}
    # the two persistent grids must stay uneven on other chips too
    for cus in (64, 228, 256, 304):
        w = set()
        for c in dc.cases(cus):
            if c.form == "mfma2":
                w |= set(dc.form_of(c, cus).groups)
        assert {1, 2, 3} <= w, (cus, w)
