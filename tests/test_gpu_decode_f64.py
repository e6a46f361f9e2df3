"""Every decode linear form (decode.hip: v3d_linear_decode_rows, v3d_linear_decode_fp8_rows), bit for bit and per element, against the f64
reference and bound of tests/decode_check.py, in bf16 and f16, for every entry of its case table.

The kernels are called through the C interface, so every buffer is the test's own: `out` is a column slice of a NaN-filled buffer with
ldo > n_out and one more row; x is a slice of a NaN-filled buffer with ldx > K whose row M is NaN; W has ldw > K with NaN (e4m3: the NaN
code) in the padding; res has its own ldr.  After each call everything that should be written is finite, the padding and the extra row
are still NaN, and a second call gives the same bits.  Per case: the *exact* family comes back bit for bit (NONE / BIAS / RES) or inside
the function-error interval (SwiGLU); the *gather* family (one-hot rows, both orientations, zero bias / residual) returns the selected
values bit for bit and a mismatch names the k that was read; the *random* family stays under the bound.  Fused RMSNorm: the fused call
equals ops.rmsnorm + the unfused call bit for bit, and that unfused call is inside the bound on the normalised rows.  A residual case
is also called as the engine calls it (res and out the same rows, ldr = ldo) and gives the bits of the out-of-place call.

RECORD (one MI355X, 256 CUs; 37 tests over 256 table cases x 2 dtypes, the product shapes and the LM head; wall time of the file 6 - 7 s).
Worst |err| / bound on the random family: r04 matrix-core 0.992 (bf16) / 0.971 (f16), persistent 0.982 / 0.909 (on normalised rows 0.944 /
0.798), K-split 0.909 / 0.598, streaming 0.970 / 0.912, VALU 0.919 / 0.846 (normalised rows 0.943 / 0.862), e4m3 VALU 0.978 / 0.962, e4m3
matrix-core 0.950 / 0.920; exact family: 0 unequal, 0 outside the SwiGLU interval; gather: 0 differences; in-place residual: the same bits.
silu_f (test_silu_function_error): C_FUNC needed 0.338 (f16, at x = -0.714: -0.234619 returned for -0.234680) and 0.000 (bf16: every
output is the rounded f64 value); C_FUNC = 4 keeps more than the margin of 2.  No kernel bug was found.
Kernel names of one rocprofv3 --kernel-trace run of this file (a record, not a test): all eight templates appeared - linear_decode_kernel
(64 instantiations), linear_decode_mfma_kernel (32), linear_decode_mfma2_kernel (84), linear_decode_mfma2_split_kernel (12) with
decode_combine_kernel (6), linear_decode_mfma_stream_kernel (16), linear_decode_fp8_kernel (32), linear_decode_fp8_mfma_kernel (16): every
instantiation decode.hip holds, in both dtypes.
"""
import json
import os

import pytest
import torch

import decode_check as dc
import gemm_check as gc
from decode_check import DEC_BIAS, DEC_NONE, DEC_RES, DEC_SWIGLU

pytestmark = pytest.mark.gpu

DT = {"bf16": torch.bfloat16, "f16": torch.float16}
NAN = float("nan")
E4M3_NAN = 0x7F
WORST = {}
CHUNK = 25          # cases per parametrised test


@pytest.fixture(scope="module")
def ops():
    assert torch.cuda.is_available()
    from v3d import ops as _ops
    return _ops


def cus():
    return torch.cuda.get_device_properties(0).multi_processor_count


def note(form, dtn, r):
    key = f"{form} {dtn}"
    WORST[key] = max(WORST.get(key, 0.0), r)
    return r


def bits(t):
    return t.contiguous().view(torch.int16)


def nan_slice(t, ld, off=0, extra_rows=0):
    """t [rows, cols] -> the same values as a column slice (at column `off`) of a NaN-filled [rows + extra_rows, ld] buffer."""
    rows, cols = t.shape
    fill = E4M3_NAN if t.dtype == torch.uint8 else NAN
    big = torch.full((rows + extra_rows, ld), fill, dtype=t.dtype, device="cuda")
    big[:rows, off:off + cols] = t
    return big[:rows, off:off + cols]


class Inputs:
    """The strided views one case hands to the kernel (built once, launched more than once)."""

    def __init__(self, x, w, bias, res, epi, norm_w=None, sw=None):
        self.M, self.K = x.shape
        self.N = w.shape[0]
        self.no = dc.n_out(self.N, epi)
        self.epi, self.dt, self.sw, self.norm_w = epi, x.dtype, sw, norm_w
        self.x = nan_slice(x, self.K + 16, 8, extra_rows=1)
        self.w = nan_slice(w, self.K + (16 if sw is not None else 8))
        self.bias = bias[:self.N].contiguous() if epi == DEC_BIAS else None
        self.res_values = res[:, :self.no] if epi == DEC_RES else None
        self.res = nan_slice(self.res_values, self.no + 40, 16) if epi == DEC_RES else None


def launch(ops, i, inplace=False):
    """One launch into a fresh NaN buffer -> (out view [M, n_out], the whole buffer)."""
    big = torch.full((i.M + 1, i.no + 24), NAN, dtype=i.dt, device="cuda")
    out = big[:i.M, 8:8 + i.no]
    res = i.res
    if inplace:
        out.copy_(i.res_values)
        res = out
    ldr = res.stride(0) if res is not None else 0
    p, lib = ops._p, ops.lib()
    if i.sw is not None:
        ops.check(lib.v3d_linear_decode_fp8_rows(p(i.x), i.x.stride(0), i.M, p(i.w), i.w.stride(0), p(i.sw), p(i.bias), p(res), ldr, p(out),
                                                 out.stride(0), i.N, i.K, ops._code(i.x), i.epi, ops._stream()), "v3d_linear_decode_fp8_rows")
    else:
        ops.check(lib.v3d_linear_decode_rows(p(i.x), i.x.stride(0), i.M, p(i.norm_w), 1e-6, p(i.w), i.w.stride(0), p(i.bias), p(res), ldr, p(out),
                                             out.stride(0), i.N, i.K, ops._code(i.x), i.epi, ops._stream()), "v3d_linear_decode_rows")
    return out, big


def run(ops, x, w, bias, res, epi, norm_w=None, sw=None, inplace=False):
    """Two launches: all of [M, n_out] finite, padding and extra row still NaN, the same bits twice -> out."""
    i = Inputs(x, w, bias, res, epi, norm_w, sw)
    out, big = launch(ops, i, inplace)
    assert bool(torch.isfinite(out).all()), "an output was not written or is not finite"
    assert int(torch.isnan(big).sum()) == big.numel() - out.numel(), "the padding or the row after M was written"
    out2, _ = launch(ops, i, inplace)
    assert torch.equal(bits(out), bits(out2)), "two launches of the same case differ"
    return out


def what(c, dtn, family):
    return f"{c.form} {dc.DEC_NAMES[c.epi]} {dtn} M={c.M} K={c.K} N={c.N} norm={c.norm} V3D_DEC_V2={c.v2} {family}"


def check_family(ops, c, dtn, family, x, w, b, r, sw=None, inplace=False):
    """Run and compare one non-gather family -> the comparison."""
    wref = dc.dequant(w, sw) if sw is not None else w
    out = run(ops, x, w, b, r, c.epi, sw=sw, inplace=inplace)
    cmp = gc.compare(out, x, wref, b, r[:, :dc.n_out(c.N, c.epi)], dc.GEMM_EPI[c.epi], exact=family == "exact",
                     lin_rel=dc.FP8_LIN_REL if sw is not None else 0.0)
    tag = what(c, dtn, family)
    print(f"DECODECHK {tag} ratio {cmp['ratio']:.3f} unequal {cmp['unequal']} outside {cmp['outside']} needs_rounding {cmp['needs_rounding']:.2f}")
    if family == "exact":
        assert cmp["ratio"] <= 1.0, (tag, cmp)
        if c.epi == DEC_SWIGLU:
            assert cmp["outside"] == 0, f"{tag}: {cmp['outside']} outputs outside the function-error interval"
        else:
            assert cmp["unequal"] == 0, f"{tag}: {cmp['unequal']} outputs differ from round(exact)"
    else:
        assert note(c.form, dtn, cmp["ratio"]) < 1.0, f"{tag}: worst |err| / bound = {cmp['ratio']}"
    return out


def check_gather(ops, c, dtn, fp8):
    """One-hot rows in both orientations with zero bias / residual: the selected values bit for bit (SwiGLU: silu of the selected gate
    times the selected up value, inside the function-error interval).  Row 0 selects a k in the last tile; the others are spread over K."""
    dt = DT[dtn]
    M, N, K = c.M, c.N, c.K
    no = dc.n_out(N, c.epi)
    zb = torch.zeros(N, dtype=dt, device="cuda")
    zr = torch.zeros(M, no, dtype=dt, device="cuda")
    down = 2.0 ** -4 if (c.epi == DEC_SWIGLU and dt == torch.float16) else 1.0          # keeps silu(gate) * up finite in f16 (exact scaling)
    for transposed in (False, True):
        rows = N if transposed else M
        stride, shift = (max(K // rows, 1) | 1), K - 3
        sw = None
        if fp8:
            x, w, sw, want, w16 = dc.gather_inputs_fp8(M, N, K, dt, stride, shift, "cuda", transposed)
            if transposed:
                x = (x.double() * down).to(dt)
            else:
                sw = sw * down
            wref = dc.dequant(w, sw)
        else:
            x, w, want = gc.gather_inputs(M, N, K, dt, stride, shift, "cuda", transposed)
            if transposed:
                x = (x.double() * down).to(dt)
            else:
                w = (w.double() * down).to(dt)
            wref = w16 = w
        out = run(ops, x, w, zb, zr, c.epi, sw=sw)
        tag = what(c, dtn, "gather transposed" if transposed else "gather")
        if c.epi == DEC_SWIGLU:
            cmp = gc.compare(out, x, wref, None, None, gc.EPI_SWIGLU, lin_rel=dc.FP8_LIN_REL if fp8 else 0.0)
            assert cmp["outside"] == 0, (tag, cmp)          # (no ratio: a selected zero has a bound of zero)
        elif not torch.equal(out, want):
            raise AssertionError(f"{tag}\n" + gc.gather_explain(out, x, w16, want, transposed))


def check_fused_norm(ops, c, dtn):
    """Fused RMSNorm == ops.rmsnorm + the unfused call, bit for bit (VALU form: the one-row kernel per row), and that unfused call inside the
    bound on the normalised rows."""
    dt = DT[dtn]
    M, N, K = c.M, c.N, c.K
    x, w, b, r = gc.random_inputs(M, N, K, dt, seed=K + 3 * M, device="cuda", a_scale=1.0)
    g = torch.Generator(device="cuda").manual_seed(K)
    lnw = (1 + 0.1 * torch.randn(K, generator=g, device="cuda")).to(dt)
    assert c.form == "valu" or ops.linear_decode_rows_fuses_norm(M, N, K, c.epi)
    h = ops.rmsnorm(x, lnw, 1e-6)
    fused = run(ops, x, w, b, r, c.epi, norm_w=lnw)
    if c.form == "valu":
        unfused = torch.cat([run(ops, h[m:m + 1], w, b, r[m:m + 1], c.epi) for m in range(M)])
    else:
        unfused = run(ops, h, w, b, r, c.epi)
    tag = what(c, dtn, "fused norm")
    assert torch.equal(bits(fused), bits(unfused)), f"{tag}: {int((bits(fused) != bits(unfused)).sum())} outputs differ from rmsnorm + unfused"
    cmp = gc.compare(unfused, h, w, b, r[:, :dc.n_out(N, c.epi)], dc.GEMM_EPI[c.epi])
    print(f"DECODECHK {tag} ratio {cmp['ratio']:.3f}")
    assert note(c.form + " norm", dtn, cmp["ratio"]) < 1.0, (tag, cmp)


def check_case(ops, c, dtn, inplace_only=False):
    dt = DT[dtn]
    fp8 = c.form.startswith("fp8")
    M, N, K = c.M, c.N, c.K
    if c.norm:
        check_fused_norm(ops, c, dtn)
        return
    target = 2.0 if c.epi == DEC_SWIGLU else None
    seed = 7 * M + K + N
    for family in ("exact", "random"):
        sw = None
        if fp8:
            make = dc.exact_inputs_fp8 if family == "exact" else dc.random_inputs_fp8
            x, w, sw, b, r = make(M, N, K, dt, seed=seed, device="cuda", **({"target": target} if family == "exact" else {}))
        elif family == "exact":
            x, w, b, r = gc.exact_inputs(M, N, K, dt, seed=seed, device="cuda", target=target)
        else:
            x, w, b, r = gc.random_inputs(M, N, K, dt, seed=seed, device="cuda")
        out = check_family(ops, c, dtn, family, x, w, b, r, sw, inplace=inplace_only)
        if c.epi == DEC_RES and not inplace_only:         # the engine's call: res = x, out = x
            same = run(ops, x, w, b, r, c.epi, sw=sw, inplace=True)
            assert torch.equal(bits(same), bits(out)), f"{what(c, dtn, family)}: the in-place residual call differs from the out-of-place one"
    check_gather(ops, c, dtn, fp8)


def _chunks():
    out = []
    for form in dc.FORMS:
        idx = [i for i, c in enumerate(dc.CASES) if c.form == form]
        out += [pytest.param(idx[j:j + CHUNK], id=f"{form}-{j // CHUNK}") for j in range(0, len(idx), CHUNK)]
    return out


@pytest.mark.parametrize("dtn", list(DT))
@pytest.mark.parametrize("idx", _chunks())
def test_every_case_of_the_table(ops, monkeypatch, idx, dtn):
    """decode_check.cases(): every kernel form, instantiation and edge (the table's comments name them), in table order - the K-split
    entries start with a small product, then the largest, so that the per-stream workspace grows once and is then reused."""
    assert "V3D_DEC_OG" not in os.environ, "the table assumes the default output-group rule"
    monkeypatch.delenv("V3D_DEC_FUSE_NORM", raising=False)
    table = dc.cases(cus())
    assert len(table) == len(dc.CASES)
    for i in idx:
        c = table[i]
        fm = dc.form_of(c, cus())
        assert fm.kernel == c.form, f"{c} would run {fm}"
        monkeypatch.setenv("V3D_DEC_V2", str(c.v2))
        check_case(ops, c, dtn)


# name, weight rows, K, epilogue, fused norm, residual in place
PRODUCT = [("qkv", 4608, 3584, DEC_BIAS, True, False), ("o", 3584, 3584, DEC_RES, False, True),
           ("gate_up", 37888, 3584, DEC_SWIGLU, True, False), ("down", 3584, 18944, DEC_RES, False, True)]


@pytest.mark.parametrize("M", [1, 32])
@pytest.mark.parametrize("name,N,K,epi,norm,inplace", PRODUCT, ids=[p[0] for p in PRODUCT])
def test_product_shapes(ops, monkeypatch, name, N, K, epi, norm, inplace, M):
    """The 7B decoder's linears as the engine calls them, under the default V3D_DEC_V2: all three families on the call without norm (the
    residual ones in place only), and the fused-norm contract where the engine fuses."""
    monkeypatch.delenv("V3D_DEC_V2", raising=False)
    form = dc.expected_form(M, N, K, epi, False, 1, cus()).kernel
    check_case(ops, dc.Case(form, M, K, N, epi, False, 1), "bf16", inplace_only=inplace)
    if norm:
        form = dc.expected_form(M, N, K, epi, True, 1, cus()).kernel
        assert form == ("valu" if M == 1 else "mfma2")
        check_fused_norm(ops, dc.Case(form, M, K, N, epi, True, 1), "bf16")


@pytest.mark.parametrize("M", [1, 32])
def test_lm_head_gather(ops, monkeypatch, M):
    """LM head 152064 x 3584: the gather family only, both orientations - its reference is an index, not a product."""
    monkeypatch.delenv("V3D_DEC_V2", raising=False)
    form = dc.expected_form(M, 152064, 3584, DEC_NONE, False, 1, cus()).kernel
    check_gather(ops, dc.Case(form, M, 3584, 152064, DEC_NONE, False, 1), "bf16", False)


@pytest.mark.parametrize("dtn", list(DT))
def test_silu_function_error(ops, dtn):
    """decode.hip's silu_f over the whole finite 16-bit grid with |x| <= 16, through the one-row SwiGLU call (x = e_0, gate row n holds grid
    value n, every up row 1: the linear outputs ARE the grid values), against f64 silu: the smallest C_FUNC that explains every output must
    leave the margin of 2 that C_FUNC = 4 claims.  Outputs below the normal range of the dtype (f16) or 2^-100 (bf16) are left to the
    bound's absolute terms."""
    dt = DT[dtn]
    grid = torch.arange(65536, device="cuda").sub(32768).to(torch.int16).view(dt)
    xg = torch.where(torch.isfinite(grid) & (grid.abs() <= 16), grid, torch.zeros_like(grid))
    wg = torch.zeros(65536, 8, dtype=dt, device="cuda")
    wu = torch.zeros(65536, 8, dtype=dt, device="cuda")
    wg[:, 0] = xg
    wu[:, 0] = 1
    x = torch.zeros(1, 8, dtype=dt, device="cuda")
    x[0, 0] = 1
    got = run(ops, x, ops.interleave_gate_up(wg, wu), None, None, DEC_SWIGLU)[0].double()
    xd = xg.double()
    v = gc.silu(xd)
    unit = (gc.func_err(xd, "silu") - gc.FTZ) / gc.C_FUNC
    need = dc.needed_c_func(got, v, unit, dt)
    floor = 2.0 ** -14 if dt == torch.float16 else 2.0 ** -100
    need = torch.where(v.abs() >= floor, need, torch.zeros_like(need))
    worst, i = need.max().item(), need.argmax()
    print(f"DECODECHK function_error silu_f {dtn}: C_FUNC needed {worst:.3f} at x = {xd[i].item()} (got {got[i].item()!r}, f64 {v[i].item()!r}; "
          f"{int((need > 2).sum())} grid points need more than 2)")
    WORST[f"silu_f C_FUNC {dtn}"] = worst
    assert 2.0 * worst <= gc.C_FUNC, f"silu_f needs C_FUNC = {worst} at x = {xd[i].item()}: C_FUNC = {gc.C_FUNC} no longer leaves a margin of 2"


def test_zz_print_worst_ratios():
    """Worst |err| / bound on the random family per form and dtype seen in this run (and the measured silu_f constant)."""
    print("DECODE_WORST " + json.dumps({k: round(v, 3) for k, v in sorted(WORST.items())}))
    assert all(v < 1.0 for k, v in WORST.items() if "C_FUNC" not in k)
