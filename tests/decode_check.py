"""f64 reference, per-element bound, structured inputs, the dispatcher's rule and the case table for the decode linears (decode.hip:
v3d_linear_decode_rows and v3d_linear_decode_fp8_rows, every kernel form).

Not a conftest: test modules import it (`import decode_check as dc`).  Built on tests/gemm_check.py: reference(), compare(), the exact,
gather and random input families and gather_explain() are the GEMM checker's, under the decode epilogues' names:
    DEC_NONE -> EPI_NONE, DEC_BIAS -> EPI_BIAS, DEC_RES -> EPI_RES (the linear output is rounded, then the residual is added and the sum
    rounded), DEC_SWIGLU -> EPI_SWIGLU (round(silu(round(gate))) * round(up), the 64-gate / 64-up row interleave of
    ops.interleave_gate_up).

Bound.  gemm_check's bound, unchanged, for the 16-bit forms: lin = C_ACC (K / 32 + C0) 2^-24 mag + h |y| with C_ACC = 2, C0 = 32 covers a
summation chain of depth K / 32 + 35 with its second-order terms, and no decode chain is deeper:
    VALU form (linear_decode_kernel)          K / 256 fmas per thread (8 per 16-byte chunk, chunks tid, tid + 256, ...), 6 adds of the xor
                                              butterfly, 3 adds of the four wave sums: K / 256 + 9;
    matrix-core forms (r04, persistent,       a term passes at most 32 roundings inside its own 16 x 16 x 32 MFMA, one add per later MFMA
    streaming)                                of its wave's slice (at most K / 32 / 8 + 3), 7 adds of the eight slices: <= K / 32 + 7;
    K-split pair                              the same inside a chunk, then at most 16 adds of decode_combine_kernel: <= K / 32 + 23;
    e4m3 forms                                VALU: K / 256 fmas (16 per chunk) + 9; matrix core: K / 32 + 7, as above.
silu.  decode.hip's silu_f is x / (1 + __expf(-x)), not gemm.hip's rcp / exp2 form; its error is charged in the same units (gemm_check's
func_err: C_FUNC 2^-23 |f| (1 + |x| log2 e)) with the project's C_FUNC = 4.
MEASURED (MI355X, silu_f through the one-row SwiGLU call over the whole finite 16-bit grid with |x| <= 16, f64 silu as the truth, smallest
C_FUNC that explains every output; tests/test_gpu_decode_f64.py::test_silu_function_error): 0.338 (f16, at x = -0.714), 0.000 (bf16).

e4m3 (W8A16) reference: the f64 product of the same dequantised weights, q.view(float8_e4m3fn).double() * sw.  The kernels multiply the
f32 sum by sw[n] once before the bias: the linear bound gains one derived term, 2^-24 |y| (gemm_check's lin_rel).
  exact   integer codes up to 16 in magnitude (they convert to e4m3 and back exactly: asserted) against integer x; scales are powers of
          two that differ from each row to the next and between the gate and up row of one SwiGLU pair (row n: 2^-((n + n // 64) % 4)),
          so every product and sum is exact and a scale taken from another row shows.
  gather  one-hot x against distinct codes (every finite byte value), and transposed: one-hot weights of code 1.0 against distinct x.

Fused RMSNorm has no exact family (the norm destroys integrality); its contract is two steps, both checked on the device: the fused call
is bit-identical to ops.rmsnorm followed by the unfused call (VALU form, up to 4 rows: the one-row kernel per row; persistent form, more
than 4 rows), and the unfused call is checked on that normalised 16-bit input.  v3d_rmsnorm itself: tests/test_gpu_rowwise_f64.py.

expected_form() restates the dispatcher (linear_decode_rows, dec_v2_plan, v3d_linear_decode_fp8_rows) in Python; cases(cus) is the table of
shapes the device test runs, each tagged with the kernel it is meant for; CASES = cases(256) is what the CPU test checks for coverage.
"""
import collections
import math

import torch

import gemm_check as gc
from gemm_check import (EPI_BIAS, EPI_NONE, EPI_RES, EPI_SWIGLU, compare, exact_inputs, gather_explain, gather_inputs,  # noqa: F401
                        random_inputs, reference)

DEC_NONE, DEC_BIAS, DEC_RES, DEC_SWIGLU = range(4)
DEC_NAMES = ("none", "bias", "res", "swiglu")
GEMM_EPI = {DEC_NONE: EPI_NONE, DEC_BIAS: EPI_BIAS, DEC_RES: EPI_RES, DEC_SWIGLU: EPI_SWIGLU}
FP8_LIN_REL = 2.0 ** -24
DEC_MAX_ROWS = 32
E4M3_ONE = 0x38


def n_out(N, epi):
    return N // 2 if epi == DEC_SWIGLU else N


def needed_c_func(got, v, unit, dt):
    """Smallest c with got in [round(v - c unit), round(v + c unit)], per element (f64 tensors; got, round(v) normal 16-bit numbers)."""
    p = 8 if dt == torch.bfloat16 else 11
    r = gc.rnd(v, dt)
    _, ex = torch.frexp(r.abs())
    ulp = torch.exp2((ex - p).double())
    one_step = (got - r).abs() <= 1.001 * ulp                       # got is r's neighbour: the boundary between them is their mean (exact)
    need = torch.where(one_step, ((r + got) / 2 - v).abs(), (got - v).abs()) / unit
    return torch.where(got == r, torch.zeros_like(need), need)


# ------------------------------------------------------------------------------ e4m3


def dequant(q, sw):
    """q [N, K] uint8 e4m3 codes, sw [N] f32 -> the f64 weights the kernels multiply by."""
    return q.view(torch.float8_e4m3fn).double() * sw.double()[:, None]


def fp8_row_scales(N, shift=0, device="cpu"):
    n = torch.arange(N, device=device)
    return torch.exp2(-(((n + n // 64) % 4) + shift).float())


def exact_inputs_fp8(M, N, K, dt, seed=0, device="cpu", target=None):
    """x, q, sw, bias, res of the exact family: x and the codes are integers (codes <= 16: e4m3 numbers), sw powers of two per row, so
    sw[n] * sum is exact in f32 in any order; bias and res as gemm_check.exact_inputs makes them (scaled alike)."""
    g = torch.Generator(device=device).manual_seed(seed)
    amax = min(gc.exact_amax(K), 16)
    bmax = 1000
    assert 8 * (K * amax * amax + bmax) < 2 ** 24, "a scaled sum could leave the exact range of f32"
    x = torch.randint(-amax, amax + 1, (M, K), generator=g, device=device).double()
    c = torch.randint(-amax, amax + 1, (N, K), generator=g, device=device).double()
    b = torch.randint(-bmax // 4, bmax // 4 + 1, (N,), generator=g, device=device).double() * 4
    r = torch.randint(-bmax // 4, bmax // 4 + 1, (M, N), generator=g, device=device).double() * 8
    s = 0
    if target is not None:
        s = max(0, round(math.log2(amax * (amax + 1) / 3.0 * math.sqrt(K) / target)))
    sx, ss = s // 2, s - s // 2
    q8 = c.to(torch.float8_e4m3fn)
    assert bool((q8.double() == c).all()), "an exact code is not an e4m3 number"
    sw = fp8_row_scales(N, ss, device)
    out = []
    for t, sc in ((x, sx), (b, s), (r, s)):
        v = (t * 2.0 ** -sc).to(dt)
        assert bool((v.double() == t * 2.0 ** -sc).all()), "an exact input is not a 16-bit number"
        out.append(v)
    return out[0], q8.view(torch.uint8), sw, out[1], out[2]


def random_inputs_fp8(M, N, K, dt, seed=0, device="cpu"):
    """Gaussian x; Gaussian weights quantised per row to e4m3 with amax / 448 scales (torch's conversion; the reference uses the codes)."""
    a, w, b, r = gc.random_inputs(M, N, K, dt, seed=seed, device=device)
    sw = (w.float().abs().amax(1).clamp_min(1e-6) / 448.0)
    q = (w.float() / sw[:, None]).to(torch.float8_e4m3fn).view(torch.uint8)
    return a, q, sw, b, r


def gather_inputs_fp8(M, N, K, dt, stride=1, shift=0, device="cpu", transposed=False):
    """(x, q, sw, want, w16): as gemm_check.gather_inputs.  Plain: codes run through the 254 finite byte values (two neighbours in a row
    never agree), power-of-two row scales; want[m, n] = code[n, k0(m)] sw[n] (4 significant bits: a 16-bit number).  Transposed: one-hot
    weights of code 1.0 with scale 1 against distinct x.  w16 = the dequantised weights as 16-bit numbers (exact), for gather_explain."""
    if transposed:
        a, w, want = gc.gather_inputs(M, N, K, dt, stride, shift, device, transposed=True)
        q = torch.where(w != 0, torch.full_like(w, E4M3_ONE, dtype=torch.uint8), torch.zeros_like(w, dtype=torch.uint8))
        return a, q, torch.ones(N, dtype=torch.float32, device=device), want, w
    a, _, _ = gc.gather_inputs(M, 1, K, dt, stride, shift, device)
    b = (torch.arange(N * K, device=device).reshape(N, K) * 37) % 254
    q = (b + (b >= 127).long()).to(torch.uint8)                    # skips 0x7f; 0xff is never reached: no NaN codes
    sw = fp8_row_scales(N, 0, device)
    wd = dequant(q, sw)
    w16 = wd.to(dt)
    assert bool((w16.double() == wd).all())
    k0 = gc.gather_k0(M, K, stride, shift, device)
    return a, q, sw, w16[:, k0].T.contiguous(), w16


# ------------------------------------------------------------------------------ the dispatcher's rule

Form = collections.namedtuple("Form", "kernel MB OG UN NT short NORM split grid groups")
# kernel: valu | mfma (r04) | mfma2 (persistent) | split (+ combine) | stream | fp8_valu | fp8_mfma
# MB: 16-row activation blocks (VALU forms: the row count M of the instantiation); OG: 16-output groups per workgroup (r04);
# UN: 128-element K tiles in flight per wave (r04); NT: tiles per wave of the instantiation, short: some wave runs the NT - 1 loop;
# NORM: the fused RMSNorm instantiation; split: (C, hi, n_hi) of the K-split; grid: workgroups (x, y); groups: the set of group counts
# that workgroups of a persistent / K-split launch walk.


def _ceil(a, b):
    return (a + b - 1) // b


def _walks(groups16, grid):
    return tuple(sorted({_ceil(groups16 - b, grid) for b in range(grid)}))


def split_plan(tiles, groups16, cus):
    """The K cut of the K-split form -> (C, hi, n_hi, G) or None (decode.hip: whole rounds of groups on as many CUs as possible)."""
    C = hi = 0
    best = 0.0
    for c in range(_ceil(tiles, 32), 17):
        h = _ceil(tiles, c)
        if h > 32 or h < 9:
            continue
        G = cus // c
        if G < 1:
            break
        G = min(G, groups16)
        eff = (groups16 / G) / _ceil(groups16, G) * (c * G) / cus
        if eff > best + 1e-9:
            best, C, hi = eff, c, h
    if C == 0:
        return None
    return C, hi, tiles - C * (hi - 1), min(cus // C, groups16)


def expected_form(M, N, K, epi, norm, v2, cus, fp8=False):
    """What the dispatcher launches for x [M, K], W [N, K] (N counts the weight rows: gate + up for SwiGLU) with V3D_DEC_V2 = v2 on a chip
    of `cus` compute units and the default V3D_DEC_OG -> Form.  Raises ValueError where the call is refused."""
    swiglu = epi == DEC_SWIGLU
    no = n_out(N, epi)
    if N % 4 or (swiglu and N % 128):
        raise ValueError("N not supported")
    if fp8:
        if norm or K % 16:
            raise ValueError("no fused norm / K % 16 for the e4m3 rows")
        mfma_ok = K % 256 == 0 and (N % 128 == 0 if swiglu else N % 16 == 0)
        if not 1 <= M <= (DEC_MAX_ROWS if mfma_ok else 4):
            raise ValueError("rows")
        if mfma_ok and M >= 2:
            short = (K // 256) % 8 != 0
            return Form("fp8_mfma", 1 if M <= 16 else 2, 1, 1, _ceil(K // 256, 8), short, False, None, (no // 16, 1), (1,))
        return Form("fp8_valu", M, 0, 0, 0, False, False, None, (N // 4, 1), (1,))
    if K % 8:
        raise ValueError("K % 8")
    mfma_shape = K % 128 == 0 and (N % 128 == 0 if swiglu else N % 16 == 0)
    tiles, groups16 = K // 128, no // 16
    v2_ok = mfma_shape and 1 <= v2 <= 2 and 9 <= tiles <= 32
    fused = bool(norm) and M > 4 and v2_ok and epi != DEC_RES
    mfma_ok = mfma_shape and (not norm or fused)
    if not 1 <= M <= (DEC_MAX_ROWS if mfma_ok else 4):
        raise ValueError("rows")
    if norm and K > 4096:
        raise ValueError("fused RMSNorm needs K <= 4096")
    if not (mfma_ok and M >= 2):
        return Form("valu", M, 0, 0, 0, False, bool(norm), None, (N // 4, 1), (1,))
    MB = 1 if M <= 16 else 2
    if v2_ok:
        grid = _ceil(groups16, _ceil(groups16, cus))
        return Form("mfma2", MB, 1, 0, _ceil(tiles, 8), tiles % 8 != 0, fused, None, (grid, 1), _walks(groups16, grid))
    if 1 <= v2 <= 2 and tiles > 32 and not swiglu:
        plan = split_plan(tiles, groups16, cus)
        if plan:
            C, hi, n_hi, G = plan
            lens = {hi} | ({hi - 1} if n_hi < C else set())
            nt = _ceil(hi, 8)
            short = any((ct - w + 7) // 8 < nt for ct in lens for w in range(8))
            return Form("split", MB, 1, 0, nt, short, False, (C, hi, n_hi), (G, C), _walks(groups16, G))
    if v2 >= 2 and tiles >= 8:
        return Form("stream", MB, 1, 0, 0, tiles % 8 != 0, False, None, (groups16, 1), (1,))
    wg32 = no // 32
    og_rule = wg32 >= 128 and not (256 <= wg32 < 1024 and M <= 16)
    OG = 2 if no % 32 == 0 and og_rule else 1
    RG = (2 if swiglu else 1) * OG
    return Form("mfma", MB, OG, 1 if RG * MB >= 8 else 2, 0, False, False, None, (no // (16 * OG), 1), (1,))


# ------------------------------------------------------------------------------ the case table

Case = collections.namedtuple("Case", "form M K N epi norm v2")       # N = weight rows (gate + up for SwiGLU)


def _n(no, epi):
    """Weight rows for `no` outputs; SwiGLU needs whole 64-output tiles."""
    if epi == DEC_SWIGLU:
        return 2 * _ceil(no, 64) * 64
    return no


def cases(cus):
    """The shapes of tests/test_gpu_decode_f64.py: the smallest that reach each edge (N only selects the form).  cus sizes the two
    persistent grids: 16 (cus + 1) outputs (one workgroup walks one group, the others two) and 16 (2 cus + 8) (workgroups walk three)."""
    out = []
    E4 = (DEC_NONE, DEC_BIAS, DEC_RES, DEC_SWIGLU)
    big_a, big_b = 16 * (cus + 1), 16 * (2 * cus + 8)
    # VALU form: every (M, EPI, NORM); K = 8 (one chunk), 520 (65 chunks: 191 idle threads), 2056 (thread 0 alone takes a second chunk),
    # 4096 (all threads two chunks: the most NORM takes), 4104; N = 4 and 36 (not a multiple of 16), SwiGLU at N = 128 and 256.
    i = 0
    for M in (1, 2, 3, 4):
        for epi in E4:
            for norm in (False, True):
                ks = (8, 520, 2056, 4096) if norm else (8, 520, 2056, 4104)
                K = ks[i % 4]
                N = (128, 256)[i % 2] if epi == DEC_SWIGLU else (4, 36)[i % 2]
                out.append(Case("valu", M, K, N, epi, norm, 1))
                i += 1
    for K in (8, 520, 2056, 4096, 4104):
        out.append(Case("valu", 1, K, 36, DEC_BIAS, False, 1))
        out.append(Case("valu", 4, K, 4, DEC_RES, False, 1))
        if K <= 4096:
            out.append(Case("valu", 3, K, 36, DEC_BIAS, True, 1))
    out.append(Case("valu", 1, 4096, 256, DEC_SWIGLU, False, 1))
    out.append(Case("valu", 4, 4096, 128, DEC_SWIGLU, True, 1))
    # r04 matrix-core form: V3D_DEC_V2 = 0, or K <= 1024 under the default.  K = 128 (seven idle waves), 1024, 1152, 2176 (17 tiles: the
    # UN = 2 tail re-reads a tile with x zeroed); outputs 16, 48, 4096 (OG = 2) and 8192 (OG = 1 up to 16 rows, 2 above).
    ks = (128, 1024, 1152, 2176)
    i = 0
    for epi in E4:
        for M, no in ((2, 16), (15, 48), (16, 4096), (17, 4096), (31, 8192), (32, 8192), (16, 8192), (32, 48)):
            K = ks[i % 4]
            out.append(Case("mfma", M, K, _n(no, epi), epi, False, 1 if K <= 1024 and i % 2 else 0))
            i += 1
        i += 1
    out.append(Case("mfma", 32, 2176, _n(4096, DEC_SWIGLU), DEC_SWIGLU, False, 0))     # RG * MB = 8: the only UN = 1 instantiation, with a tail
    # persistent form (V3D_DEC_V2 = 2): K -> (NT, a wave with NT - 1): 1152 (2, yes), 2048 (2, no), 2176 (3, yes), 3072 (3, no), 3200 and
    # 3584 (4, yes), 4096 (4, no); every EPI x MB x NORM; fused norm at M = 5, 16, 17, 32.
    i = 0
    for K in (1152, 2048, 2176, 3072, 3200, 3584, 4096):
        for epi in E4:
            for M, norm in (((2, 15, 16)[i % 3], False), ((17, 31, 32)[i % 3], False), ((5, 16)[i % 2], True), ((17, 32)[i % 2], True)):
                if norm and epi == DEC_RES:
                    continue
                no = 48
                if not norm and K == 1152:
                    no = big_a
                if not norm and K == 4096:
                    no = big_b
                out.append(Case("mfma2", M, K, _n(no, epi), epi, norm, 2))
            i += 1
    # K-split (V3D_DEC_V2 = 1): a small product first, then the largest (the workspace grows once), then the rest (it is reused)
    out.append(Case("split", 2, 4224, 128, DEC_NONE, False, 1))
    out.append(Case("split", 32, 18944, 3584, DEC_RES, False, 1))
    i = 0
    for K in (4224, 4736, 9216, 18944):
        for N in (128, 3584):
            for M in ((2, 16)[i % 2], (17, 32)[i % 2]):
                out.append(Case("split", M, K, N, (DEC_NONE, DEC_BIAS, DEC_RES)[i % 3], False, 1))
                i += 1
    out.append(Case("split", 16, 6272, 3584, DEC_BIAS, False, 1))      # 49 tiles = 25 + 24 on 256 CUs: the four-tiles-per-wave instantiation,
    out.append(Case("split", 32, 6272, 3584, DEC_RES, False, 1))       # which none of the product's K reaches; its second chunk runs NT - 1 on every wave
    # streaming form (V3D_DEC_V2 = 3): K = 1024 (8 tiles, one per wave), 1152, 2176, 18944; grids below and above the CU count
    for ki, K in enumerate((1024, 1152, 2176, 18944)):
        for ei, epi in enumerate(E4):
            M = (2, 17, 16, 32)[(ki + ei) % 4]
            out.append(Case("stream", M, K, _n(big_a if K == 1152 else 48, epi), epi, False, 3))
    # e4m3 forms
    i = 0
    for M in (1, 2, 3, 4):
        for epi in E4:
            K = (16, 400, 4112)[i % 3]
            N = (128, 512)[i % 2] if epi == DEC_SWIGLU else (16, 128, 512)[(i // 3) % 3]
            out.append(Case("fp8_valu", M, K, N, epi, False, 1))
            i += 1
    for K in (16, 400, 4112):
        out.append(Case("fp8_valu", 1, K, 16, DEC_BIAS, False, 1))
        out.append(Case("fp8_valu", 4, K, 128, DEC_SWIGLU, False, 1))
    i = 0
    for M in (2, 16, 17, 32):
        for epi in E4:
            K = (256, 2304, 18944)[i % 3]
            N = (128, 512)[i % 2] if epi == DEC_SWIGLU else (16, 128, 512)[(i // 3) % 3]
            out.append(Case("fp8_mfma", M, K, N, epi, False, 1))
            i += 1
    for K in (256, 2304, 18944):
        out.append(Case("fp8_mfma", 17, K, 16, DEC_RES, False, 1))
    return out


CASES = cases(256)
FORMS = ("valu", "mfma", "mfma2", "split", "stream", "fp8_valu", "fp8_mfma")


def form_of(case, cus):
    return expected_form(case.M, case.N, case.K, case.epi, case.norm, case.v2, cus, fp8=case.form.startswith("fp8"))
