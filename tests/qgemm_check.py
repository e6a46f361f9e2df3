"""Host model, per-element bound and structured inputs for the quantised prefill GEMMs v3d_gemm_fp8 and v3d_gemm_mxfp4 (both are
q8_gemm_tile, csrc/gemm_q8_tile.h).

Not a conftest: test modules import it (`import qgemm_check as qc`).  Built on tests/gemm_check.py: the rounding chains, the SwiGLU
interval, compare() and the residual / bias recipe of the exact family are the GEMM checker's; this module adds the decoding of the
operands and the three input families in the kernels' own number formats.

Operands, as a kernel call takes them (a Case): e4m3 activation bytes qa [M, K] with f32 row scales sa [M]; weights either e4m3 bytes
[N, K] with f32 column scales sw [N] (fmt "e4m3") or MXFP4 codes [N, K / 2] with E8M0 bytes [N, K / 32] (fmt "mxfp4"); bias [N], res
[M, N]; the epilogue code (gemm_check's EPI_NONE / EPI_BIAS / EPI_RES / EPI_SWIGLU = the kernels' codes 0 / 1 / 5 / 6), the output
type, and every tensor as the view the kernel gets (leading dimensions are strides).

Decoding.  An e4m3 byte decodes through a 256-entry table (E4M3_VALUES: 254 finite values, 0x7F and 0xFF NaN; subnormals m 2^-9, normals
(8 + m) 2^(e - 10)); MXFP4 through mxfp4_check.dequantize.  Both are exact in f64, and so is the product with a power-of-two scale.

Rounding chain (q8_epilogue): v = acc (sa sw) for e4m3, acc sa for MXFP4 (block exponents are inside the accumulator), + bias, one
rounding to the output type; RES adds the residual to that rounded value in f32 and rounds once more; SWIGLU forms
round(round(silu(round(gate))) round(up)) on the interleaved [gate64 | up64] layout.  These are gemm_check.reference()'s chains; its
silu interval [lo, hi] and func_err("silu") apply, q8_silu being gemm.hip's formula.

Bound for inexact inputs, per element, from reference quantities only (no rms term; h = 2^-8 / 2^-11, mag = |A| |W|^T + |bias| on the
dequantised, scaled operands):
  lin = C_ACC (K / 128 + 128) 2^-24 mag + (h + 3 2^-24) |y|        (+ gemm_check.TINY for f16)
A term of the sum passes through at most 128 roundings inside its own 16 x 16 x 128 MFMA (taken as no worse than a sequential f32
chain over its 128 products) and one add per later K-step: depth <= K / 128 + 128.  3 2^-24 covers sa sw, the product with the
accumulator and the bias add, contracted or not.  The epilogues propagate lin as in gemm_check.
C_ACC.  Derived: 2, as in gemm_check (the sequential f32 emulation of tests/test_qgemm_check_cpu.py keeps it).  The device does NOT keep it
on operands of wide dynamic range while the gather and exact families are bit for bit everywhere - the case of decision rule 2 of the
device tests, so C_ACC = 32, at most twice the measured need of 19.9 (MEASURED below); every mutation of the CPU file is still reported
at that constant.  The need comes from the instruction, not from the tile: it shows at 1 x 256 x 128, ONE
v_mfma_scale_f32_16x16x128_f8f6f4 per output, where the error reaches 2300 x 2^-24 of the largest |product| of the sum (a sequential
f32 chain stays below 128 x 2^-24 of it).

Input families, per format (each returns a Case; the device tests and the CPU emulation run the same ones):
  gather  one operand one-hot (code 1.0 at k0(m) = (m stride + shift) mod K, odd stride), the other holding distinct values; scales are
          powers of two that differ from row to row (2^-(m % 4)) and from column to column (decode_check.fp8_row_scales, 2^-((n + n / 64) % 4): the gate / up
          partner differs, n + 16 where it crosses a multiple of 64), so the output is ONE dequantised element times its scales, exactly, and gather_explain() names
          the k a wrong element was read from.  e4m3 operands run through all 254 finite bytes (subnormals 0x01-0x07 and -0 included);
          the MXFP4 operand has all 16 codes in both nibble positions (asserted) and another exponent in every block of every row.
          gather_exponent_walk(): the exponent byte over 103..151 and the edges 0, 1, 254, with the activation code and sa chosen per
          row so that the accumulator is a normal f32 and the output a normal 16-bit number.
  exact   integer e4m3 codes (integers the format holds, up to amax), all 16 e2m1 values with block exponents 127 +- d that differ from
          block to block and row to row, power-of-two sa / sw per row / column, bias and res as gemm_check.exact_inputs makes them.
          Asserted on the host: (sum of |products| + |bias|) in units of the smallest product quantum < 2^24, so every partial sum is an
          exact f32 number in any order; the amplitude narrows with K until that holds (e4m3: amax 64 .. 16; MXFP4: activations <= 64 with
          d = 3 down to activations <= 4 with d = 2 or <= 2 with d = 1 at K = 18944).  compare(exact=True) asserts |y| < 60000 for f16; the tests assert
          needs_rounding > 1/2.  NONE / BIAS / RES must equal `rounded`, SWIGLU must fall inside [lo, hi].
  random  draw 0: every finite byte / code uniformly, exponent bytes 121..133, arbitrary f32 scales; draw 1: Gaussians with the heavy
          channel of test_gpu_fp8._rand through the project's quantisers (the host restatements on the CPU).  Checked with the bound.

MEASURED (MI355X; the table is also in DESIGN.md section 2).
  exact and gather families: bit for bit for both formats, both output types, all four epilogues, every shape, strided and in place - the
  scaled f8f6f4 MFMA adds exactly representable products of this range exactly; decision rule 1 (the narrow variant) was not needed.
  random family, smallest C_ACC that explains every output (NONE epilogue, f16 / bf16, three seeds per shape below K = 18944):
      draw 0 (uniform bytes)       e4m3 8.2 (1 x 256 x 128), 9.0 / 7.6 (255 / 257 x 256 x 384), 12.6 (130 x 768 x 256), 15.0 (2305 x 512 x 256),
                                   0.55 (300 x 256 x 18944); MXFP4 7.7, 11.0 / 10.4, 19.1, 19.9, 0.41       -> worst 19.9
      draw 1 (quantised Gaussians) e4m3 0.43, 3.6 / 2.7, 3.0, 4.8, 0.06; MXFP4 0.0, 0.86 / 1.6, 1.2, 2.0, 0.03
  what the adder keeps (v3d_gemm_fp8, one K-step: two products +-B that cancel and 126 equal products s): the whole sum for
  s >= 2^-13 B, 120 / 126 of it for 2^-27 B <= s <= 2^-14 B, 112 / 126 below - the products are added in groups (8, then 16 consecutive k
  by these counts) and an addend under a window below its group's largest product is dropped.  Inputs that exceed C_ACC = 32 therefore
  exist (up to 7 addends of 2^-13 of the largest per group of 8); the families here are fixed and the kernels repeat bit for bit.
  worst |err| / bound on the random family at C_ACC = 32 (tests/test_gpu_qgemm_f64.py::test_zz_report_worst_ratios; these maxima are the
  output rounding h |y|): e4m3 none 0.914 bias 0.928 res 0.968 swiglu 0.737; MXFP4 none 0.930 bias 0.921 res 0.923 swiglu 0.676
"""
import collections
import math

import numpy as np
import torch

import gemm_check as gc
import mxfp4_check as MX
from decode_check import fp8_row_scales
from gemm_check import EPI_BIAS, EPI_NONE, EPI_RES, EPI_SWIGLU  # noqa: F401

EPIS = (EPI_NONE, EPI_BIAS, EPI_RES, EPI_SWIGLU)
EPI_NAMES = {EPI_NONE: "none", EPI_BIAS: "bias", EPI_RES: "res", EPI_SWIGLU: "swiglu"}
FORMATS = ("e4m3", "mxfp4")
C_ACC = 32.0            # derived: 2 (gemm_check's); the device needs 19.9 on the random family (MEASURED, decision rule 2): <= 2 x 19.9
LIN_REL = 3 * 2.0 ** -24
E4M3_ONE = 0x38
E2M1_ONE = 0x2
WALK_EXPONENTS = tuple(range(103, 152)) + (0, 1, 254)

Case = collections.namedtuple("Case", "fmt qa sa w wx bias res")      # wx = sw (e4m3) or the E8M0 bytes (mxfp4)


def depth(K):
    return K / 128.0 + 128.0


def _e4m3_values():
    b = np.arange(256)
    e, m = (b >> 3) & 15, b & 7
    v = np.where(e == 0, m * 2.0 ** -9, (8 + m) * np.exp2(e - 10.0))
    v = np.where(b & 128, -v, v)
    v[[0x7F, 0xFF]] = np.nan
    return torch.from_numpy(v)


E4M3_VALUES = _e4m3_values()


def decode_e4m3(q, table=None):
    """uint8 tensor -> f64 values (NaN for 0x7F / 0xFF), on q's device."""
    t = (E4M3_VALUES if table is None else table).to(q.device)
    return t[q.long()]


def e4m3_byte(v):
    """f64 tensor of e4m3 numbers -> their bytes (asserted exact)."""
    q = v.to(torch.float8_e4m3fn)
    assert bool((q.double() == v).all()), "not an e4m3 number"
    return q.view(torch.uint8)


def e4m3_integers(amax):
    """The integers 0 .. amax that e4m3 holds (4 significant bits)."""
    return [i for i in range(amax + 1) if i < 16 or i % (1 << (i.bit_length() - 4)) == 0]


def dequant(c, table=None):
    """Case -> (A, W) in f64 with the scales folded in: y = A W^T is the kernel's linear output before the bias."""
    a = decode_e4m3(c.qa, table) * c.sa.double()[:, None]
    if c.fmt == "e4m3":
        w = decode_e4m3(c.w, table) * c.wx.double()[:, None]
    else:
        w = torch.from_numpy(MX.dequantize(c.w, c.wx)).to(c.qa.device)
    return a, w


def compare(got, c, dt, epi, exact=False, table=None):
    """gemm_check.compare() of got [M, n_out] against the model of Case c -> ratio, unequal, outside, ymax, needs_rounding."""
    a, w = dequant(c, table)
    return gc.compare(got, a, w, c.bias, c.res, epi, exact=exact, lin_rel=LIN_REL, dt=dt, depth=depth(a.shape[1]) * C_ACC / gc.C_ACC)


def old_rule(got, c, dt, epi):
    """The rule of tests/test_gpu_fp8.py / test_gpu_fp4.py per element -> bool [M, n_out]: err <= slack (eps |ref| + 4 eps rms(ref)
    [x 0.25 without an epilogue]) against the f64 chain with the kernels' intermediate rounding points, slack 3 for RES / SWIGLU."""
    a, w = dequant(c)
    ref = a @ w.T
    if epi == EPI_BIAS:
        ref = ref + c.bias.double()
    elif epi == EPI_RES:
        ref = gc.rnd(ref, dt) + c.res.double()
    elif epi == EPI_SWIGLU:
        g, u = gc.split_gate_up(gc.rnd(ref, dt))
        ref = gc.rnd(gc.silu(g), dt) * u
    eps = gc.H[dt]
    slack = 3.0 if epi in (EPI_RES, EPI_SWIGLU) else 1.0
    rms = ref.pow(2).mean().sqrt()
    bound = slack * eps * ref.abs() + slack * 4 * eps * rms * (1.0 if epi != EPI_NONE else 0.25)
    return (got.double() - ref).abs() <= bound


def run(ops, c, dt, epi, out=None, res=None):
    """The kernel call of Case c."""
    kw = dict(bias=c.bias if epi == EPI_BIAS else None, res=(c.res if res is None else res) if epi == EPI_RES else None, epilogue=epi, out=out)
    if c.fmt == "e4m3":
        return ops.gemm_fp8(c.qa, c.sa, c.w, c.wx, dt, **kw)
    return ops.gemm_mxfp4(c.qa, c.sa, c.w, c.wx, dt, **kw)


# ------------------------------------------------------------------------------ inputs


def _gen(seed, device):
    return torch.Generator(device=device).manual_seed(seed)


def row_scales(M, shift=0, device="cpu"):
    return torch.exp2(-((torch.arange(M, device=device) % 4) + shift).float())


def all_bytes(rows, cols, device="cpu"):
    """[rows, cols] uint8 running through the 254 finite e4m3 bytes; two neighbours in a row or a column never agree."""
    b = (torch.arange(rows * cols, device=device).reshape(rows, cols) * 37 + torch.arange(rows, device=device)[:, None] * 11) % 254
    return (b + (b >= 127).long()).to(torch.uint8)


def mxfp4_codes(N, K, device="cpu"):
    """[N, K] codes 0..15: all 16 in the even and in the odd k of every row (asserted)."""
    n = torch.arange(N, device=device)[:, None]
    k = torch.arange(K, device=device)[None, :]
    c = ((n * 7 + k * 5 + (k >> 1) * 3 + (k >> 5)) % 16).to(torch.uint8)
    for par in (0, 1):
        assert all(len(set(r.tolist())) == 16 for r in c[:4, par::2].cpu()), "a nibble position misses a code"
    return c


def block_exponents(N, K, device="cpu", d=4):
    """E8M0 bytes [N, K / 32] in 127 +- d: another one in every block of every row (neighbours along both axes differ)."""
    n = torch.arange(N, device=device)[:, None]
    b = torch.arange(K // 32, device=device)[None, :]
    return (127 - d + (n + n // 64 + b) % (2 * d + 1)).to(torch.uint8)


def _pack(codes):
    return (codes[:, 0::2] | (codes[:, 1::2] << 4)).to(torch.uint8)


def _one_hot(rows, K, k0, value, device):
    q = torch.zeros(rows, K, dtype=torch.uint8, device=device)
    q[torch.arange(rows, device=device), k0] = value
    return q


def _bias_res(M, N, dt, seed, device, scale=1.0):
    g = _gen(seed + 77, device)
    b = torch.randint(-250, 251, (N,), generator=g, device=device).double() * 4 * scale
    r = torch.randint(-250, 251, (M, N), generator=g, device=device).double() * 8 * scale
    for t in (b, r):
        assert bool((t.to(dt).double() == t).all()), "an exact input is not a 16-bit number"
    return b.to(dt), r.to(dt)


def gather_inputs(fmt, M, N, K, dt, stride=1, shift=0, device="cpu", transposed=False, seed=0):
    """Case of the gather family.  Plain: A one-hot reads W back; transposed: W one-hot reads A back."""
    sa = row_scales(M, 0, device)
    bias, res = _bias_res(M, N, dt, seed, device, 2.0 ** -6)
    if not transposed:
        qa = _one_hot(M, K, gc.gather_k0(M, K, stride, shift, device), E4M3_ONE, device)
        if fmt == "e4m3":
            return Case(fmt, qa, sa, all_bytes(N, K, device), fp8_row_scales(N, 0, device), bias, res)
        return Case(fmt, qa, sa, _pack(mxfp4_codes(N, K, device)), block_exponents(N, K, device), bias, res)
    qa = all_bytes(M, K, device)
    k0 = gc.gather_k0(N, K, stride, shift, device)
    if fmt == "e4m3":
        return Case(fmt, qa, sa, _one_hot(N, K, k0, E4M3_ONE, device), fp8_row_scales(N, 0, device), bias, res)
    return Case(fmt, qa, sa, _pack(_one_hot(N, K, k0, E2M1_ONE, device)), block_exponents(N, K, device), bias, res)


def gather_exponent_walk(M, N, K, dt, device="cpu"):
    """MXFP4, A one-hot: block b of EVERY weight row carries WALK_EXPONENTS[b % 52] (K / 32 >= 52 asserted, every value met by some row's
    k0 asserted); row m reads block k0(m) / 32 with exponent E, and its activation code c = 2^clamp(127 - E, -6, 8) and scale
    sa = 2^(127 - E) / c keep the accumulator c w 2^(E - 127) a normal f32 and make the output w itself."""
    assert K // 32 >= len(WALK_EXPONENTS)
    k0 = gc.gather_k0(M, K, 45, 7, device)
    ex = torch.tensor(WALK_EXPONENTS, device=device)[torch.arange(K // 32, device=device) % len(WALK_EXPONENTS)]
    assert set(ex[k0 // 32].tolist()) == set(WALK_EXPONENTS), "a row must read every exponent of the walk"
    t = 127 - ex[k0 // 32]                                        # the output wants 2^t
    lc = t.clamp(-6, 8)
    qa = torch.zeros(M, K, dtype=torch.uint8, device=device)
    qa[torch.arange(M, device=device), k0] = e4m3_byte(torch.exp2(lc.double()))
    sa = torch.exp2((t - lc).float())
    assert bool(torch.isfinite(sa).all()) and bool((sa >= 2.0 ** -126).all())
    bias, res = _bias_res(M, N, dt, 0, device, 2.0 ** -6)
    return Case("mxfp4", qa, sa, _pack(mxfp4_codes(N, K, device)), ex.to(torch.uint8)[None, :].expand(N, -1).contiguous(), bias, res)


def gather_explain(got, c, limit=5):
    """Text for the first mismatches of a gather case without an epilogue: (m, n), the k it should have read and the k whose value it
    returned."""
    a, w = dequant(c)
    want = a @ w.T
    g = got.double()
    bad = (g != want).nonzero()
    lines = [f"{bad.shape[0]} of {want.numel()} outputs differ"]
    for m, n in bad[:limit].tolist():
        prod = a[m] * w[n]
        exp = prod.abs().argmax().item()
        alt = a[m].abs().max() * w[n] if (a[m] != 0).sum() == 1 else a[m] * w[n].abs().max()
        hit = (alt == g[m, n]).nonzero().flatten().tolist()
        lines.append(f"  out[{m}, {n}] = {g[m, n].item()} want {want[m, n].item()} (k = {exp}); that value sits at k = {hit[:4] or 'nowhere in the row'}")
    return "\n".join(lines)


def _pick(values, shape, g, device):
    v = torch.tensor(values, dtype=torch.float64, device=device)
    idx = torch.randint(0, len(values), shape, generator=g, device=device)
    sign = torch.randint(0, 2, shape, generator=g, device=device).double() * 2 - 1
    return v[idx] * sign


def exact_inputs(fmt, M, N, K, dt, epi=EPI_NONE, seed=0, device="cpu"):
    """Case of the exact family (module docstring).  Output scale: standard deviation about 1000 (most outputs need rounding), about 2
    for SwiGLU (silu away from its asymptotes); bias and res scaled alike."""
    g = _gen(seed, device)
    bmax = 1000.0 if epi == EPI_BIAS else 0.0
    target = 2.0 if epi == EPI_SWIGLU else 1000.0
    spread = 64.0                                                 # sa sw varies by 2^-6 over rows and columns: bias counts in the smallest
    if fmt == "e4m3":
        for amax in (64, 32, 16, 8):
            ints = e4m3_integers(amax)
            ms = sum(i * i for i in ints) / len(ints)
            std, quantum, total = ms * math.sqrt(K), 1.0, float(K) * amax * amax
            s = max(0, round(math.log2(std / target)))
            if total + bmax * spread * 2.0 ** s < 2 ** 24:
                break
        a, wv, d = _pick(ints, (M, K), g, device), _pick(ints, (N, K), g, device), 0
    else:
        for amax, d in ((64, 3), (32, 3), (16, 3), (8, 3), (4, 2), (2, 1)):
            ints = e4m3_integers(amax)
            ms_a = sum(i * i for i in ints) / len(ints)
            std = math.sqrt(ms_a * 10.4 * 4.0 ** d / 3 * K)         # e2m1 mean square 10.4; exponents spread over +- d
            quantum, total = 0.5 * 2.0 ** -d, float(K) * amax * 6 * 2.0 ** d
            s = max(0, round(math.log2(std / target)))
            if total / quantum + bmax * spread / quantum * 2.0 ** s < 2 ** 24:
                break
        a = _pick(ints, (M, K), g, device)
    s = max(0, round(math.log2(std / target)))
    assert total / quantum + bmax * spread / quantum * 2.0 ** s < 2 ** 24, "a partial sum could leave the exact range of f32"
    bias, res = _bias_res(M, N, dt, seed, device, 1.0 if target > 2 else 2.0 ** -8)
    qa = e4m3_byte(a)
    if fmt == "e4m3":
        sa, sw = row_scales(M, s // 2, device), fp8_row_scales(N, s - s // 2, device)
        c = Case(fmt, qa, sa, e4m3_byte(wv), sw, bias, res)
    else:
        sa = row_scales(M, s, device)
        codes = torch.randint(0, 16, (N, K), generator=g, device=device).to(torch.uint8)
        c = Case(fmt, qa, sa, _pack(codes), block_exponents(N, K, device, d), bias, res)
    # the claim itself, on the data: sum |products| + |bias| in units of the smallest quantum of this (m, n)
    au = decode_e4m3(c.qa[:256]).abs()
    wu = decode_e4m3(c.w).abs() if fmt == "e4m3" else torch.from_numpy(MX.dequantize(c.w, c.wx)).to(device).abs()
    scale = c.sa[:256].double()[:, None] * (c.wx.double()[None, :] if fmt == "e4m3" else 1.0)
    worst = ((au @ wu.T + (bias.double().abs() / scale if epi == EPI_BIAS else 0.0)).max() / quantum).item()
    assert worst < 2 ** 24, f"sum of |products| = {worst:.3g} quanta"
    return c


def host_quantize_e4m3(x):
    """Host restatement of v3d_quantize_fp8_rows (tests/test_gpu_quantize_e4m3.py checks the kernels against it): scale = amax / 448 in
    IEEE f32, floored at the smallest normal f32, 1 for an all-zero row; bytes = e4m3 round-to-nearest-even of x (1 / scale)."""
    xf = x.float().cpu().numpy()
    amax = np.abs(xf).max(1)
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        s = np.where(amax > 0, np.maximum(amax / np.float32(448.0), np.float32(2.0 ** -126)), np.float32(1.0)).astype(np.float32)
        s = np.where(np.isnan(amax), np.float32(np.nan), s).astype(np.float32)
        inv = (np.float32(1.0) / s).astype(np.float32)
        scaled = (xf * inv[:, None]).astype(np.float32)
    q = torch.from_numpy(scaled).to(torch.float8_e4m3fn).view(torch.uint8)
    return q, torch.from_numpy(s)


def gaussian(m, k, dt, seed, outlier=True):
    """tests/test_gpu_fp8.py's _rand: Gaussians with one heavy channel."""
    g = torch.Generator(device="cpu").manual_seed(seed)
    x = torch.randn(m, k, generator=g)
    if outlier:
        x[:, 3] *= 20.0
    return x.to(dt)


def random_inputs(fmt, M, N, K, dt, draw=0, seed=0, device="cpu", ops=None):
    """Case of the random family.  draw 0: uniform finite bytes / codes, exponent bytes 121..133, arbitrary f32 scales; draw 1: Gaussians
    (heavy channel in A) through the project's quantisers - ops' kernels when ops is given, else their host restatements."""
    g = _gen(seed + 1000 * draw, "cpu")
    bias = torch.randn(N, generator=g).to(dt).to(device)
    res = torch.randn(M, N, generator=g).to(dt).to(device)
    if draw == 0:
        def finite(shape):
            b = torch.randint(0, 254, shape, generator=g)
            return (b + (b >= 127).long()).to(torch.uint8).to(device)
        rms = 2.0 ** (-12 if fmt == "mxfp4" else -9) / math.sqrt(K / 128.0)
        sa = ((0.5 + torch.rand(M, generator=g)) * rms).to(device)
        if fmt == "e4m3":
            return Case(fmt, finite((M, K)), sa, finite((N, K)), ((0.5 + torch.rand(N, generator=g)) * 2.0 ** -9).to(device), bias, res)
        q = torch.randint(0, 256, (N, K // 2), generator=g).to(torch.uint8).to(device)
        ex = torch.randint(121, 134, (N, K // 32), generator=g).to(torch.uint8).to(device)
        return Case(fmt, finite((M, K)), sa, q, ex, bias, res)
    a = gaussian(M, K, dt, seed + 11 + M).to(device)
    w = (gaussian(N, K, dt, seed + 13 + N, outlier=False).float() * K ** -0.5).to(dt).to(device)
    if ops is not None:
        qa, sa = ops.quantize_fp8_rows(a)
        qw, wx = ops.quantize_fp8_rows(w) if fmt == "e4m3" else ops.quantize_mxfp4_rows(w)
    else:
        qa, sa = host_quantize_e4m3(a)
        if fmt == "e4m3":
            qw, wx = host_quantize_e4m3(w)
        else:
            qw, wx = (torch.from_numpy(t) for t in MX.quantize(w))
    return Case(fmt, qa, sa, qw, wx, bias, res)


def strided(c, epi, dt, sentinel=-7.0):
    """The operands of Case c as views of wider buffers: lda = K + 128, ldw = K + 16 (e4m3) or K / 2 + 16 (MXFP4) bytes, lde = K / 32 + 3,
    ldr = N + 24, ldo = n_out + 8 -> (Case of views, out view [M, n_out], its buffer [M + 1, n_out + 8] filled with the sentinel)."""
    def wide(t, extra, fill=0x55):
        buf = torch.full((t.shape[0], t.shape[1] + extra), fill, dtype=t.dtype, device=t.device)
        buf[:, :t.shape[1]] = t
        return buf[:, :t.shape[1]]
    M, N = c.qa.shape[0], c.w.shape[0]
    no = gc.n_out(N, epi)
    buf = torch.full((M + 1, no + 8), sentinel, dtype=dt, device=c.qa.device)
    v = Case(c.fmt, wide(c.qa, 128), c.sa, wide(c.w, 16), c.wx if c.fmt == "e4m3" else wide(c.wx, 3), c.bias, wide(c.res, 24, 3.0))
    return v, buf[:M, :no], buf
