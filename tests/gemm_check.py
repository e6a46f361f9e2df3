"""f64 reference, per-element error bound and structured inputs for v3d_gemm (every kernel, every epilogue).

Not a conftest: test modules import it (`from gemm_check import ...`; tests/ is on sys.path under pytest).

Reference.  From the same 16-bit A, W, bias, res: y = A W^T (+ bias) in f64, in row blocks on whatever device the inputs are on.  Two
values come out of it per element:
  out      the f64 chain WITHOUT any rounding, f(y) - the centre of the bound below.  (A bound centred on the rounded chain would have to
           be twice as wide: the kernel's f32 sum may land on the other side of a 16-bit rounding boundary than y does.)
  rounded  the chain WITH the kernels' rounding points (gemm.hip: the linear output acc + bias is rounded to 16 bit once, yr; each of
           GELU-erf / GELU-tanh / ReLU / + res / round(silu(yr_gate)) * yr_up takes 16-bit inputs, computes in f32 and is rounded once
           more; the GEMV does the same).  On *exact* inputs (below) yr is known bit for bit, so `rounded` is what every kernel must
           return: torch.equal for NONE / BIAS / BIAS_RES / RES / BIAS_RELU, and for the GELUs and SwiGLU the interval
           [round(f(yr) - e), round(f(yr) + e)], e = the f32 function error alone (rounding is monotone) - no tolerance for sums.
res_mod (residual row m % res_mod), the interleaved [gate64 | up64] column layout of ops.interleave_gate_up and all four leading
dimensions are part of the reference (tensors are taken as the views the kernel gets).

Bound, per element, from reference quantities only (h = 2^-8 for bf16, 2^-11 for f16: half an ulp, relative; mag = |A| |W|^T + |bias|):
  lin     = C_ACC (K / 32 + C0) 2^-24 mag + h |y|                       (+ 2^-25 for f16: half the subnormal spacing)
            A term of the sum passes through at most 32 roundings inside its own 16 x 16 x 32 MFMA (taken as no worse than a
            sequential f32 chain over its 32 products), one f32 add per later MFMA (K / 32) and at most 3 adds of the split-K tail:
            depth <= K / 32 + 35, first order (depth) 2^-24 mag.  The GEMV's chain is K / 64 fmas per lane and 6 adds of the wave
            reduction, shorter.  C_ACC = 2 with C0 = 32 covers K / 32 + 35 with the second-order terms; both were settled on the CPU
            emulation (tests/test_gemm_check_cpu.py records the ratios), not on the kernels.
  + res     lin (1 + 2h) + h |y + res|
  ReLU      lin                                                          (Lip 1, no rounding of its own)
  GELU      1.13 lin (1 + 2h) + h |f| + e_f                               (Lip <= 1.13 for both forms)
  SwiGLU    s = silu(gate), bs = 1.1 lin_gate (1 + 2h) + h |s| + e_f;  bs |up| + |s| lin_up + bs lin_up + h |s up|   (product rule on the
            two rounded factors; their f32 product is exact: 16 resp. 22 significant bits)
e_f, the f32 evaluation error of the activation (gemm.hip gelu_erf / gelu_tanh / silu), C_FUNC 2^-23 times
  tanh form, silu   |f| (1 + |z|), z = the argument of v_exp_f32 (log2 units): x * rcp(1 + exp2(z)) is a relative computation, but an
                    argument with a few f32 roundings moves exp2(z) by ln2 |z| times that;
  erf form          |f| + |x| / 2: 0.5 x (1 + erff(x / sqrt 2)) CANCELS in its left tail (1 + erf -> 0 with an absolute error of a few
                    2^-24), so its error is absolute, about |x| 2^-24, not relative - the same holds for torch's f32 formula.  At
                    x = -3.5 (f = -1.3e-6) that is ~10 % of f, far above h |f|, and far below anything an activation of size 1 feels.
plus 2^-120 (f32 flush to zero).  C_FUNC = 4: analysis gives 2.5 (erf: erff 1-2 ulp absolute, the rounding of x / sqrt 2 and of 1 + erf,
two products) and 1.5 (tanh form, silu: 3-4 roundings in z, v_exp_f32 and v_rcp_f32 1 ulp each, one add, one product); see MEASURED
below for the device figures.  On every input of these tests e_f stays below h |f| / 50 except in gelu_erf's left tail.

MEASURED (MI355X, both GELUs and silu through the kernels' epilogues over the whole finite 16-bit grid with |x| <= 16, f64 functions as
the truth, smallest C_FUNC that explains every output; tests/test_gpu_gemm_f64.py::test_activation_function_error): 0.24 (erf form, in
its cancelling tail: -3.19e-7 returned for -2.43e-7 at x = -5.34), 0.63 (tanh form), 0.08 (silu).  C_FUNC = 4 keeps more than the margin of 2.

Inputs.
  random  Gaussians (the background of the earlier tests).
  exact   integers times a power of two in A, W, bias, res, with K amax^2 + bias < 2^24 (asserted): every partial sum is then an exact
          f32 number in any order, any tile, with or without the split-K tail, so yr = round(y) bit for bit.  amax shrinks with K so
          that |y| stays below 60000 for f16 (asserted by compare()) and grows for short K so that most outputs still need rounding.
  gather  A one-hot, row m selecting k0(m) = (m stride + shift) mod K, W holding pseudo-random normal 16-bit values per (n, k):
          out[m, n] == W[n, k0(m)] exactly, and a mismatch names the k it read instead (gather_explain).  Transposed: W one-hot.
"""
import math

import torch

EPI_NONE, EPI_BIAS, EPI_BIAS_GELU_ERF, EPI_BIAS_GELU_TANH, EPI_BIAS_RES, EPI_RES, EPI_SWIGLU, EPI_BIAS_RELU = range(8)
EPI_NAMES = ("none", "bias", "gelu_erf", "gelu_tanh", "bias_res", "res", "swiglu", "bias_relu")
HAS_BIAS = (EPI_BIAS, EPI_BIAS_GELU_ERF, EPI_BIAS_GELU_TANH, EPI_BIAS_RES, EPI_BIAS_RELU)
HAS_RES = (EPI_BIAS_RES, EPI_RES)
EXACT_EPIS = (EPI_NONE, EPI_BIAS, EPI_BIAS_RES, EPI_RES, EPI_BIAS_RELU)      # bit for bit on exact inputs

H = {torch.bfloat16: 2.0 ** -8, torch.float16: 2.0 ** -11}
C_ACC, C0 = 2.0, 32.0
LIP_GELU, LIP_SILU = 1.13, 1.1
C_FUNC = 4.0
TINY = 2.0 ** -25          # half the f16 subnormal spacing
FTZ = 2.0 ** -120
F16_MAX = 65504.0
LOG2E = 1.0 / math.log(2.0)
K_TANH = 2.0 * 0.7978845608028654 * LOG2E


def rnd(x, dt):
    """f64 -> 16 bit (round to nearest even) -> f64."""
    return x.to(dt).double()


def gelu_erf(x):
    return 0.5 * x * (1.0 + torch.erf(x * 0.70710678118654752440))


def gelu_tanh(x):
    return x * torch.sigmoid(2.0 * 0.7978845608028654 * (x + 0.044715 * x ** 3))


def silu(x):
    return x * torch.sigmoid(x)


def func_err(x, kind):
    """e_f for f64 x: the f32 evaluation error of the kernel's activation."""
    if kind == "erf":
        s = gelu_erf(x).abs() + 0.5 * x.abs()
    elif kind == "tanh":
        s = gelu_tanh(x).abs() * (1.0 + K_TANH * (x * (1.0 + 0.044715 * x * x)).abs())
    else:
        s = silu(x).abs() * (1.0 + LOG2E * x.abs())
    return C_FUNC * 2.0 ** -23 * s + FTZ


def split_gate_up(y):
    """[R, N] in the interleaved layout (per 128 columns: 64 gate, 64 up) -> gate, up [R, N / 2]."""
    R, N = y.shape
    v = y.reshape(R, N // 128, 2, 64)
    return v[:, :, 0].reshape(R, N // 2), v[:, :, 1].reshape(R, N // 2)


def n_out(N, epi):
    return N // 2 if epi == EPI_SWIGLU else N


def reference(a, w, bias=None, res=None, epi=EPI_NONE, res_mod=0, rows=None, lin_rel=0.0, dt=None, depth=None):
    """The rows `rows` (a slice, default all) of epilogue(a w^T) -> dict of f64 [R, n_out]: out, bound, rounded, and for the GELUs and
    SwiGLU lo / hi (the interval a kernel must hit when yr is exact).  ymax = max |y| (linear output) of these rows.
    lin_rel (0 for v3d_gemm): a further relative f32 rounding of the linear output, lin += lin_rel |y| (tests/decode_check.py: the e4m3
    decode rows multiply the f32 sum by the row scale once, 2^-24 |y|); w may be given in f64 (dequantised weights).
    dt, depth (tests/qgemm_check.py): the output type where a is given in f64 too (dequantised activations), and the depth of the
    summation chain where it is not K / 32 + C0."""
    dt = dt or a.dtype
    h = H[dt]
    tiny = TINY if dt == torch.float16 else 0.0
    M, K = a.shape
    N = w.shape[0]
    rows = rows if rows is not None else slice(0, M)
    A = a[rows].double()
    Wd = w.double()
    y = A @ Wd.T
    mag = A.abs() @ Wd.abs().T
    if epi in HAS_BIAS:
        y = y + bias.double()
        mag = mag + bias.double().abs()
    lin = C_ACC * (depth or K / 32.0 + C0) * 2.0 ** -24 * mag + (h + lin_rel) * y.abs() + tiny
    del mag
    ymax = y.abs().max().item()
    if dt == torch.float16:
        assert ymax < F16_MAX, f"f16 case overflows: max |y| = {ymax}"
    yr = rnd(y, dt)
    o = {"ymax": ymax}
    if epi in (EPI_NONE, EPI_BIAS):
        o.update(out=y, bound=lin, rounded=yr)
    elif epi in HAS_RES:
        idx = torch.arange(M, device=a.device)[rows]
        r = res[idx % res_mod if res_mod > 0 else idx, :N].double()
        s = y + r
        o.update(out=s, bound=lin * (1 + 2 * h) + h * s.abs() + tiny, rounded=rnd(yr + r, dt))
    elif epi == EPI_BIAS_RELU:
        o.update(out=y.clamp_min(0), bound=lin, rounded=yr.clamp_min(0))
    elif epi in (EPI_BIAS_GELU_ERF, EPI_BIAS_GELU_TANH):
        kind, f = ("erf", gelu_erf) if epi == EPI_BIAS_GELU_ERF else ("tanh", gelu_tanh)
        fy, v = f(y), f(yr)
        e = func_err(yr, kind) + 2.0 ** -23 * v.abs()
        o.update(out=fy, bound=LIP_GELU * lin * (1 + 2 * h) + h * fy.abs() + tiny + func_err(y, kind), rounded=rnd(v, dt),
                 lo=rnd(v - e, dt), hi=rnd(v + e, dt))
    elif epi == EPI_SWIGLU:
        g, u = split_gate_up(y)
        lg, lu = split_gate_up(lin)
        gr, ur = split_gate_up(yr)
        s = silu(g)
        bs = LIP_SILU * lg * (1 + 2 * h) + h * s.abs() + tiny + func_err(g, "silu")
        out = s * u
        v = silu(gr)
        e = func_err(gr, "silu") + 2.0 ** -23 * v.abs()
        p1, p2 = rnd(v - e, dt) * ur, rnd(v + e, dt) * ur
        o.update(out=out, bound=bs * u.abs() + s.abs() * lu + bs * lu + h * out.abs() + tiny, rounded=rnd(rnd(v, dt) * ur, dt),
                 lo=rnd(torch.minimum(p1, p2), dt), hi=rnd(torch.maximum(p1, p2), dt))
    else:
        raise ValueError(f"epilogue {epi}")
    return o


def compare(got, a, w, bias=None, res=None, epi=EPI_NONE, res_mod=0, exact=False, block=2048, lin_rel=0.0, dt=None, depth=None):
    """Every element of got [M, n_out] against the reference, in row blocks -> dict:
    ratio     worst |got - out| / bound (inf if any element is not finite: never written, or NaN)
    unequal   elements that differ from `rounded`;  outside: elements outside [lo, hi] (GELUs, SwiGLU; = unequal for the others)
    ymax      max |y|;  needs_rounding: share of linear outputs that are not 16-bit numbers (how much an exact case can see).
    exact=True asserts the conditions of the exact family on the result (|y| < 60000 for f16)."""
    M, N = a.shape[0], w.shape[0]
    assert tuple(got.shape) == (M, n_out(N, epi)), f"got {tuple(got.shape)}"
    worst, unequal, outside, ymax, need = 0.0, 0, 0, 0.0, 0
    for r0 in range(0, M, block):
        rows = slice(r0, min(M, r0 + block))
        ref = reference(a, w, bias, res, epi, res_mod, rows, lin_rel, dt, depth)
        g = got[rows].to(ref["out"].device).double()
        if not bool(torch.isfinite(g).all()):
            worst = float("inf")
        else:
            worst = max(worst, ((g - ref["out"]).abs() / ref["bound"]).max().item())
        ne = g != ref["rounded"]
        unequal += int(ne.sum())
        outside += int(((g < ref["lo"]) | (g > ref["hi"]) | torch.isnan(g)).sum()) if "lo" in ref else int(ne.sum())
        ymax = max(ymax, ref["ymax"])
        if exact:
            y = a[rows].double() @ w.double().T + (bias.double() if epi in HAS_BIAS else 0.0)
            need += int((rnd(y, dt or a.dtype) != y).sum())
    if exact and (dt or a.dtype) == torch.float16:
        assert ymax < 60000.0, f"exact f16 case too large: max |y| = {ymax}"
    return {"ratio": worst, "unequal": unequal, "outside": outside, "ymax": ymax, "needs_rounding": need / float(M * N)}


def old_rule_ok(got, want, dt, scale=None):
    """The rule these checks replace (tests/test_gpu_gemm.py close()): err <= tol |want| + tol scale, want an f32 torch chain."""
    tol = 1.6e-2 if dt == torch.bfloat16 else 2e-3
    got, want = got.float().cpu(), want.float().cpu()
    s = want.abs().mean().item() if scale is None else scale
    return bool(torch.all((got - want).abs() <= tol * want.abs() + tol * s))


# ------------------------------------------------------------------------------ inputs


def _gen(seed, device):
    return torch.Generator(device=device).manual_seed(seed)


def random_inputs(M, N, K, dt, seed=0, device="cpu", a_scale=0.5, w_scale=0.05, res_rows=None):
    """a [M, K], w [N, K], bias [N], res [res_rows or M, N]: the Gaussians of the earlier tests."""
    g = _gen(seed, device)
    a = (torch.randn(M, K, generator=g, device=device) * a_scale).to(dt)
    w = (torch.randn(N, K, generator=g, device=device) * w_scale).to(dt)
    b = torch.randn(N, generator=g, device=device).to(dt)
    r = torch.randn(res_rows or M, N, generator=g, device=device).to(dt)
    return a, w, b, r


def exact_amax(K):
    """Largest power of two <= 32 with amax^2 <= 30000 / sqrt(K): keeps 6.3 sigma of the sum below 60000 (f16) and K amax^2 far below 2^24."""
    amax = 32
    while amax * amax > 30000.0 / math.sqrt(K):
        amax //= 2
    return amax


def exact_inputs(M, N, K, dt, seed=0, device="cpu", target=None, res_rows=None, bmax=1000):
    """Integers in -amax .. amax (A, W), -bmax .. bmax (bias) and -2 bmax .. 2 bmax in steps of 8 (res, 16-bit numbers in both dtypes),
    all times 2^-s: s = 0 by default (sums in the thousands: most outputs need rounding);
    target = the wanted standard deviation of y for the activations (s chosen so, a power of two keeps every sum exact)."""
    g = _gen(seed, device)
    amax = exact_amax(K)
    assert K * amax * amax + bmax < 2 ** 24, "a partial sum could leave the exact range of f32"
    a = torch.randint(-amax, amax + 1, (M, K), generator=g, device=device).double()
    w = torch.randint(-amax, amax + 1, (N, K), generator=g, device=device).double()
    b = torch.randint(-bmax // 4, bmax // 4 + 1, (N,), generator=g, device=device).double() * 4
    r = torch.randint(-bmax // 4, bmax // 4 + 1, (res_rows or M, N), generator=g, device=device).double() * 8
    sa = sw = 0
    if target is not None:
        std = amax * (amax + 1) / 3.0 * math.sqrt(K)
        s = max(0, round(math.log2(std / target)))
        sa, sw = s // 2, s - s // 2
    out = []
    for t, sc in ((a, sa), (w, sw), (b, sa + sw), (r, sa + sw)):
        v = (t * 2.0 ** -sc).to(dt)
        assert bool((v.double() == t * 2.0 ** -sc).all()), "an exact input is not a 16-bit number"
        out.append(v)
    return tuple(out)


def _distinct(idx, dt):
    """Pseudo-random finite normal 16-bit values from integer indices: 8192 (bf16: 32 exponents x 128 mantissas x sign) or 32768
    (f16: 16 exponents x 1024 mantissas x sign) distinct values; two indices collide only at a distance that is a multiple of that."""
    if dt == torch.bfloat16:
        v = (idx * 4099) % 8192
        bits = ((v & 1) << 15) | ((112 + ((v >> 1) & 31)) << 7) | (v >> 6)
    else:
        v = (idx * 16411) % 32768
        bits = ((v & 1) << 15) | ((8 + ((v >> 1) & 15)) << 10) | (v >> 5)
    return (bits - ((bits >> 15) << 16)).to(torch.int16).view(dt)          # the 16 bits as a signed word


def gather_k0(M, K, stride=1, shift=0, device="cpu"):
    assert stride % 2 == 1
    return (torch.arange(M, device=device) * stride + shift) % K


def gather_inputs(M, N, K, dt, stride=1, shift=0, device="cpu", transposed=False):
    """(a, w, want): a one-hot per row at k0(m), w distinct values -> want[m, n] = w[n, k0(m)];
    transposed: w one-hot per row n at k0(n), a distinct values -> want[m, n] = a[m, k0(n)]."""
    if transposed:
        k0 = gather_k0(N, K, stride, shift, device)
        w = torch.zeros(N, K, dtype=dt, device=device)
        w[torch.arange(N, device=device), k0] = 1
        a = _distinct(torch.arange(M * K, device=device).reshape(M, K), dt)
        return a, w, a[:, k0]
    k0 = gather_k0(M, K, stride, shift, device)
    a = torch.zeros(M, K, dtype=dt, device=device)
    a[torch.arange(M, device=device), k0] = 1
    w = _distinct(torch.arange(N * K, device=device).reshape(N, K), dt)
    return a, w, w[:, k0].T.contiguous()


def gather_explain(got, a, w, want, transposed=False, limit=5):
    """Text for the first mismatches of a gather case: (m, n), the k it should have read and the k whose value it returned."""
    bad = (got != want).nonzero()
    lines = [f"{bad.shape[0]} of {want.numel()} outputs differ"]
    src = a if transposed else w
    for m, n in bad[:limit].tolist():
        row = src[m] if transposed else src[n]
        hit = (row == got[m, n]).nonzero().flatten().tolist()
        exp = (w[n] if transposed else a[m]).float().argmax().item()
        lines.append(f"  out[{m}, {n}] = {got[m, n].item()} want {want[m, n].item()} (k = {exp}); that value sits at k = {hit[:4] or 'nowhere in the row'}")
    return "\n".join(lines)
