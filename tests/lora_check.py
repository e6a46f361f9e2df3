"""f64 references, per-element error bounds and structured inputs for the LoRA rank products (csrc/lora.hip: v3d_lora_down,
v3d_lora_wgrad) and for the rule of a LoRA-adapted Linear built on them.

Not a conftest: test modules import it (`from lora_check import ...`; tests/ is on sys.path under pytest).  It imports gemm_check for
the constants, the 16-bit rounding and the input families, so that the two checkers cannot drift apart.

Products, from the same 16-bit operands, in f64 (on whatever device the operands are on):
  down    y = scale x p^T          x [M, K], p [R, K]     out [M, R], rounded to the operands' dtype
  wgrad   g = scale u^T x          u [M, R], x [M, K]     out [R, K] in f32 or 16 bit; the sum runs over the M rows
Each reference returns `out` (the f64 value, the centre of the bound), `bound` and `rounded` (out rounded to the output dtype: what a
kernel must return bit for bit when every partial sum is an exact f32 number).

Bound, per element, from reference quantities only, in gemm_check's form (h = 2^-8 bf16, 2^-11 f16, 0 for an f32 output;
mag = |scale| |a| |b|^T):
  lin = C_ACC (depth / 32 + C0) 2^-24 mag + (h + 2^-24) |y|                  (+ 2^-25 for an f16 output)
  down    depth = K: K / 32 MFMAs of 32 products in ONE accumulator, k ascending - the chain of gemm_check without a split;
  wgrad   depth = M + n_chunks: a chunk of c rows is c / 32 MFMAs in one accumulator (at most 32 + c / 32 roundings on a term's way),
          then at most n_chunks - 1 f32 adds of the partial slabs in chunk order.  c >= 32, so n_chunks <= M / 32 and the true depth
          c / 32 + 32 + n_chunks stays below 2 (M / 32) + 32 <= C_ACC ((M + n_chunks) / 32 + C0).
  The 2^-24 |y| is the one f32 product with `scale` before the only rounding (exact when scale is a power of two).
C_ACC = 2 and C0 = 32 are gemm_check's; tests/test_lora_check_cpu.py holds an f32 emulation of both summations (32-wide blocks, chunked,
in order) to them and records the worst ratios.  Nothing here was tuned on the kernels.

Inputs (both products):
  random  Gaussians.
  exact   integers times a power of two with depth amax^2 < 2^24 (asserted) and scale a power of two: every partial sum is an exact
          f32 number in any order and any chunking, so the kernel's output equals `rounded` bit for bit.
  gather  one operand one-hot, the other pseudo-random distinct 16-bit values: down with p one-hot returns x[m, k0(r)]; wgrad with u
          one-hot returns x[m0(r), k] - a mismatch names the k / the row it read instead (gemm_check.gather_explain).

The rule of a LoRA linear (W [N, K], A [r, K], B [N, r], s = lora_alpha / r), with its rounding points:
  forward   u = round(x A^T);  y = round(round(x W^T (+ bias)) + round(s u B^T))      (the up-projection is a second GEMM whose
            epilogue adds the rounded base output as its residual: gemm_check's `+ res` form)
  backward  du = round(s dy B);  dA = du^T x;  dB = s dy^T u;  dx = round(round(dy W) + round(du A));  no dW
  merge     W' = round(W + round(s B A)), B A accumulated in f32.
lora_linear_f64 / lora_linear_grads_f64 return the UNROUNDED f64 chain (what torch autograd in f64 gives on the same operands);
merge_f64 the merge with its two roundings.
"""
import math

import torch

from gemm_check import C0, C_ACC, F16_MAX, H, TINY, _distinct, _gen, exact_amax, gather_explain, gather_inputs, rnd  # noqa: F401

ULP32 = 2.0 ** -24


def _h_out(dt):
    return H.get(dt, 0.0)


def _tiny(dt):
    return TINY if dt == torch.float16 else 0.0


def round_out(y, dt):
    """f64 -> the output dtype (16 bit or f32, round to nearest even) -> f64."""
    return y.to(dt).double()


def down_reference(x, p, scale=1.0):
    """scale x p^T -> dict(out, bound, rounded), f64 [M, R]."""
    dt = x.dtype
    K = x.shape[1]
    X, P = x.double(), p.double()
    y = scale * (X @ P.T)
    mag = abs(scale) * (X.abs() @ P.abs().T)
    if dt == torch.float16:
        assert y.abs().max().item() < F16_MAX, "f16 case overflows"
    bound = C_ACC * (K / 32.0 + C0) * ULP32 * mag + (H[dt] + ULP32) * y.abs() + _tiny(dt)
    return {"out": y, "bound": bound, "rounded": round_out(y, dt)}


def wgrad_reference(u, x, scale=1.0, g_dtype=torch.float32, n_chunks=1):
    """scale u^T x -> dict(out, bound, rounded), f64 [R, K]; n_chunks = ceil(M / v3d_lora_wgrad_chunk(M, R, K))."""
    M = u.shape[0]
    U, X = u.double(), x.double()
    y = scale * (U.T @ X)
    mag = abs(scale) * (U.abs().T @ X.abs())
    if g_dtype == torch.float16:
        assert y.abs().max().item() < F16_MAX, "f16 case overflows"
    bound = C_ACC * ((M + n_chunks) / 32.0 + C0) * ULP32 * mag + (_h_out(g_dtype) + ULP32) * y.abs() + _tiny(g_dtype)
    return {"out": y, "bound": bound, "rounded": round_out(y, g_dtype)}


def verdict(got, ref):
    """got against a reference dict -> dict(ratio, unequal): worst |got - out| / bound (inf when an element is not finite: NaN, or
    never written over a NaN prefill) and the number of elements that differ from `rounded`."""
    g = got.to(ref["out"].device).double()
    assert g.shape == ref["out"].shape, f"got {tuple(g.shape)}, reference {tuple(ref['out'].shape)}"
    if not bool(torch.isfinite(g).all()):
        ratio = float("inf")
    else:
        # bound == 0 only where every product is zero: there the kernel must return exactly 0
        err = (g - ref["out"]).abs()
        ratio = torch.where(ref["bound"] > 0, err / ref["bound"].clamp_min(1e-300), torch.where(err > 0, math.inf, 0.0)).max().item()
    return {"ratio": ratio, "unequal": int((g != ref["rounded"]).sum())}


# ------------------------------------------------------------------------------ inputs


def random_operands(rows_a, rows_b, depth, dt, seed=0, device="cpu", a_scale=0.5, b_scale=0.05):
    """a [rows_a, depth], b [rows_b, depth] Gaussians (the K-contiguous form; transpose for wgrad's row-major operands)."""
    g = _gen(seed, device)
    a = (torch.randn(rows_a, depth, generator=g, device=device) * a_scale).to(dt)
    b = (torch.randn(rows_b, depth, generator=g, device=device) * b_scale).to(dt)
    return a, b


def exact_operands(rows_a, rows_b, depth, dt, seed=0, device="cpu", shift=2):
    """Integers in -amax .. amax times 2^-shift (a) and 1 (b): 16-bit numbers whose products and partial sums are exact f32 numbers,
    depth amax^2 < 2^24 asserted; amax from gemm_check.exact_amax (6.3 sigma of the sum below 60000)."""
    g = _gen(seed, device)
    amax = exact_amax(depth)
    assert depth * amax * amax < 2 ** 24, "a partial sum could leave the exact range of f32"
    a = torch.randint(-amax, amax + 1, (rows_a, depth), generator=g, device=device).double() * 2.0 ** -shift
    b = torch.randint(-amax, amax + 1, (rows_b, depth), generator=g, device=device).double()
    out = []
    for t in (a, b):
        v = t.to(dt)
        assert bool((v.double() == t).all()), "an exact input is not a 16-bit number"
        out.append(v)
    return tuple(out)


def down_inputs(family, M, K, R, dt, seed=0, device="cpu"):
    """(x [M, K], p [R, K], scale, want or None): want is the exact output of the gather family."""
    if family == "random":
        x, p = random_operands(M, R, K, dt, seed, device)
        return x, p, 0.25, None
    if family == "exact":
        x, p = exact_operands(M, R, K, dt, seed, device)
        return x, p, 0.5, None
    x, p, want = gather_inputs(M, R, K, dt, stride=5, shift=3, device=device, transposed=True)      # p one-hot: out[m, r] = x[m, k0(r)]
    return x, p, 1.0, want


def wgrad_inputs(family, M, R, K, dt, seed=0, device="cpu"):
    """(u [M, R], x [M, K], scale, want or None, (a, w)): (a, w) are the gather family's operands in gemm_check's orientation, for
    gather_explain (a [R, M] one-hot at row m0(r), w [K, M])."""
    if family == "random":
        ut, xt = random_operands(R, K, M, dt, seed, device, a_scale=0.05, b_scale=0.5)
        return ut.T.contiguous(), xt.T.contiguous(), 0.25, None, None
    if family == "exact":
        ut, xt = exact_operands(R, K, M, dt, seed, device)
        return ut.T.contiguous(), xt.T.contiguous(), 0.5, None, None
    a, w, want = gather_inputs(R, K, M, dt, stride=5, shift=3, device=device)                        # u one-hot: g[r, k] = x[m0(r), k]
    return a.T.contiguous(), w.T.contiguous(), 1.0, want, (a, w)


# ------------------------------------------------------------------------------ emulation of the kernels' summation (CPU, f32)


def emulate_down(x, p, scale, mut=None):
    """csrc/lora.hip lora_down_kernel in f32: one accumulator, k in 32-wide blocks ascending, one product with scale, one rounding."""
    dt = x.dtype
    xf, pf = x.float().clone(), p.float()
    K = xf.shape[1]
    if mut == "kstep_twice":
        xf[:, 64:128] = xf[:, 0:64]
    acc = torch.zeros(xf.shape[0], pf.shape[0])
    for k in range(0, K, 32):
        if mut == "drop_block" and k == 32 * ((K // 32) // 2):
            continue
        acc = acc + xf[:, k:k + 32] @ pf[:, k:k + 32].T
    if mut == "double_round":
        return (acc.to(dt).float() * scale).to(dt)
    return (acc * scale).to(dt)


def emulate_wgrad(u, x, scale, g_dtype, chunk, mut=None):
    """lora_wgrad_partial_kernel + lora_wgrad_sum_kernel in f32: per chunk of `chunk` rows one accumulator over 32-row blocks in order,
    the chunks' slabs added in order, one product with scale, one rounding."""
    uf, xf = u.float(), x.float()
    M = uf.shape[0]
    total = None
    for c0 in range(0, M, chunk):
        c1 = min(M, c0 + chunk)
        acc = torch.zeros(uf.shape[1], xf.shape[1])
        for r in range(c0, c1, 32):
            r1 = min(c1, r + 32)
            if mut == "tail_rows_dropped" and r1 - r < 32:
                continue
            acc = acc + uf[r:r1].T @ xf[r:r1]
        if mut == "slabs16":
            acc = acc.to(torch.bfloat16).float()
        if mut == "last_chunk_dropped" and c1 == M and c0 > 0:
            continue
        total = acc if total is None else total + acc
    return (total * scale).to(g_dtype)


# ------------------------------------------------------------------------------ the rule of a LoRA linear


def lora_linear_f64(x, w, bias, a, b, s):
    """y = x W^T (+ bias) + s (x A^T) B^T in f64 without roundings; operands of any dtype."""
    X = x.double()
    y = X @ w.double().T + s * ((X @ a.double().T) @ b.double().T)
    return y + bias.double() if bias is not None else y


def lora_linear_grads_f64(x, w, a, b, s, dy):
    """The rule's backward in f64 without roundings -> dict(dx, dA, dB) (no dW: the base weight is frozen)."""
    X, DY, A, B = x.double(), dy.double(), a.double(), b.double()
    u = X @ A.T
    du = s * (DY @ B)
    return {"dx": DY @ w.double() + du @ A, "dA": du.T @ X, "dB": s * (DY.T @ u)}


def merge_f64(w, a, b, s):
    """W' = round16(W + round16(s B A)), the product in f64 (the device accumulates it in f32): f64 [N, K] of 16-bit numbers."""
    dt = w.dtype
    delta = rnd(s * (b.double() @ a.double()), dt)
    return rnd(w.double() + delta, dt)


def merge_bound(w, a, b, s):
    """Per-element bound of a device merge against the UNROUNDED f64 W + s B A: the product's f32 accumulation over r terms (lin of
    gemm_check with depth r, s folded into the B operand: one more 16-bit rounding of s B, h |s B| |A|), its rounding, and the sum's."""
    dt = w.dtype
    h = H[dt]
    A, B = a.double(), b.double()
    r = a.shape[0]
    prod = s * (B @ A)
    mag = abs(s) * (B.abs() @ A.abs())
    lin = C_ACC * (r / 32.0 + C0) * ULP32 * mag + h * mag + h * prod.abs() + _tiny(dt)
    return lin * (1 + 2 * h) + h * (w.double() + prod).abs() + _tiny(dt)


def _acc(depth, mag):
    return C_ACC * (depth / 32.0 + C0) * ULP32 * mag


def linear_bounds(x, w, bias, a, b, s, dy, g_dtype, chunks_a=1, chunks_b=1):
    """The whole rule of one LoRA linear against the UNROUNDED f64 chain: dict name -> (out, bound) for y, dx, dA, dB, composed from
    the products' own bounds and the propagation of the two rounded intermediates (every quantity from the f64 reference):
      e_u  = down bound of u = x A^T            e_du = down bound of du = s dy B
      y    base lin (depth K) + up lin (depth Rp, magnitude |s| (|u| + e_u) |B|^T, + h |s B| rounding when s is no power of two)
           + |s| e_u |B|^T, all (1 + 2 h), + h |y|                                  (gemm_check's `+ res` form)
      dx   base lin (depth N) + lin of du A (depth Rp) + e_du |A|, all (1 + 2 h), + h |dx|
      dA   wgrad bound of du^T x (depth M + chunks) + e_du^T |x|
      dB   wgrad bound of s dy^T u + |s| |dy|^T e_u"""
    dt = x.dtype
    h, tiny = H[dt], _tiny(dt)
    X, W, A, B, DY = x.double(), w.double(), a.double(), b.double(), dy.double()
    M, K = X.shape
    N, R = B.shape
    Rp = (R + 63) // 64 * 64
    pow2 = math.log2(abs(s)).is_integer()
    hs = 0.0 if pow2 else h
    u = X @ A.T
    e_u = _acc(K, X.abs() @ A.abs().T) + (h + ULP32) * u.abs() + tiny
    base = X @ W.T + (bias.double() if bias is not None else 0.0)
    lin_base = _acc(K, X.abs() @ W.abs().T + (bias.double().abs() if bias is not None else 0.0)) + h * base.abs() + tiny
    up = s * (u @ B.T)
    mag_up = abs(s) * ((u.abs() + e_u) @ B.abs().T)
    lin_up = _acc(Rp, mag_up) + hs * mag_up + h * up.abs() + tiny
    y = base + up
    out = {"y": (y, (lin_base + lin_up + abs(s) * (e_u @ B.abs().T)) * (1 + 2 * h) + h * y.abs() + tiny)}
    du = s * (DY @ B)
    e_du = _acc(N, abs(s) * (DY.abs() @ B.abs())) + (h + ULP32) * du.abs() + tiny
    dxb = DY @ W
    lin_dxb = _acc(N, DY.abs() @ W.abs()) + h * dxb.abs() + tiny
    dxa = du @ A
    mag_dxa = (du.abs() + e_du) @ A.abs()
    lin_dxa = _acc(Rp, mag_dxa) + h * dxa.abs() + tiny
    dx = dxb + dxa
    out["dx"] = (dx, (lin_dxb + lin_dxa + e_du @ A.abs()) * (1 + 2 * h) + h * dx.abs() + tiny)
    ho, to = _h_out(g_dtype), _tiny(g_dtype)
    dA = du.T @ X
    out["dA"] = (dA, _acc(M + chunks_a, (du.abs() + e_du).T @ X.abs()) + (ho + ULP32) * dA.abs() + e_du.T @ X.abs() + to)
    dB = s * (DY.T @ u)
    out["dB"] = (dB, _acc(M + chunks_b, abs(s) * (DY.abs().T @ (u.abs() + e_u))) + (ho + ULP32) * dB.abs() + abs(s) * (DY.abs().T @ e_u) + to)
    return out


def worst_ratio(got, out, bound):
    g = got.to(out.device).double()
    if not bool(torch.isfinite(g).all()):
        return float("inf")
    return ((g - out).abs() / bound.clamp_min(1e-300)).max().item()
