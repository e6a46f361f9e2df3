"""f64 references, per-element error bounds and structured inputs for the row-wise kernels of the training path: v3d_rmsnorm,
v3d_layernorm, v3d_rmsnorm_grad, v3d_layernorm_grad, v3d_swiglu(_grad), v3d_gelu(_grad) and the rotation's transpose (v3d_rope_apply
on the inverse table).

Not a conftest: test modules import it (`from rowwise_check import ...`; tests/ is on sys.path under pytest).

Reference.  The mathematical function of the 16-bit inputs in f64, on whatever device the inputs are on - not another rounded chain.

Bound.  Per element, from reference quantities only; u = 2^-8 (bf16) / 2^-11 (f16) as attention_check.U, e = 2^-24 the f32 unit roundoff,
tiny = half the subnormal spacing of the 16-bit type (2^-25 for f16, 2^-134 for bf16).  A rounding to 16 bit moves v by at most half the
spacing of the type at v, hs(v) = max(u 2^floor(log2 |v|), tiny), which lies between u/2 |v| and u |v|: "u/2 |v|" below is shorthand for
hs(v) (u/2 |v| itself is exceeded by every v just above a power of two - the emulation shows it).  The rounding of an OUTPUT is taken at
|v| + (the other terms), since the kernel rounds its own value and a power of two may lie between.  One term per rounding point of the
kernels (norm_rope.hip, train.hip).  A row of `cols` elements is summed as cols/64 fused adds per lane plus six shuffle adds, so a row sum
carries at most (cols/64 + 6) e of the sum of absolute values: CH = cols/64 + 6.

  r      r = 1/sqrtf(ss/cols + eps): ss is a sum of squares (CH e, relative - every term is positive), then a division, an add, a square
         root and a division (one e each; eps itself is an f32):            |dr| <= rho r,  rho = (CH/2 + 4) e
  RMSNorm forward   y = T(w T(x r)):   n = x r is rounded to 16 bit, w n^ is exact in f32 (two 16-bit factors), y is rounded once:
         e_n = u/2 |n| + tiny + (rho + e) |n|;       |dy| <= |w| e_n + u/2 |y| + tiny
  RMSNorm backward  n^ = T(x r) as in the forward, g = dy w exact;  dot = mean(g n^);  dx = r (g - n^ dot) [+ add]:
         ddot = mean(|g| e_n) + (CH + 2) e mean|g n|                    (the rounding of n on the row dot: u/2 mean|g n|; the f32 chain + /cols)
         |ddx| <= r (|n| ddot + e_n |dot|)                                (= r (u/2 |n| |dot| + |n| u/2 mean|g n|) to first order)
                  + 2 e r (|g| + |n dot|) + rho |dx|                      (f32 product, difference, product; r)
                  + u/2 |dx| + tiny                                       (output rounding)
         with add: T(dx) + add in f32, rounded:  + e |dx + add| + u/2 |dx + add| + tiny
         dweight = sum_rows dy n^:  sum_rows |dy| e_n  +  L e sum_rows |dy n|  +  out,
         L = 8 + 3 + ceil(n_part / 64) + 63 the f32 chain the code has (eight rows in order per wave, four waves through LDS, colsum_final:
         every 64th partial in order, then the 64 group sums in order), n_part = ceil(rows / 32); out = e |dw| (f32) or u/2 |dw| + tiny.
  LayerNorm   mean is a plain f32 sum:  dmean = (CH + 1) e mean|x|  - the term a large row mean brings; xh = (x - mean) rstd then carries
         e_xh = rstd dmean + (rho' + 2 e) |xh|,   rho' = rho + (rstd dmean)^2    (sum (x - mean^)^2 = sum (x - mean)^2 + cols dmean^2)
         and everything downstream inherits it.  xh is NOT rounded to 16 bit (the backward recomputes it in f32).
         forward  y = T(xh w + b):     |dy| <= |w| e_xh + e (|xh w| + |y|) + u/2 |y| + tiny
         backward g = dy w, sg = mean(g), sgx = mean(g xh), dx = rstd (g - sg - xh sgx) [+ add]:
         dsg = (CH + 1) e mean|g|,   dsgx = mean(|g| e_xh) + (CH + 2) e mean|g xh|
         |ddx| <= rstd (dsg + |xh| dsgx + e_xh |sgx|) + 2 e rstd (|g| + |sg| + |xh sgx|) + rho' |dx| + output terms as above
         dweight = sum_rows dy xh:  sum |dy| e_xh + L e sum |dy xh| + out;      dbias = sum_rows dy:  L e sum |dy| + out
  SwiGLU  s = 1 / (1 + __expf(-x)):  __expf is exp2 of an f32 product, so exp(-x) carries (|x| + 4) e relative;
         ds = s ((1 - s)(|x| + 4) + 3) e + 2^-126                       (2^-126: f32 results below the normal range may be flushed;
         the same absolute term is added to every f32 product of the activations)
         a = x s,  da = |x| ds + e |a|;   h = T(T(a) u):  |dh| <= |u| (da + u/2 |a| + tiny) + u/2 |h| + tiny     (T(a) u exact in f32)
         du = T(dh T(a)):   |dh| (da + u/2 |a| + tiny) + u/2 |du| + tiny
         dg = T(T(dh u) s'),  s' = s (1 + x (1 - s)):   ds' = (1 + |x|) ds + 4 e s (1 + |x|)   (1 + x (1 - s) cancels near x = -1.28: absolute)
                            |s'| (u/2 |dh u| + tiny) + |dh u| ds' + e |dg| + u/2 |dg| + tiny
  GELU   erff and tanhf are taken as accurate to 4 ulp of their result (|.| <= 1, so 4 e absolute where 1 + erf or 1 - t^2 cancel for x << 0).
         erf:   P = (1 + erf(z)) / 2, z = x / sqrt 2:   dP = (4 |erf z| + |z| erf'(z) + (1 + erf z)) e / 2;   y = T(x P):  |x| dP + 2 e |y| + u/2 |y| + tiny
                y' = P + x phi(x), phi through __expf(-x^2/2):  dy' = dP + |x| phi (x^2/2 + 6) e + 2 e (P + |x| phi);   dz = T(dy y'):  |dy| dy' + e |dz| + u/2 |dz| + tiny
         tanh:  v = k (x + c x^3), t = tanhf(v):  dt = (1 - t^2) 4 e |v| + 4 e |t|;   y = T(x (1 + t) / 2):  |x| (dt + e (1 + t)) / 2 + 2 e |y| + u/2 |y| + tiny
                y' = (1 + t)/2 + x (1 - t^2) k (1 + 3 c x^2) / 2:   dy' = dt / 2 + |x| k (1 + 3 c x^2) (2 |t| dt + 2 e + 4 e (1 - t^2)) / 2 + 2 e ((1 + t)/2 + |second term|)
         ReLU (kind 2) and its gradient are exact: bound 0, any difference is an error.
  rope   out = T(T(a c) + T(b s)) (two rounded products, exact in f32 before rounding):  u/2 (|a c| + |b s|) + 2 tiny + e |out| + u/2 |out| + tiny

C16 = 1.25 multiplies the propagated 16-bit terms and C32 = 2 the f32 ones; they cover second-order effects only (a rounding taken at the
rounded instead of the exact value) and were settled on the CPU against the emulation in tests/test_rowwise_check_cpu.py.  The final output
rounding is taken at 1.0 x.

Inputs (seeded, both dtypes; `norm_inputs(family, ...)`):
  random    the background.
  outlier   fixed columns (the first, the last and a few between) 100 x .. 1000 x the rest, in x and, at other columns, in dy: the mass of
            every row reduction sits in a few lanes and the projection term dominates the ordinary elements.
  offset    row means many standard deviations from zero, both signs in one tensor, at values the type still resolves.
  scaled    whole rows times powers of two across the type's range (below overflow of the inputs; x^2 is f32), an all-zero row (eps decides
            r) and a row whose rms is near sqrt(eps).
  exact     eps = 0, x = +-2^k per row (LayerNorm: equally many of each sign, so mean = 0), small-integer dy and w with mean(g n) = P and
            mean(g) = Q zero or a power of two: r = 2^-k, n = +-1, every intermediate is exact in f32 and every output representable, so
            the kernel's result is known bit for bit; dy differs per row and column, so a dropped row, wave or partial moves dweight / dbias
            by an integer.
"""
import math

import torch

U = {torch.bfloat16: 2.0 ** -8, torch.float16: 2.0 ** -11}
TINY = {torch.bfloat16: 2.0 ** -134, torch.float16: 2.0 ** -25}       # half the subnormal spacing
E32 = 2.0 ** -24
F32MIN = 2.0 ** -126
C16, C32 = 1.25, 2.0
ROWS_PER_PARTIAL = 32
FAMILIES = ("random", "outlier", "offset", "scaled", "exact")
K_TANH, C_TANH = 0.7978845608028654, 0.044715


def chain(cols):
    return cols / 64 + 6


def colsum_chain(rows):
    n_part = -(-rows // ROWS_PER_PARTIAL)
    return 8 + 3 + -(-n_part // 64) + 63


def half_spacing(v, dt):
    """Half the spacing of the 16-bit type at v: u 2^floor(log2 |v|), at least tiny - the most one rounding to nearest moves v."""
    _, e = torch.frexp(v.abs())
    hs = torch.ldexp(torch.full_like(v, U[dt]), e - 1)
    return torch.where(v == 0, torch.zeros_like(v), hs).clamp_min(TINY[dt])


def _out(v, dt, out_dtype=None, b=0.0):
    """b + the rounding of the stored value (f64): the kernel rounds a value within b of v, so half the spacing of a 16-bit output is
    taken at |v| + b (a power of two may lie between); e |v| for an f32 output."""
    if out_dtype == torch.float32:
        return b + E32 * v.abs()
    return b + half_spacing(v.abs() + b, dt)


def _mean(t):
    return t.mean(-1, keepdim=True)


def _rho(cols):
    return (chain(cols) / 2 + 4) * E32


# ------------------------------------------------------------------------------ norms


def rmsnorm(x, w, eps):
    """-> (y, bound) f64 [rows, cols]."""
    dt, cols = x.dtype, x.shape[1]
    u = U[dt]
    xd, wd = x.double(), w.double()
    r = (_mean(xd * xd) + eps) ** -0.5
    n = xd * r
    y = wd * n
    e_n = C16 * half_spacing(n, dt) + C32 * (_rho(cols) + E32) * n.abs()
    return y, _out(y, dt, b=wd.abs() * e_n)


def rmsnorm_grad(x, w, dy, eps, add=None, dw_dtype=None):
    """-> {"dx": (ref, bound) [rows, cols], "dw": (ref, bound) [cols]} in f64."""
    dt, (rows, cols) = x.dtype, x.shape
    u, rho = U[dt], _rho(cols)
    xd, wd, dyd = x.double(), w.double(), dy.double()
    r = (_mean(xd * xd) + eps) ** -0.5
    n = xd * r
    g = dyd * wd
    dot = _mean(g * n)
    dx = r * (g - n * dot)
    e_n = C16 * half_spacing(n, dt) + C32 * (rho + E32) * n.abs()
    ddot = _mean(g.abs() * e_n) + C32 * (chain(cols) + 2) * E32 * _mean((g * n).abs())
    b = r * (n.abs() * ddot + e_n * dot.abs()) + C32 * (2 * E32 * r * (g.abs() + (n * dot).abs()) + rho * dx.abs())
    b = _out(dx, dt, b=b)
    if add is not None:
        dx = dx + add.double()
        b = _out(dx, dt, b=b + C32 * E32 * dx.abs())
    dw = (dyd * n).sum(0)
    bw = _out(dw, dt, dw_dtype, (dyd.abs() * e_n).sum(0) + C32 * colsum_chain(rows) * E32 * (dyd * n).abs().sum(0))
    return {"dx": (dx, b), "dw": (dw, bw)}


def _ln_stats(xd, eps, cols):
    mean = _mean(xd)
    d = xd - mean
    rstd = (_mean(d * d) + eps) ** -0.5
    xh = d * rstd
    dmean = C32 * (chain(cols) + 1) * E32 * _mean(xd.abs())
    rho = _rho(cols) + (rstd * dmean) ** 2
    e_xh = rstd * dmean + C32 * (rho + 2 * E32) * xh.abs()
    return rstd, xh, rho, e_xh


def layernorm(x, w, b, eps):
    dt, cols = x.dtype, x.shape[1]
    wd, bd = w.double(), b.double()
    rstd, xh, rho, e_xh = _ln_stats(x.double(), eps, cols)
    y = xh * wd + bd
    return y, _out(y, dt, b=wd.abs() * e_xh + C32 * E32 * ((xh * wd).abs() + y.abs()))


def layernorm_grad(x, w, dy, eps, add=None, dw_dtype=None):
    """-> {"dx", "dw", "db"}: (ref, bound) in f64."""
    dt, (rows, cols) = x.dtype, x.shape
    wd, dyd = w.double(), dy.double()
    rstd, xh, rho, e_xh = _ln_stats(x.double(), eps, cols)
    g = dyd * wd
    sg, sgx = _mean(g), _mean(g * xh)
    dx = rstd * (g - sg - xh * sgx)
    dsg = C32 * (chain(cols) + 1) * E32 * _mean(g.abs())
    dsgx = _mean(g.abs() * e_xh) + C32 * (chain(cols) + 2) * E32 * _mean((g * xh).abs())
    b = rstd * (dsg + xh.abs() * dsgx + e_xh * sgx.abs()) + C32 * (2 * E32 * rstd * (g.abs() + sg.abs() + (xh * sgx).abs()) + rho * dx.abs())
    b = _out(dx, dt, b=b)
    if add is not None:
        dx = dx + add.double()
        b = _out(dx, dt, b=b + C32 * E32 * dx.abs())
    L = colsum_chain(rows)
    dw = (dyd * xh).sum(0)
    bw = _out(dw, dt, dw_dtype, (dyd.abs() * e_xh).sum(0) + C32 * L * E32 * (dyd * xh).abs().sum(0))
    db = dyd.sum(0)
    bb = _out(db, dt, dw_dtype, C32 * L * E32 * dyd.abs().sum(0))
    return {"dx": (dx, b), "dw": (dw, bw), "db": (db, bb)}


# ------------------------------------------------------------------------------ activations


def _sigmoid(x):
    """s, 1 - s (both accurate in either tail) and the bound ds of the f32 evaluation."""
    s = torch.sigmoid(x)
    s1 = torch.sigmoid(-x)
    ds = s * (s1 * (x.abs() + 4) + 3) * E32 + F32MIN
    return s, s1, ds


def _silu(x, dt):
    """a = silu(x) and the error of its 16-bit value T(a) as the kernels form it."""
    s, s1, ds = _sigmoid(x)
    a = x * s
    da = C32 * (x.abs() * ds + E32 * a.abs()) + F32MIN + C16 * half_spacing(a, dt)
    return a, da, s, s1, ds


def swiglu(gu):
    dt, inter = gu.dtype, gu.shape[1] // 2
    g, up = gu[:, :inter].double(), gu[:, inter:].double()
    a, da, *_ = _silu(g, dt)
    h = a * up
    return h, _out(h, dt, b=up.abs() * da)


def swiglu_grad(gu, dh):
    """-> (dgu, bound) [rows, 2 inter], planar [dgate | dup]."""
    dt, inter = gu.dtype, gu.shape[1] // 2
    g, up, d = gu[:, :inter].double(), gu[:, inter:].double(), dh.double()
    a, da, s, s1, ds = _silu(g, dt)
    du = d * a
    bu = _out(du, dt, b=d.abs() * da)
    sp = s * (1 + g * s1)
    dsp = C32 * ((1 + g.abs()) * ds + 4 * E32 * s * (1 + g.abs()))
    p = d * up
    dg = p * sp
    bg = _out(dg, dt, b=sp.abs() * C16 * half_spacing(p, dt) + p.abs() * dsp + C32 * E32 * dg.abs())
    return torch.cat([dg, du], 1), torch.cat([bg, bu], 1)


GELU_KINDS = (0, 1, 2)          # ops.gelu(z, tanh_form): False / 0 = erf, True / 1 = tanh, 2 = ReLU


def _gelu_parts(x, kind):
    """(y, dy_f32, y', dy'_f32): the function, its derivative and the bounds of their f32 evaluation."""
    ax = x.abs()
    if kind == 2:
        z = torch.zeros_like(x)
        return x.clamp_min(0), z, (x > 0).double(), z
    if kind == 0:
        zz = x * math.sqrt(0.5)
        er = torch.erf(zz)
        one_p = torch.erfc(-zz)                                   # 1 + erf(z) without the cancellation
        P = one_p / 2
        derf = 2 / math.sqrt(math.pi) * torch.exp(-zz * zz)
        dP = (4 * er.abs() + zz.abs() * derf + one_p) * E32 / 2
        y = x * P
        phi = torch.exp(-0.5 * x * x) / math.sqrt(2 * math.pi)
        yp = P + x * phi
        dyp = dP + ax * phi * (x * x / 2 + 6) * E32 + 2 * E32 * (P + ax * phi) + F32MIN
        return y, ax * dP + 2 * E32 * y.abs() + F32MIN, yp, dyp
    v = K_TANH * (x + C_TANH * x ** 3)
    t = torch.tanh(v)
    one_t = 2 * torch.sigmoid(2 * v)                              # 1 + tanh(v) without the cancellation
    sech2 = 4 * torch.sigmoid(2 * v) * torch.sigmoid(-2 * v)      # 1 - t^2
    dtv = sech2 * 4 * E32 * v.abs() + 4 * E32 * t.abs()
    y = x * one_t / 2
    poly = K_TANH * (1 + 3 * C_TANH * x * x)
    second = x * sech2 * poly / 2
    yp = one_t / 2 + second
    dyp = dtv / 2 + ax * poly * (2 * t.abs() * dtv + 2 * E32 + 4 * E32 * sech2) / 2 + 2 * E32 * (one_t / 2 + second.abs())
    return y, ax * (dtv + E32 * one_t) / 2 + 2 * E32 * y.abs() + F32MIN, yp, dyp + F32MIN


def gelu(z, kind):
    dt = z.dtype
    y, dy32, _, _ = _gelu_parts(z.double(), int(kind))
    if int(kind) == 2:
        return y, torch.zeros_like(y)
    return y, _out(y, dt, b=C32 * dy32)


def gelu_grad(z, dy, kind):
    dt = z.dtype
    _, _, yp, dyp = _gelu_parts(z.double(), int(kind))
    d = dy.double()
    dz = d * yp
    if int(kind) == 2:
        return dz, torch.zeros_like(dz)
    return dz, _out(dz, dt, b=C32 * (d.abs() * dyp + E32 * dz.abs()))


def rope_transpose(dy, cos, sin, n_heads, hd):
    """The transpose of the forward rotation y_lo = a c - b s, y_hi = b c + a s (cos / sin [tokens, hd / 2], the FORWARD table's rows):
    da = dy_lo c + dy_hi s, db = dy_hi c - dy_lo s, on the first n_heads * hd columns of dy [tokens, >=] -> (ref, bound) [tokens, n_heads, hd]."""
    dt, tokens, half = dy.dtype, dy.shape[0], hd // 2
    v = dy[:, :n_heads * hd].double().view(tokens, n_heads, hd)
    lo, hi = v[..., :half], v[..., half:]
    c, s = cos.double()[:, None, :], sin.double()[:, None, :]
    ref = torch.cat([lo * c + hi * s, hi * c - lo * s], -1)
    bnd = torch.cat([half_spacing(lo * c, dt) + half_spacing(hi * s, dt), half_spacing(hi * c, dt) + half_spacing(lo * s, dt)], -1)
    return ref, _out(ref, dt, b=bnd + C32 * E32 * ref.abs())


# ------------------------------------------------------------------------------ comparison


def ratio(got, ref):
    """Worst |got - ref| / bound for ref = (reference, bound); inf for any non-finite output the reference does not have, and for any
    difference where the bound is zero (an exact operation)."""
    want, bound = ref
    g = got.to(want.device).double()
    if tuple(g.shape) != tuple(want.shape):
        g = g.reshape(want.shape)
    fin = torch.isfinite(want)
    if not bool(torch.isfinite(g[fin]).all()):
        return float("inf")
    err = (g - want).abs()[fin]
    b = bound[fin]
    q = torch.where(err == 0, torch.zeros_like(err), err / b)          # 0 / 0 = 0, x / 0 = inf
    return q.max().item() if q.numel() else 0.0


def worst_index(got, ref):
    """Index of the element with the worst ratio (for failure messages)."""
    want, bound = ref
    q = (got.to(want.device).double().reshape(want.shape) - want).abs() / bound
    q = torch.nan_to_num(q, nan=float("inf"))
    return tuple(int(i) for i in torch.unravel_index(q.argmax(), q.shape))


def old_rule_ratio(got, want, rel, elem, floor=1e-30):
    """The suite's earlier rule _close(got, ref, rel, elem) of tests/test_gpu_train_dense.py: norm-wise relative error < rel and
    max |err| / max |ref| < elem -> the larger of the two shares (below 1: that rule passes)."""
    g, w = got.double().cpu(), want.double().cpu()
    err = (g - w).norm() / w.norm().clamp_min(floor)
    worst = (g - w).abs().max() / w.abs().max().clamp_min(floor)
    return max(err.item() / rel, worst.item() / elem)


# ------------------------------------------------------------------------------ inputs


def outlier_columns(cols, n=6):
    """Fixed columns: the first, the last, and a few between (not a multiple of 8 or 64 apart)."""
    if cols <= 8:
        return [0, cols - 1]
    return sorted({0, cols - 1, cols // 3 + 1, cols // 2 - 3, (2 * cols) // 3 + 5, cols - 9} & set(range(cols)))[:n]


def _weights(cols, g):
    w = 1 + 0.2 * torch.randn(cols, generator=g)
    b = 0.1 * torch.randn(cols, generator=g)
    return w, b


def norm_inputs(family, rows, cols, dtype, seed=0, norm="rms", device="cpu"):
    """-> dict x, dy, add [rows, cols], w, b [cols] (16 bit, on device) and eps.  norm: "rms" or "ln" (matters to the exact family only)."""
    g = torch.Generator().manual_seed(seed * 1000003 + rows * 131 + cols)
    eps = 1e-6
    if family == "exact":
        x, w, b, dy, add = _exact(rows, cols, norm, g)
        eps = 0.0
    else:
        x = torch.randn(rows, cols, generator=g, dtype=torch.float64) * 1.5
        dy = torch.randn(rows, cols, generator=g, dtype=torch.float64)
        add = torch.randn(rows, cols, generator=g, dtype=torch.float64)
        w, b = _weights(cols, g)
        if family == "outlier":
            oc = outlier_columns(cols)
            amp = torch.tensor([100.0, 1000.0, 300.0, 150.0, 700.0, 250.0])[: len(oc)].double()
            x[:, oc] *= amp
            dc = [(c + 1) % cols for c in oc]                     # dy's outliers sit beside x's, not on them
            dy[:, dc] *= amp.flip(0)
        elif family == "offset":
            mus = (4.0, -16.0, 32.0, -4.0, 16.0, -32.0) if dtype == torch.bfloat16 else (16.0, -128.0, 256.0, -16.0, 128.0, -256.0)
            mu = torch.tensor([mus[i % len(mus)] for i in range(rows)], dtype=torch.float64)
            x = x / 1.5 + mu[:, None]
        elif family == "scaled":
            pw = (-40, -20, -10, -4, 0, 4, 8, 20, 40) if dtype == torch.bfloat16 else (-24, -14, -10, -4, 0, 4, 8, 12)
            sc = [2.0 ** pw[i % len(pw)] for i in range(rows)]
            x = x * torch.tensor(sc, dtype=torch.float64)[:, None]
            if rows > 1:
                x[1 % rows] = 0                                   # eps decides r
            if rows > 2:
                x[2] = torch.randn(cols, generator=g, dtype=torch.float64) * math.sqrt(eps)        # rms near sqrt(eps)
        elif family != "random":
            raise ValueError(family)
    to = lambda t: t.to(dtype).to(device)       # noqa: E731
    return {"x": to(x), "w": to(w), "b": to(b), "dy": to(dy), "add": to(add), "eps": eps}


def _exact(rows, cols, norm, g):
    """See the module docstring.  q = cols / 4, h = cols / 2.  Signs s_j (j < q) are random, s_{j+q} = s_j; the second half repeats the
    first (RMSNorm) or negates it (LayerNorm: mean 0).  w has period q, |w| in {1, 2}.  Per row, with targets P = mean(g n) (RMSNorm) or
    Q = mean(g) and P = mean(g xh) (LayerNorm), each zero or +-2^m:
      RMSNorm    g_{j+h} n_{j+h} = 2 P - g_j n_j                                        (j < h)
      LayerNorm  g_{j+q} = 2 Q - g_j + 2 P s_j (j < q),   g_{j+h} = 2 Q - g_j (j < h)
    with g = dy w and first-quarter (RMSNorm: first-half) dy = distinct non-zero integers per row and column."""
    q, h = cols // 4, cols // 2
    ri, ci = torch.arange(rows)[:, None], torch.arange(cols)[None, :]
    k = (ri % 7) - 3                                                          # x = +-2^k, k in [-3, 3]
    wq = torch.tensor([1.0, -2.0, 2.0, -1.0])[torch.randint(0, 4, (q,), generator=g)]
    w = wq.repeat(4)
    sq = (torch.randint(0, 2, (rows, q), generator=g) * 2 - 1).double()
    mag = ((ri * 7 + ci * 3) % 6 + 1).double()                                # 1 .. 6, differs along rows and columns
    sgn = (((ri + ci) % 2) * 2 - 1).double()
    dy = mag * sgn
    targets = torch.tensor([0.0, 2.0, -1.0, 4.0, 0.0, -2.0])
    P = targets[(ri[:, 0] % 6)][:, None].double()
    Q = targets[((ri[:, 0] + 2) % 6)][:, None].double()
    wd = w.double()[None, :]
    if norm == "rms":
        s2 = (torch.randint(0, 2, (rows, h), generator=g) * 2 - 1).double()
        s = torch.cat([sq, sq, s2], 1)
        gn = dy[:, :h] * wd[:, :h] * s[:, :h]
        dy[:, h:] = (2 * P - gn) * s[:, h:] / wd[:, h:]
    else:
        s = torch.cat([sq, sq, -sq, -sq], 1)
        g0 = dy[:, :q] * wd[:, :q]
        dy[:, q:h] = (2 * Q - g0 + 2 * P * sq) / wd[:, q:h]
        gh = dy[:, :h] * wd[:, :h]
        dy[:, h:] = (2 * Q - gh) / wd[:, h:]
    x = s * 2.0 ** k.double()
    b = ((ci[0] % 5) - 2).double()
    add = (((ri * 3 + ci) % 9) - 4).double() * 2.0 ** (-k.double())          # integers on dx's own scale 2^-k
    return x, w.double(), b, dy, add


def act_random(rows, cols, dtype, seed=0, device="cpu"):
    g = torch.Generator().manual_seed(seed * 7919 + rows * 31 + cols)
    z = (torch.randn(rows, cols, generator=g) * 2).to(dtype).to(device)
    d = torch.randn(rows, cols, generator=g).to(dtype).to(device)
    return z, d


def sweep_values(dtype, lim=64.0, device="cpu"):
    """Every representable value of the type with |v| <= lim (zeros of both signs and subnormals included), ascending bit patterns.  64 is
    far into both tails of every activation here: silu(-64) ~ 1e-26, gelu(-64) underflows in f64, and both are x itself at +64."""
    bits = torch.arange(-32768, 32768, dtype=torch.int32).to(torch.int16)
    v = bits.view(dtype)
    keep = torch.isfinite(v.float()) & (v.float().abs() <= lim)
    return v[keep].to(device)


def sweep_rows(dtype, cols, seed=0, device="cpu"):
    """The sweep laid out as [rows, cols] (the tail of the last row repeats the start) with a second operand drawn from a small set
    of multipliers that includes 1, 0 and both signs."""
    v = sweep_values(dtype)
    rows = -(-v.numel() // cols)
    z = torch.cat([v, v[: rows * cols - v.numel()]]).view(rows, cols)
    g = torch.Generator().manual_seed(seed + cols)
    pick = torch.tensor([1.0, -1.0, 0.75, -3.0, 0.0, 2.5, 1.0, -0.0625])
    d = pick[torch.randint(0, pick.numel(), (rows, cols), generator=g)].to(dtype)
    return z.to(device), d.to(device)
