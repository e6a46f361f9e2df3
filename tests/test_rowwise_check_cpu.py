"""The row-wise checker (tests/rowwise_check.py) is neither loose nor wrong: an f32 emulation of each kernel passes it, and emulations
with one thing wrong fail it - under the bound on a structured family, or bit for bit on the exact one.  No GPU: -m "not gpu".

The emulations follow norm_rope.hip / train.hip: a row is held as 16-byte vectors, lane l of the wave owns vectors l, l + 64, ...; a row
reduction is one fused add per element in that order per lane, then the xor butterfly 32, 16, .. 1; r = 1 / sqrtf(ss / cols + eps); n is
rounded to 16 bit (RMSNorm only); dweight / dbias: eight rows in order per wave, ((w0 + w1) + w2) + w3 through LDS, every 64th partial row in
order per group in colsum_final, then the 64 group sums in order.  Fused adds are formed in f64 and rounded once.

Worst |err| / bound of the emulation (70 rows; dx / dweight [/ dbias], worst over add on / off and f32 / 16-bit dweight, over the widths
8 .. 3584; the constants C16 = 1.25, C32 = 2 of rowwise_check were settled here).  The dx and 16-bit dweight figures sit just under 1 by
construction: the last term of every bound is the exact half spacing of the output type, which a rounding reaches:
                 RMSNorm backward                          LayerNorm backward
            random   outlier  offset   scaled       random        outlier       offset        scaled
    bf16  1.00/0.43 1.00/0.48 0.99/0.35 1.00/0.45  1.00/0.99/0.99 1.00/0.98/0.99 1.00/0.96/0.99 1.00/0.99/0.99
    f16   1.00/0.39 1.00/0.49 1.00/0.32 1.00/0.50  1.00/0.93/0.94 1.00/0.93/0.94 0.99/0.41/0.94 1.00/0.93/0.94
(with f32 dweight alone RMSNorm's dweight figure is the one shown, LayerNorm's 0.2 .. 0.6); forward norms: < 1 on every family and width up to
4096, bit-identical on the exact family.  Activations (random / sweep of every value in [-64, 64]): swiglu 0.91 / 0.99, swiglu_grad 0.92 / 0.99,
gelu and gelu_grad of both kinds 0.999 .. 1.000 (one output rounding; the f32 terms matter only in the tails), ReLU exact.

Mutants: worst ratio on the bound family that carries each (bf16 | f16), and the exact family (bit for bit):
    mutant               carried by        RMSNorm            LayerNorm            exact family
    projection dropped   outlier @ 3584    99.7 | 784         mean(g) 3.0e3 | 1.6e4, mean(g xh) 425 | 3.0e3   fails
    mean over padded n   outlier @ 520     41 | 332           3.3e3 | 2.3e4        fails
    last vector missing  outlier @ 3584    43 | 337           2.2e3 | 1.1e4        fails   (the last column is an outlier column)
    eps omitted          scaled @ 1152     inf | inf          inf | inf            -       (the all-zero row: NaN; the exact family has eps = 0)
    w omitted from g     random @ 3584     468 | 3.7e3        699 | 5.1e3          fails
    r applied twice      random @ 3584     159 | 1.3e3        171 | 1.3e3          fails
    add from wrong row   random @ 3584     3.6e4 | 2.9e5      8.0e4 | 3.0e5        fails
    row missing in dw    random @ 1152     49 | 383           1.2e4 | 1.2e4        fails   (db: 6.9e3 | 6.9e3)
    wave partial missing random @ 1152     62 | 484           1.8e4 | 1.8e4        fails
    last partial missing random @ 1152     63 | 497           1.6e4 | 1.6e4        fails
    n left unrounded     nothing           1.00 / 1.00 / 1.00 (random / outlier / scaled @ 3584, both dtypes): within one rounding of the truth,
                                           inside the bound; the exact family has n = +-1 either way, so it does not carry it either.
    dgate / dup swapped  random, sweep     1.6e7 | 1.4e7
    silu' without x(1-s) random, sweep     5.9e4 | 3.2e5
    dh u left unrounded  nothing           0.90 / 0.99: inside the bound (one rounding)
    GELU kinds swapped   random, sweep     forward 79 .. 97 | 250 .. 269, gradient 112 .. 152 | 385 .. 599
    relu' at >= 0        sweep (x = +-0)   inf (the bound of an exact operation is zero)
(a dropped row is visible to the bound at 70 rows because sum |dy| e_n grows with the row count and one row's share does not; at 6794 and
23 328 rows it is the exact family that carries it.)

The old rule (_close of tests/test_gpu_train_dense.py: norm-wise relative error and max |err| / max |ref|, with those tests' tolerances, bf16,
their shapes, random inputs), as shares of its two tolerances (norm-wise / element-wise; below 1 = passes), beside the new ratio:
    RMSNorm 300 x 3584   projection dropped 2.88 / 2.66 (new 24);  row missing in dweight 15.1 / 20.9 (new 10.5);  last vector missing 0.30 / 0.18
    LayerNorm 1458 x 1152  mean(g xh) dropped 4.89 / 3.17 (new 1.1e4);  mean(g) dropped 5.01 / 1.02;  row missing 14.0 / 14.9;  last vector
                         missing 0.49 / 0.17 (new 2.2e3)
On random inputs the old rule does NOT let the dropped projection term or the dropped dweight row through: its norm-wise part sees them (the
projection is 1 / sqrt(cols) of the gradient's norm, 1.7 % at 3584 columns against a tolerance of 0.6 %; the gradient sums grow as sqrt(rows),
so one row of 300 is 6 %).  What it lets through is the partial loss of a reduction - the last 8-wide vector missing from it - on random rows
and on outlier rows alike (0.34 / 0.11 for RMSNorm with outlier channels, where the new bound gives 88), and everything it never ran: f16, the
width forms, the row and stride edges.  test_old_rule_against_the_bound asserts exactly that.
"""
import pytest
import torch

import rowwise_check as rc

DT = {"bf16": torch.bfloat16, "f16": torch.float16}
WIDTHS = (8, 64, 136, 504, 512, 520, 1152, 1536, 1544, 2048, 3584)
ROWS = 70                       # two full 32-row blocks and a partial one


def fma(a, b, c):
    return (a.double() * b.double() + c.double()).float()


def r16(x, dt):
    return x.to(dt).float()


def lanes(v, pad_value=0.0):
    """[rows, cols] -> [rows, steps, 64, 8]: vector k = i * 64 + lane; missing vectors are pad_value."""
    rows, cols = v.shape
    nv = cols // 8
    steps = -(-nv // 64)
    out = torch.full((rows, steps * 64 * 8), pad_value, dtype=v.dtype)
    out[:, :cols] = v
    return out.view(rows, steps, 64, 8)


def wave_sum(x):
    """x [rows, 64] -> [rows, 1]: the xor butterfly."""
    idx = torch.arange(64)
    for off in (32, 16, 8, 4, 2, 1):
        x = x + x[:, idx ^ off]
    return x[:, :1]


def row_reduce(a, b=None, fused=True, skip_last_vec=False):
    """sum over the row of a * b (fused adds) or of a (plain adds) in the kernel's order."""
    A = lanes(a)
    B = lanes(b) if b is not None else None
    if skip_last_vec:
        nv = a.shape[1] // 8
        A = A.clone()
        A.view(A.shape[0], -1, 8)[:, nv - 1] = 0
    acc = torch.zeros(a.shape[0], 64)
    for i in range(A.shape[1]):
        for j in range(8):
            acc = fma(A[:, i, :, j], B[:, i, :, j], acc) if fused and B is not None else acc + A[:, i, :, j]
    return wave_sum(acc)


def padded_count(cols):
    return -(-(cols // 8) // 64) * 64 * 8


def colsum_emulated(contrib, mut=None):
    """contrib [rows, cols] f32 products' factors are applied by the caller through `step`: here contrib is a pair (d, n) or (d, None)."""
    d, n = contrib
    rows, cols = d.shape
    n_part = -(-rows // 32)
    pad = n_part * 32 - rows
    dz = torch.cat([d, torch.zeros(pad, cols)])
    nz = torch.cat([n, torch.zeros(pad, cols)]) if n is not None else None
    if mut == "drop_row":
        dz[5 % rows] = 0
    dz = dz.view(n_part, 8, 4, cols)                               # row = 32 b + 4 round + wave
    nz = nz.view(n_part, 8, 4, cols) if nz is not None else None
    acc = torch.zeros(n_part, 4, cols)
    for rnd in range(8):
        acc = fma(dz[:, rnd], nz[:, rnd], acc) if nz is not None else acc + dz[:, rnd]
    if mut == "drop_wave":
        acc[0, 2] = 0
    part = ((acc[:, 0] + acc[:, 1]) + acc[:, 2]) + acc[:, 3]       # [n_part, cols]
    if mut == "drop_last_partial":
        part = part[:-1] if n_part > 1 else part * 0
        n_part = part.shape[0]
    groups = torch.zeros(64, cols)
    for b in range(n_part):
        groups[b % 64] = groups[b % 64] + part[b]
    t = groups[0]
    for i in range(1, 64):
        t = t + groups[i]
    return t


def _store(v, dt):
    return v.to(dt)


def em_rmsnorm(p, dt, mut=None):
    x, w = p["x"].float(), p["w"].float()
    cols = x.shape[1]
    ss = row_reduce(x, x)
    r = 1.0 / torch.sqrt(ss / float(cols) + (0.0 if mut == "no_eps" else torch.tensor(p["eps"], dtype=torch.float32)))
    return _store(w * r16(x * r, dt), dt)


def em_rmsnorm_grad(p, dt, add=True, dw_dtype=torch.float32, mut=None):
    x, w, dy = p["x"].float(), p["w"].float(), p["dy"].float()
    rows, cols = x.shape
    eps = torch.tensor(0.0 if mut == "no_eps" else p["eps"], dtype=torch.float32)
    ss = row_reduce(x, x)
    r = 1.0 / torch.sqrt(ss / float(cols) + eps)
    n = x * r if mut == "n_unrounded" else r16(x * r, dt)
    g = dy if mut == "no_w" else dy * w
    count = float(padded_count(cols) if mut == "pad_mean" else cols)
    dot = row_reduce(g, n, skip_last_vec=mut == "drop_last_vec") / count
    if mut == "no_proj":
        dot = dot * 0
    o = r * fma(-n, dot.expand_as(n), g)
    if mut == "r_twice":
        o = r * o
    if add:
        a = p["add"].float()
        if mut == "add_wrong_row":
            a = torch.roll(a, 1, 0)
        o = r16(o, dt) + a
    cm = {"dw_drop_row": "drop_row", "drop_wave": "drop_wave", "drop_last_partial": "drop_last_partial"}.get(mut)
    dw = colsum_emulated((dy, n), cm)
    return _store(o, dt), dw.to(dw_dtype)


def _ln_stats(x, eps, mut=None):
    cols = x.shape[1]
    mean = row_reduce(x, fused=False) / float(cols)
    d = x - mean
    q = row_reduce(d, d)
    rstd = 1.0 / torch.sqrt(q / float(cols) + eps)
    return mean, rstd


def em_layernorm(p, dt, mut=None):
    x, w, b = p["x"].float(), p["w"].float(), p["b"].float()
    eps = torch.tensor(0.0 if mut == "no_eps" else p["eps"], dtype=torch.float32)
    mean, rstd = _ln_stats(x, eps)
    return _store(fma((x - mean) * rstd, w.expand_as(x), b.expand_as(x)), dt)


def em_layernorm_grad(p, dt, add=True, dw_dtype=torch.float32, mut=None):
    x, w, dy = p["x"].float(), p["w"].float(), p["dy"].float()
    rows, cols = x.shape
    eps = torch.tensor(0.0 if mut == "no_eps" else p["eps"], dtype=torch.float32)
    mean, rstd = _ln_stats(x, eps)
    xh = (x - mean) * rstd
    g = dy if mut == "no_w" else dy * w
    count = float(padded_count(cols) if mut == "pad_mean" else cols)
    sg = row_reduce(g, fused=False, skip_last_vec=mut == "drop_last_vec") / count
    sgx = row_reduce(g, xh) / count
    if mut == "no_mean_g":
        sg = sg * 0
    if mut == "no_mean_gx":
        sgx = sgx * 0
    o = rstd * fma(-xh, sgx.expand_as(xh), g - sg)
    if mut == "r_twice":
        o = rstd * o
    if add:
        a = p["add"].float()
        if mut == "add_wrong_row":
            a = torch.roll(a, 1, 0)
        o = r16(o, dt) + a
    cm = {"drop_wave": "drop_wave", "drop_last_partial": "drop_last_partial"}.get(mut)
    dw = colsum_emulated((dy, xh), "drop_row" if mut == "dw_drop_row" else cm)
    db = colsum_emulated((dy, None), "drop_row" if mut == "db_drop_row" else cm)
    return _store(o, dt), dw.to(dw_dtype), db.to(dw_dtype)


def f_sigmoid(x):
    return 1.0 / (1.0 + torch.exp(-x))


def em_swiglu(gu, mut=None):
    dt, inter = gu.dtype, gu.shape[1] // 2
    g, u = gu[:, :inter].float(), gu[:, inter:].float()
    return (r16(g * f_sigmoid(g), dt) * u).to(dt)


def em_swiglu_grad(gu, dh, mut=None):
    dt, inter = gu.dtype, gu.shape[1] // 2
    g, u, d = gu[:, :inter].float(), gu[:, inter:].float(), dh.float()
    s = f_sigmoid(g)
    ou = d * r16(g * s, dt)
    sp = s if mut == "silu_no_x_term" else s * (1.0 + g * (1.0 - s))
    p = d * u
    og = (p if mut == "dhu_unrounded" else r16(p, dt)) * sp
    halves = [ou, og] if mut == "swap_halves" else [og, ou]
    return torch.cat(halves, 1).to(dt)


def f_gelu(x, kind):
    if kind == 2:
        return x.clamp_min(0)
    if kind == 1:
        u = 0.7978845608028654 * (x + 0.044715 * x * x * x)
        return 0.5 * x * (1.0 + torch.tanh(u))
    return 0.5 * x * (1.0 + torch.erf(x * 0.70710678118654752440))


def f_gelu_d(x, kind, relu_ge0=False):
    if kind == 2:
        return ((x >= 0) if relu_ge0 else (x > 0)).float()
    if kind == 1:
        u = 0.7978845608028654 * (x + 0.044715 * x * x * x)
        t = torch.tanh(u)
        return 0.5 * (1.0 + t) + 0.5 * x * (1.0 - t * t) * 0.7978845608028654 * (1.0 + 3.0 * 0.044715 * x * x)
    return 0.5 * (1.0 + torch.erf(x * 0.70710678118654752440)) + x * 0.3989422804014327 * torch.exp(-0.5 * x * x)


def em_gelu(z, kind, mut=None):
    if mut == "kind_swap":
        kind = {0: 1, 1: 0, 2: 2}[kind]
    return f_gelu(z.float(), kind).to(z.dtype)


def em_gelu_grad(z, dy, kind, mut=None):
    if mut == "kind_swap":
        kind = {0: 1, 1: 0, 2: 2}[kind]
    return (dy.float() * f_gelu_d(z.float(), kind, mut == "relu_ge0")).to(z.dtype)


def em_rope(x, cos, sin, n_heads, hd):
    dt, tokens, half = x.dtype, x.shape[0], hd // 2
    v = x[:, :n_heads * hd].float().view(tokens, n_heads, hd)
    a, b = v[..., :half], v[..., half:]
    c, s = cos.float()[:, None, :], sin.float()[:, None, :]
    return torch.cat([r16(a * c, dt) + r16(-b * s, dt), r16(b * c, dt) + r16(a * s, dt)], -1).to(dt)


# ------------------------------------------------------------------------------ verdicts


def norm_grad_ratios(norm, p, dt, out, add, dw_dtype):
    """{name: ratio} of an emulated (dx, dw[, db]) against the checker; exact family: 0 if bit-identical to the rounded reference, else inf."""
    fn = rc.rmsnorm_grad if norm == "rms" else rc.layernorm_grad
    ref = fn(p["x"], p["w"], p["dy"], p["eps"], add=p["add"] if add else None, dw_dtype=dw_dtype)
    return {k: rc.ratio(o, ref[k]) for k, o in zip(("dx", "dw", "db"), out)}, ref


def exact_equal(out, ref, dt, dw_dtype):
    ok = torch.equal(out[0], ref["dx"][0].to(dt))
    for o, k in zip(out[1:], ("dw", "db")):
        ok = ok and torch.equal(o, ref[k][0].to(dw_dtype))
    return ok


def run_norm_grad(norm, family, cols, dt, mut=None, add=True, dw_dtype=torch.float32, rows=ROWS):
    p = rc.norm_inputs(family, rows, cols, dt, seed=1, norm=norm)
    em = em_rmsnorm_grad if norm == "rms" else em_layernorm_grad
    out = em(p, dt, add=add, dw_dtype=dw_dtype, mut=mut)
    ratios, ref = norm_grad_ratios(norm, p, dt, out, add, dw_dtype)
    worst = max(ratios.values())
    if family == "exact":
        return 0.0 if exact_equal(out, ref, dt, dw_dtype) else float("inf")
    return worst


NORM_MUTANTS = {
    "rms": ("no_proj", "pad_mean", "drop_last_vec", "no_eps", "no_w", "r_twice", "add_wrong_row", "dw_drop_row", "drop_wave", "drop_last_partial",
            "n_unrounded"),
    "ln": ("no_mean_g", "no_mean_gx", "pad_mean", "drop_last_vec", "no_eps", "no_w", "r_twice", "add_wrong_row", "dw_drop_row", "db_drop_row",
           "drop_wave", "drop_last_partial"),
}
INSIDE_THE_BOUND = {"n_unrounded"}          # within one rounding of the truth: nothing carries it (the exact family has n = +-1 either way)
# the bound family that must reject each structural mutant, and the width where it does
CARRIER = {"no_proj": ("outlier", 3584), "no_mean_g": ("outlier", 3584), "no_mean_gx": ("outlier", 3584), "pad_mean": ("outlier", 520),
           "drop_last_vec": ("outlier", 3584), "no_eps": ("scaled", 1152), "no_w": ("random", 3584), "r_twice": ("random", 3584),
           "add_wrong_row": ("random", 3584), "dw_drop_row": ("random", 1152), "db_drop_row": ("random", 1152), "drop_wave": ("random", 1152),
           "drop_last_partial": ("random", 1152)}


@pytest.mark.parametrize("dtn", list(DT))
@pytest.mark.parametrize("norm", ["rms", "ln"])
@pytest.mark.parametrize("cols", WIDTHS)
def test_emulated_norm_backward_is_inside_the_bound_on_every_family(norm, cols, dtn):
    dt = DT[dtn]
    for family in rc.FAMILIES:
        for add, dwt in ((True, torch.float32), (False, dt)):
            got = run_norm_grad(norm, family, cols, dt, add=add, dw_dtype=dwt)
            assert got < 1.0, (norm, family, cols, dtn, add, got)


@pytest.mark.parametrize("dtn", list(DT))
@pytest.mark.parametrize("cols", WIDTHS + (4096,))
def test_emulated_norm_forward_is_inside_the_bound_on_every_family(cols, dtn):
    dt = DT[dtn]
    for family in rc.FAMILIES:
        p = rc.norm_inputs(family, ROWS, cols, dt, seed=2, norm="ln")
        for name, em, ref in (("rms", em_rmsnorm(p, dt), rc.rmsnorm(p["x"], p["w"], p["eps"])),
                              ("ln", em_layernorm(p, dt), rc.layernorm(p["x"], p["w"], p["b"], p["eps"]))):
            if family == "exact":
                assert torch.equal(em, ref[0].to(dt)), (name, cols, dtn)
            else:
                assert rc.ratio(em, ref) < 1.0, (name, family, cols, dtn, rc.ratio(em, ref))


@pytest.mark.parametrize("dtn", list(DT))
@pytest.mark.parametrize("norm", ["rms", "ln"])
def test_every_norm_backward_mutant_is_rejected(norm, dtn):
    dt = DT[dtn]
    for mut in NORM_MUTANTS[norm]:
        if mut in INSIDE_THE_BOUND:
            for family in ("random", "outlier", "scaled"):
                assert run_norm_grad(norm, family, 3584, dt, mut=mut) < 1.0
            continue
        family, cols = CARRIER[mut]
        got = run_norm_grad(norm, family, cols, dt, mut=mut)
        assert got > 1.0, (norm, mut, family, cols, dtn, got)
        if mut != "no_eps":                 # (eps = 0 in the exact family)
            ecols = 520 if mut == "pad_mean" else 1152
            assert run_norm_grad(norm, "exact", ecols, dt, mut=mut) == float("inf"), (norm, mut, dtn)


def act_cases(dt):
    z, d = rc.act_random(64, 1160, dt, seed=3)
    zs, ds = rc.sweep_rows(dt, 1160, seed=3)
    return {"random": (z, d), "sweep": (zs, ds)}


@pytest.mark.parametrize("dtn", list(DT))
def test_emulated_activations_are_inside_the_bound_and_their_mutants_are_not(dtn):
    dt = DT[dtn]
    for family, (z, d) in act_cases(dt).items():
        for kind in rc.GELU_KINDS:
            assert rc.ratio(em_gelu(z, kind), rc.gelu(z, kind)) < 1.0, (family, kind)
            assert rc.ratio(em_gelu_grad(z, d, kind), rc.gelu_grad(z, d, kind)) < 1.0, (family, kind)
        # SwiGLU: the gate takes the family's values, the up half and dh the second operand / a shifted copy
        gu = torch.cat([z, d], 1)
        dh = torch.roll(d, 3, 1)
        assert rc.ratio(em_swiglu(gu), rc.swiglu(gu)) < 1.0, family
        assert rc.ratio(em_swiglu_grad(gu, dh), rc.swiglu_grad(gu, dh)) < 1.0, family
    z, d = act_cases(dt)["sweep"]
    gu, dh = torch.cat([z, d], 1), torch.roll(d, 3, 1)
    for kind in (0, 1):
        assert rc.ratio(em_gelu(z, kind, "kind_swap"), rc.gelu(z, kind)) > 1.0
        assert rc.ratio(em_gelu_grad(z, d, kind, "kind_swap"), rc.gelu_grad(z, d, kind)) > 1.0
    assert rc.ratio(em_gelu_grad(z, d.abs() + 1, 2, "relu_ge0"), rc.gelu_grad(z, d.abs() + 1, 2)) == float("inf")      # carried by x = +-0
    zr, dr = act_cases(dt)["random"]
    gur, dhr = torch.cat([zr, dr], 1), torch.roll(dr, 3, 1)
    for mut in ("swap_halves", "silu_no_x_term", "dhu_unrounded"):
        got = max(rc.ratio(em_swiglu_grad(gur, dhr, mut), rc.swiglu_grad(gur, dhr)), rc.ratio(em_swiglu_grad(gu, dh, mut), rc.swiglu_grad(gu, dh)))
        if mut == "dhu_unrounded":
            assert got < 1.0            # within one rounding of the truth: inside the bound, nothing carries it
        else:
            assert got > 1.0, (mut, got)


@pytest.mark.parametrize("dtn", list(DT))
def test_emulated_rotation_transpose_is_inside_the_bound(dtn):
    dt = DT[dtn]
    g = torch.Generator().manual_seed(4)
    tokens, heads, hd = 50, 6, 128
    ang = torch.arange(tokens, dtype=torch.float64)[:, None] * (1e6 ** (-torch.arange(0, hd, 2, dtype=torch.float64) / hd))[None, :]
    cos, sin = torch.cos(ang).to(dt), torch.sin(ang).to(dt)
    dy = torch.randn(tokens, heads * hd + 64, generator=g).to(dt)
    ref = rc.rope_transpose(dy, cos, sin, heads, hd)
    assert rc.ratio(em_rope(dy, cos, -sin, heads, hd), ref) < 1.0                   # the kernel on the inverse table (cos, -sin)
    assert rc.ratio(em_rope(dy, cos, sin, heads, hd), ref) > 1.0                    # the forward rotation is not its transpose


def _old_and_new(norm, family, rows, cols, mut, key, tol, dt=torch.bfloat16):
    p = rc.norm_inputs(family, rows, cols, dt, seed=5, norm=norm)
    em = em_rmsnorm_grad if norm == "rms" else em_layernorm_grad
    out = dict(zip(("dx", "dw", "db"), em(p, dt, add=False, mut=mut)))
    ref = (rc.rmsnorm_grad if norm == "rms" else rc.layernorm_grad)(p["x"], p["w"], p["dy"], p["eps"], dw_dtype=torch.float32)
    return rc.old_rule_ratio(out[key], ref[key][0], *tol), rc.ratio(out[key], ref[key])


def test_old_rule_against_the_bound():
    """The rule the direct tests use (restated as rowwise_check.old_rule_ratio, with their tolerances, dtype and shapes) beside the new bound.
    A reduction that loses its last 8-wide vector passes the old rule on random and on outlier rows and fails the new bound; the dropped
    projection term and the dropped dweight row fail both on random inputs (figures in the module docstring)."""
    dx_tol, dw_rms, dw_ln = (6e-3, 1.5e-2), (4e-3, 6e-3), (2e-3, 4e-3)
    for norm, family, rows, cols in (("ln", "random", 1458, 1152), ("rms", "outlier", 300, 3584), ("ln", "outlier", 1458, 1152)):
        old, new = _old_and_new(norm, family, rows, cols, "drop_last_vec", "dx", dx_tol)
        print(norm, family, "drop_last_vec", old, new)
        if not (norm == "ln" and family == "outlier"):
            assert old < 1.0 < new, (norm, family, old, new)
        assert new > 1.0
    for norm, rows, cols, mut, key, tol in (("rms", 300, 3584, "no_proj", "dx", dx_tol), ("ln", 1458, 1152, "no_mean_gx", "dx", dx_tol),
                                            ("rms", 300, 3584, "dw_drop_row", "dw", dw_rms), ("ln", 1458, 1152, "dw_drop_row", "dw", dw_ln)):
        old, new = _old_and_new(norm, "random", rows, cols, mut, key, tol)
        print(norm, mut, old, new)
        assert new > 1.0, (norm, mut, old, new)
        assert old > 1.0, (norm, mut, old, new)          # the norm-wise part of the old rule sees these on random inputs
