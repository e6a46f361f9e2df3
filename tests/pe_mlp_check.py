"""The learned MLP position encoding (PositionEmbeddingMLP: Linear(3, 512) -> LayerNorm(512) -> ReLU -> Linear(512, E)) restated on the
CPU, the bounds its kernels are held to, an f32 emulation of v3d_pe_mlp_hidden's arithmetic, and the seeded inputs.

Not a conftest: test modules import it (`import pe_mlp_check as MC`; tests/ is on sys.path under pytest).

The rule ("The MLP position encoding, stated once") - the rounding points of the 16-bit torch modules, T = the model dtype:
    z  = T(x w0^T + b0)
    h  = relu(T(LN(z) g + beta))      LayerNorm statistics of the ROUNDED z in f32, eps = 1e-5
    pe = T(h w3^T + b3)
`restate` evaluates it in f64 with exactly these roundings; tests/test_pe_mlp_check_cpu.py holds it against the reference module's own
outputs (tests/golden/pe_mlp.npz: the final rows, |b3| offset so that a unit in the last place is meaningful; tests/golden/pe_mlp_stages.npz:
z, h and pe with the weights as drawn, each stage held to one ulp or to the reference's own f32 error; both written by
tools/gen_pe_mlp_golden.py).

Bounds for the hidden kernel (per element, from reference quantities only; e = 2^-24, hs = rowwise_check.half_spacing):
    z : the f64 linear y, within  hs(y) + 4 e (sum_a |x_a w0_a| + |b0|)        - three fused multiply-adds, one rounding
    h : relu(rowwise_check.layernorm(z_kernel, g, beta, 1e-5)) within that function's own bound, the reference centred on the kernel's
        own z (a legitimate flip of z is not charged to the norm); relu is 1-Lipschitz and exact.
    dw0 : sum_r dz x in f64 within  L e sum_r |dz x| + the output rounding,  L = rowwise_check.colsum_chain(rows) (the f32 chain of
        v3d_colsum's scheme; the products of two 16-bit values are exact in f32).
"""
import numpy as np
import torch

import rowwise_check as RC

DT = {"f16": torch.float16, "bf16": torch.bfloat16}
HIDDEN = 512
KEYS = ("w0", "b0", "ln_w", "ln_b", "w3", "b3")
REF_KEYS = {"w0": "mlp.0.weight", "b0": "mlp.0.bias", "ln_w": "mlp.1.weight", "ln_b": "mlp.1.bias", "w3": "mlp.3.weight", "b3": "mlp.3.bias"}
SD_PREFIX = "model.world_position_embedding."
EPS = 1e-5
SEED = 40417
ROWS = {256: 128, 3584: 20}          # rows per module case of tests/golden/pe_mlp.npz (the file stays well below 1 MiB)
B3_OFFSET = 2.0
E32 = 2.0 ** -24
MIN_XYZ, MAX_XYZ, VOXEL = (-15, -15, -5), (15, 15, 5), 0.1
# the stage cases of tests/golden/pe_mlp_stages.npz: the weights as drawn (no b3 offset), the reference's z, h and pe stored
STAGE_ROWS = {256: 32, 3584: 8}
STAGE_CASES = [(kind, src) for kind in ("f16", "bf16") for src in ("ids", "cont")]
MODULE_CASES = [(E, kind, src) for E in (256, 3584) for kind in ("f16", "bf16") for src in ("ids", "cont")]
MUTATIONS = ("no_b0", "swap_g_beta", "unbiased_var", "relu_first")


def seeded_mlp(E, kind, seed=SEED, w3_scale=1.0, b3_offset=B3_OFFSET):
    """The six tensors in the model dtype: nn.Linear's uniform(+-1/sqrt(fan_in)) for both linears (w3 and b3 times w3_scale), LayerNorm
    weight and bias seeded AWAY from 1 and 0 (swapping or dropping them shows).
    b3_offset: |b3| is moved up by it (random signs kept).  The module cases are compared with the reference in units of the last place of
    each OUTPUT element; the reference's second Linear accumulates 512 products in f32 in an order of its own, an error of about 1e-6 that is
    tens to hundreds of 16-bit ulps of an output that cancels to near zero (measured with b3_offset = 0: up to 613 ulp, only where
    |pe| < 2^-4, also when the restatement starts from the reference's own h) and far below one ulp of an output of ordinary size.  With
    |b3| >= 2 and |h w3^T| below about 1.5 no output cancels, and the comparison measures the rule instead of that noise."""
    g = np.random.default_rng(seed + E)
    u = lambda shape, k: torch.from_numpy(((g.random(shape, dtype=np.float32) * 2 - 1) * k).astype(np.float32))      # noqa: E731
    k0, k3 = 3 ** -0.5, HIDDEN ** -0.5
    p = {"w0": u((HIDDEN, 3), k0), "b0": u((HIDDEN,), k0),
         "ln_w": 1.0 + 0.5 * torch.from_numpy(g.standard_normal(HIDDEN).astype(np.float32)),
         "ln_b": 0.3 * torch.from_numpy(g.standard_normal(HIDDEN).astype(np.float32)),
         "w3": u((E, HIDDEN), k3 * w3_scale), "b3": u((E,), k3 * w3_scale)}
    p["b3"] = p["b3"] + b3_offset * torch.sign(p["b3"])
    return {k: v.to(DT[kind]) for k, v in p.items()}


def seeded_inputs(kind, src, rows, seed=SEED):
    """x [rows, 3] in the model dtype.  'ids': integer-VALUED voxel coordinates as discrete_coords returns them, 0 and 300 and ids above
    256 included (in bf16 such an id is rounded to the type: the rounded value is what the reference feeds).  'cont': continuous
    coordinates in +-15 / +-15 / +-5, negative ones included."""
    g = np.random.default_rng(seed + (1000 if src == "cont" else 0) + rows)
    if src == "cont":
        x = (g.random((rows, 3), dtype=np.float32) - 0.5) * np.array([30, 30, 10], np.float32)
    else:
        x = g.integers(0, 301, (rows, 3)).astype(np.float32)
        x[0] = (0.0, 300.0, 257.0)
        if rows > 1:
            x[1] = (299.0, 1.0, 263.0)
    return torch.from_numpy(x).to(DT[kind])


def _round(v, dt):
    return v.to(torch.float32).to(dt).double() if dt == torch.bfloat16 else v.to(dt).double()


def restate(x, p, stages=False):
    """The rule in f64 with the module's rounding points.  x [N, 3] 16-bit, p the six tensors -> pe [N, E] in x's dtype
    (stages=True: (z, h, pe))."""
    dt = x.dtype
    xd = x.double()
    z = _round(xd @ p["w0"].double().T + p["b0"].double(), dt)
    mean = z.mean(-1, keepdim=True)
    var = ((z - mean) ** 2).mean(-1, keepdim=True)
    y = _round((z - mean) / torch.sqrt(var + EPS) * p["ln_w"].double() + p["ln_b"].double(), dt)
    h = torch.relu(y)
    pe = _round(h @ p["w3"].double().T + p["b3"].double(), dt)
    return (z.to(dt), h.to(dt), pe.to(dt)) if stages else pe.to(dt)


def restate_f32(x, p):
    """The same function in f32 torch ops WITHOUT the 16-bit roundings, differentiable in the six tensors: what torch autograd is run on
    for the training tests' gradient reference."""
    z = x.float() @ p["w0"].T + p["b0"]
    y = torch.nn.functional.layer_norm(z, (HIDDEN,), p["ln_w"], p["ln_b"], EPS)
    return torch.relu(y) @ p["w3"].T + p["b3"]


def ordered(bits16):
    """uint16 bit patterns -> integers ordered like the values (adjacent representable values differ by 1; -0 and +0 coincide)."""
    b = bits16.astype(np.int32)
    return np.where(b & 0x8000, -(b & 0x7FFF), b)


def bits(t):
    return t.contiguous().view(torch.int16).numpy().view(np.uint16)


def from_bits(a, kind):
    return torch.from_numpy(np.ascontiguousarray(a).view(np.int16)).view(DT[kind])


def ulp_shares(got, want_bits):
    """(share of elements that differ, largest difference in units of the last place of the 16-bit type)."""
    d = np.abs(ordered(bits(got)) - ordered(want_bits))
    return float((d != 0).mean()), int(d.max())


# ------------------------------------------------------------------------------ bounds


def z_reference(x, p):
    """-> (y, bound) f64 [N, 512]: the f64 linear and hs(y) + 4 e (sum |x w0| + |b0|)."""
    dt = x.dtype
    xd, wd, bd = x.double(), p["w0"].double(), p["b0"].double()
    y = xd @ wd.T + bd
    mass = xd.abs() @ wd.abs().T + bd.abs()
    return y, RC.half_spacing(y, dt) + 4 * E32 * mass


def h_reference(z_kernel, p):
    """-> (relu(LN(z_kernel) g + beta), bound) f64: rowwise_check.layernorm on the kernel's own rounded z, its own bound."""
    y, b = RC.layernorm(z_kernel, p["ln_w"], p["ln_b"], EPS)
    return torch.relu(y), b


def last_linear_slack(h, p):
    """Per element, what the reference's own second Linear may differ by from the exact sum before its one rounding: it adds 512 products
    and the bias in f32 in an order of its own, at most (K - 1 + 1) e sum |terms| for any order (K = 512, e = 2^-24).  f64 [N, E]."""
    return HIDDEN * E32 * (h.double().abs() @ p["w3"].double().abs().T + p["b3"].double().abs())


def wgrad_reference(dz, x, out_dtype=None):
    """-> (dw0 f64 [512, 3], bound): colsum_chain(rows) e sum |dz x| + the rounding of the output."""
    dt, rows = dz.dtype, dz.shape[0]
    dzd, xd = dz.double(), x.double()
    dw = dzd.T @ xd
    mass = dzd.abs().T @ xd.abs()
    return dw, RC._out(dw, dt, out_dtype, RC.C32 * RC.colsum_chain(rows) * E32 * mass)


def colsum_reference(dz, out_dtype=None):
    dt, rows = dz.dtype, dz.shape[0]
    s = dz.double().sum(0)
    return s, RC._out(s, dt, out_dtype, RC.C32 * RC.colsum_chain(rows) * E32 * dz.double().abs().sum(0))


# ------------------------------------------------------------------------------ f32 emulation of v3d_pe_mlp_hidden


def _f32(v):
    return v.float().double()


def _fma(a, b, c):
    """fmaf on f32 values held in f64 (a b is exact in f64 for the operands used here)."""
    return _f32(a * b + c)


def _wave_sum(s):
    """s [N, 64] per-lane partial sums -> the xor-butterfly total of the kernel (offsets 32 .. 1), every add rounded to f32; [N, 1]."""
    lanes = torch.arange(64)
    for off in (32, 16, 8, 4, 2, 1):
        s = _f32(s + s[:, lanes ^ off])
    return s[:, :1]


def emulate_hidden(x, p, mutate=None):
    """The kernel's arithmetic step by step (f32 values carried in f64): three fused multiply-adds on b0, one rounding to T; per-lane sums
    of 8 then six shuffle adds; the sum of squared differences likewise; (z - mean) * rstd * g + beta, each f32 op rounded; T; relu.
    mutate: one of MUTATIONS - a wrong kernel the bounds must reject.  Returns (z, h) in x's dtype."""
    dt = x.dtype
    xd, w, b = x.double(), p["w0"].double(), p["b0"].double()
    g, beta = p["ln_w"].double(), p["ln_b"].double()
    if mutate == "swap_g_beta":
        g, beta = beta, g
    acc = (torch.zeros_like(b) if mutate == "no_b0" else b).expand(x.shape[0], HIDDEN)
    for a in range(3):
        acc = _fma(xd[:, a:a + 1], w[:, a][None, :], acc)
    z = _round(acc, dt)
    zz = torch.relu(z) if mutate == "relu_first" else z
    lanes = zz.reshape(-1, 64, 8)
    s = torch.zeros(lanes.shape[:2], dtype=torch.float64)
    for j in range(8):
        s = _f32(s + lanes[:, :, j])
    mean = _f32(_wave_sum(s) / HIDDEN)
    d = _f32(lanes - mean[:, :, None])
    q = torch.zeros_like(s)
    for j in range(8):
        q = _fma(d[:, :, j], d[:, :, j], q)
    den = HIDDEN - 1 if mutate == "unbiased_var" else HIDDEN
    rstd = _f32(1.0 / _f32(torch.sqrt(_f32(_f32(_wave_sum(q) / den) + np.float32(EPS)))))
    y = _f32(_f32(_f32(_f32(zz - mean) * rstd) * g) + beta)
    h = _round(y, dt)
    if mutate != "relu_first":
        h = torch.relu(h)
    return z.to(dt), h.to(dt)
