"""f64 reference, per-element error bound and structured inputs for the attention forward kernels.

Not a conftest: test modules import it (`from attention_check import ...`; tests/ is on sys.path under pytest).

Reference.  softmax(scale q k^T) v in f64 from the same 16-bit q, k, v, with the causal offset q_pos0 (query i sits at key
position q_pos0 + i and sees keys j <= q_pos0 + i) and GQA grouping (query head h reads kv head h // (Hq / Hkv)).  It works on
whatever device the inputs are on, one query head and one block of rows at a time, so the [S, S] matrix of all heads is never
formed; long sequences are checked on the device.

Bound.  Per element, from reference quantities only (p = the f64 probabilities, o = the f64 output, u = 2^-8 for bf16 and
2^-11 for f16, the unit roundoff being u / 2).  It follows the rounding points the kernels have (attn_prefill_kernel, its
16x16 / 64-query / SigLIP forms, the decode split, matrix-core split, merge and shared-prefix kernels):

  score  Q is multiplied by scale log2(e) in f32 and rounded to 16 bit before Q K^T (the prefill kernels; the decode kernels keep
         it in f32, which only removes this term).  That moves score j by at most e_ij = u/2 scale sum_d |q_id k_jd| (natural
         units), so p_j by the factor exp(delta_j), |delta_j| <= e_ij, and, to first order,
             |delta o_i| <= sum_j p_ij e_ij |v_j - o_i| <= (p e) |v| + |o_i| sum_j p_ij e_ij          (C_SCORE = 2)
  P      the probabilities are rounded to 16 bit before P.V, the row sum l takes them unrounded (f32):
             |delta o_i| <= u/2 sum_j p_ij |v_j|                                                       (C_P = 1.25)
         f16 only: probabilities below 2^-14 of the running maximum are subnormal, spaced 2^-24.  The running maximum m never
         exceeds the row's true maximum M, so l >= 2^(M - m) and the absolute error of one key is at most 2^-25 / Z after
         normalising, Z = sum_j exp(s_j - M):      |delta o_i| <= 2^-25 sum_j |v_j| / Z                (C_P)
  acc    f32 accumulation of P.V and l over n visible keys in chains of at most n / 8 + 64 additions:
             |delta o_i| <= (n / 8 + 64) 2^-24 (p |v| + |o_i|)                                         (C_ACC = 2)
  out    the final rounding of the output, u/2 |o_i| (plus 2^-25, half the f16 subnormal spacing, for f16; 1.0 x).
The constants only cover second-order terms and exp2 / f32 product errors, which are far below every term they scale.

lse (v3d_attention_train) is m + log2(l) in the kernel's scaled log2 units; the reference is log2(e) (max_j s_j + ln Z).  The score
term is the same rounding of Q, bounded through it directly: the first-order change is sum_j p_j delta_j = sum_d eps_d c q_d kbar_d
with |eps_d| <= u/2, c = scale log2(e) and kbar = sum_j p_j k_j, and the second-order one is at most ln(2)/2 sum_j p_j (e_j log2 e)^2:
    |delta lse| <= C_SCORE (u/2 c sum_d |q_d kbar_d| + ln2 sum_j p_j (e_j log2 e)^2) + C_ACC (n / 8 + 64) 2^-24 log2(e)
                   + 2^-20 (1 + |lse|)                     (f32 rounding of m + log2(l) and v_log_f32)
The P term is absent: l sums the unrounded probabilities.

Inputs.  Random q, k, v stay as a background; two structured families put the softmax mass where a tiled kernel can lose it:
diagonal-peaked rows (RoPE-style rotations whose dot product peaks at j = i) and needles (keys at chosen positions that every
query sees with score about log S + 3).
"""
import math

import torch

U = {torch.bfloat16: 2.0 ** -8, torch.float16: 2.0 ** -11}
LOG2E = 1.0 / math.log(2.0)
C_SCORE, C_P, C_ACC = 2.0, 1.25, 2.0
TINY = 2.0 ** -25          # half the f16 subnormal spacing


def rows_of(Sq, *groups):
    """Sorted distinct row indices in [0, Sq) from ints / ranges (negative counts from the end)."""
    out = set()
    for g in groups:
        for r in (g if isinstance(g, (range, list, tuple)) else [g]):
            r = r + Sq if r < 0 else r
            if 0 <= r < Sq:
                out.add(r)
    return sorted(out)


def reference(q, k, v, scale, causal=True, q_pos0=0, rows=None, d_out=None, block=1024, keys=None, near=0):
    """q [Sq, Hq, D], k / v [Sk, Hkv, D] (16 bit, any device) -> dict of f64 tensors on that device:
    o [R, Hq, d_out], bound [R, Hq, d_out], lse / lse_bound [Hq, R] (scaled log2 units), rows [R];
    mass_keys [R, Hq, len(keys)] = p at the given key positions (if keys), near [R, Hq] = p on keys q_pos0 + i - near .. q_pos0 + i."""
    dt = q.dtype
    u = U[dt]
    Sq, Hq, D = q.shape
    Sk, Hkv = k.shape[0], k.shape[1]
    G = Hq // Hkv
    d_out = d_out or v.shape[2]
    dev = q.device
    rows = torch.arange(Sq, device=dev) if rows is None else torch.as_tensor(rows, device=dev, dtype=torch.long)
    R = rows.numel()
    res = {n: torch.empty(R, Hq, d_out, dtype=torch.float64, device=dev) for n in ("o", "bound")}
    res["lse"] = torch.empty(Hq, R, dtype=torch.float64, device=dev)
    res["lse_bound"] = torch.empty(Hq, R, dtype=torch.float64, device=dev)
    res["rows"] = rows
    if keys is not None:
        keys_t = torch.as_tensor(keys, device=dev, dtype=torch.long)
        res["mass_keys"] = torch.empty(R, Hq, keys_t.numel(), dtype=torch.float64, device=dev)
    if near:
        res["near"] = torch.empty(R, Hq, dtype=torch.float64, device=dev)
    jj = torch.arange(Sk, device=dev)
    c = scale * LOG2E
    for hk in range(Hkv):
        kh = k[:, hk, :D].double()
        vh = v[:, hk, :d_out].double()
        ka, va = kh.abs(), vh.abs()
        for h in range(hk * G, hk * G + G):
            for r0 in range(0, R, block):
                rr = rows[r0:r0 + block]
                qh = q[rr, h, :D].double()
                if d_out < D:       # dims past d_out belong to no head (SigLIP's 72 of 96): zero, as the kernel zeroes them in Q
                    qh[:, d_out:] = 0
                s = scale * (qh @ kh.T)
                vis = (jj[None, :] <= (rr[:, None] + q_pos0)) if causal else torch.ones(rr.numel(), Sk, dtype=torch.bool, device=dev)
                s = s.masked_fill(~vis, float("-inf"))
                m = s.max(1, keepdim=True).values
                e = torch.exp(s - m)
                Z = e.sum(1, keepdim=True)
                p = e / Z
                del e
                o = p @ vh
                E = (scale * u / 2) * (qh.abs() @ ka.T)          # e_ij, natural units
                pe = p * E
                pv = p @ va
                n = vis.sum(1, keepdim=True).double()
                bnd = C_SCORE * (pe @ va + o.abs() * pe.sum(1, keepdim=True)) + C_P * (u / 2) * pv
                bnd += C_ACC * (n / 8 + 64) * 2.0 ** -24 * (pv + o.abs()) + (u / 2) * o.abs()
                if dt == torch.float16:
                    bnd += C_P * TINY * (vis.double() @ va) / Z + TINY
                res["o"][r0:r0 + block, h] = o
                res["bound"][r0:r0 + block, h] = bnd
                lse = LOG2E * (m[:, 0] + torch.log(Z[:, 0]))
                kbar = p @ kh
                t1 = (u / 2) * c * (qh.abs() * kbar.abs()).sum(1)
                t2 = math.log(2.0) * (pe * E).sum(1) * LOG2E ** 2
                res["lse"][h, r0:r0 + block] = lse
                res["lse_bound"][h, r0:r0 + block] = C_SCORE * (t1 + t2) + C_ACC * (n[:, 0] / 8 + 64) * 2.0 ** -24 * LOG2E + \
                    2.0 ** -20 * (1 + lse.abs())
                if keys is not None:
                    res["mass_keys"][r0:r0 + block, h] = p[:, keys_t]
                if near:
                    lo = rr[:, None] + q_pos0 - near
                    res["near"][r0:r0 + block, h] = (p * ((jj[None, :] >= lo) & vis)).sum(1)
                del s, p, pe, E, vis
    return res


def ratio(got, ref):
    """Worst |got - o| / bound over the reference's rows (got [>= R rows indexed by ref['rows'], Hq, d_out] or already [R, ...]).
    NaN anywhere (an output the kernel never wrote) gives inf."""
    g = got.to(ref["o"].device).double()
    if g.shape[0] != ref["o"].shape[0]:
        g = g[ref["rows"]]
    g = g[..., : ref["o"].shape[-1]]
    if not bool(torch.isfinite(g).all()):
        return float("inf")
    return ((g - ref["o"]).abs() / ref["bound"]).max().item()


def lse_ratio(got, ref):
    """got [Hq, >= R] f32 lse in scaled log2 units."""
    g = got.to(ref["lse"].device).double()
    if g.shape[1] != ref["lse"].shape[1]:
        g = g[:, ref["rows"]]
    if not bool(torch.isfinite(g).all()):
        return float("inf")
    return ((g - ref["lse"]).abs() / ref["lse_bound"]).max().item()


def old_rule_ratio(got, ref, dtype, ulps=3.0, floor=0.3):
    """The suite's earlier rule close(..., ulps, floor): |err| <= ulps 2u (|o| + floor) (EPS = 2u)."""
    g = got.to(ref["o"].device).double()
    if g.shape[0] != ref["o"].shape[0]:
        g = g[ref["rows"]]
    b = ulps * 2 * U[dtype] * (ref["o"].abs() + floor)
    return ((g - ref["o"]).abs() / b).max().item()


# ------------------------------------------------------------------------------ inputs


def _rot(base, pos, freqs):
    """Rotate pairs (d, d + D/2) of base [H, D] by angle pos * freqs[f] -> [S, H, D] (RoPE's half-split layout)."""
    half = base.shape[-1] // 2
    ang = pos[:, None].double() * freqs[None, :].double()           # [S, half]
    cs, sn = torch.cos(ang)[:, None, :], torch.sin(ang)[:, None, :]
    a, b = base[None, :, :half].double(), base[None, :, half:].double()
    return torch.cat([a * cs - b * sn, a * sn + b * cs], -1)


def diagonal_inputs(Sq, Sk, Hq, Hkv, D, dtype, q_pos0=0, peak=None, noise=0.05, seed=0, device="cpu"):
    """Diagonal-peaked q, k and random v: q_i = rot(q_pos0 + i) a_h, k_j = rot(j) a_hk with one vector a per kv head shared by its
    query heads (head-scaled), so q_i . k_j = sum_f r_f^2 cos(w_f (i - j)): the peak sits on the query's own key and decays within a
    few keys (frequencies spread over [0.05, 0.8] rad: key i - 1 scores about 0.1 peak below key i, key i - 3 about
    0.75 peak below it), plus a little noise so rows and heads differ.  peak = the diagonal score in
    natural units (default log Sk + 6)."""
    g = torch.Generator().manual_seed(seed)
    peak = peak if peak is not None else math.log(Sk) + 6.0
    half = D // 2
    freqs = 0.05 + 0.75 * torch.rand(half, generator=g, dtype=torch.float64)
    scale = 1.0 / math.sqrt(D)
    base = torch.randn(Hkv, D, generator=g, dtype=torch.float64)
    r2 = base[:, :half] ** 2 + base[:, half:] ** 2
    base = base / torch.sqrt(r2.sum(1, keepdim=True)) * math.sqrt(peak / scale)      # |a|^2 scale = peak
    qb = base.repeat_interleave(Hq // Hkv, 0) * (0.9 + 0.2 * torch.rand(Hq, 1, generator=g, dtype=torch.float64))
    q = _rot(qb, torch.arange(Sq) + q_pos0, freqs) + noise * torch.randn(Sq, Hq, D, generator=g, dtype=torch.float64)
    k = _rot(base, torch.arange(Sk), freqs) + noise * torch.randn(Sk, Hkv, D, generator=g, dtype=torch.float64)
    v = torch.randn(Sk, Hkv, D, generator=g)
    return q.to(dtype).to(device), k.to(dtype).to(device), v.to(dtype).to(device)


def needle_positions(Sk, kps=256, chunk=256, prefix=None, tile=64):
    """Key 0, 64-key tile edges, split / prefix-chunk edges, P - 1 and P of a shared prefix, Sk - 1 (distinct, sorted, < Sk)."""
    pos = {0, Sk - 1, tile - 1, tile, 2 * tile - 1, 2 * tile}
    for e in (kps, chunk):
        for m in range(1, 4):
            pos.update((m * e - 1, m * e))
    for frac in (0.5, 0.75):              # edges far into the row (late tiles, late splits)
        t = int(Sk * frac) // tile * tile
        pos.update((t - 1, t))
    if prefix:
        pos.update((prefix - 1, prefix))
    return sorted(p for p in pos if 0 <= p < Sk)


def needle_inputs(Sq, Sk, Hq, Hkv, D, dtype, positions, q_pos0=0, boost=3.0, seed=0, device="cpu", nd=8, bg=0.5, vs=2.0):
    """Random background (q, k ~ bg N(0, 1) off the needle dims) plus needles: dims [0, nd) of every q hold alpha / sqrt(nd), of the
    needle keys beta / sqrt(nd) (zero elsewhere), so a needle scores scale alpha beta = log Sk + boost for every query that sees it.
    The needle dims are kept apart from the background, which keeps sum_d |q_d k_d| (the score-rounding term) close to |q . k|.
    Needle values are vs x larger than the background's, so each carries a visible share of the output."""
    g = torch.Generator().manual_seed(seed)
    scale = 1.0 / math.sqrt(D)
    s_n = math.log(Sk) + boost
    alpha = 4.0
    beta = s_n / (scale * alpha)
    q = bg * torch.randn(Sq, Hq, D, generator=g, dtype=torch.float64)
    k = torch.randn(Sk, Hkv, D, generator=g, dtype=torch.float64)
    v = torch.randn(Sk, Hkv, D, generator=g, dtype=torch.float64)
    q[..., :nd] = alpha / math.sqrt(nd)
    k[..., :nd] = 0
    pos = torch.as_tensor(positions, dtype=torch.long)
    k[pos, :, :nd] = beta / math.sqrt(nd)
    k[pos, :, nd:] = 0                        # needle keys: the shared direction alone
    v[pos] *= vs
    return q.to(dtype).to(device), k.to(dtype).to(device), v.to(dtype).to(device)


def random_inputs(Sq, Sk, Hq, Hkv, D, dtype, seed=0, device="cpu"):
    g = torch.Generator().manual_seed(seed)
    q = torch.randn(Sq, Hq, D, generator=g)
    k = torch.randn(Sk, Hkv, D, generator=g)
    v = torch.randn(Sk, Hkv, D, generator=g)
    return q.to(dtype).to(device), k.to(dtype).to(device), v.to(dtype).to(device)
