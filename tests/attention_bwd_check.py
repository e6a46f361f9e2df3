"""f64 reference, per-element error bound and structured inputs for the attention backward kernels (attention_bwd.hip).

Not a conftest and not collected: test modules import it (tests/ is on sys.path under pytest).  The constants, the three q / k / v input
families and the forward reference (for the end-to-end bound) come from attention_check.py.

The function under test.  v3d_attention_backward is a function of (q, k, v, o, dO, lse).  The primary tests hand it o = T(o_ref) and
lse = f32(lse_ref) from the f64 forward, so the only input errors are one rounding each and a forward defect can neither hide nor
mimic a backward one.  The end-to-end tests chain the device forward in front and widen the bound by the forward's own bounds.

Reference.  f64, on whatever device the inputs are on, one query head and one block of rows at a time (no [Hq, S, S] tensor), kv head
h // (Hq / Hkv), causal (key j <= query i) or not, over a batch of sequences:
    p = softmax(scale q k^T)      dp = dO v^T      delta_i = sum_d dO_id o_id (the exact f64 o)      ds = p (dp - delta)
    dq = scale ds k               dk_g = scale sum_{h in g} ds_h^T q_h                               dv_g = sum_{h in g} p_h^T dO_h

Bound.  Per element of dq, dk and dv, from reference quantities only (r = 2^-8 for bf16, 2^-11 for f16: the unit roundoff, half the
spacing of the numbers in [1, 2) - attention_check's U, taken whole, see below; c = scale log2(e); GAMMA = 128 x 2^-24, the worst-case constant of an f32 sum of 128 terms, which is what one head-dim dot product is).
One term per rounding point of the kernels:

  1 cQ     attn_bwd_dq_kernel rounds c Q to 16 bit before K (cQ)^T, as the forward does: score j moves by at most
           E_ij = r scale sum_d |q_id k_jd| (natural units) and p_ij, hence ds_ij, by the relative factor E_ij (C_SCORE = 2 covers
           exp(E) - 1 against E).  attn_bwd_dkv_kernel forms S = Q K^T from the unrounded Q and applies c in f32 (fmaf): no such term.
  2 lse    both kernels take exp2(score - lse).  The given lse carries its f32 rounding, 2^-24 |lse|; the score is an f32 sum of 128
           products that starts from -lse (dQ) or is scaled and shifted by one fmaf (dK/dV), GAMMA (|lse| + c sum_d |q k|); exp2 itself
           is good to 2^-22.  Times ln 2 these are a relative error of every p_ij of the row:
               F_ij = ln2 ((GAMMA + 2^-24) |lse_i| + GAMMA c sum_d |q_id k_jd|) + 2^-22            (x C_ACC = 2)
           End to end, F_ij grows by ln2 lse_bound_i, the forward's own bound.
           Together: rel_q = C_SCORE E + C_ACC F in the dQ kernel, rel_kv = C_ACC F in the dK/dV kernel.
  3 delta  attn_delta_kernel sums dO o in f32 (a pair per lane, then a 6-step shuffle tree) from the 16-bit o it is given:
               Ddelta_i = r sum_d |dO_id o_id|  (+ 2^-25 sum_d |dO_id| for f16: o below 2^-14 is subnormal)
                          (+ sum_d |dO_id| bound_id end to end, the forward's output bound)
           and dp = dO v^T is an MFMA sum in another order.  Both enter ds_ij times p_ij as an ABSOLUTE error
               p_ij (GAMMA (sum_d |dO_id v_jd| + sum_d |dO_id o_id|) + Ddelta_i)                    (x C_DELTA = 1.25: p (1 + rel))
           which is all there is where dp and delta cancel (S = 1: dq = dk = 0 exactly in the reference, the kernel's two sums differ in
           their last bits).  Terms 1-3 make   ErrDS = rel |ds| + C_DELTA p (GAMMA (|dO| |v|^T + B) + Ddelta),  ErrP = rel_kv p.
  4 P, dS  rounded to 16 bit before the second products: r (p + ErrP) into dV, r (|ds| + ErrDS) into dQ and dK (x C_P = 1.25:
           the product with the 16-bit operand is exact in f32).  f16 only: values below 2^-14 are subnormal, spaced 2^-24, so every
           visible (i, j) adds 2^-25, summed against |k_jd|, |q_id|, |dO_id|.
  5 acc    f32 accumulation of the second products: each 64-row tile adds four MFMAs (k = 16) into the accumulator, so n visible
           rows make a chain of n / 16 accumulator roundings plus the 16 terms inside one MFMA; the forward's n / 8 + 64 covers that:
               C_ACC (n / 8 + 64) 2^-24 |ds|   (n = visible keys of the query for dQ, visible queries of the key for dK / dV; p for dV)
           and attn_bwd_reduce_kernel adds the group's f32 per-head partials in head order: group 2^-24 sum_h |partial_h| (which
           also covers the f32 product with scale in front of the partial).
  6 out    scale in f32 and the final rounding to 16 bit: (r + 2^-23) |out|, plus 2^-25 for f16.

  dq_bound = scale (Wq |k|) + out,       Wq = ErrDS_q + C_P r (|ds| + ErrDS_q) [+ 2^-25 visible] + acc
  dk_bound = sum_h scale (Wk^T |q_h|) + reduce + out,   Wk the same with rel_kv and the key's chain
  dv_bound = sum_h (Wv^T |dO_h|) + reduce + out,        Wv = ErrP + C_P r (p + ErrP) [+ 2^-25 visible] + acc
Every term is a matrix product of non-negative reference quantities.
The roundoff.  attention_check.py writes its rounding terms with u / 2 = half the unit roundoff, which is the error of a rounding on
average, not at worst; the forward's outputs are sums over many keys and stay inside it.  The backward has elements that are a single
product rounded once or twice (dv of the last key: one query per head), and the CPU emulation of the exact kernel arithmetic exceeds a
bound written with r / 2 there (1.1 x at S = 200).  A round-to-nearest to 8 (11) significant bits errs by up to 2^-8 (2^-11) of the
value, so every rounding term here takes r whole.  Where the bound is exactly 0 (bf16, rows and keys that only
meet dO = 0) the result has to be exactly 0.

Upstream gradients.  Dense: dO ~ N(0, 1).  Sparse: dO = 0 except on query rows at tile and wave edges (HOT_ROWS, all heads): rows with
dO = 0 have dp = delta = ds = 0, so every cold row of dQ is exactly 0 and, under the causal mask, so is every row of dK and dV past
the last hot row (zero_claims) - a contribution from a stale stage, a wrong tile or a padded row breaks that without any tolerance.
"""
import math

import torch

from attention_check import (C_ACC, C_P, C_SCORE, LOG2E, TINY, U, diagonal_inputs, needle_inputs, needle_positions, random_inputs,
                             reference)

LN2 = math.log(2.0)
GAMMA = 128 * 2.0 ** -24
C_DELTA = 1.25
HOT_ROWS = (0, 31, 32, 63, 64, 127, 128)     # plus S // 2 and S - 1
NEAR_SHARE, NEEDLE_SHARE = 0.5, 0.02
FAMILIES = ("random", "diagonal", "needles")


def _b4(x):
    return x if x.dim() == 4 else x.unsqueeze(0)


def reference_bwd(q, k, v, dO, scale, causal=True, end_to_end=False, keys=None, block=1024):
    """q, dO [B, S, Hq, D], k / v [B, S, Hkv, D] (16 bit, any device; B may be left out) -> dict of f64 tensors on that device:
    o [B, S, Hq, D], lse [B, Hq, S] (scaled log2 units), dq / dq_bound [B, S, Hq, D], dk / dv / dk_bound / dv_bound [B, S, Hkv, D],
    near [B, S, Hq] = p on keys i - 3 .. i, mass_keys [B, S, Hq, len(keys)] (if keys).  end_to_end: the bound for a backward fed with
    the device forward's o and lse (widened by the forward's bounds)."""
    q, k, v, dO = _b4(q), _b4(k), _b4(v), _b4(dO)
    dt = q.dtype
    r = U[dt]
    f16 = dt == torch.float16
    B, S, Hq, D = q.shape
    Hkv = k.shape[2]
    G = Hq // Hkv
    dev = q.device
    c = scale * LOG2E
    f8 = dict(dtype=torch.float64, device=dev)
    res = {n: torch.zeros(B, S, Hq, D, **f8) for n in ("o", "dq", "dq_bound")}
    res.update({n: torch.zeros(B, S, Hkv, D, **f8) for n in ("dk", "dv", "dk_bound", "dv_bound")})
    res["lse"] = torch.zeros(B, Hq, S, **f8)
    res["near"] = torch.zeros(B, S, Hq, **f8)
    if keys is not None:
        keys_t = torch.as_tensor(keys, device=dev, dtype=torch.long)
        res["mass_keys"] = torch.zeros(B, S, Hq, keys_t.numel(), **f8)
    jj = torch.arange(S, device=dev)
    n_key = (S - jj).double() if causal else torch.full((S,), float(S), **f8)          # visible queries of key j
    chain_key = C_ACC * (n_key / 8 + 64) * 2.0 ** -24
    for b in range(B):
        fwd = reference(q[b], k[b], v[b], scale, causal=causal)
        res["o"][b], res["lse"][b] = fwd["o"], fwd["lse"]
        for hk in range(Hkv):
            kh, vh = k[b, :, hk].double(), v[b, :, hk].double()
            ka, va = kh.abs(), vh.abs()
            abs_dk = torch.zeros(S, D, **f8)
            abs_dv = torch.zeros(S, D, **f8)
            for h in range(hk * G, hk * G + G):
                for r0 in range(0, S, block):
                    rr = jj[r0:r0 + block]
                    qh, doh, oh = q[b, rr, h].double(), dO[b, rr, h].double(), fwd["o"][rr, h]
                    qa, doa = qh.abs(), doh.abs()
                    lse = fwd["lse"][h, rr]
                    vis = (jj[None, :] <= rr[:, None]) if causal else torch.ones(rr.numel(), S, dtype=torch.bool, device=dev)
                    p = torch.exp(scale * (qh @ kh.T) - (lse / LOG2E)[:, None]).masked_fill(~vis, 0.0)
                    delta = (doh * oh).sum(1)
                    ds = p * (doh @ vh.T - delta[:, None])
                    res["dq"][b, rr, h] = scale * (ds @ kh)
                    res["dk"][b, :, hk] += scale * (ds.T @ qh)
                    res["dv"][b, :, hk] += p.T @ doh
                    res["near"][b, rr, h] = (p * ((jj[None, :] >= rr[:, None] - 3) & (jj[None, :] <= rr[:, None]))).sum(1)
                    if keys is not None:
                        res["mass_keys"][b, rr, h] = p[:, keys_t]
                    # ---- the bound
                    qk_abs = qa @ ka.T
                    F = LN2 * ((GAMMA + 2.0 ** -24) * lse.abs()[:, None] + GAMMA * c * qk_abs) + 2.0 ** -22
                    Bi = (doa * oh.abs()).sum(1)
                    Dd = r * Bi
                    if f16:
                        Dd = Dd + TINY * doa.sum(1)
                    if end_to_end:
                        F = F + LN2 * fwd["lse_bound"][h, rr][:, None]
                        Dd = Dd + (doa * fwd["bound"][rr, h]).sum(1)
                    rel_kv = C_ACC * F
                    rel_q = rel_kv + C_SCORE * r * scale * qk_abs
                    del qk_abs, F
                    abs_d = C_DELTA * p * (GAMMA * (doa @ va.T + Bi[:, None]) + Dd[:, None])
                    dsa = ds.abs()
                    tiny = TINY * vis.double() if f16 else 0.0
                    n_q = vis.sum(1, keepdim=True).double()
                    err = rel_q * dsa + abs_d
                    Wq = err + C_P * r * (dsa + err) + tiny + C_ACC * (n_q / 8 + 64) * 2.0 ** -24 * dsa
                    dq = res["dq"][b, rr, h]
                    res["dq_bound"][b, rr, h] = scale * (Wq @ ka) + (r + 2.0 ** -23) * dq.abs() + (TINY if f16 else 0.0)
                    del Wq, rel_q
                    err = rel_kv * dsa + abs_d
                    Wk = err + C_P * r * (dsa + err) + tiny + chain_key[None, :] * dsa
                    res["dk_bound"][b, :, hk] += scale * (Wk.T @ qa)
                    del Wk, err, abs_d
                    Wv = rel_kv * p
                    Wv = Wv + C_P * r * (p + Wv) + tiny + chain_key[None, :] * p
                    res["dv_bound"][b, :, hk] += Wv.T @ doa
                    abs_dk += scale * (dsa.T @ qa)
                    abs_dv += p.T @ doa
                    del Wv, rel_kv, p, ds, dsa, vis
            for name, a in (("dk", abs_dk), ("dv", abs_dv)):
                res[name + "_bound"][b, :, hk] += G * 2.0 ** -24 * a + (r + 2.0 ** -23) * res[name][b, :, hk].abs() + (TINY if f16 else 0.0)
    return res


def _as_dict(got):
    if not isinstance(got, dict):
        got = dict(zip(("dq", "dk", "dv"), got))
    return got


def worst_bwd(got, ref):
    """got: dict or (dq, dk, dv), shaped as the reference's (B may be left out) -> {name: (ratio, (batch, row, head, column))}: the worst
    |err| / bound of every element and where it sits.  A non-finite output gives inf; an element whose bound is 0 has to be exactly 0."""
    out = {}
    for name, g in _as_dict(got).items():
        r = ref[name]
        g = _b4(g).to(r.device).double()
        assert g.shape == r.shape, f"{name}: shape {tuple(g.shape)} against the reference's {tuple(r.shape)}"
        bad = ~torch.isfinite(g)
        if bool(bad.any()):
            out[name] = (float("inf"), tuple(bad.nonzero()[0].tolist()))
            continue
        err = (g - r).abs()
        ratio = torch.where(err == 0, torch.zeros_like(err), err / ref[name + "_bound"])       # x / 0 = inf for x > 0
        i = int(ratio.argmax())
        out[name] = (ratio.flatten()[i].item(), tuple(int(x) for x in torch.unravel_index(torch.tensor(i), ratio.shape)))
    return out


def ratio_bwd(got, ref):
    """-> {"dq": r, "dk": r, "dv": r}, the worst |err| / bound over EVERY element (inf on any non-finite output)."""
    return {n: w[0] for n, w in worst_bwd(got, ref).items()}


def describe(worst):
    return ", ".join(f"{n} {r:.3g} at (batch, row, head, column) = {at}" for n, (r, at) in worst.items())


def old_rule_bwd(got, ref, rel=1.2e-2, elem=3e-2, floor=1e-30):
    """The suite's earlier rule, _close(got, ref, 1.2e-2, 3e-2) of test_gpu_train_dense.py, per gradient -> {name: passes}."""
    out = {}
    for name, g in _as_dict(got).items():
        r = ref[name].float()
        g = _b4(g).to(r.device).float()
        err = (g - r).norm() / r.norm().clamp_min(floor)
        w = (g - r).abs().max() / r.abs().max().clamp_min(floor)
        out[name] = bool(err < rel) and bool(w < elem)
    return out


# ------------------------------------------------------------------------------ inputs


def qkv_inputs(family, S, Hq, Hkv, D, dtype, B=1, seed=0, device="cpu"):
    """-> q [B, S, Hq, D], k, v [B, S, Hkv, D], needle positions (or None); batch element b is drawn with seed + b."""
    pos = needle_positions(S) if family == "needles" else None
    parts = []
    for b in range(B):
        if family == "random":
            parts.append(random_inputs(S, S, Hq, Hkv, D, dtype, seed=seed + b, device=device))
        elif family == "diagonal":
            parts.append(diagonal_inputs(S, S, Hq, Hkv, D, dtype, seed=seed + b, device=device))
        else:
            parts.append(needle_inputs(S, S, Hq, Hkv, D, dtype, pos, seed=seed + b, device=device))
    q, k, v = (torch.stack([p[i] for p in parts]) for i in range(3))
    return q, k, v, pos


def hot_rows(S):
    return sorted({r for r in HOT_ROWS + (S // 2, S - 1) if 0 <= r < S})


def grad_inputs(kind, B, S, Hq, D, dtype, seed=0, device="cpu", hot_batches=None):
    """Upstream gradient [B, S, Hq, D]: "dense" N(0, 1), or "sparse" / "sparse_early": N(0, 1) on hot_rows(S) (all heads, batch elements
    hot_batches, default all) and zero elsewhere.  -> dO, hot rows (None for dense)."""
    g = torch.Generator().manual_seed(seed + 1000)
    dO = torch.randn(B, S, Hq, D, generator=g)
    if kind == "dense":
        return dO.to(dtype).to(device), None
    hot = hot_rows(S)
    if kind == "sparse_early":      # without row S - 1 (when another row is left): the dK / dV claim of zero_claims then covers the keys past S // 2
        hot = [r for r in hot if r != S - 1] or hot
    keep = torch.zeros(B, S, 1, 1)
    for b in (range(B) if hot_batches is None else hot_batches):
        keep[b, hot] = 1.0
    return (dO * keep).to(dtype).to(device), hot


def check_family(family, ref, pos, causal=True):
    """The q / k / v inputs do their job."""
    if family == "diagonal":
        assert ref["near"].min().item() >= NEAR_SHARE, f"diagonal-peaked rows keep only {ref['near'].min().item():.3f} on keys i-3 .. i"
    if family == "needles":
        S = ref["near"].shape[1]
        dev = ref["near"].device
        pos_t = torch.as_tensor(pos, device=dev)
        seen = (pos_t[None, :] <= torch.arange(S, device=dev)[:, None]) if causal else torch.ones(S, pos_t.numel(), dtype=torch.bool, device=dev)
        share = ref["mass_keys"].amin((0, 2))                                          # [S, n]: weakest batch element and head
        assert share[seen].min().item() >= NEEDLE_SHARE, f"a needle holds only {share[seen].min().item():.4f} of its row"
        if bool((~seen).any()):
            assert ref["mass_keys"].amax((0, 2))[~seen].max().item() == 0.0


def check_sparse(hot, S):
    """At least one hot row in the first, a middle and the last 128-row tile."""
    tiles = {r // 128 for r in hot}
    assert 0 in tiles and (S // 2) // 128 in tiles and (S - 1) // 128 in tiles, f"hot rows {hot} miss a 128-row tile of S = {S}"


def zero_claims(got, hot, causal, hot_batches=None):
    """The exact zeros a sparse dO implies -> list of broken claims (empty = all hold).  got: dict or (dq, dk, dv), [B, S, H, D]."""
    got = {n: _b4(g) for n, g in _as_dict(got).items()}
    B, S = got["dq"].shape[:2]
    broken = []
    cold = torch.ones(S, dtype=torch.bool)
    cold[hot] = False
    for b in range(B):
        if hot_batches is not None and b not in hot_batches:
            for n, g in got.items():
                if not bool((g[b] == 0).all()):
                    broken.append(f"{n} of batch element {b} (no hot row) is not exactly 0")
            continue
        if not bool((got["dq"][b][cold.to(got["dq"].device)] == 0).all()):
            rows = (got["dq"][b] != 0).flatten(1).any(1).cpu() & cold
            broken.append(f"dq rows with dO = 0 are not exactly 0 (batch element {b}, first at row {int(rows.nonzero()[0])})")
        if causal and max(hot) + 1 < S:
            for n in ("dk", "dv"):
                if not bool((got[n][b, max(hot) + 1:] == 0).all()):
                    broken.append(f"{n} rows past the last hot row are not exactly 0 (batch element {b})")
    return broken
