"""The attention backward checker (tests/attention_bwd_check.py) has power: a CPU emulation of the kernels' arithmetic passes it, and
emulations with one defect each fail it; what the suite's earlier rule, _close(1.2e-2, 3e-2), says about each is recorded below.
No GPU: these run under -m "not gpu".

The emulation follows attention_bwd.hip in torch f32: delta = sum_d dO o from the 16-bit o; the dQ pass with c Q rounded to 16 bit,
p = exp2(K (cQ)^T - lse), dS rounded to 16 bit, 64-key tiles accumulated in tile order, one product with scale, one rounding; the
dK/dV pass with the unrounded Q, c applied in f32, P and dS rounded to 16 bit, 64-query tiles accumulated in tile order into per-head
f32 partials (dK times scale), the partials of a kv group summed in head order, one rounding.

Mutants (MUTANTS below; every one has to fail the checker on all three q / k / v families, with dense and with sparse dO, in both
dtypes) and what the earlier rule says about each on the random family at S = 700, Hq / Hkv = 4 / 2, dense dO, bf16, as
test_old_rule_on_the_mutants prints it (it judges each gradient on its own; the ones not named pass it):
  (a) dQ skips key tile 5 (of 11)                   _close fails on dq (also when the tile is the last one)
  (b) dK/dV skips query tile 10 (the last)          _close fails on dk, dv
  (c) dK/dV reads tile 9's Q / dO image for tile 10 _close fails on dk, dv
  (d) causal mask off by one, key i + 1 leaks       _close fails on all three;   key i dropped: fails on all three
  (e) clamped rows >= S take part                   _close fails on dk, dv
  (f) delta from head h ^ 1                         _close fails on dq, dk
  (g) delta omitted                                 _close fails on dq, dk
  (h) one head of a kv group not reduced            _close fails on dk, dv (group 2, and one head of seven at S = 200);
      heads of group g + 1 reduced into g           _close fails on dk, dv
  (i) scale missing from dK                         _close fails on dk
  (j) lse off by 0.01                               _close PASSES on all three (the checker: dv 1.5 x, dk 1.03 x its bound)
  (k) kv head h % Hkv                               _close fails on all three
  (l) dO of batch element 1 read from element 0     _close fails on dk, dv
So on the emulation the norm-wise rule is stronger than it was taken to be: of these defects it lets only (j) through whole (a skipped
tile costs a few per cent of max |ref| at S = 700).  What the checker adds is the per-element statement - every defect above is
rejected on the gradient it touches, in every family and dtype, by at least: (a) 3 x (1.3 x on random q, k, v under the sparse dO
in bf16, where two hot rows see the tile), (b) - (e), (h), (i), (k), (l) 35 x or more, (f), (g) 45 x, (j) 1.3 x (an lse off by 0.01 is 0.7 % of every p, against two 16-bit roundings) - and the exact zeros of the sparse family.
"""
import math

import pytest
import torch

from attention_bwd_check import (FAMILIES, check_family, check_sparse, describe, grad_inputs, old_rule_bwd, qkv_inputs, ratio_bwd,
                                 reference_bwd, worst_bwd, zero_claims)

DT = {"bf16": torch.bfloat16, "f16": torch.float16}
D = 128
TILE = 64
F32 = torch.float32


def emulate(q, k, v, o, dO, lse, scale, causal=True, m=None, dO_kv=None):
    """Kernel arithmetic on the CPU for one sequence: q, o, dO [S, Hq, D], k / v [S, Hkv, D] 16 bit, lse [Hq, S] f32
    -> dq [S, Hq, D], dk, dv [S, Hkv, D] (16 bit).  m: the defect to build in (MUTANTS); dO_kv: the dO the dK/dV pass reads."""
    m = m or {}
    dt = q.dtype
    S, Hq, _ = q.shape
    Hkv = k.shape[1]
    G = Hq // Hkv
    scale32 = torch.tensor(scale, dtype=F32)
    c = scale32 * torch.tensor(1.44269504088896340736, dtype=F32)
    L = lse.float() + m.get("lse_shift", 0.0)
    delta = (dO.float() * o.float()).sum(-1).T.contiguous()              # [Hq, S]
    if m.get("no_delta"):
        delta = torch.zeros_like(delta)
    if m.get("delta_head_xor"):
        delta = delta[[h ^ 1 for h in range(Hq)]]
    ii = torch.arange(S)
    vis = (ii[None, :] <= ii[:, None] + m.get("mask_shift", 0)) if causal else torch.ones(S, S, dtype=torch.bool)
    nt = (S + TILE - 1) // TILE
    dq = torch.empty(S, Hq, D, dtype=dt)
    pk, pv = torch.zeros(Hq, S, D), torch.zeros(Hq, S, D)
    zero = torch.zeros(())
    for h in range(Hq):
        hk = h % Hkv if m.get("kv_mod") else h // G
        qf, kf, vf, dof = q[:, h].float(), k[:, hk].float(), v[:, hk].float(), dO[:, h].float()
        # the dQ pass
        qs = (qf * c).to(dt).float()
        p = torch.where(vis, torch.exp2(qs @ kf.T - L[h][:, None]), zero)
        ds = (p * (dof @ vf.T - delta[h][:, None])).to(dt).float()
        acc = torch.zeros(S, D)
        for t in range(nt):
            if t != m.get("dq_skip_key_tile"):
                acc += ds[:, t * TILE:(t + 1) * TILE] @ kf[t * TILE:(t + 1) * TILE]
        dq[:, h] = (acc * scale32).to(dt)
        # the dK/dV pass
        dok = (dO if dO_kv is None else dO_kv)[:, h].float()
        dk, dv = torch.zeros(S, D), torch.zeros(S, D)
        for t in range(nt):
            if t == m.get("kv_skip_q_tile"):
                continue
            rows = torch.arange(t * TILE, min(S, (t + 1) * TILE))
            src = rows - TILE if t == m.get("kv_stale_tile") else rows           # the image of the previous tile, this tile's statistics
            if m.get("clamped_rows") and t == nt - 1 and S % TILE:                 # the image's rows past S re-read row S - 1
                pad = torch.full((TILE - S % TILE,), S - 1)
                rows, src = torch.cat([rows, pad]), torch.cat([src, pad])
            qi, doi = qf[src], dok[src]
            pt = torch.where(vis[rows], torch.exp2((qi @ kf.T) * c - L[h][rows][:, None]), zero)
            dst = pt * (doi @ vf.T - delta[h][rows][:, None])
            dv += pt.to(dt).float().T @ doi
            dk += dst.to(dt).float().T @ qi
        pk[h] = dk if m.get("dk_no_scale") else dk * scale32
        pv[h] = dv
    dk_out, dv_out = torch.empty(S, Hkv, D, dtype=dt), torch.empty(S, Hkv, D, dtype=dt)
    for g in range(Hkv):
        src_g = (g + 1) % Hkv if m.get("reduce_next_group") else g
        a, b = torch.zeros(S, D), torch.zeros(S, D)
        for j in range(G):
            if j != m.get("reduce_skip"):
                a += pk[src_g * G + j]
                b += pv[src_g * G + j]
        dk_out[:, g], dv_out[:, g] = a.to(dt), b.to(dt)
    return dq, dk_out, dv_out


_cache = {}


def setup(family, S, kind, causal=True, do_kind="dense", Hq=4, Hkv=2, B=1):
    """Inputs, the f64 reference (once per configuration) and the backward's o = T(o_ref), lse = f32(lse_ref)."""
    key = (family, S, kind, causal, do_kind, Hq, Hkv, B)
    if key not in _cache:
        dt = DT[kind]
        q, k, v, pos = qkv_inputs(family, S, Hq, Hkv, D, dt, B=B)
        dO, hot = grad_inputs(do_kind, B, S, Hq, D, dt)
        scale = 1.0 / math.sqrt(D)
        ref = reference_bwd(q, k, v, dO, scale, causal=causal, keys=pos)
        _cache[key] = dict(q=q, k=k, v=v, dO=dO, scale=scale, pos=pos, hot=hot, ref=ref, causal=causal, o=ref["o"].to(dt),
                           lse=ref["lse"].float())
    return _cache[key]


def run(s, m=None, dO_kv=None):
    """The emulation over the batch -> (dq, dk, dv) [B, S, H, D]."""
    outs = [emulate(s["q"][b], s["k"][b], s["v"][b], s["o"][b], s["dO"][b], s["lse"][b], s["scale"], s["causal"], m,
                    None if dO_kv is None else dO_kv[b]) for b in range(s["q"].shape[0])]
    return tuple(torch.stack([o[i] for o in outs]) for i in range(3))


def check_inputs(family, do_kind, s):
    check_family(family, s["ref"], s["pos"], s["causal"])
    if do_kind == "sparse":
        check_sparse(s["hot"], s["q"].shape[1])


@pytest.mark.parametrize("kind", ["bf16", "f16"])
@pytest.mark.parametrize("causal", [True, False], ids=["causal", "full"])
@pytest.mark.parametrize("do_kind", ["dense", "sparse"])
@pytest.mark.parametrize("family", FAMILIES)
@pytest.mark.parametrize("S", [1, 200, 700])
def test_checker_accepts_the_kernel_arithmetic(S, family, do_kind, causal, kind):
    s = setup(family, S, kind, causal, do_kind)
    check_inputs(family, do_kind, s)
    got = run(s)
    w = worst_bwd(got, s["ref"])
    print(f"{family} {do_kind} S={S} {kind} causal={causal}: {describe(w)}")
    assert max(r for r, _ in w.values()) <= 1.0, describe(w)
    if do_kind == "sparse":
        assert zero_claims(got, s["hot"], causal) == []


@pytest.mark.parametrize("kind", ["bf16", "f16"])
@pytest.mark.parametrize("family", FAMILIES)
@pytest.mark.parametrize("do_kind", ["dense", "sparse_early"])
def test_checker_accepts_group_of_seven(do_kind, family, kind):
    s = setup(family, 200, kind, True, do_kind, Hq=7, Hkv=1)
    got = run(s)
    w = worst_bwd(got, s["ref"])
    print(f"{family} {do_kind} 7/1 {kind}: {describe(w)}")
    assert max(r for r, _ in w.values()) <= 1.0, describe(w)
    if do_kind != "dense":
        assert s["hot"][-1] == 128 and zero_claims(got, s["hot"], True) == []          # dK, dV of keys 129 .. 199 exactly 0


S_MUT = 700      # 10 x 64 + 60: a partial last tile
ALL = FAMILIES

MUTANTS = {      # name -> (defect, the families that have to reject it, keyword arguments of setup)
    "a: dQ skips key tile 5": (dict(dq_skip_key_tile=5), ALL, {}),
    "b: dK/dV skips query tile 10": (dict(kv_skip_q_tile=10), ALL, {}),
    "c: dK/dV reads the stale stage for tile 10": (dict(kv_stale_tile=10), ALL, {}),
    "d: causal mask leaks key i + 1": (dict(mask_shift=1), ALL, {}),
    "d: causal mask drops key i": (dict(mask_shift=-1), ALL, {}),
    "e: clamped rows take part": (dict(clamped_rows=True), ALL, {}),
    "f: delta from head h ^ 1": (dict(delta_head_xor=True), ALL, {}),
    "g: delta omitted": (dict(no_delta=True), ALL, {}),
    "h: last head of a group not reduced": (dict(reduce_skip=1), ALL, {}),
    "h: one head of seven not reduced": (dict(reduce_skip=3), ALL, dict(S=200, Hq=7, Hkv=1)),
    "h: group g + 1 reduced into g": (dict(reduce_next_group=True), ALL, {}),
    "i: scale missing from dK": (dict(dk_no_scale=True), ALL, {}),
    "j: lse off by 0.01": (dict(lse_shift=0.01), ALL, {}),
    "k: kv head h % Hkv": (dict(kv_mod=True), ALL, {}),
}
CASES = [(name, fam) for name, (_, fams, _) in MUTANTS.items() for fam in fams]


def rejected(got, s):
    r = ratio_bwd(got, s["ref"])
    broken = zero_claims(got, s["hot"], s["causal"]) if s["hot"] else []
    return max(r.values()) > 1.0 or bool(broken), r, broken


@pytest.mark.parametrize("kind", ["bf16", "f16"])
@pytest.mark.parametrize("do_kind", ["dense", "sparse"])
@pytest.mark.parametrize("mutant,family", CASES)
def test_checker_rejects_mutants(mutant, family, do_kind, kind):
    m, _, kw = MUTANTS[mutant]
    kw = dict(dict(S=S_MUT), **kw)
    s = setup(family, kw.pop("S"), kind, True, do_kind, **kw)
    bad, r, broken = rejected(run(s, m), s)
    print(f"{mutant} ({family}, {do_kind}, {kind}): err/bound {r}, zero claims broken: {broken}")
    assert bad


@pytest.mark.parametrize("kind", ["bf16", "f16"])
@pytest.mark.parametrize("family", FAMILIES)
def test_checker_rejects_clamped_rows_without_causal_mask(family, kind):
    """(e) in the SigLIP form: the mask is all there is to keep the re-read rows out."""
    s = setup(family, 200, kind, False, "dense")
    bad, r, _ = rejected(run(s, dict(clamped_rows=True)), s)
    print(f"clamped rows, non-causal ({family}, {kind}): err/bound {r}")
    assert bad


@pytest.mark.parametrize("kind", ["bf16", "f16"])
@pytest.mark.parametrize("do_kind", ["dense", "sparse"])
@pytest.mark.parametrize("family", FAMILIES)
def test_checker_rejects_dO_of_the_wrong_batch_element(family, do_kind, kind):
    """(l) B = 2, non-causal, S = 65: the dK/dV pass reads batch element 0's dO for batch element 1 (sparse: hot rows in element 1 only,
    so element 1's dK and dV come out exactly 0 - and wrong)."""
    key = ("batch", family, do_kind, kind)
    if key not in _cache:
        dt = DT[kind]
        q, k, v, pos = qkv_inputs(family, 65, 4, 4, D, dt, B=2)
        dO, hot = grad_inputs(do_kind, 2, 65, 4, D, dt, hot_batches=[1])
        ref = reference_bwd(q, k, v, dO, 1.0 / math.sqrt(D), causal=False, keys=pos)
        _cache[key] = dict(q=q, k=k, v=v, dO=dO, scale=1.0 / math.sqrt(D), pos=pos, hot=hot, ref=ref, causal=False, o=ref["o"].to(dt),
                           lse=ref["lse"].float())
    s = _cache[key]
    check_family(family, s["ref"], s["pos"], False)
    good = run(s)
    assert max(ratio_bwd(good, s["ref"]).values()) <= 1.0
    if do_kind == "sparse":
        assert zero_claims(good, s["hot"], False, hot_batches=[1]) == []
    got = run(s, dO_kv=s["dO"][[0, 0]])
    r = ratio_bwd(got, s["ref"])
    print(f"dO of batch element 0 ({family}, {do_kind}, {kind}): err/bound {r}; the earlier rule passes: {old_rule_bwd(got, s['ref'])}")
    assert max(r.values()) > 1.0


def test_old_rule_on_the_mutants():
    """What _close(1.2e-2, 3e-2) says about each mutant on the random family (S = 700, 4 / 2, dense dO, bf16): recorded in the module
    docstring.  Asserted: it lets an lse off by 0.01 through, which the checker rejects (test_checker_rejects_mutants); the other
    verdicts are printed, not asserted."""
    s = setup("random", S_MUT, "bf16")
    passes = {}
    for name, (m, _, kw) in MUTANTS.items():
        if kw:
            continue
        passes[name] = old_rule_bwd(run(s, m), s["ref"])
        print(f"{name}: the earlier rule passes {passes[name]}")
    assert all(passes["j: lse off by 0.01"].values())


def test_old_rule_on_one_head_of_seven_missing():
    """(h) at the 7B layer's group size: one head of seven missing from the reduce."""
    s = setup("random", 200, "bf16", Hq=7, Hkv=1)
    got = run(s, dict(reduce_skip=3))
    old = old_rule_bwd(got, s["ref"])
    r = ratio_bwd(got, s["ref"])
    print(f"one head of seven not reduced: the earlier rule passes {old}; err/bound {r}")
    assert max(r.values()) > 1.0
