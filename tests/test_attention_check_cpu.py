"""The attention checker (tests/attention_check.py) has power: a CPU emulation of the kernels' arithmetic passes it, and emulations with
one wrong key, tile, split, needle or kv head - or an lse off by 0.01 - fail it, where the suite's earlier rule let the long-row ones
through.  No GPU: these run under -m "not gpu".

The emulation follows attn_prefill_kernel: Q times scale log2(e) in f32, rounded to 16 bit; scores in f32; 64-key tiles; the running
maximum fixed by tile 0 and raised only past 2^8; probabilities in f32 for the row sum and rounded to 16 bit for P.V; O and l in f32;
the output o / l rounded once; lse = m + log2(l)."""
import math

import pytest
import torch

from attention_check import (diagonal_inputs, lse_ratio, needle_inputs, needle_positions, old_rule_ratio, random_inputs, ratio,
                             reference, rows_of)

DT = {"bf16": torch.bfloat16, "f16": torch.float16}
HQ, HKV, D = 8, 2, 128
TILE = 64


def emulate(q, k, v, scale, rows, q_pos0=0, vis_fn=None, kv_of=None):
    """Kernel arithmetic on the CPU for the given rows -> (o [R, Hq, D] 16 bit, lse [Hq, R] f32).  vis_fn(vis, rows) may edit the
    [R, Sk] visibility (the mutants); kv_of(h) picks the kv head (default h // group)."""
    dt = q.dtype
    Sq, Hq, Dq = q.shape
    Sk, Hkv = k.shape[0], k.shape[1]
    G = Hq // Hkv
    rows = torch.as_tensor(rows, dtype=torch.long)
    c = torch.tensor(scale, dtype=torch.float32) * torch.tensor(1.44269504088896340736, dtype=torch.float32)
    qs = (q[rows].float() * c).to(dt).float()
    vis = torch.arange(Sk)[None, :] <= (rows[:, None] + q_pos0)
    if vis_fn is not None:
        vis = vis_fn(vis.clone(), rows)
    R = rows.numel()
    out = torch.empty(R, Hq, Dq, dtype=dt)
    lse = torch.empty(Hq, R, dtype=torch.float32)
    for h in range(Hq):
        hk = kv_of(h) if kv_of else h // G
        s = (qs[:, h] @ k[:, hk].float().T).masked_fill(~vis, float("-inf"))
        vf = v[:, hk].float()
        m = torch.zeros(R)
        l = torch.zeros(R)
        o = torch.zeros(R, Dq)
        for t in range(0, Sk, TILE):
            st = s[:, t:t + TILE] - m[:, None]
            mx = st.max(1).values
            if t == 0:
                d = torch.where(torch.isinf(mx), torch.zeros_like(mx), mx)
            else:
                d = torch.where(mx > 8.0, mx, torch.zeros_like(mx))
            st = st - d[:, None]
            alpha = torch.exp2(-d) if t else torch.ones(R)
            m = m + d
            e = torch.exp2(st)
            l = l * alpha + e.sum(1)
            o = o * alpha[:, None] + e.to(dt).float() @ vf[t:t + TILE]
        inv = torch.where(l > 0, 1.0 / l, torch.zeros_like(l))
        out[:, h] = (o * inv[:, None]).to(dt)
        lse[h] = m + torch.log2(l)
    return out, lse


def family(name, S, dt, seed=0):
    scale = 1.0 / math.sqrt(D)
    if name == "random":
        q, k, v = random_inputs(S, S, HQ, HKV, D, dt, seed=seed)
        pos = None
    elif name == "diagonal":
        q, k, v = diagonal_inputs(S, S, HQ, HKV, D, dt, seed=seed)
        pos = None
    else:
        pos = needle_positions(S)
        q, k, v = needle_inputs(S, S, HQ, HKV, D, dt, pos, seed=seed)
    return q, k, v, scale, pos


def rows_for(S):
    return rows_of(S, range(0, 4), range(62, 67), range(126, 131), range(254, 259), range(S // 2 - 2, S // 2 + 2), range(S - 160, S))


_cache = {}


def setup(name, S, kind):
    key = (name, S, kind)
    if key not in _cache:
        dt = DT[kind]
        q, k, v, scale, pos = family(name, S, dt)
        rows = rows_for(S)
        ref = reference(q, k, v, scale, rows=rows, keys=pos, near=3 if name == "diagonal" else 0)
        _cache[key] = (q, k, v, scale, pos, rows, ref)
    return _cache[key]


def check_family(name, ref, pos):
    """The inputs do their job (the same self-checks the GPU tests make)."""
    if name == "diagonal":
        assert ref["near"].min().item() >= 0.5, "diagonal-peaked rows must keep half their mass on keys i-3 .. i"
    if name == "needles":
        rows = ref["rows"]
        seen = torch.as_tensor(pos)[None, :] <= rows[:, None]
        share = ref["mass_keys"].min(1).values                       # [R, n] (weakest head)
        assert share[seen].min().item() >= 0.02, "every visible needle must hold at least 2 % of the mass"
        assert share[~seen].max().item() == 0.0


@pytest.mark.parametrize("kind", ["bf16", "f16"])
@pytest.mark.parametrize("name", ["random", "diagonal", "needles"])
@pytest.mark.parametrize("S", [200, 2100])
def test_checker_accepts_the_kernel_arithmetic(kind, name, S):
    q, k, v, scale, pos, rows, ref = setup(name, S, kind)
    check_family(name, ref, pos)
    o, lse = emulate(q, k, v, scale, rows)
    r, rl = ratio(o, ref), lse_ratio(lse, ref)
    print(f"{name} S={S} {kind}: output err/bound {r:.3g}, lse {rl:.3g}")
    assert r <= 1.0 and rl <= 1.0


S_MUT = 2100     # partial last tile (2100 = 32 x 64 + 52)


def _drop(keys):
    def f(vis, rows):
        vis[:, keys] = False
        return vis
    return f


def _diag(vis, rows):
    vis[torch.arange(rows.numel()), rows] = False
    return vis


def _leak(vis, rows):
    nxt = rows + 1
    ok = nxt < vis.shape[1]
    vis[torch.arange(rows.numel())[ok], nxt[ok]] = True
    return vis


MUTANTS = {     # name -> (input family, visibility edit, kv map)
    "diagonal key dropped": ("diagonal", _diag, None),
    "key i+1 leaked": ("diagonal", _leak, None),
    "one needle dropped": ("needles", _drop([1024]), None),
    "one 64-key tile dropped": ("needles", _drop(list(range(1536, 1600))), None),
    "one split dropped": ("needles", _drop(list(range(512, 768))), None),
    "last key of the partial tile dropped": ("diagonal", _drop([S_MUT - 1]), None),
    "kv head h % Hkv": ("random", None, lambda h: h % HKV),
}


@pytest.mark.parametrize("kind", ["bf16", "f16"])
@pytest.mark.parametrize("mutant", list(MUTANTS))
def test_checker_rejects_mutants(kind, mutant):
    name, vis_fn, kv_of = MUTANTS[mutant]
    q, k, v, scale, pos, rows, ref = setup(name, S_MUT, kind)
    if name == "needles":
        assert 1024 in pos and 1536 in pos and 512 in pos
    o, _ = emulate(q, k, v, scale, rows, vis_fn=vis_fn, kv_of=kv_of)
    r = ratio(o, ref)
    print(f"{mutant} ({name}, S={S_MUT}, {kind}): err/bound {r:.3g}")
    assert r > 1.0


@pytest.mark.parametrize("kind,name", [("bf16", "random"), ("f16", "random"), ("f16", "diagonal"), ("f16", "needles")])
def test_checker_rejects_lse_off_by_a_hundredth(kind, name):
    """(Not bf16 on peaked rows: there rounding Q to bf16 alone may move lse by up to u/2 peak log2(e) ~ 0.04.)"""
    q, k, v, scale, pos, rows, ref = setup(name, S_MUT, kind)
    _, lse = emulate(q, k, v, scale, rows)
    r = lse_ratio(lse + 0.01, ref)
    print(f"lse + 0.01 ({name}, {kind}): err/bound {r:.3g}")
    assert r > 1.0


@pytest.mark.parametrize("kind", ["bf16", "f16"])
def test_old_rule_accepts_long_row_mutants(kind):
    """On long rows (S = 6794, the last 160 rows) the suite's earlier rule, close(ulps=3, floor=0.3) on random bf16 inputs, accepts a
    dropped diagonal key and a leaked future key (f16's rule is 8x tighter and sees them at this length); the new checker rejects both,
    in both dtypes, on diagonal-peaked rows."""
    S = 6794
    dt = DT[kind]
    rows = rows_of(S, range(S - 160, S))
    scale = 1.0 / math.sqrt(D)
    if kind == "bf16":
        q, k, v = random_inputs(S, S, HQ, HKV, D, dt, seed=3)
        ref = reference(q, k, v, scale, rows=rows)
        for fn in (_diag, _leak):
            o, _ = emulate(q, k, v, scale, rows, vis_fn=fn)
            r_old = old_rule_ratio(o, ref, dt)
            print(f"old rule, {fn.__name__} (random, S={S}, {kind}): err/bound {r_old:.3g}")
            assert r_old <= 1.0
    qd, kd, vd = diagonal_inputs(S, S, HQ, HKV, D, dt, seed=3)
    refd = reference(qd, kd, vd, scale, rows=rows, near=3)
    assert refd["near"].min().item() >= 0.5
    for fn in (_diag, _leak):
        o, _ = emulate(qd, kd, vd, scale, rows, vis_fn=fn)
        r = ratio(o, refd)
        print(f"checker, {fn.__name__} (diagonal, S={S}, {kind}): err/bound {r:.3g}")
        assert r > 1.0
    o, _ = emulate(qd, kd, vd, scale, rows)
    assert ratio(o, refd) <= 1.0
