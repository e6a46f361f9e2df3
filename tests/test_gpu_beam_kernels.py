"""The three beam-search kernels on their own (csrc/beam.hip): v3d_beam_topk under tests/beam_check.py's check_topk against f64 scores,
v3d_beam_step bit for bit against its host twin on the scripted streams of tests/test_beam_check_cpu.py, v3d_beam_kv_gather bit for bit
against index_select with everything it must not touch poisoned.

Top-K shapes: V = 1000 behind a leading dimension of 1024, V = 4099 (odd: rows start on 2-byte boundaries; two chunks), V = 70 000 with 16
rows (the only size range where a workgroup walks several 4096-key tiles and the merge several passes: chunks are capped at 256 / M per row),
and the model's 152 064 once at five beams.  bound = 4 e_ref + 2^-22 |score| with e_ref measured here (torch-CPU f32 log_softmax against f64
on the same logits); the test prints e_ref and the worst error it saw.
MEASURED on one MI355X (this file, -s): V = 1000 / 4099: e_ref 2.4e-9 .. 9.9e-7 over the cases, the kernel's worst |score - f64| 5.4e-7 .. 9.9e-7 (at
most 1.3 x the largest e_ref; the rule allows 4 x + 2^-22 |score|); V = 152 064, five beams: e_ref 2.9e-6, worst 4.7e-7."""
import pytest
import torch

import beam_check as bc
from v3d import ops
from v3d._native import V3DError

pytestmark = pytest.mark.gpu


def _topk(x, V, running, K, done=None):
    M = x.shape[0]
    cs = torch.full((K,), float("nan"), dtype=torch.float32, device="cuda")
    cf = torch.full((K,), -7, dtype=torch.int32, device="cuda")
    ws = torch.empty(int(ops.lib().v3d_beam_topk_workspace_bytes(M, V, K)) // 4 + 4, dtype=torch.int32, device="cuda")
    ops.beam_topk(x, running.cuda(), K, cs, cf, ws, done=done, V=V)
    torch.cuda.synchronize()
    return cs.cpu(), cf.cpu()


def _check(x, V, running, K, label):
    """check_topk of the kernel's answer on logits x [M, ldx] (16-bit, host) -> (e_ref, worst error)"""
    M = x.shape[0]
    cs, cf = _topk(x.cuda(), V, running, K)
    xv = x[:, :V]
    lp64 = torch.log_softmax(xv.double(), -1)
    alive = running[:M] > bc.NEG
    s64 = torch.where(alive[:, None], running[:M, None].double() + lp64, torch.tensor(float("-inf"), dtype=torch.float64)).reshape(-1)
    e_ref = bc.e_ref_log_softmax(xv[alive])
    own = s64[cf.long().clamp(0, s64.numel() - 1)]
    worst = bc.check_topk(cs, cf, s64, bc.kernel_bound(e_ref, torch.where(torch.isfinite(own), own, torch.zeros_like(own))), label=label)
    return e_ref, worst, cs, cf


def _logits(M, V, ldx, dtype, seed):
    g = torch.Generator().manual_seed(seed)
    x = (torch.randn(M, ldx, generator=g) * 1.5).to(dtype)
    x[:, V:] = 60.0                                       # behind the vocab: must never be read as a candidate
    return x


def _running(B, seed):
    g = torch.Generator().manual_seed(seed)
    r = -(torch.rand(B, generator=g) * 6.0).sort().values
    r[0] = -0.75
    return r.to(torch.float32)


def _boundaries(M, V):
    """columns on both sides of every cut the kernel makes in a row: chunk boundaries and, inside a chunk, 4096-key tile boundaries"""
    chunk = ops.beam_topk_chunk(M, V)
    assert 0 < chunk <= V + 8
    cols = set()
    for lo in range(0, V, chunk):
        for edge in [lo] + list(range(lo + 4096, min(lo + chunk, V), 4096)):
            cols |= {edge - 1, edge}
    return sorted(c for c in cols if 0 <= c < V), chunk


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16])
@pytest.mark.parametrize("V,ldx", [(1000, 1024), (4099, 4099)])
def test_topk_against_f64(dtype, V, ldx):
    figures = []
    for B in (1, 2, 4, 5, 16):
        for K in (2 * B, 3 * B):
            for M in sorted({1, B}):
                x = _logits(M, V, ldx, dtype, 7 * B + K + M)
                run = _running(B, B + K) if M > 1 else torch.tensor([0.0] + [bc.NEG] * (B - 1))
                figures.append(_check(x, V, run, K, f"V={V} B={B} M={M} K={K}")[:2])
    print(f"\n[beam_topk {dtype} V={V}] e_ref {min(f[0] for f in figures):.2e} .. {max(f[0] for f in figures):.2e}, worst error {max(f[1] for f in figures):.2e}")


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16])
@pytest.mark.parametrize("V,B", [(4099, 4), (4099, 16), (70000, 16)])
def test_topk_planted_winners(dtype, V, B):
    """Winners at token 0 and V - 1, on both sides of every chunk and tile boundary, all in one beam, all in the last chunk."""
    K = 3 * B
    cols, chunk = _boundaries(B, V)
    if V == 70000:
        assert chunk > 4096 and B * ((V + chunk - 1) // chunk) * K > 4096, "this case is here for the multi-tile and multi-pass paths"
    run = _running(B, 5)
    spots = sorted(set([0, V - 1] + cols))
    plans = {
        "edges": [(i % B, c) for i, c in enumerate(spots)],
        "one beam": [(B - 1, c) for c in spots[:K]] + [(B - 1, 17 + 3 * i) for i in range(K)],
        "last chunk": [(i % B, V - 1 - i) for i in range(min(2 * K, V - (V - 1) // chunk * chunk))],
    }
    for name, plan in plans.items():
        x = _logits(B, V, V, dtype, 23)
        for i, (b, c) in enumerate(plan):
            x[b, c] = 6.0 + 0.125 * (i % 29)              # above the N(0, 1.5) rest (exact in both 16-bit types)
        r = run
        if name == "one beam":                            # ... and that beam far ahead: every winner is one of its own
            r = torch.full((B,), -9.0)
            r[B - 1] = 0.0
        e_ref, worst, cs, cf = _check(x, V, r, K, f"{name} V={V} B={B}")
        planted = {b * V + c for b, c in plan}
        assert planted & set(cf.tolist()), (name, sorted(planted), cf.tolist())      # (which of them win is check_topk's business: rule 4)
        if name == "one beam":
            assert all(int(f) // V == B - 1 for f in cf), cf.tolist()
    x = _logits(B, V, V, dtype, 29)
    for b in range(B):
        for c in spots:
            x[b, c] = 9.0
    _check(x, V, torch.zeros(B), K, f"every edge in every beam V={V} B={B}")


def test_topk_at_the_models_vocab():
    V, B, K = 152064, 5, 10
    x = _logits(B, V, V + 64, torch.bfloat16, 31)
    cols, chunk = _boundaries(B, V)
    for i, c in enumerate(cols[::7][: 2 * K]):
        x[i % B, c] = 7.0 + 0.0625 * i
    e_ref, worst, cs, cf = _check(x, V, _running(B, 6), K, "V=152064 B=5")
    print(f"\n[beam_topk bf16 V={V} B={B}] chunk {chunk}, e_ref {e_ref:.2e}, worst error {worst:.2e}")


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16])
def test_topk_never_selects_a_dead_beam_and_orders_exact_ties(dtype):
    V, B, K = 4099, 5, 15
    x = _logits(B, V, V, dtype, 37)
    run = torch.tensor([-1.0, bc.NEG, -2.5, bc.NEG - 64.0, -0.5])
    x[1, 5] = x[3, 4000] = 50.0                            # tempting, in dead rows
    ties = [3, 2055, 2056, 4098]                           # one beam, equal 16-bit logits, across the chunk boundary
    for c in ties:
        x[4, c] = 11.0
    e_ref, worst, cs, cf = _check(x, V, run, K, "dead beams + ties")
    assert all(int(f) // V in (0, 2, 4) for f in cf)
    assert cf[:4].tolist() == [4 * V + c for c in ties], cf.tolist()
    assert len(set(cs[:4].view(torch.int32).tolist())) == 1, "equal logits of one beam must give one score, bit for bit"
    # the whole answer equals the specification's stable sort over the kernel's own f32 scores wherever those are reproducible: flats ascend in every tie group
    for k in range(1, K):
        assert cs[k] < cs[k - 1] or cf[k] > cf[k - 1]


def test_topk_done_and_bad_arguments():
    V, B, K = 1000, 4, 8
    x = _logits(B, V, 1024, torch.bfloat16, 41).cuda()
    done = torch.ones(1, dtype=torch.int32, device="cuda")
    cs, cf = _topk(x, V, _running(B, 1), K, done=done)
    assert bool(torch.isnan(cs).all()) and cf.tolist() == [-7] * K, "with done set nothing may be written"
    run = _running(B, 1).cuda()
    out = (torch.empty(80, dtype=torch.float32, device="cuda"), torch.empty(80, dtype=torch.int32, device="cuda"))
    ws = torch.empty(1 << 20, dtype=torch.int32, device="cuda")
    with pytest.raises(V3DError):
        ops.beam_topk(x, run, 65, *out, ws, V=V)                                   # K > 64
    with pytest.raises(V3DError):
        ops.beam_topk(x[:, :6], run, 8, *out, ws, V=6)                             # K > V
    with pytest.raises(V3DError):
        ops.beam_topk(x, run, 8, *out, ws[:16], V=V)                               # workspace too small
    with pytest.raises(V3DError):
        ops.beam_topk(x.float(), run, 8, *out, ws, V=V)                            # 16-bit logits only


# ------------------------------------------------------------------ v3d_beam_step


@pytest.mark.parametrize("B", [1, 2, 4, 5, 16])
@pytest.mark.parametrize("n_eos", [1, 2])
def test_step_kernel_equals_host_twin_bit_for_bit(B, n_eos):
    V, L = 67, 12                                          # (V >= K = 48: the state object also sizes the top-K workspace)
    eos = (3,) if n_eos == 1 else (3, 11)
    K = bc.beams_to_keep(B, n_eos)
    for lp, seed in ((1.0, 0), (0.6, 1), (0.6, 2), (1.0, 3)):
        stream = bc.scripted_stream(B, K, V, L, eos, 100 * B + seed, bc.PLANTS[seed % 2])
        bs = ops.BeamState(B, L, K, V, eos, lp)
        words = bs.init.clone()
        div = bs.div.cpu()
        ts, tf_ = torch.zeros((L, K)), torch.zeros((L, K), dtype=torch.int32)
        ref = bc.BeamRef(B, V, L, eos, lp)
        for t, (sc, flat) in enumerate(stream):
            bs.cand_score.copy_(sc)
            bs.cand_flat.copy_(flat)
            was_done = int(words[0])
            ops.beam_step(bs, t)
            nxt, par = ops.beam_step_host(words, sc, flat, B, V, L, t, eos, div, ts, tf_)
            ref.step(sc, flat)
            assert torch.equal(bs.state.cpu(), words), (B, K, seed, t)              # every word: flags, scores, the plan, all four sequence buffers
            if not was_done:
                assert torch.equal(bs.next_tokens.cpu(), nxt) and torch.equal(bs.parents.cpu(), par)
                assert bc.views_snapshot(bs.views()) == ref.snapshot()
        assert int(words[0]) == 1
        assert torch.equal(bs.trace_score.cpu().view(torch.int32), ts.view(torch.int32)) and torch.equal(bs.trace_flat.cpu(), tf_)
    with pytest.raises(V3DError):
        ops.beam_step(bs, L)                                                        # step == max_new_tokens
    with pytest.raises(V3DError):
        ops.BeamState(17, 4, 34, 100)


# ------------------------------------------------------------------ v3d_beam_kv_gather

POISON = 0x7FC1                                            # a NaN pattern in both 16-bit types


def _kv(n_layers, rows, width=2 * 4 * 128, seed=0):
    g = torch.Generator(device="cuda").manual_seed(seed)
    return [torch.randint(-32768, 32767, (32, rows, width), dtype=torch.int16, device="cuda", generator=g).view(torch.bfloat16) for _ in range(n_layers)]


@pytest.mark.parametrize("n_layers,S,n,parents", [(2, 70, 1, [0, 0, 2, 1]), (2, 70, 5, [0, 1, 2, 3]), (2, 128, 5, [2, 2, 2, 2]), (2, 128, 1, [0]),
                                                 (28, 70, 5, [15, 0, 7, 7, 3, 12, 1, 14, 2, 9, 9, 4, 0, 11, 6, 5])])
def test_kv_gather_equals_index_select(n_layers, S, n, parents):
    B = len(parents)
    kv = _kv(n_layers, S + n + 3, seed=S + n)
    ptrs = ops.beam_kv_layers(kv)
    par = torch.tensor(parents, dtype=torch.int32, device="cuda")
    for src, dst in ((0, 16), (16, 0)):
        for k in kv:                                       # poison what must stay: the destination set's rows below S, from S + n on, slices >= B
            k.view(torch.int16)[dst: dst + 16, :S] = POISON
            k.view(torch.int16)[dst: dst + 16, S + n:] = POISON
            k.view(torch.int16)[dst + B: dst + 16] = POISON
        want = [k.clone() for k in kv]
        for w in want:
            w[dst: dst + B, S: S + n] = torch.index_select(w[src: src + 16], 0, par.long())[:, S: S + n]
        done = torch.ones(1, dtype=torch.int32, device="cuda")
        before = [k.clone() for k in kv]
        ops.beam_kv_gather(kv, ptrs, S, n, src, dst, par, done=done)
        assert all(torch.equal(a.view(torch.int16), b.view(torch.int16)) for a, b in zip(kv, before)), "with done set nothing may be written"
        done.zero_()
        ops.beam_kv_gather(kv, ptrs, S, n, src, dst, par, done=done)
        for i, (a, b) in enumerate(zip(kv, want)):
            assert torch.equal(a.view(torch.int16), b.view(torch.int16)), (i, src, dst)
    with pytest.raises(V3DError):
        ops.beam_kv_gather(kv, ptrs, S, n, 0, 8, torch.zeros(16, dtype=torch.int32, device="cuda"))      # overlapping slice sets
    with pytest.raises(V3DError):
        ops.beam_kv_gather(kv, ptrs, S, n + 4, 0, 16, par)                                              # rows past the slice
    bad = torch.tensor([B + 40] * B, dtype=torch.int32, device="cuda")                                   # a parent outside the set is never followed
    before = [k.clone() for k in kv]
    ops.beam_kv_gather(kv, ptrs, S, n, 0, 16, bad)
    assert all(torch.equal(a.view(torch.int16), b.view(torch.int16)) for a, b in zip(kv, before))
