"""v3d_attention_backward against the f64 reference and per-element bound of tests/attention_bwd_check.py: EVERY element of dq, dk and dv,
at the smallest shapes that reach each mechanism of attention_bwd.hip (one-row tails in a new 128-row workgroup, both LDS stages
re-used, lengths that are no multiple of 64, group sizes 1 / 7, 65 key tiles, the non-causal batched SigLIP form with heads
zero-padded from 72 columns, strided operands and three separate gradient buffers).

The backward is isolated from the forward: it is fed o = T(o_ref) and lse = f32(lse_ref) of the f64 forward, so a forward defect can
neither hide nor mimic a backward one; test_end_to_end chains the device forward in front under the widened bound.  q, k, v come from
the three families of attention_check.py, crossed with a dense and a sparse upstream gradient; the sparse one implies exact zeros (cold
rows of dQ; dK and dV of keys past the last hot row, or of a batch element without hot rows), asserted with ==.  Every family's
self-check is asserted, and every output buffer starts as NaN.

Worst |err| / bound measured on the MI355X (every case of this file; the bound is derived, these only show its headroom):
                                                     dq       dk       dv
  causal 4/2, S = 1 .. 2100   random   dense        0.125    0.583    0.765
                              random   sparse       0.065    0.739    0.769
                              diagonal dense        0.162    0.247    0.651
                              diagonal sparse       0.121    0.914    0.971
                              needles  dense        0.834    0.884    0.679
                              needles  sparse       0.164    0.848    0.969
  groups 2/2, 7/1, 28/4       random   dense        0.129    0.857    0.662
  (S = 300)                   random   sparse       0.059    0.857    0.923
                              needles  dense        0.870    0.765    0.825
                              needles  sparse       0.101    0.887    0.994
  65 tiles (S = 4100, 2/1)    needles  dense        0.113    0.337    0.572
                              needles  sparse       0.040    0.454    0.787
                              diagonal dense        0.150    0.208    0.640
                              diagonal sparse       0.096    0.309    0.800
  SigLIP form (B = 1, 2, 3)   random   dense        0.094    0.339    0.461
                              random   sparse       0.073    0.667    0.725
                              needles  dense        0.097    0.120    0.347
                              needles  sparse       0.079    0.392    0.890
  strided, separate buffers   needles  dense        0.920    0.216    0.591
  end to end                  diagonal dense        0.012    0.016    0.141
                              needles  dense        0.675    0.184    0.492
The ratios near 1 belong to elements that are one or two products rounded twice (dv and dk of late keys under a sparse dO; f16
values below 2^-14, whose rounding error is the subnormal spacing): there the bound is the two roundings themselves, and a CPU
emulation of the kernels' arithmetic (tests/test_attention_bwd_check_cpu.py) gives the same ratios to three digits.  No case
exceeded the bound, no exact zero was broken, and the kernel needed no change.
"""
import math
import os
import sys

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (os.path.join(ROOT, "tests"), ROOT, os.path.join(ROOT, "video-3d-llm_amd")):
    if _p not in sys.path:
        sys.path.insert(0, _p)

from attention_bwd_check import (FAMILIES, check_family, check_sparse, describe, grad_inputs, qkv_inputs, reference_bwd,  # noqa: E402
                                 worst_bwd, zero_claims)

pytestmark = pytest.mark.gpu

DT = {"bf16": torch.bfloat16, "f16": torch.float16}
D = 128
NAN = float("nan")


def _ops():
    from v3d import ops
    return ops


def fused(q, k, v):
    B, S = q.shape[:2]
    return torch.cat([q.reshape(B * S, -1), k.reshape(B * S, -1), v.reshape(B * S, -1)], 1).contiguous()


def split(dqkv, B, S, Hq, Hkv):
    a, b = Hq * D, (Hq + Hkv) * D
    return (dqkv[:, :a].reshape(B, S, Hq, D), dqkv[:, a:b].reshape(B, S, Hkv, D), dqkv[:, b:].reshape(B, S, Hkv, D))


def backward(q, k, v, o, dO, lse, scale, causal):
    """ops.attention_backward on q, o, dO [B, S, Hq, D], k / v [B, S, Hkv, D], lse [B, Hq, S] f32 -> (dq, dk, dv) [B, S, H, D]; the
    gradient buffer starts as NaN."""
    ops = _ops()
    B, S, Hq, _ = q.shape
    Hkv = k.shape[2]
    dqkv = torch.full((B * S, (Hq + 2 * Hkv) * D), NAN, dtype=q.dtype, device="cuda")
    ops.attention_backward(fused(q, k, v), o.reshape(B * S, Hq * D).contiguous(), dO.reshape(B * S, Hq * D).contiguous(), lse.contiguous(),
                           dqkv, S, Hq, Hkv, scale, B=B, causal=causal)
    torch.cuda.synchronize()
    return split(dqkv, B, S, Hq, Hkv)


def make(family, do_kind, S, kind, Hq=4, Hkv=2, B=1, causal=True, scale=None, cols=D, hot_batches=None, end_to_end=False):
    """Inputs on the GPU, the f64 reference (with the families' self-checks) and the backward's o = T(o_ref), lse = f32(lse_ref)."""
    dt = DT[kind]
    q, k, v, pos = qkv_inputs(family, S, Hq, Hkv, D, dt, B=B)
    dO, hot = grad_inputs(do_kind, B, S, Hq, D, dt, hot_batches=hot_batches)
    if cols < D:                       # a narrower head, zero-padded to 128 columns
        for t in (q, k, v, dO):
            t[..., cols:] = 0
    q, k, v, dO = q.cuda(), k.cuda(), v.cuda(), dO.cuda()
    scale = scale if scale is not None else 1.0 / math.sqrt(D)
    ref = reference_bwd(q, k, v, dO, scale, causal=causal, keys=pos, end_to_end=end_to_end)
    check_family(family, ref, pos, causal)
    if do_kind == "sparse":
        check_sparse(hot, S)
    return dict(q=q, k=k, v=v, dO=dO, scale=scale, causal=causal, ref=ref, hot=hot, o=ref["o"].to(dt), lse=ref["lse"].float().contiguous())


def check(tag, got, s, hot_batches=None):
    w = worst_bwd(got, s["ref"])
    print(f"BWD {tag}: " + " ".join(f"{n}={r:.3g}" for n, (r, _) in w.items()))
    assert max(r for r, _ in w.values()) <= 1.0, f"{tag}: {describe(w)}"
    if s["hot"] is not None:
        assert zero_claims(got, s["hot"], s["causal"], hot_batches) == [], tag


def run(s):
    return backward(s["q"], s["k"], s["v"], s["o"], s["dO"], s["lse"], s["scale"], s["causal"])


@pytest.mark.parametrize("kind", ["bf16", "f16"])
@pytest.mark.parametrize("do_kind", ["dense", "sparse"])
@pytest.mark.parametrize("family", FAMILIES)
@pytest.mark.parametrize("S", [1, 40, 64, 65, 127, 128, 129, 193, 257, 700, 2100])
def test_causal(S, family, do_kind, kind):
    """193: the first length at which both LDS stages are re-used; 129 and 257: a one-row tail in a new 128-row workgroup; 700 and 2100:
    no multiple of 64."""
    s = make(family, do_kind, S, kind)
    check(f"causal {family} {do_kind} S={S} 4/2 {kind}", run(s), s)


@pytest.mark.parametrize("kind", ["bf16", "f16"])
@pytest.mark.parametrize("S", [193, 700])
def test_causal_keys_past_the_last_hot_row(S, kind):
    """dO's last hot row is S // 2: dK and dV of every later key are exactly 0, whatever the later query tiles hold."""
    s = make("random", "sparse_early", S, kind)
    assert s["hot"][-1] == max(128, S // 2)
    check(f"causal random sparse_early S={S} 4/2 {kind}", run(s), s)


@pytest.mark.parametrize("kind", ["bf16", "f16"])
@pytest.mark.parametrize("do_kind", ["dense", "sparse"])
@pytest.mark.parametrize("family", ["random", "needles"])
@pytest.mark.parametrize("Hq,Hkv", [(2, 2), (7, 1), (28, 4)])
def test_group_sizes(Hq, Hkv, family, do_kind, kind):
    """28 / 4 is the 7B layer's grouping: the in-order reduce over seven heads and head / group."""
    s = make(family, do_kind, 300, kind, Hq=Hq, Hkv=Hkv)
    check(f"groups {family} {do_kind} S=300 {Hq}/{Hkv} {kind}", run(s), s)


@pytest.mark.parametrize("do_kind", ["dense", "sparse"])
@pytest.mark.parametrize("family", ["needles", "diagonal"])
def test_many_tiles(family, do_kind):
    """65 key tiles: long dK / dV sums over every query tile; the needle keys collect mass from every later query."""
    s = make(family, do_kind, 4100, "bf16", Hq=2, Hkv=1)
    check(f"tiles {family} {do_kind} S=4100 2/1 bf16", run(s), s)


def _zero_columns(tag, got, cols):
    for n, g in zip(("dq", "dk", "dv"), got):
        assert bool((g[..., cols:] == 0).all()), f"{tag}: columns {cols} .. 127 of {n} are not exactly 0"


@pytest.mark.parametrize("kind", ["bf16", "f16"])
@pytest.mark.parametrize("do_kind", ["dense", "sparse"])
@pytest.mark.parametrize("family", ["random", "needles"])
@pytest.mark.parametrize("B", [1, 3])
def test_siglip_form(B, family, do_kind, kind):
    """The SigLIP tower's call: non-causal, a batch of frames of 729 patches, heads of 72 columns zero-padded to 128, scale 72^-0.5."""
    s = make(family, do_kind, 729, kind, Hq=4, Hkv=4, B=B, causal=False, scale=72 ** -0.5, cols=72)
    got = run(s)
    tag = f"siglip {family} {do_kind} B={B} S=729 4/4 {kind}"
    check(tag, got, s)
    _zero_columns(tag, got, 72)


@pytest.mark.parametrize("kind", ["bf16", "f16"])
@pytest.mark.parametrize("family", ["random", "needles"])
def test_siglip_form_cold_batch_element(family, kind):
    """B = 2, S = 65 (a one-row second tile), hot rows in batch element 1 only: every gradient row of batch element 0 is exactly 0."""
    s = make(family, "sparse", 65, kind, Hq=4, Hkv=4, B=2, causal=False, scale=72 ** -0.5, cols=72, hot_batches=[1])
    got = run(s)
    tag = f"siglip {family} sparse(b=1) B=2 S=65 4/4 {kind}"
    check(tag, got, s, hot_batches=[1])
    _zero_columns(tag, got, 72)
    s = make(family, "dense", 65, kind, Hq=4, Hkv=4, B=2, causal=False, scale=72 ** -0.5, cols=72)
    check(f"siglip {family} dense B=2 S=65 4/4 {kind}", run(s), s)


@pytest.mark.parametrize("kind", ["bf16", "f16"])
@pytest.mark.parametrize("causal", [True, False], ids=["causal", "full"])
def test_strided_operands_and_separate_gradients(causal, kind):
    """Through the C entry: q | k | v as column windows of one wide buffer (ld > (Hq + 2 Hkv) 128, rows between the batch elements), o and
    dO with strides of their own, dq, dk and dv into three SEPARATE buffers with different row and batch strides (the Python wrapper only
    ever passes one fused buffer).  Nothing outside each gradient's own rows and columns is written (the buffers start as NaN)."""
    ops = _ops()
    B, S, Hq, Hkv = 2, 129, 4, 2
    s = make("needles", "dense", S, kind, Hq=Hq, Hkv=Hkv, B=B, causal=causal)
    dt = DT[kind]
    wq, wk = Hq * D, Hkv * D

    def strided(x, ld, rows, col0, fill):
        """x [B, S, H, D] -> buffer [B, rows, ld] holding it at columns col0 .., rows 0 .. S of each batch element."""
        buf = torch.full((B, rows, ld), fill, dtype=x.dtype, device="cuda")
        buf[:, :S, col0:col0 + x.shape[2] * D] = x.reshape(B, S, -1)
        return buf

    ld = wq + 2 * wk + 264                                   # q at column 8, k at 8 + wq + 128, v at 8 + wq + wk + 256
    rows = S + 3
    cq, ck, cv = 8, 8 + wq + 128, 8 + wq + wk + 256
    wide = torch.full((B, rows, ld), 3.0, dtype=dt, device="cuda")
    wide[:, :S, cq:cq + wq] = s["q"].reshape(B, S, -1)
    wide[:, :S, ck:ck + wk] = s["k"].reshape(B, S, -1)
    wide[:, :S, cv:cv + wk] = s["v"].reshape(B, S, -1)
    o = strided(s["o"], wq + 64, S + 1, 32, 3.0)
    do = strided(s["dO"], wq + 128, S + 2, 64, 3.0)
    grads = {"dq": (wq + 72, S + 5, 16, wq), "dk": (wk + 136, S + 2, 40, wk), "dv": (wk + 8, S, 8, wk)}      # ld, rows, first column, width
    bufs = {n: torch.full((B, r, l), NAN, dtype=dt, device="cuda") for n, (l, r, _, _) in grads.items()}
    win = {n: bufs[n][:, :, c0:] for n, (_, _, c0, _) in grads.items()}
    nbytes = ops.lib().v3d_attention_backward_workspace_bytes(B, S, Hq)
    ws = torch.empty(nbytes // 4, dtype=torch.float32, device="cuda")
    p = ops._p
    ops.check(ops.lib().v3d_attention_backward(
        p(wide[:, :, cq:]), p(wide[:, :, ck:]), p(wide[:, :, cv:]), p(o[:, :, 32:]), p(do[:, :, 64:]), p(s["lse"]),
        p(win["dq"]), p(win["dk"]), p(win["dv"]), ops._code(wide), B, S, Hq, Hkv,
        ld, ld, ld, o.stride(1), do.stride(1), bufs["dq"].stride(1), bufs["dk"].stride(1), bufs["dv"].stride(1),
        wide.stride(0), wide.stride(0), wide.stride(0), o.stride(0), do.stride(0), bufs["dq"].stride(0), bufs["dk"].stride(0), bufs["dv"].stride(0),
        1 if causal else 0, float(s["scale"]), p(ws), nbytes, ops._stream()), "v3d_attention_backward")
    torch.cuda.synchronize()
    got = {}
    for n, (_, _, c0, w) in grads.items():
        inside = torch.zeros_like(bufs[n], dtype=torch.bool)
        inside[:, :S, c0:c0 + w] = True
        assert bool(torch.isnan(bufs[n][~inside]).all()), f"{n}: written outside its own rows and columns"
        got[n] = bufs[n][:, :S, c0:c0 + w].reshape(B, S, -1, D)
    check(f"strided needles dense B=2 S=129 4/2 {kind} causal={causal}", got, s)
    plain = run(s)
    for n, g in zip(("dq", "dk", "dv"), plain):
        assert torch.equal(g, got[n]), f"{n}: the strided call and the fused one differ"


@pytest.mark.parametrize("kind", ["bf16", "f16"])
@pytest.mark.parametrize("family", ["diagonal", "needles"])
@pytest.mark.parametrize("S", [257, 2100])
def test_end_to_end(S, family, kind):
    """ops.attention_train, then ops.attention_backward on the device's own o and lse, under the bound widened by the forward's."""
    ops = _ops()
    Hq, Hkv = 4, 2
    s = make(family, "dense", S, kind, Hq=Hq, Hkv=Hkv, end_to_end=True)
    o = torch.full((S, Hq * D), NAN, dtype=DT[kind], device="cuda")
    lse = ops.attention_train(fused(s["q"], s["k"], s["v"]), o, S, Hq, Hkv, s["scale"])
    torch.cuda.synchronize()
    assert bool(torch.isfinite(o.float()).all()) and bool(torch.isfinite(lse).all())
    got = backward(s["q"], s["k"], s["v"], o.reshape(1, S, Hq, D), s["dO"], lse, s["scale"], True)
    check(f"end-to-end {family} dense S={S} 4/2 {kind}", got, s)


@pytest.mark.parametrize("shape", [dict(S=700, Hq=7, Hkv=1), dict(S=729, Hq=4, Hkv=4, B=3, causal=False, scale=72 ** -0.5, cols=72)],
                         ids=["group7", "siglip"])
def test_two_calls_give_the_same_bits(shape):
    """No atomics: the kv-group reduce runs in a fixed order."""
    s = make("random", "dense", kind="bf16", **shape)
    a, b = run(s), run(s)
    for n, x, y in zip(("dq", "dk", "dv"), a, b):
        assert torch.equal(x, y), n
    check(f"determinism random dense {shape['S']} {shape['Hq']}/{shape['Hkv']} bf16", a, s)
