"""Attention forward kernels against the f64 reference and per-element bound of tests/attention_check.py, on inputs that put the
softmax mass on the keys a tiled kernel can lose: diagonal-peaked rows (the query's own key and its nearest past keys) and needles
(key 0, 64-key tile edges, split and prefix-chunk edges, P - 1 and P of a shared prefix, Sk - 1; a leaked future needle moves the
output far past the bound).
Every case asserts that its input does that job; every output buffer starts as NaN, and the prefill ones are checked whole for
elements never written (the f64 comparison reads a subset of the rows past 1100).

Switches read once per process (V3D_ATTN_XCD, V3D_DEC_KEYS_PER_SPLIT, V3D_DEC_ATTN) run in a fresh child process: this file run as
a script with --child, which prints its worst error / bound ratios as JSON."""
import json
import math
import os
import subprocess
import sys

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (os.path.join(ROOT, "tests"), ROOT, os.path.join(ROOT, "video-3d-llm_amd")):
    if _p not in sys.path:
        sys.path.insert(0, _p)

from attention_check import (diagonal_inputs, lse_ratio, needle_inputs, needle_positions, random_inputs, ratio,  # noqa: E402
                             reference, rows_of)

DT = {"bf16": torch.bfloat16, "f16": torch.float16}
HQ, HKV, D = 28, 4, 128
NAN = float("nan")
NEAR_SHARE = 0.5        # diagonal-peaked rows: p on keys i-3 .. i
NEEDLE_SHARE = 0.02     # needles: every visible needle


def _ops():
    from v3d import ops
    return ops


def make(family, Sq, Sk, dt, q_pos0=0, Hq=HQ, Hkv=HKV, Dh=D, positions=None, seed=0):
    """-> q [Sq, Hq, Dh], k / v [Sk, Hkv, Dh] on the GPU, needle positions (or None)."""
    if family == "diagonal":
        q, k, v = diagonal_inputs(Sq, Sk, Hq, Hkv, Dh, dt, q_pos0=q_pos0, seed=seed)
        positions = None
    elif family == "needles":
        positions = positions or needle_positions(Sk)
        q, k, v = needle_inputs(Sq, Sk, Hq, Hkv, Dh, dt, positions, seed=seed)
    else:
        q, k, v = random_inputs(Sq, Sk, Hq, Hkv, Dh, dt, seed=seed)
        positions = None
    return q.cuda(), k.cuda(), v.cuda(), positions


def ref_checked(family, q, k, v, scale, positions, causal=True, q_pos0=0, rows=None, d_out=None):
    """f64 reference on the device + the input family's self-check."""
    ref = reference(q, k, v, scale, causal=causal, q_pos0=q_pos0, rows=rows, d_out=d_out, keys=positions,
                    near=3 if family == "diagonal" else 0)
    if family == "diagonal":
        assert ref["near"].min().item() >= NEAR_SHARE, f"diagonal-peaked input too flat: {ref['near'].min().item():.3f}"
    elif family == "needles":
        pos = torch.as_tensor(positions, device=q.device)
        seen = (pos[None, :] <= ref["rows"][:, None] + q_pos0) if causal else torch.ones(ref["rows"].numel(), pos.numel(), dtype=torch.bool,
                                                                                       device=q.device)
        share = ref["mass_keys"].amin(1)
        assert share[seen].min().item() >= NEEDLE_SHARE, f"a needle holds only {share[seen].min().item():.4f} of its row"
        if bool((~seen).any()):     # input setup only: the needles counted as future are past the row's position (the reference
            assert ref["mass_keys"].amax(1)[~seen].max().item() == 0.0      # masks them); a kernel that leaks one fails the output bound
    return ref


def rows_for(Sq):
    if Sq <= 1100:
        return None
    return rows_of(Sq, range(0, 130), range(250, 260), range(Sq // 2 - 64, Sq // 2 + 64), range(Sq - 300, Sq))


def prefill(q, k, v, causal=True, q_pos0=0, scale=None, lse=False):
    """One sequence: q [Sq, Hq, Dh], k / v [Sk, Hkv, Dh] -> out [Sq, Hq, Dh] (NaN-filled before the launch) [, lse [Hq, Sq]]."""
    ops = _ops()
    Sq, Hq, Dh = q.shape
    Sk, Hkv = k.shape[0], k.shape[1]
    scale = scale if scale is not None else 1.0 / math.sqrt(Dh)
    out = torch.full((Sq, Hq, Dh), NAN, dtype=q.dtype, device="cuda")
    if lse:
        assert causal and q_pos0 == 0 and Sq == Sk
        qkv = torch.cat([q.reshape(Sq, -1), k.reshape(Sk, -1), v.reshape(Sk, -1)], 1).contiguous()
        o2 = out.view(Sq, Hq * Dh)
        # ops.attention_train's call with a NaN-filled lse (the wrapper allocates it with torch.empty)
        l = torch.full((1, Hq, Sq), NAN, dtype=torch.float32, device="cuda")
        w = qkv.stride(0)
        ops.check(ops.lib().v3d_attention_train(ops._p(qkv), ops._p(qkv[:, Hq * Dh:]), ops._p(qkv[:, (Hq + Hkv) * Dh:]), ops._p(o2), ops._p(l),
                                                ops._code(qkv), 1, Sq, Sq, Hq, Hkv, w, w, w, o2.stride(0), Sq * w, Sq * w, Sq * o2.stride(0),
                                                Dh, Dh, Dh, 1, 0, float(scale), ops._stream()), "v3d_attention_train")
        torch.cuda.synchronize()
        assert_written(out, "attention_train output")
        assert_written(l, "attention_train lse")
        return out, l[0]
    ops.attention(q, k, v, out, 1, Sq, Sk, Hq, Hkv, Dh, Dh, q.stride(0), k.stride(0), v.stride(0), out.stride(0), q.numel(), k.numel(),
                  out.numel(), q.stride(1), k.stride(1), out.stride(1), causal, q_pos0, scale)
    torch.cuda.synchronize()
    assert_written(out, "attention output")
    return out


def assert_written(t, what):
    """Every element of a NaN-filled buffer was written (the f64 comparison may read only a subset of the rows)."""
    bad = ~torch.isfinite(t.float())
    if bool(bad.any()):
        first = bad.nonzero()[0].tolist()
        raise AssertionError(f"{what}: {int(bad.sum())} elements not written (first at {first})")


def prefill_ratio(family, S, kind, Sq=None, q_pos0=0, seed=0):
    dt = DT[kind]
    Sq = Sq or S
    q, k, v, pos = make(family, Sq, S, dt, q_pos0=q_pos0, seed=seed)
    out = prefill(q, k, v, q_pos0=q_pos0)
    ref = ref_checked(family, q, k, v, 1.0 / math.sqrt(D), pos, q_pos0=q_pos0, rows=rows_for(Sq))
    return ratio(out, ref)


def decode_cache(k, v, extra=3):
    """k / v [Sk, Hkv, D] -> one cache [Sk + extra, 2 Hkv D] (k | v per row), rows past Sk poisoned with NaN."""
    Sk = k.shape[0]
    c = torch.full((Sk + extra, 2 * k.shape[1] * k.shape[2]), NAN, dtype=k.dtype, device="cuda")
    c[:Sk, : k.shape[1] * k.shape[2]] = k.reshape(Sk, -1)
    c[:Sk, k.shape[1] * k.shape[2]:] = v.reshape(Sk, -1)
    return c


def decode_ratio(family, Sk, kind, seed=0):
    """attention_decode: the query at position Sk - 1 over Sk cached keys (split-KV + merge)."""
    ops = _ops()
    dt = DT[kind]
    q, k, v, pos = make(family, 1, Sk, dt, q_pos0=Sk - 1, seed=seed)
    c = decode_cache(k, v)
    out = torch.full((HQ * D,), NAN, dtype=dt, device="cuda")
    ws = ops.decode_workspace(HQ, HKV, "cuda")
    ops.attention_decode(q.reshape(-1), c, c[:, HKV * D:], out, Sk, HQ, HKV, 1.0 / math.sqrt(D), ws)
    torch.cuda.synchronize()
    ref = ref_checked(family, q, k, v, 1.0 / math.sqrt(D), pos, q_pos0=Sk - 1)
    return ratio(out.view(1, HQ, D), ref)


def decode_rows_ratio(family, lens, kind, prefix=0, seed=0):
    """attention_decode_rows over M scenes of the given lengths (one key sequence, each row its own query at its last position and
    its own cache copy); prefix > 0: the first `prefix` keys are read from the first cache alone, the others' copies are NaN."""
    ops = _ops()
    dt = DT[kind]
    L = max(lens)
    M = len(lens)
    positions = needle_positions(L, prefix=prefix or None) if family == "needles" else None
    qa, k, v, pos = make(family, L, L, dt, positions=positions, seed=seed)
    q = torch.stack([qa[n - 1] for n in lens]).reshape(M, HQ * D).contiguous()
    caches = [decode_cache(k[:n], v[:n]) for n in lens]
    if prefix:
        for c in caches[1:]:
            c[:prefix] = NAN
    ws = torch.empty(ops.decode_workspace(HQ, HKV, "cuda").numel() * M, dtype=torch.float32, device="cuda")
    out = torch.full((M, HQ * D), NAN, dtype=dt, device="cuda")
    ops.attention_decode_rows(q, caches, [c[:, HKV * D:] for c in caches], out, lens, HQ, HKV, 1.0 / math.sqrt(D), ws, prefix=prefix)
    torch.cuda.synchronize()
    worst = 0.0
    for m, n in enumerate(lens):
        ref = ref_checked(family, q[m].view(1, HQ, D), k[:n], v[:n], 1.0 / math.sqrt(D), [p for p in pos if p < n] if pos else None,
                          q_pos0=n - 1)
        worst = max(worst, ratio(out[m].view(1, HQ, D), ref))
    return worst


def assert_ratio(r, what):
    print(f"{what}: err/bound {r:.3g}")
    assert r <= 1.0, f"{what}: error {r:.3g} x the bound"


FAMILIES = ["diagonal", "needles"]


# ------------------------------------------------------------------------------ prefill


@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["bf16", "f16"])
@pytest.mark.parametrize("family", FAMILIES)
@pytest.mark.parametrize("S", [9, 63, 64, 65, 127, 129, 1000, 6794, 8192])
def test_prefill_causal_vs_f64(kind, family, S):
    """attn_prefill_kernel (XCD mapping where it applies): last partial 64-key tile, last 128-query tile, long rows."""
    assert_ratio(prefill_ratio(family, S, kind, seed=S), f"prefill S={S} {family} {kind}")


@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["bf16", "f16"])
def test_prefill_random_background_vs_f64(kind):
    assert_ratio(prefill_ratio("random", 1000, kind, seed=5), f"prefill S=1000 random {kind}")


@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["bf16", "f16"])
@pytest.mark.parametrize("family", FAMILIES)
def test_prefill_up_to_8_rows_goes_to_the_decode_kernel(kind, family):
    assert_ratio(prefill_ratio(family, 6, kind, seed=6), f"prefill S=6 {family} {kind}")
    assert_ratio(prefill_ratio(family, 300, kind, Sq=5, q_pos0=295, seed=7), f"5 rows over 300 keys {family} {kind}")


@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["bf16", "f16"])
@pytest.mark.parametrize("family", FAMILIES)
def test_prefill_question_rows_over_a_scene(kind, family):
    """Sq = 60 question rows at q_pos0 = Sk - 60 over Sk = 6794 keys."""
    assert_ratio(prefill_ratio(family, 6794, kind, Sq=60, q_pos0=6734, seed=8), f"60 rows over 6794 keys {family} {kind}")


@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["bf16", "f16"])
@pytest.mark.parametrize("switch", [pytest.param(("V3D_ATTN_MFMA", "16"), id="switch1")])     # (the id it has had since it was the second of two)
@pytest.mark.parametrize("S", [65, 1000, 6794])
def test_prefill_optin_kernels_vs_f64(kind, switch, S, monkeypatch):
    """attn_prefill16_kernel (16x16x32), which reads its switch on every call."""
    monkeypatch.setenv(*switch)
    for family in FAMILIES:
        assert_ratio(prefill_ratio(family, S, kind, seed=S + 1), f"{switch[0]}={switch[1]} S={S} {family} {kind}")


@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["bf16", "f16"])
@pytest.mark.parametrize("S", [129, 6794])
def test_attention_train_lse_vs_f64(kind, S):
    """v3d_attention_train: the output and the row log-sum-exp (scaled log2 units) per row and head."""
    dt = DT[kind]
    for family in FAMILIES:
        q, k, v, pos = make(family, S, S, dt, seed=S + 2)
        out, lse = prefill(q, k, v, lse=True)
        ref = ref_checked(family, q, k, v, 1.0 / math.sqrt(D), pos, rows=rows_for(S))
        assert_ratio(ratio(out, ref), f"attention_train out S={S} {family} {kind}")
        assert_ratio(lse_ratio(lse, ref), f"attention_train lse S={S} {family} {kind}")


# ------------------------------------------------------------------------------ SigLIP


_siglip_cache = {}


def _siglip_case(family, dt, B, S, H, Dh, scale):
    """Inputs and f64 references of the 32 frames (shared by both kernel forms)."""
    key = (family, dt)
    if key not in _siglip_cache:
        q, k, v = _siglip_inputs(family, dt, B, S, H, Dh)
        refs = [ref_checked(family, q[b], k[b], v[b], scale, needle_positions(S) if family == "needles" else None, causal=False)
                for b in range(B)]
        for other in [o for o in _siglip_cache if o[1] != dt]:       # keep one dtype's (both families)
            del _siglip_cache[other]
        _siglip_cache[key] = (q, k, v, refs)
    return _siglip_cache[key]


def _pad_garbage(ld, dt):
    return torch.randn(ld, generator=torch.Generator().manual_seed(7)).to(dt).cuda()


def _siglip_inputs(family, dt, B, S, H, Dh):
    qs, ks, vs = [], [], []
    for b in range(B):
        if family == "needles":
            q, k, v = needle_inputs(S, S, H, H, Dh, dt, needle_positions(S), seed=100 + b)
        else:
            q, k, v = random_inputs(S, S, H, H, Dh, dt, seed=100 + b)
        qs.append(q); ks.append(k); vs.append(v)
    return torch.stack(qs).cuda(), torch.stack(ks).cuda(), torch.stack(vs).cuda()


@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["bf16", "f16"])
@pytest.mark.parametrize("env", [None, "V3D_ATTN_KS6"])
def test_siglip_attention_vs_f64(kind, env, monkeypatch):
    """Non-causal, 16 heads of 72 on the 96-wide tile (d_out 72, scale 72^-0.5), B = 32 frames of 729 tokens: zero-padded heads and the
    engine's heads packed at stride 72; default and 6-step (V3D_ATTN_KS6=1) forms."""
    ops = _ops()
    dt = DT[kind]
    if env:
        monkeypatch.setenv(env, "1")
    B, S, H, Dh, DP = 32, 729, 16, 72, 96
    scale = Dh ** -0.5
    for family in ("needles", "random"):
        q, k, v, refs = _siglip_case(family, dt, B, S, H, Dh, scale)
        # zero-padded heads [B, S, H, 96]
        pad = torch.zeros(B, S, 3, H, DP, dtype=dt, device="cuda")
        pad[:, :, 0, :, :Dh], pad[:, :, 1, :, :Dh], pad[:, :, 2, :, :Dh] = q, k, v
        out = torch.full((B, S, H, Dh), NAN, dtype=dt, device="cuda")
        qp, kp, vp = pad[:, :, 0], pad[:, :, 1], pad[:, :, 2]
        ops.attention(qp, kp, vp, out, B, S, S, H, H, DP, Dh, qp.stride(1), kp.stride(1), vp.stride(1), out.stride(1), qp.stride(0),
                      kp.stride(0), out.stride(0), qp.stride(2), kp.stride(2), out.stride(2), False, 0, scale)
        torch.cuda.synchronize()
        assert_ratio(max(ratio(out[b], refs[b]) for b in range(B)), f"SigLIP padded {env} {family} {kind}")
        # packed at the true stride: q | k | v blocks of H x 72 in one row; the 96-wide tile reads 24 columns of the next head / padding
        ld = 3584
        row = torch.empty(B * S, ld, dtype=dt, device="cuda")
        row[:] = _pad_garbage(ld, dt)                  # finite garbage in the pad columns (one random row, broadcast)
        row[:, : H * Dh] = q.reshape(B * S, -1)
        row[:, H * Dh: 2 * H * Dh] = k.reshape(B * S, -1)
        row[:, 2 * H * Dh: 3 * H * Dh] = v.reshape(B * S, -1)
        out2 = torch.full((B * S, H * Dh), NAN, dtype=dt, device="cuda")
        ops.attention(row, row[:, H * Dh:], row[:, 2 * H * Dh:], out2, B, S, S, H, H, DP, Dh, ld, ld, ld, out2.stride(0), S * ld, S * ld,
                      S * out2.stride(0), Dh, Dh, Dh, False, 0, scale)
        torch.cuda.synchronize()
        o2 = out2.view(B, S, H, Dh)
        assert_ratio(max(ratio(o2[b], refs[b]) for b in range(B)), f"SigLIP packed {env} {family} {kind}")


# ------------------------------------------------------------------------------ shared prefix (question rows of an answer batch)


@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["bf16", "f16"])
@pytest.mark.parametrize("family", FAMILIES)
def test_attention_shared_prefix_vs_f64(kind, family):
    """v3d_attention_shared_prefix: B = 3 questions x 60 rows at q_pos0 = P = 6734 over Sk = 6794 keys; key tiles below 6720 from the
    scene's one cache, the rest (the prefix's partial tile and the question's own keys) from each question's cache, whose rows below
    6720 and past Sk are NaN.  The questions share q and k, and differ in the values of their own keys."""
    ops = _ops()
    dt = DT[kind]
    B, Sq, P = 3, 60, 6734
    Sk = P + Sq
    P0 = P // 64 * 64
    kvw = HKV * D
    positions = needle_positions(Sk, prefix=P) if family == "needles" else None
    qa, k, v, pos = make(family, Sq, Sk, dt, q_pos0=P, positions=positions, seed=11)
    g = torch.Generator().manual_seed(12)
    cap = Sk + 5
    scene = torch.full((cap, 2 * kvw), NAN, dtype=dt, device="cuda")
    scene[:P, :kvw] = k[:P].reshape(P, -1)
    scene[:P, kvw:] = v[:P].reshape(P, -1)
    own = torch.full((B, cap, 2 * kvw), NAN, dtype=dt, device="cuda")
    vs = []
    for b in range(B):
        vb = v.clone()
        vb[P:] = torch.randn(Sq, HKV, D, generator=g).to(dt).cuda() * (1 + b)
        own[b, P0:Sk, :kvw] = k[P0:].reshape(Sk - P0, -1)
        own[b, P0:Sk, kvw:] = vb[P0:].reshape(Sk - P0, -1)
        vs.append(vb)
    q = qa.reshape(Sq, HQ * D).repeat(B, 1).contiguous()
    got = torch.full((B * Sq, HQ * D), NAN, dtype=dt, device="cuda")
    o2 = own.view(-1, 2 * kvw)
    ops.attention_shared_prefix(q, o2, o2[:, kvw:], scene, scene[:, kvw:], P0, got, B, Sq, Sk, HQ, HKV, q.stride(0), o2.stride(0), o2.stride(0),
                                got.stride(0), Sq * q.stride(0), own.stride(0), Sq * got.stride(0), D, D, D, P, 1.0 / math.sqrt(D))
    torch.cuda.synchronize()
    worst = 0.0
    for b in range(B):
        ref = ref_checked(family, qa, k, vs[b], 1.0 / math.sqrt(D), pos, q_pos0=P)
        worst = max(worst, ratio(got[b * Sq:(b + 1) * Sq].view(Sq, HQ, D), ref))
    assert_ratio(worst, f"shared prefix {family} {kind}")


# ------------------------------------------------------------------------------ decode


@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["bf16", "f16"])
@pytest.mark.parametrize("Sk", [1, 63, 64, 65, 256, 257, 6800, 8192])
def test_attention_decode_vs_f64(kind, Sk):
    for family in FAMILIES:
        assert_ratio(decode_ratio(family, Sk, kind, seed=Sk), f"decode Sk={Sk} {family} {kind}")


@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["bf16", "f16"])
def test_attention_decode_rows_ragged_vs_f64(kind):
    lens = [1, 64, 65, 257, 1000, 3000, 6800]
    for family in FAMILIES:
        assert_ratio(decode_rows_ratio(family, lens, kind, seed=21), f"decode rows ragged {family} {kind}")


@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["bf16", "f16"])
@pytest.mark.parametrize("mm", [0, 1])
def test_attention_decode_rows_shared_prefix_32_rows_vs_f64(kind, mm, monkeypatch):
    """The cached-question group: M = 32 rows over one scene's P = 6734-key prefix (V3D_DEC_PREFIX_MM=0: the split kernels walk it;
    1: one matrix-core launch over 256-key chunks), own tails of 1 .. 94 keys."""
    monkeypatch.setenv("V3D_DEC_PREFIX_MM", str(mm))
    P = 6734
    lens = [P + 1 + (37 * m) % 94 for m in range(32)]
    for family in FAMILIES:
        assert_ratio(decode_rows_ratio(family, lens, kind, prefix=P, seed=22), f"decode rows prefix mm={mm} {family} {kind}")


# ------------------------------------------------------------------------------ once-per-process switches (child process)


CHILD_CASES = {
    "V3D_ATTN_XCD=0": [("prefill", S, kind, fam) for S in (129, 6794) for kind in DT for fam in FAMILIES],
    "V3D_DEC_ATTN=valu": [("decode", Sk, kind, fam) for Sk in (65, 6800) for kind in DT for fam in FAMILIES],
    "V3D_DEC_KEYS_PER_SPLIT=64": [("decode", Sk, kind, fam) for Sk in (65, 257, 8192) for kind in DT for fam in FAMILIES],
}


def _child(mode):
    res = {}
    for what, S, kind, fam in CHILD_CASES[mode]:
        r = prefill_ratio(fam, S, kind, seed=S + 3) if what == "prefill" else decode_ratio(fam, S, kind, seed=S + 3)
        res[f"{what} {S} {kind} {fam}"] = r
    print("RESULT " + json.dumps(res))


@pytest.mark.gpu
@pytest.mark.parametrize("mode", list(CHILD_CASES))
def test_once_per_process_switches_vs_f64(mode):
    name, val = mode.split("=")
    env = dict(os.environ)
    env[name] = val
    p = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", mode], env=env, capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-4000:]
    line = [ln for ln in p.stdout.splitlines() if ln.startswith("RESULT ")][-1]
    res = json.loads(line[len("RESULT "):])
    assert len(res) == len(CHILD_CASES[mode])
    for k, r in res.items():
        assert_ratio(r, f"{mode}: {k}")


if __name__ == "__main__" and len(sys.argv) == 3 and sys.argv[1] == "--child":
    _child(sys.argv[2])
