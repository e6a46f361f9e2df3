"""FP8 (OCP e4m3) LLM linears - BASELINE.json configs[3].  Not a reference code path (the reference runs bf16 only,
scripts/3d/train/train_multi.sh:57-58), so the tolerance is re-stated here instead of being pinned by a golden:

  * v3d_quantize_fp8_rows is checked BIT-EXACT against torch's float8_e4m3fn cast of x * (1 / scale), scale = amax/448;
  * v3d_gemm_fp8 is checked against an f64 matmul of the SAME dequantised operands: the only error left is f32
    accumulation + one rounding to the output type -> |err| <= 2^-8 |ref| + 2^-10 rms(ref)  (bf16 output);
  * against the bf16 v3d_gemm of the unquantised operands the relative Frobenius error must stay below 6 %
    (e4m3 carries 3 mantissa bits: <= 2^-4 relative error per operand, ~3.6 % rms for both operands).
"""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from v3d import ops  # noqa: E402

DEV = "cuda"


def _deq(q, s):
    return q.view(torch.float8_e4m3fn).to(torch.float64) * s.to(torch.float64)[:, None]


def _rand(m, k, dtype, seed, outlier=True):
    g = torch.Generator(device="cpu").manual_seed(seed)
    x = torch.randn(m, k, generator=g)
    if outlier:
        x[:, 3] *= 20.0          # a heavy channel, as LLM activations have
    return x.to(dtype).to(DEV)


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16])
@pytest.mark.parametrize("rows,cols", [(1, 128), (5, 3584), (300, 18944), (6794, 3584)])
def test_quantize_rows_bit_exact(dtype, rows, cols):
    x = _rand(rows, cols, dtype, rows * 7 + cols)
    x[rows // 2] = 0                                           # an all-zero row keeps scale 1
    q, s = ops.quantize_fp8_rows(x)
    # IEEE f32 divisions on the host (torch's GPU "tensor / scalar" multiplies by a rounded reciprocal instead)
    amax = x.float().abs().amax(1).cpu().numpy()
    s_ref = np.where(amax > 0, amax / np.float32(448.0), np.float32(1.0)).astype(np.float32)
    assert np.array_equal(s.cpu().numpy(), s_ref)
    inv = (np.float32(1.0) / s_ref).astype(np.float32)
    scaled = torch.from_numpy(x.float().cpu().numpy() * inv[:, None])
    q_ref = scaled.to(torch.float8_e4m3fn).view(torch.uint8)
    assert torch.equal(q.cpu(), q_ref)
    assert int(q[rows // 2].max()) == 0


CASES = [
    # M, N, K, epilogue
    (256, 256, 128, "none"),
    (1, 256, 256, "none"),
    (300, 512, 3584, "bias"),
    (777, 3584, 3584, "res"),
    (1000, 1024, 18944, "res"),
    (513, 2048, 3584, "swiglu"),
    (6794, 4608, 3584, "bias"),
    (2305, 512, 256, "swiglu"),     # ten m-tiles (short last group of 8), 20 workgroups (XCD remainder), one-row M tail, two K-steps, two n-tiles
]


@pytest.mark.parametrize("M,N,K,epi", CASES)
@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16])
def test_gemm_fp8_vs_dequantised_f64(M, N, K, epi, dtype):
    a = _rand(M, K, dtype, 11 + M)
    w = (_rand(N, K, dtype, 13 + N, outlier=False).float() * K ** -0.5).to(dtype)
    qa, sa = ops.quantize_fp8_rows(a)
    qw, sw = ops.quantize_fp8_rows(w)
    ref = _deq(qa, sa) @ _deq(qw, sw).T
    kw = {}
    if epi == "bias":
        bias = _rand(1, N, dtype, 5, outlier=False)[0]
        kw = dict(bias=bias, epilogue=ops.EPI_BIAS)
        ref = ref + bias.double()
    elif epi == "res":
        res = _rand(M, N, dtype, 6, outlier=False)
        kw = dict(res=res, epilogue=ops.EPI_RES)
        # the kernel rounds the product to the output type, then adds the residual (as v3d_gemm's RES epilogue)
        ref = ref.to(dtype).double() + res.double()
    elif epi == "swiglu":
        kw = dict(epilogue=ops.EPI_SWIGLU)
        r = ref.to(dtype).float().view(M, N // 128, 2, 64)
        g, u = r[:, :, 0], r[:, :, 1]
        ref = (torch.nn.functional.silu(g).to(dtype).float() * u).reshape(M, N // 2).double()
    out = ops.gemm_fp8(qa, sa, qw, sw, dtype, **kw)
    assert out.shape == ref.shape
    eps = 2.0 ** -8 if dtype == torch.bfloat16 else 2.0 ** -11
    # "res"/"swiglu" round an intermediate to the output type first: one more half-ulp of that intermediate
    slack = 3.0 if epi in ("res", "swiglu") else 1.0
    rms = ref.pow(2).mean().sqrt()
    err = (out.double() - ref).abs()
    bound = slack * eps * ref.abs() + slack * 4 * eps * rms * (1.0 if epi != "none" else 0.25)
    assert bool((err <= bound).all()), f"max excess {(err - bound).max().item():.3e}"


@pytest.mark.parametrize("M,N,K", [(1024, 4608, 3584), (2000, 3584, 18944)])
def test_gemm_fp8_close_to_bf16(M, N, K):
    dtype = torch.bfloat16
    a = _rand(M, K, dtype, 3)
    w = (_rand(N, K, dtype, 4, outlier=False).float() * K ** -0.5).to(dtype)
    full = ops.gemm(a, w).float()
    qa, sa = ops.quantize_fp8_rows(a)
    qw, sw = ops.quantize_fp8_rows(w)
    out = ops.gemm_fp8(qa, sa, qw, sw, dtype).float()
    rel = (out - full).norm() / full.norm()
    assert rel < 0.06, rel.item()


def test_gemm_fp8_rejects_bad_shapes():
    qa = torch.zeros(4, 128, dtype=torch.uint8, device=DEV)
    sa = torch.ones(4, device=DEV)
    qw = torch.zeros(128, 128, dtype=torch.uint8, device=DEV)     # N not a multiple of 256
    sw = torch.ones(128, device=DEV)
    with pytest.raises(Exception, match="multiple of 256"):
        ops.gemm_fp8(qa, sa, qw, sw, torch.bfloat16)


def test_engine_prefill_fp8_close_to_bf16():
    """Whole decoder prefill with e4m3 linears vs the bf16 engine on the same weights and inputs: relative L2 error
    of the last hidden state below 8 % (two layers; the per-GEMM error is ~3.6 %, see the module docstring) and the
    K/V cache rows of layer 0 below 6 %."""
    from v3d.engine import Engine, EngineConfig, LlmConfig, VitConfig, random_state_dict
    cfg = EngineConfig(vit=VitConfig(hidden=144, inter=272, layers=1, heads=2),
                       llm=LlmConfig(hidden=256, inter=384, layers=2, heads=2, kv_heads=1, vocab=320, max_pos=1024))
    sd = random_state_dict(cfg, torch.float32, "cpu", seed=5, std=0.05)
    a = Engine(cfg, sd, dtype=torch.bfloat16, device=DEV, max_frames=1)
    b = Engine(cfg, sd, dtype=torch.bfloat16, device=DEV, max_frames=1, llm_fp8=True)
    g = torch.Generator().manual_seed(6)
    x = (torch.randn(300, 256, generator=g) * 0.5).bfloat16().to(DEV)
    la = a.llm_forward(x.clone(), 0).clone()
    lb = b.llm_forward(x.clone(), 0).clone()
    rel = lambda u, v: ((u.float() - v.float()).norm() / v.float().norm()).item()
    assert rel(b.kv[0][:300], a.kv[0][:300]) < 0.06
    assert rel(b.last_hidden(), a.last_hidden()) < 0.08
    assert rel(lb, la) < 0.10
    # decode after an fp8 prefill runs the 16-bit weight-streaming path against the fp8-built cache
    tok = torch.zeros(1, 256, dtype=torch.bfloat16, device=DEV)
    tok[0] = x[5]
    lb2 = b.decode_forward(tok, 300)
    assert torch.isfinite(lb2).all()


@pytest.mark.parametrize("M", [1, 2, 4, 9, 16, 23, 32])
@pytest.mark.parametrize("K,N", [(3584, 512), (18944, 256), (256, 384), (400, 64)])
def test_linear_decode_fp8_rows(M, K, N):
    """W8A16 decode linear: e4m3 weights (per-row scales) x 16-bit activations, against an f64 product of the SAME
    dequantised weights: only f32 accumulation and the output rounding remain (|err| <= 2^-8 |ref| + 2^-9 rms)."""
    dt = torch.bfloat16
    g = torch.Generator().manual_seed(7 * M + K)
    x = torch.randn(M, K, generator=g).to(dt).to(DEV)
    w = (torch.randn(N, K, generator=g) * K ** -0.5).to(dt).to(DEV)
    qw, sw = ops.quantize_fp8_rows(w)
    if M > 4 and K % 256:                              # odd shapes have no matrix-core form: up to 4 rows only
        with pytest.raises(Exception, match="activation rows"):
            ops.linear_decode_fp8_rows(x, qw, sw, torch.empty(M, N, dtype=dt, device=DEV))
        return
    wd = _deq(qw, sw)                                            # [N, K] f64
    ref = x.double() @ wd.T
    b = torch.randn(N, generator=g).to(dt).to(DEV)
    r = torch.randn(M, N, generator=g).to(dt).to(DEV)

    def check(out, want, slack=1.0):
        rms = want.pow(2).mean().sqrt()
        err = (out.double() - want).abs()
        bound = slack * (2.0 ** -8 * want.abs() + 2.0 ** -9 * rms)
        assert bool((err <= bound).all()), (err - bound).max().item()

    out = torch.empty(M, N, dtype=dt, device=DEV)
    ops.linear_decode_fp8_rows(x, qw, sw, out)
    check(out, ref)
    ops.linear_decode_fp8_rows(x, qw, sw, out, bias=b, epilogue=ops.DEC_BIAS)
    check(out, ref + b.double())
    ops.linear_decode_fp8_rows(x, qw, sw, out, res=r, epilogue=ops.DEC_RES)
    check(out, ref.to(dt).double() + r.double(), slack=3.0)
    if N % 128 == 0:
        act = torch.empty(M, N // 2, dtype=dt, device=DEV)
        ops.linear_decode_fp8_rows(x, qw, sw, act, epilogue=ops.DEC_SWIGLU)
        rr = ref.to(dt).float().view(M, N // 128, 2, 64)
        want = (torch.nn.functional.silu(rr[:, :, 0]).to(dt).float() * rr[:, :, 1]).reshape(M, N // 2).double()
        check(act, want, slack=4.0)
    # a row's result does not depend on the other rows of the batch (nor on M within the same form: M >= 2 matrix-core
    # when K % 256 == 0, else VALU)
    ops.linear_decode_fp8_rows(x, qw, sw, out)
    if M >= 3:
        sub = torch.empty(2, N, dtype=dt, device=DEV)
        ops.linear_decode_fp8_rows(x[M - 2:], qw, sw, sub)
        assert torch.equal(out[M - 2:], sub)
    if M == 1 or K % 256:
        one = torch.empty(1, N, dtype=dt, device=DEV)
        ops.linear_decode_fp8_rows(x[M - 1: M], qw, sw, one)
        assert torch.equal(out[M - 1], one[0])


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16])
@pytest.mark.parametrize("rows,cols", [(5, 3584), (300, 256), (6794, 3584)])
def test_rmsnorm_quantize_fused_bit_identical_to_two_calls(dtype, rows, cols):
    x = _rand(rows, cols, dtype, rows + cols)
    w = (1 + 0.1 * _rand(1, cols, dtype, 3, outlier=False)[0]).to(dtype)
    h = ops.rmsnorm(x, w, 1e-6)
    q_ref, s_ref = ops.quantize_fp8_rows(h)
    q = torch.empty_like(q_ref)
    s = torch.empty_like(s_ref)
    ops.rmsnorm_quantize_fp8(x, w, 1e-6, q, s)
    assert torch.equal(s, s_ref) and torch.equal(q, q_ref)
