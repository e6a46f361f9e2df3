"""MXFP4 (OCP MX v1.0) LLM weights: v3d_quantize_mxfp4_rows, v3d_gemm_mxfp4 (prefill, W4A8), v3d_linear_decode_mxfp4_rows (decode,
W4A16) and Engine(llm_fp4=True).  Not a reference code path (the reference runs 16-bit only), so the contract is stated here, as
tests/test_gpu_fp8.py does for e4m3; the format itself is restated on the host in tests/mxfp4_check.py (pinned by
tests/test_mxfp4_check_cpu.py):

  * the quantiser is BIT-EXACT against that restatement (bf16 and f16);
  * operand and scale placement: a one-hot e4m3 activation matrix reads deq(W) back EXACTLY (every block has its own exponent);
  * v3d_gemm_mxfp4 against an f64 matmul of the SAME dequantised operands, with the bound of test_gpu_fp8.py (f32 accumulation +
    one rounding):  |err| <= slack (eps |ref| + 4 eps rms(ref) [x 0.25 without an epilogue]),  eps = 2^-8 (bf16) / 2^-11 (f16);
  * v3d_linear_decode_mxfp4_rows against the f64 product with deq(W): |err| <= slack (2^-8 |ref| + 2^-9 rms(ref)) as the e4m3
    decode test (f16: 2^-11, 2^-12);
  * quantisation error budget at (512, 512, 1024), seeds 3 / 4: the f64 product of the host-quantised operands (e4m3 rows x MXFP4
    weights) is 11.67 % (relative Frobenius) away from the f64 product of the originals - 11.44 % of it from the weights alone;
    the GPU result against the bf16 v3d_gemm must be within 1.10 x that figure, recomputed here on the host;
  * engine: the two-layer figure is not derived from a host run of the stack (that would need a host restatement of the whole
    decoder with its e4m3 activation rows); it is asserted against 2 x the per-GEMM figure above (0.2333), as the issue allows.
"""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import mxfp4_check as MX  # noqa: E402
from v3d import ops  # noqa: E402

DEV = "cuda"
PER_GEMM_REL = 0.1167          # host f64 figure of test_quantisation_error_budget (see the module docstring)


def _rand(m, k, dtype, seed, outlier=True):
    g = torch.Generator(device="cpu").manual_seed(seed)
    x = torch.randn(m, k, generator=g)
    if outlier:
        x[:, 3] *= 20.0          # a heavy channel, as LLM activations have
    return x.to(dtype).to(DEV)


def _weights(n, k, dtype, seed):
    return (_rand(n, k, dtype, seed, outlier=False).float() * k ** -0.5).to(dtype)


def _deq8(q, s):
    return q.view(torch.float8_e4m3fn).to(torch.float64).cpu() * s.to(torch.float64).cpu()[:, None]


def _deq4(q, e):
    return torch.from_numpy(MX.dequantize(q, e))


# ------------------------------------------------------------------------------------------------ quantiser
@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16])
@pytest.mark.parametrize("rows,cols", [(1, 128), (5, 3584), (256, 18944)])
def test_quantize_mxfp4_bit_exact(dtype, rows, cols):
    w = _rand(rows, cols, dtype, rows * 7 + cols, outlier=False)
    nb = cols // 32
    # a row whose 32-blocks span 2^-20 .. 2^10, one all-zero block in it, and (with more than one row) an all-zero row
    span = torch.pow(2.0, torch.linspace(-20, 10, nb).round()).repeat_interleave(32).to(DEV)
    w[0] = (w[0].float() * span).to(dtype)
    w[0, 32 * (nb // 2): 32 * (nb // 2) + 32] = 0
    if rows > 1:
        w[rows // 2] = 0
        w[1, :32] = torch.tensor([6, 0.25, 0.75, 1.25, 1.75, 2.5, 3.5, 5, -0.25, -0.75, -1.25, -1.75, -2.5, -3.5, -5, 7] * 2, dtype=dtype)   # ties
    q, e = ops.quantize_mxfp4_rows(w)
    q_ref, e_ref = MX.quantize(w)
    assert q.shape == (rows, cols // 2) and e.shape == (rows, nb) and q.dtype == torch.uint8 and e.dtype == torch.uint8
    assert np.array_equal(e.cpu().numpy(), e_ref)
    assert np.array_equal(q.cpu().numpy(), q_ref)
    assert int(e.max()) < 255
    if rows > 1:
        assert int(q[rows // 2].max()) == 0 and bool((e[rows // 2] == 127).all())


def test_quantize_mxfp4_refuses_non_finite_weights():
    w = torch.ones(4, 128, dtype=torch.bfloat16, device=DEV)
    w[2, 5] = float("inf")
    with pytest.raises(Exception, match="non-finite"):
        ops.quantize_mxfp4_rows(w)
    w[2, 5] = float("nan")
    with pytest.raises(Exception, match="non-finite"):
        ops.quantize_mxfp4_rows(w)


# ------------------------------------------------------------------------------------------------ placement
@pytest.mark.parametrize("K", [128, 256, 384])
def test_gemm_mxfp4_operand_and_scale_placement(K):
    """Random codes, another exponent in every block of every row, identity activations: the output IS deq(W)^T.  A wrong nibble,
    lane, scale byte or double-buffer swap shows as a wrong element."""
    N = 256
    rng = np.random.default_rng(K)
    c = rng.integers(0, 16, size=(N, K)).astype(np.uint8)
    e = (127 - 4 + ((np.arange(N)[:, None] + np.arange(K // 32)[None, :]) % 9)).astype(np.uint8)
    q = MX.pack(c)
    qa = torch.zeros(K, K, dtype=torch.uint8)
    qa[torch.arange(K), torch.arange(K)] = 0x38                  # e4m3 1.0
    sa = torch.ones(K, dtype=torch.float32, device=DEV)
    out = ops.gemm_mxfp4(qa.to(DEV), sa, torch.from_numpy(q).to(DEV), torch.from_numpy(e).to(DEV), torch.bfloat16)
    want = torch.from_numpy(MX.dequantize(q, e)).T.contiguous()   # [K, N]: e2m1 x 2^(-4..4) is exact in bf16
    got = out.double().cpu()
    bad = (got != want).nonzero()
    assert bad.numel() == 0, f"{bad.shape[0]} wrong elements, first (m=k, n) {bad[0].tolist()}: {got[tuple(bad[0])].item()} != {want[tuple(bad[0])].item()}"


# ------------------------------------------------------------------------------------------------ prefill GEMM
CASES = [
    # M, N, K, epilogue
    (1, 256, 128, "none"),
    (257, 256, 384, "none"),
    (300, 512, 3584, "bias"),
    (513, 512, 1024, "swiglu"),
    (300, 256, 18944, "res"),
    (2305, 512, 256, "swiglu"),     # ten m-tiles (short last group of 8), 20 workgroups (XCD remainder), one-row M tail, two K-steps, two n-tiles
]


@pytest.mark.parametrize("M,N,K,epi", CASES)
@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16])
def test_gemm_mxfp4_vs_dequantised_f64(M, N, K, epi, dtype):
    a = _rand(M, K, dtype, 11 + M)
    w = _weights(N, K, dtype, 13 + N)
    qa, sa = ops.quantize_fp8_rows(a)
    q, e = ops.quantize_mxfp4_rows(w)
    ref = _deq8(qa, sa) @ _deq4(q, e).T
    kw = {}
    if epi == "bias":
        bias = _rand(1, N, dtype, 5, outlier=False)[0]
        kw = dict(bias=bias, epilogue=ops.EPI_BIAS)
        ref = ref + bias.double().cpu()
    elif epi == "res":
        res = _rand(M, N, dtype, 6, outlier=False)
        kw = dict(res=res, epilogue=ops.EPI_RES)
        ref = ref.to(dtype).double() + res.double().cpu()         # the product is rounded to the output type, then the residual is added
    elif epi == "swiglu":
        kw = dict(epilogue=ops.EPI_SWIGLU)
        r = ref.to(dtype).float().view(M, N // 128, 2, 64)
        g, u = r[:, :, 0], r[:, :, 1]
        ref = (torch.nn.functional.silu(g).to(dtype).float() * u).reshape(M, N // 2).double()
    out = ops.gemm_mxfp4(qa, sa, q, e, dtype, **kw)
    assert out.shape == ref.shape
    eps = 2.0 ** -8 if dtype == torch.bfloat16 else 2.0 ** -11
    slack = 3.0 if epi in ("res", "swiglu") else 1.0
    rms = ref.pow(2).mean().sqrt()
    err = (out.double().cpu() - ref).abs()
    bound = slack * eps * ref.abs() + slack * 4 * eps * rms * (1.0 if epi != "none" else 0.25)
    print(f"max err/bound {(err / bound).max().item():.3f}")
    assert bool((err <= bound).all()), f"max excess {(err - bound).max().item():.3e}"


def test_mxfp4_wrappers_refuse_wrong_types_and_strides():
    qa = torch.zeros(4, 128, dtype=torch.uint8, device=DEV)
    sa = torch.ones(4, device=DEV)
    q = torch.zeros(256, 64, dtype=torch.uint8, device=DEV)
    e = torch.full((256, 4), 127, dtype=torch.uint8, device=DEV)
    x = torch.zeros(2, 128, dtype=torch.bfloat16, device=DEV)
    out = torch.empty(2, 256, dtype=torch.bfloat16, device=DEV)
    ops.gemm_mxfp4(qa, sa, q, e, torch.bfloat16)
    ops.linear_decode_mxfp4_rows(x, q, e, out)
    with pytest.raises(Exception, match="expected torch.uint8"):
        ops.gemm_mxfp4(qa, sa, q.to(torch.int8), e, torch.bfloat16)
    with pytest.raises(Exception, match="expected torch.uint8"):
        ops.gemm_mxfp4(qa.to(torch.int32), sa, q, e, torch.bfloat16)
    with pytest.raises(Exception, match="expected torch.float32"):
        ops.gemm_mxfp4(qa, sa.double(), q, e, torch.bfloat16)
    with pytest.raises(Exception, match="unit inner stride"):
        ops.gemm_mxfp4(qa, sa, torch.zeros(64, 256, dtype=torch.uint8, device=DEV).T, e, torch.bfloat16)
    with pytest.raises(Exception, match="unit inner stride"):
        ops.linear_decode_mxfp4_rows(x, q, torch.full((4, 256), 127, dtype=torch.uint8, device=DEV).T, out)
    with pytest.raises(Exception, match="on the device of q"):
        ops.linear_decode_mxfp4_rows(x, q, e.cpu(), out)
    with pytest.raises(Exception, match="do not match"):
        ops.linear_decode_mxfp4_rows(x, q, e[:, :3], out)
    with pytest.raises(Exception, match="expected torch.bfloat16"):
        ops.linear_decode_mxfp4_rows(x, q, e, out.half())


def test_gemm_mxfp4_rejects_bad_shapes():
    qa = torch.zeros(4, 128, dtype=torch.uint8, device=DEV)
    sa = torch.ones(4, device=DEV)
    q = torch.zeros(128, 64, dtype=torch.uint8, device=DEV)       # N not a multiple of 256
    e = torch.full((128, 4), 127, dtype=torch.uint8, device=DEV)
    with pytest.raises(Exception, match="multiple of 256"):
        ops.gemm_mxfp4(qa, sa, q, e, torch.bfloat16)


# ------------------------------------------------------------------------------------------------ decode linears
_DEC = {}


def _decode_case(K, N, dt):
    """weights, their f64 image and 32 activation rows of one (K, N): made once, shared by every M, never modified"""
    key = (K, N, dt)
    if key not in _DEC:
        g = torch.Generator().manual_seed(7 * K + N)
        x = torch.randn(32, K, generator=g).to(dt).to(DEV)
        w = (torch.randn(N, K, generator=g) * K ** -0.5).to(dt).to(DEV)
        q, e = ops.quantize_mxfp4_rows(w)
        wd = _deq4(q, e).to(dt).double()                          # deq(W) rounded to the activation type (exact here)
        b = torch.randn(N, generator=g).to(dt).to(DEV)
        r = torch.randn(32, N, generator=g).to(dt).to(DEV)
        _DEC[key] = (x, q, e, x.double().cpu() @ wd.T, b, r)
    return _DEC[key]


@pytest.mark.parametrize("M", [1, 2, 9, 16, 32])
@pytest.mark.parametrize("K,N,dt", [(256, 384, torch.bfloat16), (3584, 512, torch.bfloat16), (18944, 256, torch.bfloat16), (3584, 512, torch.float16)])
def test_linear_decode_mxfp4_rows(M, K, N, dt):
    x32, q, e, ref32, b, r32 = _decode_case(K, N, dt)
    x, ref, r = x32[:M], ref32[:M], r32[:M]
    e1, e2 = (2.0 ** -8, 2.0 ** -9) if dt == torch.bfloat16 else (2.0 ** -11, 2.0 ** -12)

    def check(out, want, slack=1.0):
        rms = want.pow(2).mean().sqrt()
        err = (out.double().cpu() - want).abs()
        bound = slack * (e1 * want.abs() + e2 * rms)
        assert bool((err <= bound).all()), (err - bound).max().item()

    out = torch.empty(M, N, dtype=dt, device=DEV)
    ops.linear_decode_mxfp4_rows(x, q, e, out)
    check(out, ref)
    ops.linear_decode_mxfp4_rows(x, q, e, out, bias=b, epilogue=ops.DEC_BIAS)
    check(out, ref + b.double().cpu())
    ops.linear_decode_mxfp4_rows(x, q, e, out, res=r, epilogue=ops.DEC_RES)
    check(out, ref.to(dt).double() + r.double().cpu(), slack=3.0)
    act = torch.empty(M, N // 2, dtype=dt, device=DEV)
    ops.linear_decode_mxfp4_rows(x, q, e, act, epilogue=ops.DEC_SWIGLU)
    rr = ref.to(dt).float().view(M, N // 128, 2, 64)
    want = (torch.nn.functional.silu(rr[:, :, 0]).to(dt).float() * rr[:, :, 1]).reshape(M, N // 2).double()
    check(act, want, slack=4.0)


@pytest.mark.parametrize("K,N", [(256, 384), (3584, 512), (18944, 256)])
def test_linear_decode_mxfp4_row_does_not_depend_on_m(K, N):
    dt = torch.bfloat16
    x32, q, e, _, b, r32 = _decode_case(K, N, dt)
    for kw32, kw9, n_out in ((dict(), dict(), N), (dict(bias=b, epilogue=ops.DEC_BIAS),) * 2 + (N,),
                             (dict(res=r32, epilogue=ops.DEC_RES), dict(res=r32[:9], epilogue=ops.DEC_RES), N),
                             (dict(epilogue=ops.DEC_SWIGLU),) * 2 + (N // 2,)):
        o32 = torch.empty(32, n_out, dtype=dt, device=DEV)
        o9 = torch.empty(9, n_out, dtype=dt, device=DEV)
        ops.linear_decode_mxfp4_rows(x32, q, e, o32, **kw32)
        ops.linear_decode_mxfp4_rows(x32[:9], q, e, o9, **kw9)
        assert torch.equal(o32[:9], o9)
        o2 = torch.empty(2, n_out, dtype=dt, device=DEV)
        kw2 = dict(kw9, res=r32[7:9]) if "res" in kw9 else kw9
        ops.linear_decode_mxfp4_rows(x32[7:9], q, e, o2, **kw2)    # ... nor on the other rows
        assert torch.equal(o32[7:9], o2)


def test_linear_decode_mxfp4_rejects_many_rows_without_a_matrix_core_shape():
    dt = torch.bfloat16
    x = torch.zeros(9, 384, dtype=dt, device=DEV)                  # K % 256 != 0: VALU form, up to 4 rows
    q = torch.zeros(64, 192, dtype=torch.uint8, device=DEV)
    e = torch.full((64, 12), 127, dtype=torch.uint8, device=DEV)
    with pytest.raises(Exception, match="activation rows"):
        ops.linear_decode_mxfp4_rows(x, q, e, torch.empty(9, 64, dtype=dt, device=DEV))
    g = torch.Generator().manual_seed(1)
    x = torch.randn(3, 384, generator=g).to(dt).to(DEV)
    w = (torch.randn(64, 384, generator=g) * 0.05).to(dt).to(DEV)
    q, e = ops.quantize_mxfp4_rows(w)
    out = torch.empty(3, 64, dtype=dt, device=DEV)
    ops.linear_decode_mxfp4_rows(x, q, e, out)
    ref = x.double().cpu() @ _deq4(q, e).T
    err = (out.double().cpu() - ref).abs()
    assert bool((err <= 2.0 ** -8 * ref.abs() + 2.0 ** -9 * ref.pow(2).mean().sqrt()).all())
    one = torch.empty(1, 64, dtype=dt, device=DEV)
    ops.linear_decode_mxfp4_rows(x[2:3], q, e, one)
    assert torch.equal(out[2], one[0])


# ------------------------------------------------------------------------------------------------ error budget
def test_quantisation_error_budget():
    """(512, 512, 1024), seeds 3 / 4.  Host figure (f64 product of the host-quantised operands against the f64 product of the originals):
    0.11665 - recomputed below; the GPU result against the bf16 v3d_gemm of the unquantised operands must be within 1.10 x of it
    (the 10 % covers f32 accumulation and the two output roundings; the quantisation is deterministic and the same on both sides)."""
    M, N, K = 512, 512, 1024
    dtype = torch.bfloat16
    a = _rand(M, K, dtype, 3)
    w = _weights(N, K, dtype, 4)
    # host: e4m3 rows as test_gpu_fp8.py restates them, MXFP4 weights from the helper
    af = a.float().cpu().numpy()
    amax = np.abs(af).max(1)
    s = np.where(amax > 0, amax / np.float32(448.0), np.float32(1.0)).astype(np.float32)
    inv = (np.float32(1.0) / s).astype(np.float32)
    da = torch.from_numpy(af * inv[:, None]).to(torch.float8_e4m3fn).to(torch.float64) * torch.from_numpy(s).double()[:, None]
    dw = torch.from_numpy(MX.dequantize(*MX.quantize(w)))
    exact = a.double().cpu() @ w.double().cpu().T
    cpu_rel = ((da @ dw.T - exact).norm() / exact.norm()).item()
    assert abs(cpu_rel - PER_GEMM_REL) < 5e-4, cpu_rel              # the figure the docstrings and DESIGN.md quote
    full = ops.gemm(a, w).float()
    qa, sa = ops.quantize_fp8_rows(a)
    q, e = ops.quantize_mxfp4_rows(w)
    out = ops.gemm_mxfp4(qa, sa, q, e, dtype).float()
    rel = ((out - full).norm() / full.norm()).item()
    print(f"host {cpu_rel:.5f} gpu {rel:.5f}")
    assert rel <= 1.10 * cpu_rel, (rel, cpu_rel)


# ------------------------------------------------------------------------------------------------ engine
def _tiny(layers_vit=1):
    from v3d.engine import EngineConfig, LlmConfig, VitConfig
    return EngineConfig(vit=VitConfig(hidden=144, inter=272, layers=layers_vit, heads=2),
                        llm=LlmConfig(hidden=256, inter=384, layers=2, heads=2, kv_heads=1, vocab=320, max_pos=1024))


def test_engine_prefill_fp4_close_to_bf16(monkeypatch):
    """The tiny config of test_engine_prefill_fp8_close_to_bf16 with MXFP4 linears: finite logits, last hidden state within 2 x the
    per-GEMM figure of the bf16 engine (see the module docstring), and the bf16 engine never reaches an MXFP4 entry."""
    from v3d.engine import Engine, random_state_dict
    cfg = _tiny()
    sd = random_state_dict(cfg, torch.float32, "cpu", seed=5, std=0.05)
    calls = {"n": 0}
    for name in ("quantize_mxfp4_rows", "gemm_mxfp4", "linear_decode_mxfp4_rows"):
        real = getattr(ops, name)

        def spy(*a, _real=real, **kw):
            calls["n"] += 1
            return _real(*a, **kw)
        monkeypatch.setattr(ops, name, spy)
    a = Engine(cfg, sd, dtype=torch.bfloat16, device=DEV, max_frames=1)
    g = torch.Generator().manual_seed(6)
    x = (torch.randn(300, 256, generator=g) * 0.5).bfloat16().to(DEV)
    la = a.llm_forward(x.clone(), 0).clone()
    ha, kva = a.last_hidden().clone(), a.kv[0][:300].clone()
    tok = torch.zeros(1, 256, dtype=torch.bfloat16, device=DEV)
    tok[0] = x[5]
    a.decode_forward(tok.clone(), 300)
    assert calls["n"] == 0 and not a.llm_quant and a.ws.l_q8 is None and all("wqkv4" not in L and "wqkv8" not in L for L in a.l_layers)
    b = Engine(cfg, sd, dtype=torch.bfloat16, device=DEV, max_frames=1, llm_fp4=True)
    assert calls["n"] == 2 * 4                                   # four weight matrices per layer, quantised once
    for L in b.l_layers:                                         # ... and their 16-bit copies dropped: the layers hold codes + exponents only
        assert not any(k in L for k in ("wqkv", "wo", "wgu", "wd"))
        assert all(L[k + "4"][0].dtype == torch.uint8 and L[k + "4"][1].dtype == torch.uint8 for k in ("wqkv", "wo", "wgu", "wd"))
    bytes16 = sum(L[k].numel() * 2 for L in a.l_layers for k in ("wqkv", "wo", "wgu", "wd"))
    bytes4 = sum(t.numel() for L in b.l_layers for k in ("wqkv", "wo", "wgu", "wd") for t in L[k + "4"])
    assert abs(bytes4 / bytes16 - 4.25 / 16) < 1e-9                # 4.25 bits per weight against 16
    lb = b.llm_forward(x.clone(), 0).clone()
    assert calls["n"] == 2 * 4 + 2 * 4                           # four GEMMs per layer
    assert torch.isfinite(lb).all()
    rel = lambda u, v: ((u.float() - v.float()).norm() / v.float().norm()).item()      # noqa: E731
    print(f"kv {rel(b.kv[0][:300], kva):.4f} hidden {rel(b.last_hidden(), ha):.4f} logits {rel(lb, la):.4f}")
    assert rel(b.kv[0][:300], kva) < 2 * PER_GEMM_REL
    assert rel(b.last_hidden(), ha) < 2 * PER_GEMM_REL
    lb2 = b.decode_forward(tok, 300)                             # W4A16 decode against the cache the W4A8 prefill built
    assert calls["n"] == 2 * 4 + 2 * 4 + 2 * 4
    assert torch.isfinite(lb2).all()
    assert not hasattr(b, "l_head8") and b.l_head.dtype == torch.bfloat16      # the LM head stays 16-bit


def test_engine_fp4_short_prefill_and_wide_decode_group_run_on_the_codes():
    """With the 16-bit copies gone, a prefill of up to 8 rows runs through the W4A16 decode linears: its K/V rows and last hidden state
    are those of the W4A8 prefill of the same rows up to the activation precision (bound: the 2 x per-GEMM figure, as above).  The test
    model's intermediate size is 384 (K % 256 == 128 for the down projection: VALU form, 4 rows per launch), so a decode group of 9
    rows also checks the engine's 4-row launches: row m's residual stream after the layers (every MXFP4 linear has run on it) is
    bit-equal to the same scene decoded in a group of 2."""
    from v3d.engine import Engine, random_state_dict
    cfg = _tiny()
    sd = random_state_dict(cfg, torch.float32, "cpu", seed=5, std=0.05)
    eng = Engine(cfg, sd, dtype=torch.bfloat16, device=DEV, max_frames=1, llm_fp4=True)
    g = torch.Generator().manual_seed(6)
    x = (torch.randn(12, 256, generator=g) * 0.5).bfloat16().to(DEV)
    rel = lambda u, v: ((u.float() - v.float()).norm() / v.float().norm()).item()      # noqa: E731
    long_logits = eng.llm_forward(x.clone(), 0).clone()           # 12 rows: W4A8 GEMMs
    kv_long = eng.kv[1][:7].clone()                               # last layer's K/V rows: everything below them took part
    eng.llm_forward(x[:7].clone(), 0)                             # 7 rows: W4A16 decode linears (causality: the same rows 0..6)
    assert torch.isfinite(eng.kv[1][:7]).all() and torch.isfinite(long_logits).all()
    print(f"short-vs-long prefill kv {rel(eng.kv[1][:7], kv_long):.4f}")
    assert rel(eng.kv[1][:7], kv_long) < 2 * PER_GEMM_REL
    ctxs = [eng.new_context() for _ in range(9)]
    for c in ctxs:                                                # the same 9 prompt rows everywhere; the new tokens differ
        eng.use(c)
        eng.llm_forward(x[:9].clone(), 0, head=False)
    grp = eng.new_group(9)
    grp.x[:9].copy_(x[:9])
    all9 = eng.decode_forward_rows(grp, ctxs, [9] * 9).clone()
    assert torch.isfinite(all9).all() and torch.isfinite(grp.x[:9]).all()
    pair = eng.new_group(2)
    pair.x[:2].copy_(x[6:8])
    for c in ctxs[6:8]:
        c.kv_len = 9
    two = eng.decode_forward_rows(pair, ctxs[6:8], [9, 9])
    assert torch.equal(pair.x[:2], grp.x[6:8])
    assert torch.isfinite(two).all()


def test_engine_fp8_and_fp4_are_exclusive():
    from v3d._native import V3DError
    from v3d.engine import Engine, random_state_dict
    cfg = _tiny()
    sd = random_state_dict(cfg, torch.float32, "cpu", seed=5, std=0.05)
    with pytest.raises(V3DError, match="exclusive"):
        Engine(cfg, sd, dtype=torch.bfloat16, device=DEV, max_frames=1, llm_fp8=True, llm_fp4=True)


def test_engine_fp4_answer_group_returns_generates_tokens():
    """After prefill_scene, answer_group of four questions returns the tokens generate() gives for [prefix | question] on the same
    MXFP4 engine, unless generate()'s own top-2 logit margin at the first differing step is inside the rounding noise (the batched
    rows and the group decode sum in another f32 order) - the excuse of tests/test_gpu_engine.py, same threshold."""
    from oracle import pipeline_oracle as PO
    from v3d.engine import Engine, random_state_dict
    cfg = _tiny(layers_vit=2)
    sd = random_state_dict(cfg, torch.float32, "cpu", seed=35, std=0.08)
    eng = Engine(cfg, sd, dtype=torch.bfloat16, device=DEV, max_frames=2, llm_fp4=True)
    g = torch.Generator().manual_seed(36)
    images = torch.randn(2, 3, 384, 384, generator=g).cuda()
    coords = ((torch.rand(2, 384, 384, 3, generator=g) - 0.5) * 20).cuda()
    prefix = torch.cat([torch.randint(0, 320, (14,), generator=g), torch.tensor([PO.IMAGE_TOKEN_INDEX])])
    questions = [torch.randint(0, 320, (n,), generator=g) for n in (60, 17, 33, 9)]
    steps = 6
    alone, margins = [], []
    for qs in questions:                                          # generate()'s launches, keeping each step's top-2 margin
        ids = torch.cat([prefix, qs])
        c = eng.use(eng.new_context())
        x = eng.build_inputs_embeds(ids, eng.encode_images(images), eng.voxel_ids(coords.to(eng.dtype)))
        S = x.shape[0]
        logits = eng.llm_forward(x, 0, last_rows=[S - 1])
        toks, mg = [], []
        for st in range(steps):
            top2 = torch.topk(logits.float(), 2).values
            mg.append(((top2[0] - top2[1]) / logits.float().abs().max()).item())
            tok = torch.zeros(1, dtype=torch.int64, device=DEV)
            ops.argmax(logits, tok)
            toks.append(int(tok))
            if st + 1 < steps:
                xe = ops.embed_gather(eng.embed, tok, out=c.l_x[S + st: S + st + 1])
                logits = eng.decode_forward(xe, S + st)
        assert eng.generate(ids, images, coords, max_new_tokens=steps).tolist() == toks
        alone.append(toks)
        margins.append(mg)
    eng.use(eng.new_context())
    eng.prefill_scene(prefix, images, coords)
    together = eng.answer_group(questions, max_new_tokens=steps)
    for gi in range(len(questions)):
        got = together[gi].tolist()
        assert len(got) == steps
        for st in range(steps):
            if got[st] != alone[gi][st]:
                assert margins[gi][st] < 0.02, (gi, st, got, alone[gi], margins[gi][st])
                break
