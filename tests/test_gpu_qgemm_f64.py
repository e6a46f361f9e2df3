"""v3d_gemm_fp8 and v3d_gemm_mxfp4 (q8_gemm_tile) against the host model of tests/qgemm_check.py: bit for bit on the gather and exact
families, within the per-element bound (no rms term) on the random family - both formats x bf16 / f16 x NONE / BIAS / RES / SWIGLU.

Shapes: the smallest at which each mechanism of the tile is live.
    1 x 256 x 128                one row; one K-step (the prefetch branch is never taken)
    255, 256, 257 x 256 x 384    the tile edge; three K-steps (the last one sits in buffer 0)
    130 x 768 x 256              rows across the 128-row wave boundary; three n-tiles (SwiGLU output of 384 columns)
    2305 x 512 x 256             ten m-tiles with a short last group, 20 workgroups (XCD remainder), a one-row tail
    300 x 256 x 18944            the longest K of the product (148 steps): exact family with narrowed amplitude, and random
Strided (M = 257, 2305): lda = K + 128, ldw = K + 16 / K / 2 + 16, lde = K / 32 + 3, ldr = N + 24, ldo = n_out + 8, the output a view
inside a sentinel-filled buffer, and once more with the residual in place (res is out), as a decoder layer calls it.
Every case runs twice and must repeat bit for bit.  The proof that these checks see a wrong kernel is tests/test_qgemm_check_cpu.py.

MEASURED: tests/qgemm_check.py (module docstring) and DESIGN.md section 2.
"""
import json

import pytest
import torch

import qgemm_check as qc
from qgemm_check import EPI_BIAS, EPI_NONE, EPI_RES, EPI_SWIGLU
from v3d import _native, ops

pytestmark = pytest.mark.gpu

DEV = "cuda"
DT = {"bf16": torch.bfloat16, "f16": torch.float16}
SHAPES = [(1, 256, 128), (255, 256, 384), (256, 256, 384), (257, 256, 384), (130, 768, 256), (2305, 512, 256), (300, 256, 18944)]
STRIDED = [(257, 256, 384), (2305, 512, 256)]
WORST = {}

each = lambda f: pytest.mark.parametrize("epi", qc.EPIS, ids=lambda e: qc.EPI_NAMES[e])(
    pytest.mark.parametrize("dt", sorted(DT))(pytest.mark.parametrize("fmt", qc.FORMATS)(f)))


def run_twice(c, dt, epi, **kw):
    got = qc.run(ops, c, dt, epi, **kw).clone()
    again = qc.run(ops, c, dt, epi, **kw)
    assert torch.equal(got.view(torch.int16), again.view(torch.int16)), "two runs of one case differ"
    return got


def bit_exact(got, c, dt, epi, what, exact=False):
    r = qc.compare(got, c, dt, epi, exact=exact)
    if epi == EPI_SWIGLU:
        assert r["outside"] == 0, f"{what}: {r}"
    else:
        assert r["unequal"] == 0, f"{what}: {r}" + ("\n" + qc.gather_explain(got, c) if epi == EPI_NONE and not exact else "")
    return r


@each
@pytest.mark.parametrize("M,N,K", SHAPES[:-1])
def test_gather(fmt, dt, epi, M, N, K):
    """One product per output: the element read, its scales, its block exponent, exactly - in both directions."""
    for transposed in (False, True):
        c = qc.gather_inputs(fmt, M, N, K, DT[dt], stride=37, shift=5, device=DEV, transposed=transposed)
        bit_exact(run_twice(c, DT[dt], epi), c, DT[dt], epi, f"gather{'_t' if transposed else ''} {fmt} {M}x{N}x{K}")


@pytest.mark.parametrize("dt", sorted(DT))
def test_gather_exponent_walk(dt):
    """MXFP4: every exponent byte in 103..151 and the edges 0, 1, 254 inside the MFMA's scale operand."""
    c = qc.gather_exponent_walk(256, 256, 1792, DT[dt], device=DEV)
    bit_exact(run_twice(c, DT[dt], EPI_NONE), c, DT[dt], EPI_NONE, "exponent walk")


@each
@pytest.mark.parametrize("M,N,K", SHAPES)
def test_exact(fmt, dt, epi, M, N, K):
    """Every product and every partial sum an exact f32 number: one bit pattern per element, whatever the order of the sum."""
    c = qc.exact_inputs(fmt, M, N, K, DT[dt], epi, seed=M + K, device=DEV)
    r = bit_exact(run_twice(c, DT[dt], epi), c, DT[dt], epi, f"exact {fmt} {M}x{N}x{K}", exact=True)
    assert r["needs_rounding"] > 0.5, r


@each
@pytest.mark.parametrize("M,N,K", SHAPES)
def test_random(fmt, dt, epi, M, N, K):
    """Every finite byte and code, and Gaussians through the project's quantisers, with arbitrary f32 scales: inside the bound."""
    for draw in (0, 1):
        c = qc.random_inputs(fmt, M, N, K, DT[dt], draw=draw, seed=M + K, device=DEV, ops=ops)
        r = qc.compare(run_twice(c, DT[dt], epi), c, DT[dt], epi)
        key = f"{fmt} {qc.EPI_NAMES[epi]}"
        WORST[key] = max(WORST.get(key, 0.0), r["ratio"])
        print(f"random{draw} {fmt} {dt} {qc.EPI_NAMES[epi]} {M}x{N}x{K}: ratio {r['ratio']:.3f}")
        assert r["ratio"] <= 1.0, r


@each
@pytest.mark.parametrize("M,N,K", STRIDED)
def test_strided_and_in_place(fmt, dt, epi, M, N, K):
    """Every leading dimension larger than the row, the output inside a sentinel-filled buffer; RES once more with res = out."""
    for family in ("exact", "gather"):
        c = (qc.exact_inputs(fmt, M, N, K, DT[dt], epi, seed=M + K, device=DEV) if family == "exact" else
             qc.gather_inputs(fmt, M, N, K, DT[dt], stride=37, shift=5, device=DEV))
        v, out, buf = qc.strided(c, epi, DT[dt])
        assert v.qa.stride(0) == K + 128 and v.w.stride(0) == c.w.shape[1] + 16 and v.res.stride(0) == N + 24 and out.stride(0) == out.shape[1] + 8
        assert fmt == "e4m3" or v.wx.stride(0) == K // 32 + 3
        run_twice(v, DT[dt], epi, out=out)
        bit_exact(out, c, DT[dt], epi, f"strided {family} {fmt} {M}x{N}x{K}", exact=family == "exact")
        assert bool((buf[M] == -7.0).all()) and bool((buf[:, out.shape[1]:] == -7.0).all()), "a store went outside the output view"
        if epi == EPI_RES:
            buf.fill_(-7.0)
            out.copy_(c.res)
            qc.run(ops, v, DT[dt], epi, out=out, res=out)
            bit_exact(out, c, DT[dt], epi, f"in place {family} {fmt} {M}x{N}x{K}", exact=family == "exact")
            assert bool((buf[M] == -7.0).all()) and bool((buf[:, out.shape[1]:] == -7.0).all())


@pytest.mark.parametrize("fmt", qc.FORMATS)
def test_nan_bytes_stay_in_their_row_and_column(fmt):
    """A NaN byte at one (m, k) of A and at one (n, k) of the e4m3 W: exactly row m and column n are NaN, the rest is unchanged."""
    M, N, K, dt = 257, 256, 384, torch.bfloat16
    c = qc.exact_inputs(fmt, M, N, K, dt, EPI_NONE, seed=1, device=DEV)
    clean = qc.run(ops, c, dt, EPI_NONE)
    m0, n0 = 130, 77
    qa = c.qa.clone()
    qa[m0, 200] = 0x7F
    w = c.w.clone()
    if fmt == "e4m3":
        w[n0, 5] = 0xFF
    got = qc.run(ops, c._replace(qa=qa, w=w), dt, EPI_NONE)
    want_nan = torch.zeros(M, N, dtype=torch.bool, device=DEV)
    want_nan[m0] = True
    if fmt == "e4m3":
        want_nan[:, n0] = True
    assert torch.equal(torch.isnan(got), want_nan)
    assert torch.equal(got[~want_nan], clean[~want_nan])


def test_refusals_are_errors_not_launches():
    dt = torch.bfloat16
    qa = torch.zeros(8, 256, dtype=torch.uint8, device=DEV)
    sa = torch.ones(8, device=DEV)
    qw = torch.zeros(256, 256, dtype=torch.uint8, device=DEV)
    sw = torch.ones(256, device=DEV)
    q4 = torch.zeros(256, 128, dtype=torch.uint8, device=DEV)
    e4 = torch.full((256, 8), 127, dtype=torch.uint8, device=DEV)
    out = torch.empty(8, 256, dtype=dt, device=DEV)
    ops.gemm_fp8(qa, sa, qw, sw, dt, out=out)
    ops.gemm_mxfp4(qa, sa, q4, e4, dt, out=out)
    calls = {"e4m3": lambda **kw: ops.gemm_fp8(kw.pop("qa", qa), sa, qw, sw, dt, **kw),
             "mxfp4": lambda **kw: ops.gemm_mxfp4(kw.pop("qa", qa), sa, q4, kw.pop("e", e4), dt, **kw)}
    for fmt, call in calls.items():
        with pytest.raises(_native.V3DError, match="leading dimensions"):
            call(qa=qa.as_strided((8, 256), (128, 1)))                        # lda < K
        with pytest.raises(_native.V3DError, match="leading dimensions"):
            call(out=torch.empty(8, 260, dtype=dt, device=DEV)[:, :256])      # ldo % 8 != 0
        with pytest.raises(_native.V3DError, match="bias epilogue without bias"):
            call(epilogue=EPI_BIAS)
        with pytest.raises(_native.V3DError, match="residual epilogue without residual"):
            call(epilogue=EPI_RES)
    with pytest.raises(_native.V3DError, match="leading dimensions"):
        calls["mxfp4"](e=e4.as_strided((256, 8), (4, 1)))                     # lde < K / 32
    # an operand of 2^31 bytes, by the shape arguments alone (the checks run before any device call): M lda, N ldw
    lib = _native.lib()
    p = lambda t: t.data_ptr()
    big = 1 << 16
    rc = lib.v3d_gemm_fp8(p(qa), big, p(sa), p(qw), 256, p(sw), None, None, 0, p(out), 256, 1 << 15, 256, 256, ops._DT[dt], EPI_NONE, None)
    assert rc < 0 and b"2 GiB" in lib.v3d_last_error()
    rc = lib.v3d_gemm_fp8(p(qa), 256, p(sa), p(qw), 1 << 23, p(sw), None, None, 0, p(out), 256, 8, 256, 256, ops._DT[dt], EPI_NONE, None)
    assert rc < 0 and b"2 GiB" in lib.v3d_last_error()
    rc = lib.v3d_gemm_mxfp4(p(qa), big, p(sa), p(q4), 128, p(e4), 8, None, None, 0, p(out), 256, 1 << 15, 256, 256, ops._DT[dt], EPI_NONE, None)
    assert rc < 0 and b"2 GiB" in lib.v3d_last_error()
    rc = lib.v3d_gemm_mxfp4(p(qa), 256, p(sa), p(q4), 1 << 23, p(e4), 8, None, None, 0, p(out), 256, 8, 256, 256, ops._DT[dt], EPI_NONE, None)
    assert rc < 0 and b"2 GiB" in lib.v3d_last_error()
    torch.cuda.synchronize()


def test_zz_report_worst_ratios():
    """Worst |err| / bound on the random family per format and epilogue seen in this run."""
    print("QGEMM_WORST " + json.dumps({k: round(v, 3) for k, v in sorted(WORST.items())}))
    assert all(v <= 1.0 for v in WORST.values())
