"""GPU tests of csrc/pe_mlp.hip: the hidden kernel of PositionEmbeddingMLP, its PE rows on v3d_gemm, the fused visual-token kernel that
reads PE rows, and the backward pieces - against the f64 references and per-element bounds of tests/pe_mlp_check.py (settled on the CPU
in tests/test_pe_mlp_check_cpu.py), tests/rowwise_check.py and tests/gemm_check.py.  Outputs start as NaN and sit between NaN border
rows / columns: afterwards everything that should be written is inside the bound and the borders are still NaN."""
import pytest
import torch

import gemm_check as GC
import pe_mlp_check as MC
import rowwise_check as RC

pytestmark = pytest.mark.gpu
NAN = float("nan")
KINDS = ["f16", "bf16"]


@pytest.fixture(scope="module")
def ops():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    from v3d import ops as _ops
    return _ops


def cuda(p):
    return {k: v.cuda() for k, v in p.items()}


def mixed_inputs(kind, N):
    """integer-valued rows (ids above 256 included) and continuous rows (negative ones included), interleaved."""
    a, b = MC.seeded_inputs(kind, "ids", N), MC.seeded_inputs(kind, "cont", N)
    x = a.clone()
    x[1::2] = b[1::2]
    return x.cuda()


def call_hidden(ops, x, p, want_z=True):
    """v3d_pe_mlp_hidden through the C interface into rows 1 .. N of NaN-filled [N + 2, 512] buffers -> (z, h, borders intact)."""
    N = x.shape[0]
    hb = torch.full((N + 2, MC.HIDDEN), NAN, dtype=x.dtype, device="cuda")
    zb = torch.full((N + 2, MC.HIDDEN), NAN, dtype=x.dtype, device="cuda") if want_z else None
    z = zb[1:N + 1] if want_z else None
    ops.check(ops.lib().v3d_pe_mlp_hidden(ops._p(x), ops._p(p["w0"]), ops._p(p["b0"]), ops._p(p["ln_w"]), ops._p(p["ln_b"]), MC.EPS, N, MC.HIDDEN,
                                          ops._code(x), ops._p(z), ops._p(hb[1:N + 1]), ops._stream()), "v3d_pe_mlp_hidden")
    clean = bool(torch.isnan(hb[[0, N + 1]]).all()) and (not want_z or bool(torch.isnan(zb[[0, N + 1]]).all()))
    return z, hb[1:N + 1], clean


# ------------------------------------------------------------------------------ the hidden kernel


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("N", [1, 7, 64, 65, 393])
def test_hidden_kernel_against_f64(ops, N, kind):
    p, x = cuda(MC.seeded_mlp(256, kind)), mixed_inputs(kind, N)
    z, h, clean = call_hidden(ops, x, p)
    assert clean, "border rows written"
    rz = RC.ratio(z, MC.z_reference(x, p))
    rh = RC.ratio(h, MC.h_reference(z, p))                  # centred on the kernel's own z
    print(f"N={N} {kind}: worst |err| / bound  z {rz:.3f}  h {rh:.3f}")
    assert rz <= 1.0, (rz, RC.worst_index(z, MC.z_reference(x, p)))
    assert rh <= 1.0, (rh, RC.worst_index(h, MC.h_reference(z, p)))
    assert bool((h >= 0).all())
    # the optional z changes nothing, and the wrapper gives the same bits
    _, h2, clean2 = call_hidden(ops, x, p, want_z=False)
    assert clean2 and torch.equal(h2, h)
    zw, hw = ops.pe_mlp_hidden(x, p["w0"], p["b0"], p["ln_w"], p["ln_b"], MC.EPS, want_z=True)
    assert torch.equal(zw, z) and torch.equal(hw, h)
    # the kernel follows the rule: its stages are the CPU restatement's up to rounding flips (below 1 % of the elements, one ulp)
    sz, sh, _ = MC.restate(x.cpu(), {k: v.cpu() for k, v in p.items()}, stages=True)
    for got, want in ((z, sz), (h, sh)):
        share, worst = MC.ulp_shares(got.cpu(), MC.bits(want))
        assert share <= 0.01 and worst <= 1, (share, worst)


@pytest.mark.parametrize("kind", KINDS)
def test_hidden_kernel_nan_row_stays_in_its_row(ops, kind):
    N = 65
    p, x = cuda(MC.seeded_mlp(256, kind)), mixed_inputs(kind, N)
    z0, h0, _ = call_hidden(ops, x, p)
    z0, h0 = z0.clone(), h0.clone()
    xn = x.clone()
    xn[33, 1] = NAN
    z1, h1, clean = call_hidden(ops, xn, p)
    assert clean
    keep = [r for r in range(N) if r != 33]
    assert torch.equal(z1[keep], z0[keep]) and torch.equal(h1[keep], h0[keep])
    assert bool(torch.isnan(z1[33]).all()) and bool(torch.isnan(h1[33]).all())      # a NaN PE row, as in the reference


def test_hidden_kernel_refuses_other_widths(ops):
    from v3d._native import V3DError
    x = torch.zeros((4, 3), dtype=torch.bfloat16, device="cuda")
    w = torch.zeros((256, 3), dtype=torch.bfloat16, device="cuda")
    v = torch.zeros(256, dtype=torch.bfloat16, device="cuda")
    with pytest.raises(V3DError, match="512"):
        ops.pe_mlp_hidden(x, w, v, v, v)
    lib = ops.lib()
    assert lib.v3d_pe_mlp_hidden(None, None, None, None, None, 1e-5, 1, 512, ops.BF16, None, None, None) < 0
    assert lib.v3d_pe_mlp_hidden(ops._p(x), ops._p(w), ops._p(v), ops._p(v), ops._p(v), 1e-5, 0, 512, ops.BF16, None, ops._p(w), None) < 0     # N = 0
    assert lib.v3d_pe_mlp_hidden(ops._p(x), ops._p(w), ops._p(v), ops._p(v), ops._p(v), 1e-5, 4, 512, ops.F32, None, ops._p(w), None) < 0      # f32


# ------------------------------------------------------------------------------ the PE rows (the second Linear on v3d_gemm)


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("E", [256, 3584])
def test_pe_rows_on_the_gemm(ops, E, kind):
    p = cuda(MC.seeded_mlp(E, kind, b3_offset=0.0))
    for M in (1, 50, 393):
        x = mixed_inputs(kind, M)
        h = ops.pe_mlp_hidden(x, p["w0"], p["b0"], p["ln_w"], p["ln_b"], MC.EPS)
        pe = ops.pe_mlp(x, p)
        assert torch.equal(pe, ops.gemm(h, p["w3"], bias=p["b3"], epilogue=ops.EPI_BIAS))
        c = GC.compare(pe, h, p["w3"], p["b3"], epi=GC.EPI_BIAS)             # on the kernel's own h
        print(f"E={E} M={M} {kind}: worst |err| / bound {c['ratio']:.3f}")
        assert c["ratio"] <= 1.0


def test_pe_mlp_into_the_callers_buffers(ops):
    """out / h_out (the engine's preallocated rows): the same bits in the first N rows, nothing behind them."""
    p, x = cuda(MC.seeded_mlp(256, "bf16")), mixed_inputs("bf16", 393)
    hb = torch.full((400, MC.HIDDEN), NAN, dtype=torch.bfloat16, device="cuda")
    ob = torch.full((400, 256), NAN, dtype=torch.bfloat16, device="cuda")
    pe = ops.pe_mlp(x, p, out=ob, h_out=hb)
    assert pe.data_ptr() == ob.data_ptr() and tuple(pe.shape) == (393, 256) and torch.equal(pe, ops.pe_mlp(x, p))
    assert torch.equal(hb[:393], ops.pe_mlp_hidden(x, p["w0"], p["b0"], p["ln_w"], p["ln_b"], MC.EPS))
    assert bool(torch.isnan(hb[393:]).all()) and bool(torch.isnan(ob[393:]).all())
    from v3d._native import V3DError
    with pytest.raises(V3DError):
        ops.pe_mlp(x, p, out=ob[:100], h_out=hb)
    with pytest.raises(V3DError):
        ops.pe_mlp(x, p, out=ob, h_out=hb[:100])


# ------------------------------------------------------------------------------ the fused kernel with PE rows


def add16(a, b):
    """T(a + b) for 16-bit a, b: the sum of two 16-bit values is exact in f32, one rounding."""
    return (a.float() + b.float()).to(a.dtype)


def rows_case(ops, V, C, kind, side=27, n=14, out_pad=24, pe_pad=8):
    dt = MC.DT[kind]
    g = torch.Generator().manual_seed(V * 1000 + C)
    feat = torch.randn(V, side * side, C, generator=g).to(dt).cuda()
    newline = torch.randn(C, generator=g).to(dt).cuda()
    pe_big = torch.full((V * n * n, C + pe_pad), NAN, dtype=dt, device="cuda")
    pe_big[:, :C] = torch.randn(V * n * n, C, generator=g).to(dt).cuda()
    pe = pe_big[:, :C]
    rows = V * n * (n + 1)
    big = torch.full((rows + 2, C + out_pad), NAN, dtype=dt, device="cuda")
    out = ops.visual_tokens_rows(feat, pe, newline, side=side, n=n, pool=True, out=big[1:rows + 1, :C])
    assert bool(torch.isnan(big[[0, rows + 1]]).all()) and bool(torch.isnan(big[:, C:]).all()), "borders written"
    pooled = ops.visual_tokens(feat, side=side, n=n, pool=True).view(V, n, n, C)          # pool only
    want = torch.empty((V, n, n + 1, C), dtype=dt, device="cuda")
    want[:, :, :n] = add16(pooled, pe.reshape(V, n, n, C))
    want[:, :, n] = newline
    assert torch.equal(out, want.view(rows, C))
    return feat, pe, newline, out


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("C", [256, 3584])
def test_visual_tokens_rows_bit_equal(ops, C, kind):
    """bit-equal to ops.visual_tokens(pool only) followed by a 16-bit add of the same rows, newline rows in place; out_stride > C, pe
    stride > C, NaN borders."""
    feat, pe, newline, out = rows_case(ops, 2, C, kind)
    # without the newline rows, and without the pool (n * n input tokens)
    no_nl = ops.visual_tokens_rows(feat, pe, None, pool=True)
    assert torch.equal(no_nl.view(2, 14, 14, C), out.view(2, 14, 15, C)[:, :, :14])
    f14 = feat[:, :196].contiguous()
    flat = ops.visual_tokens_rows(f14, pe, newline, pool=False)
    assert torch.equal(flat.view(2, 14, 15, C)[:, :, :14], add16(f14.view(2, 14, 14, C), pe.reshape(2, 14, 14, C)))


def test_visual_tokens_rows_32_frames(ops):
    rows_case(ops, 32, 3584, "bf16")


def test_visual_tokens_rows_refuses_bad_arguments(ops):
    from v3d._native import V3DError
    feat = torch.zeros((2, 729, 256), dtype=torch.float16, device="cuda")
    pe = torch.zeros((2 * 196, 256), dtype=torch.float16, device="cuda")
    with pytest.raises(V3DError, match="pe must be"):
        ops.visual_tokens_rows(feat, pe[:100])
    with pytest.raises(V3DError, match="pe must be"):
        ops.visual_tokens_rows(feat, pe.bfloat16())
    lib = ops.lib()
    a = (ops._p(feat), ops._p(pe))
    assert lib.v3d_visual_tokens_rows(*a, 252, None, ops._p(pe), 256, ops.F16, 2, 27, 14, 256, 3, None) < 0        # pe_stride < C
    assert lib.v3d_visual_tokens_rows(*a, 256, None, ops._p(pe), 256, ops.F16, 2, 27, 14, 256, 7, None) < 0        # NEWLINE without a row
    assert lib.v3d_visual_tokens_rows(*a, 256, None, ops._p(pe), 256, ops.F32, 2, 27, 14, 256, 3, None) < 0        # 16-bit only
    assert lib.v3d_visual_tokens_rows(*a, 256, None, ops._p(pe), 256, ops.F16, 2, 27, 14, 256, 11, None) < 0       # CONTINUOUS is not a flag here


# ------------------------------------------------------------------------------ backward pieces


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("C", [256, 3584])
def test_visual_tokens_rows_grad(ops, C, kind):
    """dfeat and dnewline bit-equal to v3d_visual_tokens_grad, dpe an exact copy of the non-newline rows."""
    V, n, dt = 2, 14, MC.DT[kind]
    g = torch.Generator().manual_seed(C)
    big = torch.full((V * n * (n + 1), C + 16), NAN, dtype=dt, device="cuda")
    big[:, :C] = torch.randn(V * n * (n + 1), C, generator=g).to(dt).cuda()
    dout = big[:, :C]
    dfeat0, dnl0 = ops.visual_tokens_grad(dout, V)
    dfeat, dnl, dpe = ops.visual_tokens_rows_grad(dout, V)
    assert torch.equal(dfeat, dfeat0) and torch.equal(dnl, dnl0)
    assert tuple(dpe.shape) == (V * n * n, C) and torch.equal(dpe.view(V, n, n, C), dout.reshape(V, n, n + 1, C)[:, :, :n])
    dfeat1, dnl1, dpe1 = ops.visual_tokens_rows_grad(dout[: V * n * n].contiguous(), V, newline=False)
    assert dnl1 is None and torch.equal(dpe1, dout[: V * n * n])
    assert torch.equal(dfeat1, ops.visual_tokens_grad(dout[: V * n * n].contiguous(), V, newline=False)[0])


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("rows", [1, 33, 393 + 1 + 6])
def test_first_linear_gradients(ops, rows, kind):
    """dw0 (v3d_pe_mlp_wgrad) and db0 (v3d_colsum) against f64 within a colsum_chain-style bound on sum |dz x|; two runs bit-identical; an
    integer-valued case is bit-exact, so a dropped row or partial would move the result by an integer."""
    dt = MC.DT[kind]
    g = torch.Generator().manual_seed(rows)
    big = torch.full((rows, MC.HIDDEN + 8), NAN, dtype=dt, device="cuda")
    big[:, :MC.HIDDEN] = torch.randn(rows, MC.HIDDEN, generator=g).to(dt).cuda()
    dz, x = big[:, :MC.HIDDEN], mixed_inputs(kind, rows)
    for out_dtype in (None, torch.float32):
        dw = ops.pe_mlp_wgrad(dz, x, dtype=out_dtype)
        assert tuple(dw.shape) == (MC.HIDDEN, 3) and torch.equal(dw, ops.pe_mlp_wgrad(dz, x, dtype=out_dtype))
        r = RC.ratio(dw, MC.wgrad_reference(dz, x, out_dtype))
        db = ops.colsum(dz, dtype=out_dtype)
        rb = RC.ratio(db, MC.colsum_reference(dz, out_dtype))
        print(f"rows={rows} {kind} out={out_dtype}: worst |err| / bound  dw0 {r:.3f}  db0 {rb:.3f}")
        assert r <= 1.0 and rb <= 1.0
    # integers: every product and partial sum is exact
    dzi = torch.randint(-3, 4, (rows, MC.HIDDEN), generator=g).to(dt).cuda() + (torch.arange(MC.HIDDEN) % 5).to(dt).cuda()
    xi = (torch.randint(0, 8, (rows, 3), generator=g) + torch.arange(rows)[:, None] % 3).to(dt).cuda()
    want = dzi.double().T @ xi.double()
    assert torch.equal(ops.pe_mlp_wgrad(dzi, xi, dtype=torch.float32).double(), want)
    assert torch.equal(ops.colsum(dzi, dtype=torch.float32).double(), dzi.double().sum(0))


def test_wgrad_refuses_bad_arguments(ops):
    from v3d._native import V3DError
    dz = torch.zeros((8, 256), dtype=torch.bfloat16, device="cuda")
    x = torch.zeros((8, 3), dtype=torch.bfloat16, device="cuda")
    with pytest.raises(V3DError, match="512"):
        ops.pe_mlp_wgrad(dz, x)
    with pytest.raises(V3DError, match="x must be"):
        ops.pe_mlp_wgrad(torch.zeros((8, 512), dtype=torch.bfloat16, device="cuda"), x[:4])
    assert ops.lib().v3d_pe_mlp_wgrad_workspace_bytes(400, 512) == 13 * 1536 * 4
    assert ops.lib().v3d_pe_mlp_wgrad_workspace_bytes(0, 512) == 0


@pytest.mark.parametrize("kind", KINDS)
def test_layernorm_and_relu_backward_at_512(ops, kind):
    """v3d_layernorm_grad and v3d_gelu_grad kind 2 at the module's width, within rowwise_check's bounds."""
    dt, rows, cols = MC.DT[kind], 400, MC.HIDDEN
    for family in ("random", "offset"):
        p = RC.norm_inputs(family, rows, cols, dt, seed=5, norm="ln", device="cuda")
        dx, dw, db = ops.layernorm_grad(p["x"], p["w"], p["dy"], MC.EPS, dw_dtype=torch.float32)
        ref = RC.layernorm_grad(p["x"], p["w"], p["dy"], MC.EPS, dw_dtype=torch.float32)
        for name, got in (("dx", dx), ("dw", dw), ("db", db)):
            r = RC.ratio(got, ref[name])
            print(f"layernorm_grad {family} {kind} {name}: {r:.3f}")
            assert r < 1.0, (family, name, r)
    z, dy = RC.act_random(rows, cols, dt, seed=cols, device="cuda")
    z[::7] = 0                                                              # relu'(0) = 0
    dz = ops.gelu_grad(z, dy, tanh_form=2)
    assert RC.ratio(dz, RC.gelu_grad(z, dy, 2)) == 0.0                      # exact: any difference is an error
