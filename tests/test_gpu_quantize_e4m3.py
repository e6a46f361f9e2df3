"""The quantisers that feed the quantised prefill GEMMs, bit for bit against their host restatements.

e4m3 (v3d_quantize_fp8_rows' two kernels, v3d_rmsnorm_quantize_fp8; qgemm_check.host_quantize_e4m3, pinned by hand in
tests/test_qgemm_check_cpu.py): scale = amax / 448 in IEEE f32, floored at the smallest normal f32 (2^-126), 1 for an all-zero row;
bytes = e4m3 round-to-nearest-even of x (1 / scale).
  exhaustive   every finite 16-bit pattern with |x| <= 448 2^j in rows whose amax is exactly 448 2^j: the scale is 2^j and x / scale is
               exact, so each pattern meets the conversion's rounding, subnormal range and ties with no reference arithmetic in between;
               rows of 4096 (wave-per-row kernel) and 4104 columns (workgroup-per-row kernel);
  dispatch     cols 8 / 4096 / 4104 / 32768 / 32776 (back on the wave-per-row kernel) x rows 1, 3, 4, 5 with an all-zero row, ldx > cols,
               q a view of a wider sentinel-filled buffer (as the engine's l_q8 is); a row zero-padded from 4096 to 4104 columns gives
               the same scale and bytes from the other kernel;
  fused norm   cols 8 / 520 (a partial vector slot) / 3584 / 4096 (all eight slots): more than 4 rows bit-identical to the two calls;
               rows 1..4 equal to the same rows inside a 9-row batch (one wave per row: neither the row count nor the place in the
               block of four matters); strided q;
  tiny rows    bf16 rows with amax 2^-133, 1e-37, 448 2^-126 holding zeros and both signs: amax / 448 is an f32 subnormal there and its
               reciprocal is inf; before the floor on the scale the zeros of such a row became 0 x inf = the NaN byte (127 / 255 / 255
               for [1e-37, 0, -5e-38]) and the GEMM row NaN;
  non-finite   an Inf or a NaN in one row leaves every other row alone; what the kernels do with the row itself is pinned.
MXFP4 (v3d_quantize_mxfp4_rows; tests/mxfp4_check.py): every finite f16 pattern, and every finite bf16 pattern in 2^-40 .. 2^40, as a
block element under a block maximum 2^(floor(log2 |x|) + s), s = 0..4 (codes 4 .. 6 down to the 0 / 0.5 tie); ldq / lde larger than
needed with sentinels; bf16 blocks whose amax has the exponent field 0, 1, 2 (the clamp of the exponent byte at 0).
"""
import numpy as np
import pytest
import torch

import mxfp4_check as MX
import qgemm_check as qc
from v3d import _native, ops

pytestmark = pytest.mark.gpu

DEV = "cuda"
DT = {"bf16": torch.bfloat16, "f16": torch.float16}
SENT = 0xA5


def finite_patterns(dt):
    """Every finite value of the 16-bit type, one per bit pattern."""
    v = torch.arange(-32768, 32768, dtype=torch.int32).to(torch.int16).view(dt)
    return v[torch.isfinite(v)]


def quantize_into_view(x, extra=40):
    """v3d_quantize_fp8_rows into a [rows, cols] view of a [rows + 1, cols + extra] buffer -> (q view, scale, whole buffer)."""
    rows, cols = x.shape
    buf = torch.full((rows + 1, cols + extra), SENT, dtype=torch.uint8, device=DEV)
    q, s = ops.quantize_fp8_rows(x, buf[:rows, :cols], torch.full((rows + 1,), -3.0, device=DEV)[:rows])
    return q, s, buf


def untouched(buf, rows, cols):
    return bool((buf[rows] == SENT).all()) and bool((buf[:, cols:] == SENT).all())


def check_against_host(x, q, s):
    q_ref, s_ref = qc.host_quantize_e4m3(x)
    assert np.array_equal(s.cpu().numpy().view(np.uint32), s_ref.numpy().view(np.uint32)), (s.cpu(), s_ref)
    bad = (q.cpu() != q_ref).nonzero()
    assert bad.numel() == 0, (f"{bad.shape[0]} bytes differ, first at {bad[0].tolist()}: x = {x[tuple(bad[0])].item()!r}, "
                              f"got {q[tuple(bad[0])].item():#x} want {q_ref[tuple(bad[0])].item():#x}")


@pytest.mark.parametrize("dt,j", [("f16", -6), ("f16", 0), ("f16", 7), ("bf16", -100), ("bf16", -20), ("bf16", 0), ("bf16", 100)])
@pytest.mark.parametrize("cols", [4096, 4104])
def test_every_pattern_under_a_power_of_two_scale(dt, j, cols):
    top = 448.0 * 2.0 ** j
    v = finite_patterns(DT[dt])
    v = v[v.double().abs() <= top]
    per = cols - 8                                               # first vector of a row: the amax and seven zeros
    rows = -(-v.numel() // per)
    x = torch.zeros(rows, cols, dtype=DT[dt])
    x[:, 0] = top
    body = torch.zeros(rows * per, dtype=DT[dt])
    body[:v.numel()] = v
    x[:, 8:] = body.reshape(rows, per)
    assert x[:, 0].double().tolist() == [top] * rows             # 448 2^j is a number of the type
    x = x.to(DEV)
    q, s, buf = quantize_into_view(x)
    assert bool((s == 2.0 ** j).all())
    check_against_host(x, q, s)
    assert untouched(buf, rows, cols)


def gaussian_rows(rows, cols, dt, seed, ldx_extra=16):
    wide = qc.gaussian(rows, cols + ldx_extra, dt, seed).to(DEV)
    return wide[:, :cols]


@pytest.mark.parametrize("dt", sorted(DT))
@pytest.mark.parametrize("rows", [1, 3, 4, 5])
@pytest.mark.parametrize("cols", [8, 4096, 4104, 32768, 32776])
def test_dispatch_edges_and_strides(dt, rows, cols):
    x = gaussian_rows(rows, cols, DT[dt], rows * 7 + cols)
    if rows > 1:
        x[rows - 2] = 0
    assert x.stride(0) > cols
    q, s, buf = quantize_into_view(x)
    check_against_host(x, q, s)
    assert untouched(buf, rows, cols)
    if rows > 1:
        assert s[rows - 2].item() == 1.0 and int(q[rows - 2].max()) == 0


@pytest.mark.parametrize("dt", sorted(DT))
def test_zero_padded_row_is_the_same_from_both_kernels(dt):
    x = gaussian_rows(5, 4096, DT[dt], 3)
    padded = torch.zeros(5, 4104, dtype=DT[dt], device=DEV)
    padded[:, :4096] = x
    q, s = ops.quantize_fp8_rows(x.contiguous())
    qp, sp = ops.quantize_fp8_rows(padded)
    assert torch.equal(s, sp) and torch.equal(q, qp[:, :4096]) and int(qp[:, 4096:].max()) == 0


@pytest.mark.parametrize("dt", sorted(DT))
@pytest.mark.parametrize("cols", [8, 520, 3584, 4096])
def test_fused_norm_rows_and_strides(dt, cols):
    x = gaussian_rows(9, cols, DT[dt], cols)
    w = (1 + 0.1 * qc.gaussian(1, cols, DT[dt], 3, outlier=False)[0]).to(DT[dt]).to(DEV)
    h = ops.rmsnorm(x, w, 1e-6)
    q_ref, s_ref = ops.quantize_fp8_rows(h)
    check_against_host(h, q_ref, s_ref)
    buf = torch.full((10, cols + 40), SENT, dtype=torch.uint8, device=DEV)
    q, s = buf[:9, :cols], torch.empty(9, device=DEV)
    ops.rmsnorm_quantize_fp8(x, w, 1e-6, q, s)
    assert torch.equal(s, s_ref) and torch.equal(q, q_ref) and untouched(buf, 9, cols)
    for rows in (1, 2, 3, 4):
        for first in (0, 5):                                     # rows first .. first + rows of the batch, alone
            buf.fill_(SENT)
            q1, s1 = buf[:rows, :cols], torch.empty(rows, device=DEV)
            ops.rmsnorm_quantize_fp8(x[first:first + rows], w, 1e-6, q1, s1)
            assert torch.equal(s1, s_ref[first:first + rows]) and torch.equal(q1, q_ref[first:first + rows]) and untouched(buf, rows, cols)


TINY = [2.0 ** -133, 1e-37, 448 * 2.0 ** -126]


def tiny_rows(cols):
    x = torch.zeros(len(TINY) + 1, cols, dtype=torch.bfloat16)
    for i, a in enumerate(TINY):
        x[i, :8] = torch.tensor([a, 0.0, -a / 2, a / 4, -a, 0.0, a / 8, -0.0], dtype=torch.float64).to(torch.bfloat16)
    x[len(TINY), :3] = torch.tensor([1e-37, 0.0, -5e-38]).to(torch.bfloat16)           # the row of the report
    assert x[:, :8].double().abs().amax(1).tolist()[:3] == [torch.tensor(a).to(torch.bfloat16).double().item() for a in TINY]
    return x.to(DEV)


def check_tiny(x, q, s):
    print("tiny rows: scales", s.tolist(), "bytes", q[:, :8].tolist())
    assert int(((q & 0x7F) == 0x7F).sum()) == 0, f"NaN bytes: {q[:, :8].tolist()}"
    assert bool((s >= 2.0 ** -126).all()) and bool(torch.isfinite(1.0 / s).all())
    deq = qc.decode_e4m3(q) * s.double()[:, None]
    assert bool((deq[x == 0] == 0).all())
    check_against_host(x, q, s)


@pytest.mark.parametrize("cols", [8, 4096, 4104])
def test_tiny_rows_have_a_normal_scale_and_no_nan_bytes(cols):
    x = tiny_rows(cols)
    q, s = ops.quantize_fp8_rows(x)
    check_tiny(x, q, s)
    if cols == 8:
        assert s.tolist() == [2.0 ** -126] * 4
        # by hand: 2^-133 x 2^126 = 2^-7 = 4 x 2^-9; halves and quarters of the smallest bf16 subnormal are (signed) zeros already
        assert q[0, :8].tolist() == [0x04, 0x00, 0x80, 0x00, 0x84, 0x00, 0x00, 0x80]
        assert q[3, :3].tolist() == [0x50, 0x00, 0xC8]            # 1e-37 -> 9.99e-38 (bf16) x 2^126 = 8.5 -> 8, -4.25 -> -4 (ties to even)


@pytest.mark.parametrize("cols", [8, 520, 4096])
def test_tiny_rows_through_the_fused_norm(cols):
    x = tiny_rows(cols)
    w = torch.ones(cols, dtype=torch.bfloat16, device=DEV)
    h = ops.rmsnorm(x, w, 1e-6)
    assert float(h.double().abs().max()) < 2.0 ** -100            # eps = 1e-6 bounds the gain at 1000: the normalised rows stay tiny
    q, s = torch.empty(x.shape, dtype=torch.uint8, device=DEV), torch.empty(x.shape[0], device=DEV)
    ops.rmsnorm_quantize_fp8(x, w, 1e-6, q, s)
    check_tiny(h, q, s)


@pytest.mark.parametrize("dt", sorted(DT))
@pytest.mark.parametrize("cols", [4096, 4104])
def test_non_finite_input_stays_in_its_row(dt, cols):
    x = gaussian_rows(6, cols, DT[dt], 9).contiguous()
    q0, s0 = ops.quantize_fp8_rows(x)
    y = x.clone()
    y[1, 17] = float("inf")
    y[4, 100] = float("nan")
    q, s = ops.quantize_fp8_rows(y)
    keep = [0, 2, 3, 5]
    assert torch.equal(q[keep], q0[keep]) and torch.equal(s[keep], s0[keep])
    deq = qc.decode_e4m3(q) * s.double()[:, None]
    assert not bool(torch.isfinite(deq[1]).all()) and not bool(torch.isfinite(deq[4]).all())
    # pinned: Inf makes the scale inf and 1 / scale 0 - finite elements become signed zeros, the Inf itself 0 x inf = the NaN byte;
    # fmaxf drops a NaN, so a NaN row keeps its scale and its other bytes, and the NaN element becomes the NaN byte
    assert s[1].item() == float("inf") and (q[1, 17].item() & 0x7F) == 0x7F
    rest = torch.ones(cols, dtype=torch.bool, device=DEV)
    rest[17] = False
    assert bool(((q[1][rest] & 0x7F) == 0).all())
    assert s[4].item() == s0[4].item() and (q[4, 100].item() & 0x7F) == 0x7F
    rest[17], rest[100] = True, False
    assert torch.equal(q[4][rest], q0[4][rest])


# ------------------------------------------------------------------------------ MXFP4


def quantize_mxfp4_into_views(w, extra_q=12, extra_e=5):
    rows, cols = w.shape
    qb = torch.full((rows + 1, cols // 2 + extra_q), SENT, dtype=torch.uint8, device=DEV)
    eb = torch.full((rows + 1, cols // 32 + extra_e), SENT, dtype=torch.uint8, device=DEV)
    _native.check(_native.lib().v3d_quantize_mxfp4_rows(ops._p(w), w.stride(0), rows, cols, ops._code(w), ops._p(qb), qb.stride(0), ops._p(eb),
                                                        eb.stride(0), ops._stream()), "v3d_quantize_mxfp4_rows")
    assert bool((qb[rows] == SENT).all()) and bool((qb[:, cols // 2:] == SENT).all()), "code bytes outside the view"
    assert bool((eb[rows] == SENT).all()) and bool((eb[:, cols // 32:] == SENT).all()), "exponent bytes outside the view"
    return qb[:rows, :cols // 2], eb[:rows, :cols // 32]


def blocks_under_fixed_maxima(dt, lo, hi):
    """[rows, 1024]: blocks [2^(f + s), 31 patterns of the binade f] for every finite pattern with lo <= |x| <= hi and s = 0..4."""
    v = finite_patterns(dt)
    mag = v.double().abs()
    v = v[(mag >= lo) & (mag <= hi)]
    f = torch.frexp(v.double().abs())[1] - 1
    top = torch.finfo(dt).max
    out = []
    for s in range(5):
        for b in f.unique().tolist():
            if 2.0 ** (b + s) > min(top, hi * 32):
                continue
            sel = v[f == b]
            pad = torch.zeros(-(-sel.numel() // 31) * 31, dtype=dt)
            pad[:sel.numel()] = sel
            blk = torch.empty(pad.numel() // 31, 32, dtype=dt)
            blk[:, 0] = 2.0 ** (b + s)
            blk[:, 1:] = pad.reshape(-1, 31)
            out.append(blk)
    blk = torch.cat(out)
    rows = -(-blk.shape[0] // 32)
    w = torch.zeros(rows * 32, 32, dtype=dt)
    w[:blk.shape[0]] = blk
    return w.reshape(rows, 1024)


@pytest.mark.parametrize("dt", sorted(DT))
def test_mxfp4_every_pattern_under_fixed_block_maxima(dt):
    w = blocks_under_fixed_maxima(DT[dt], 0.0, 65504.0) if dt == "f16" else blocks_under_fixed_maxima(DT[dt], 2.0 ** -40, 2.0 ** 40)
    q_ref, e_ref = MX.quantize(w)
    assert len(np.unique(MX.unpack(q_ref))) == 15                # every code but -0, which the format never writes
    q, e = quantize_mxfp4_into_views(w.to(DEV))
    assert np.array_equal(e.cpu().numpy(), e_ref)
    bad = np.argwhere(q.cpu().numpy() != q_ref)
    assert bad.shape[0] == 0, f"{bad.shape[0]} code bytes differ, first at {bad[0].tolist()}"


def test_mxfp4_exponent_clamp_at_zero():
    """bf16 blocks whose amax has the f32 exponent field 0 (a subnormal), 1 and 2: ex - 2 clamps at 0, the codes are w 2^127 rounded."""
    w = torch.zeros(2, 128, dtype=torch.bfloat16)
    for b, a in enumerate((5 * 2.0 ** -133, 2.0 ** -126, 1.5 * 2.0 ** -125, 1.75 * 2.0 ** -124)):
        w[0, 32 * b: 32 * b + 8] = torch.tensor([a, -a, a / 2, -a / 4, 3 * a / 4, 0.0, a / 8, -a / 16], dtype=torch.float64).to(torch.bfloat16)
    field = (w[0].float().view(torch.int32).reshape(4, 32) >> 23 & 0xFF).amax(1).tolist()
    assert field == [0, 1, 2, 3]
    q_ref, e_ref = MX.quantize(w)
    assert e_ref[0].tolist() == [0, 0, 0, 1] and e_ref[1].tolist() == [127] * 4
    q, e = quantize_mxfp4_into_views(w.to(DEV))
    assert np.array_equal(e.cpu().numpy(), e_ref) and np.array_equal(q.cpu().numpy(), q_ref)
