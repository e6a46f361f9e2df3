"""v3d_lora_down and v3d_lora_wgrad (csrc/lora.hip) per element against the f64 references and bounds of tests/lora_check.py, bf16 and
f16, called through the C ABI so that every leading dimension is chosen here.

Every case: each operand is a window of a larger NaN-filled buffer - a leading dimension above its minimum (NaN in the gap) and NaN rows
behind row M (a kernel that read a row past M, or a column past its width, would return NaN) - and the output is a NaN-prefilled
window of a buffer of sentinels that must come back untouched (guard rows and columns); wgrad's workspace is followed by sentinels
that must survive.  Families (lora_check): *random* under the bound, *exact* (integer sums: bit-equal to the rounded f64 value) and
*gather* (one-hot p resp. u: the output names the k resp. the token row that was read).  Every launch is repeated and must give
identical bits.

Shapes.  down (M, K, R): one row, one K step, one rank block; 65 rows (a 32-row tile with one row), R = 48 (a rank bucket not filled);
the decoder widths 3584, 4608 (q|k|v stacked, R = 384: the widest bucket) and 18944 (down_proj's input, R = 192).  wgrad (M, R, K):
one row; 7 rows with R = 48; 129 rows (one row past four 32-row steps); the flagship 6794 x 64 x 3584 (10 chunks of 704 rows); and at
(R, K) = (192, 4608), with c = v3d_lora_wgrad_chunk(6794, 192, 4608), M = 3 c, 3 c + 1, 3 c - 1, plus the M that are whole multiples
of their OWN chunk (M = n chunk(M)) and one row to either side: the last chunk full, one row long, and one row short.

Measured on one MI355X (85 tests, 3.3 s): every exact case bit-equal, no gather mismatch; worst |err| / bound on random inputs 0.977
(down, bf16, K = 128) and 0.992 (wgrad to a bf16 output, M = 129: almost all of it the output rounding); with an f32 output the wgrad ratio is 0.0007 .. 0.02 - the bound's accumulation
term is a worst case, see tests/test_lora_check_cpu.py.
"""
import ctypes

import pytest
import torch

import lora_check as lc

pytestmark = pytest.mark.gpu

DT = {"bf16": torch.bfloat16, "f16": torch.float16}
CODE = {torch.float32: 0, torch.float16: 1, torch.bfloat16: 2}
SENT = 7.0
GUARD_ROWS, GUARD_COLS, LD_PAD, WS_GUARD = 8, 64, 8, 256
FAMILIES = ("random", "exact", "gather")

DOWN_SHAPES = [(1, 64, 16), (65, 128, 48), (200, 3584, 64), (257, 4608, 384), (333, 18944, 192)]
WGRAD_SHAPES = [(1, 16, 128), (7, 48, 128), (129, 64, 3584), (6794, 64, 3584)]


@pytest.fixture(scope="module")
def lib():
    assert torch.cuda.is_available()
    from v3d import _native
    return _native.lib()


def _ptr(t):
    return ctypes.c_void_p(t.data_ptr())


def _stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def stored(x):
    """x [rows, cols] as the kernel gets it: the window [:rows, :cols] of a NaN buffer with LD_PAD more columns and GUARD_ROWS more rows."""
    rows, cols = x.shape
    buf = torch.full((rows + GUARD_ROWS, cols + LD_PAD), float("nan"), dtype=x.dtype, device=x.device)
    buf[:rows, :cols] = x
    return buf[:rows, :cols]


def framed(rows, cols, dt):
    frame = torch.full((rows + GUARD_ROWS, cols + GUARD_COLS), SENT, dtype=dt, device="cuda")
    out = frame[:rows, :cols]
    out.fill_(float("nan"))
    return frame, out


def guards_ok(frame, rows, cols):
    return bool((frame[rows:] == SENT).all()) and bool((frame[:, cols:] == SENT).all())


def bits(t):
    return t.contiguous().view(torch.int32 if t.dtype == torch.float32 else torch.int16)


def run_down(lib, x, p, scale):
    M, K = x.shape
    R = p.shape[0]
    sx, sp = stored(x), stored(p)
    outs = []
    for _ in range(2):
        frame, out = framed(M, R, x.dtype)
        rc = lib.v3d_lora_down(_ptr(sx), sx.stride(0), _ptr(sp), sp.stride(0), scale, _ptr(out), out.stride(0), M, R, K, CODE[x.dtype], _stream())
        assert rc == 0, lib.v3d_last_error()
        torch.cuda.synchronize()
        assert guards_ok(frame, M, R), "v3d_lora_down wrote guard rows / columns"
        outs.append(out)
    assert torch.equal(bits(outs[0]), bits(outs[1])), "two calls of v3d_lora_down differ"
    return outs[0]


def run_wgrad(lib, u, x, scale, gd):
    M, R = u.shape
    K = x.shape[1]
    su, sx = stored(u), stored(x)
    n_ws = lib.v3d_lora_wgrad_workspace_bytes(M, R, K) // 4
    chunk = lib.v3d_lora_wgrad_chunk(M, R, K)
    assert n_ws > 0 and chunk > 0
    outs = []
    for _ in range(2):
        ws = torch.full((n_ws + WS_GUARD,), SENT, dtype=torch.float32, device="cuda")
        ws[:n_ws] = float("nan")
        frame, out = framed(R, K, gd)
        rc = lib.v3d_lora_wgrad(_ptr(su), su.stride(0), _ptr(sx), sx.stride(0), scale, _ptr(out), out.stride(0), CODE[gd], M, R, K, CODE[u.dtype],
                                _ptr(ws), _stream())
        assert rc == 0, lib.v3d_last_error()
        torch.cuda.synchronize()
        assert guards_ok(frame, R, K), "v3d_lora_wgrad wrote guard rows / columns"
        assert bool((ws[n_ws:] == SENT).all()), "v3d_lora_wgrad wrote past its workspace"
        outs.append(out)
    assert torch.equal(bits(outs[0]), bits(outs[1])), "two calls of v3d_lora_wgrad differ"
    return outs[0], -(-M // chunk)


def check_down(lib, family, M, K, R, dt, seed):
    x, p, scale, want = lc.down_inputs(family, M, K, R, dt, seed=seed, device="cuda")
    got = run_down(lib, x, p, scale)
    if family == "gather":
        assert torch.equal(got, want), "row m of the output read another k:\n" + lc.gather_explain(got, x, p, want, transposed=True)
        return None
    v = lc.verdict(got, lc.down_reference(x, p, scale))
    print(f"down {family} {dt} M={M} K={K} R={R}: worst |err| / bound {v['ratio']:.3f}, unequal {v['unequal']}")
    assert v["ratio"] <= 1.0, v
    if family == "exact":
        assert v["unequal"] == 0, v
    return v


def check_wgrad(lib, family, M, R, K, dt, gd, seed):
    u, x, scale, want, aw = lc.wgrad_inputs(family, M, R, K, dt, seed=seed, device="cuda")
    got, n_chunks = run_wgrad(lib, u, x, scale, gd)
    if family == "gather":
        want = want.to(gd)
        assert torch.equal(got, want), "row r of the output read another token row (k below):\n" + lc.gather_explain(got, aw[0], aw[1], want)
        return None
    v = lc.verdict(got, lc.wgrad_reference(u, x, scale, gd, n_chunks))
    print(f"wgrad {family} {dt} -> {gd} M={M} R={R} K={K} ({n_chunks} chunks): worst |err| / bound {v['ratio']:.4f}, unequal {v['unequal']}")
    assert v["ratio"] <= 1.0, v
    if family == "exact":
        assert v["unequal"] == 0, v
    return v


@pytest.mark.parametrize("family", FAMILIES)
@pytest.mark.parametrize("shape", DOWN_SHAPES, ids=lambda s: "x".join(map(str, s)))
@pytest.mark.parametrize("dt", list(DT))
def test_down(lib, dt, shape, family):
    M, K, R = shape
    check_down(lib, family, M, K, R, DT[dt], seed=M + K + R)


@pytest.mark.parametrize("family", FAMILIES)
@pytest.mark.parametrize("g", ["f32", "same"])
@pytest.mark.parametrize("shape", WGRAD_SHAPES, ids=lambda s: "x".join(map(str, s)))
@pytest.mark.parametrize("dt", list(DT))
def test_wgrad(lib, dt, shape, g, family):
    M, R, K = shape
    check_wgrad(lib, family, M, R, K, DT[dt], torch.float32 if g == "f32" else DT[dt], seed=M + K + R)


@pytest.mark.parametrize("family", FAMILIES)
@pytest.mark.parametrize("dt", list(DT))
def test_wgrad_at_the_chunk_boundaries(lib, dt, family):
    R, K = 192, 4608
    c = lib.v3d_lora_wgrad_chunk(6794, R, K)
    assert c > 0 and c % 32 == 0
    ms = [3 * c, 3 * c + 1, 3 * c - 1]
    own = [m for m in range(c, 2 * c + 1, 32) if m % lib.v3d_lora_wgrad_chunk(m, R, K) == 0 and m // lib.v3d_lora_wgrad_chunk(m, R, K) >= 2]
    assert own, "no M in this range is a whole number of its own chunks"
    m0 = own[0]
    ms += [m0, m0 + 1, m0 - 1]
    for M in ms:
        for gd in (torch.float32, DT[dt]):                 # both forms of the sum kernel's store
            check_wgrad(lib, family, M, R, K, DT[dt], gd, seed=M)


def test_ops_wrappers_take_views_and_refuse_what_the_kernels_cannot(lib):
    """ops.lora_down / ops.lora_wgrad on column slices of wider buffers (row stride kept, no copy) equal the direct calls; a rank the
    kernels do not cover raises by name."""
    from v3d import ops
    from v3d._native import V3DError
    dt = torch.bfloat16
    x, p, scale, _ = lc.down_inputs("exact", 70, 128, 32, dt, seed=5, device="cuda")
    wide = torch.full((70, 256), float("nan"), dtype=dt, device="cuda")
    wide[:, 64:192] = x
    got = ops.lora_down(wide[:, 64:192], p, scale)
    assert torch.equal(got, run_down(lib, x, p, scale))
    u, xx, scale, _, _ = lc.wgrad_inputs("exact", 70, 32, 128, dt, seed=6, device="cuda")
    g32 = ops.lora_wgrad(u, xx, scale)
    want, _ = run_wgrad(lib, u, xx, scale, torch.float32)
    assert g32.dtype == torch.float32 and torch.equal(g32, want)
    ws = ops.lora_wgrad_workspace(70, 32, 128, "cuda")
    assert torch.equal(ops.lora_wgrad(u, xx, scale, dtype=dt, workspace=ws), run_wgrad(lib, u, xx, scale, dt)[0])
    with pytest.raises(V3DError, match="R=24"):
        ops.lora_down(x, p[:24], scale)
    with pytest.raises(V3DError, match="no kernel"):
        ops.lora_wgrad(u[:, :24], xx, scale)
