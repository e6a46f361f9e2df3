"""GPU tests of csrc/pe_points.hip: the sampled-point and min/max coordinate kernels, PositionEmbeddingSine3D with n_points, its table
and the fused visual-token kernel with P points, against the reference's own outputs (tests/golden/pe_points.npz) and, where a golden
would be too large to store, the CPU restatement that reproduces that golden (tests/pe_points_check.py, test_pe_points_check_cpu.py)."""
import numpy as np
import pytest
import torch

import pe_points_check as PC
from test_gpu_visual import EPS16, ulp16

pytestmark = pytest.mark.gpu

MODE_OF_P = {9: "sample9", 5: "sample5", 2: "minmax"}


@pytest.fixture(scope="module")
def ops():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    from v3d import ops as _ops
    return _ops


def same_values(got, want):
    """equal with NaN positions equal (values, not zero signs)."""
    got, want = got.float().cpu().numpy(), want.float().cpu().numpy()
    return got.shape == want.shape and np.array_equal(np.isnan(got), np.isnan(want)) and np.array_equal(np.nan_to_num(got), np.nan_to_num(want))


# ------------------------------------------------------------------------------ coordinates


@pytest.mark.parametrize("kind", ["f32", "f16", "bf16"])
@pytest.mark.parametrize("mode", list(PC.MODES))
def test_coord_points_voxel_golden(ops, golden, mode, kind):
    g = golden("pe_points")
    pts, vox, ids = ops.coord_points_voxel(PC.seeded_coords(kind).cuda(), mode)
    want_pts, want_vox = PC.from_bits(g[f"{mode}_pts_{kind}"], kind), PC.from_bits(g[f"{mode}_vox_{kind}"], kind)
    assert same_values(pts, want_pts)
    assert same_values(vox, want_vox)
    assert torch.isnan(want_pts.float()).any()
    ok = ~torch.isnan(want_vox.float())               # an id is defined where the voxel coordinate is a number
    assert ids.dtype == torch.int32 and ids.shape == want_vox.shape
    assert torch.equal(ids.cpu()[ok], torch.from_numpy(g[f"{mode}_ids_{kind}"].astype(np.int32))[ok])
    only_ids = ops.coord_points_voxel(PC.seeded_coords(kind).cuda(), mode, want_pts=False, want_vox=False)
    assert only_ids[0] is None and only_ids[1] is None and torch.equal(only_ids[2], ids)


@pytest.mark.parametrize("kind", ["f32", "bf16"])
def test_sample_modes_nest(ops, kind):
    x = PC.seeded_coords(kind).cuda()
    nine = ops.coord_points_voxel(x, "sample9")
    five = ops.coord_points_voxel(x, "sample5")
    one = ops.coord_points_voxel(x, "sample1")
    for a, b, c in zip(nine, five, one):
        assert same_values(b, a[:, :, :, [0, 2, 4, 6, 8]])
        assert c.shape == (2, 14, 14, 3) and same_values(c, a[:, :, :, 4])


def test_coord_points_voxel_refuses_bad_arguments(ops):
    from v3d._native import V3DError
    with pytest.raises(V3DError, match="384"):
        ops.coord_points_voxel(torch.zeros((1, 192, 192, 3), device="cuda"), "sample9")
    x = torch.zeros((1, 384, 384, 3), device="cuda")
    with pytest.raises(V3DError, match="27"):
        ops.coord_points_voxel(x, "minmax", patch=26)
    with pytest.raises(V3DError, match="unknown mode"):
        ops.coord_points_voxel(x, 7)
    with pytest.raises(V3DError, match="unknown mode"):
        ops.coord_points_voxel(x, "sample3")


# ------------------------------------------------------------------------------ PE


@pytest.mark.parametrize("kind", ["f16", "bf16"])
@pytest.mark.parametrize("continuous", [False, True])
@pytest.mark.parametrize("E,P", PC.PE_CASES)
def test_sin3d_pe_points_golden(ops, golden, E, P, continuous, kind):
    """the rule of tests/test_gpu_visual.py:190-198: at most 1 ulp16 off, a share of differing elements below 2e-3."""
    g = golden("pe_points")
    x = PC.pe_inputs(E, P, kind, continuous)
    out = ops.sin3d_pe(x[None].cuda(), E, n_points=P)[0].float().cpu().numpy()
    ref = PC.from_bits(g[f"pe_E{E}_P{P}_{'cont' if continuous else 'ids'}_{kind}"], kind).float().numpy()
    d = ulp16(out, ref, kind)
    print(f"E={E} P={P} {kind} continuous={continuous}: max ulp16 {d.max()}, differing share {(d != 0).mean():.2e}")
    assert d.max() <= 1 and (d != 0).mean() < 2e-3


@pytest.mark.parametrize("continuous", [False, True])
@pytest.mark.parametrize("P", [9, 5, 2])
def test_sin3d_pe_points_f32(ops, golden, P, continuous):
    """the bound of tests/test_gpu_visual.py:201-206."""
    g = golden("pe_points")
    out = ops.sin3d_pe(PC.pe_inputs(256, P, "f32", continuous)[None].cuda(), 256, n_points=P)[0].cpu().numpy()
    np.testing.assert_allclose(out, g[f"pe_E256_P{P}_{'cont' if continuous else 'ids'}_f32"], rtol=0, atol=5e-7)


def test_points_table_copies(ops):
    """E = 3584, P = 9, f16: nf = 132, segments start 0 or 4 elements past a 16-byte boundary -> two copies; each holds T(value) at its
    shift and zero bits elsewhere (the property of tests/test_gpu_visual.py:181-187)."""
    E, P, nf = 3584, 9, 132
    t = ops.Sin3DTable(E, 301, torch.float16, "cuda", n_points=P)
    assert t.shifts == [0, 4] and t.row_elems == 144 and tuple(t.table.shape) == (2, 301, 144)
    ids = torch.arange(301, dtype=torch.float32)[:, None, None].expand(301, P, 3).contiguous().half()
    ref16 = PC.pe(ids, E, P)[:, :nf].float().numpy()
    tab = t.table.float().cpu().numpy()
    bits = t.table.view(torch.int16).cpu().numpy()
    for c, shift in enumerate(t.shifts):
        d = ulp16(tab[c][:, shift:shift + nf], ref16, "f16")
        assert d.max() <= 1 and (d != 0).mean() < 1e-3
        assert np.all(bits[c][:, :shift] == 0) and np.all(bits[c][:, shift + nf:] == 0)
    # a layout with every shift taken (E = 256, P = 5, f16: nf = 17 -> 8 distinct shifts)
    t = ops.Sin3DTable(256, 301, torch.float16, "cuda", n_points=5)
    assert sorted(t.shifts) == list(range(8)) and t.shifts[:3] == [0, 1, 2]


# ------------------------------------------------------------------------------ fused


def _fused_inputs(ops, C, P, kind, V=2):
    dt = PC.DT[kind]
    gen = torch.Generator().manual_seed(1000 * C + P)
    feat = torch.randn((V, 729, C), generator=gen).to(dt).cuda()
    newline = torch.randn(C, generator=gen).to(dt).cuda()
    coords = torch.nan_to_num(PC.seeded_coords(kind).float(), nan=0.0).to(dt).cuda()      # a NaN coordinate has no voxel id: not this test's
    pts, vox, ids = ops.coord_points_voxel(coords, MODE_OF_P[P])
    return feat, newline, pts, vox, ids


def _with_newline(rows, newline, V):
    C = rows.shape[-1]
    grid = rows.reshape(V, 14, 14, C)
    return torch.cat([grid, newline.reshape(1, 1, 1, C).expand(V, 14, 1, C)], dim=2).reshape(V * 14 * 15, C)


@pytest.mark.parametrize("kind", ["f16", "bf16"])
@pytest.mark.parametrize("continuous", [False, True])
@pytest.mark.parametrize("C,P", PC.PE_CASES)
def test_fused_points(ops, C, P, continuous, kind):
    dt = PC.DT[kind]
    feat, newline, pts, vox, ids = _fused_inputs(ops, C, P, kind)
    table = None if continuous else ops.Sin3DTable(C, 301, dt, "cuda", n_points=P)
    src = dict(pts=pts) if continuous else dict(ids=ids, table=table)
    out = ops.visual_tokens(feat, newline=newline, n_points=P, **src)
    assert out.shape == (2 * 210, C)
    # expected, from the bit-pinned pieces: pooled rows (v3d_visual_tokens), + the PE rows in the model dtype (one rounded add), + newline rows
    pooled = ops.visual_tokens(feat, pool=True)
    pe = PC.pe((pts if continuous else vox).cpu().reshape(-1, P, 3), C, P)
    want = _with_newline(pooled.cpu() + pe, newline.cpu(), 2).float().numpy()
    bound = _with_newline(EPS16[kind] * (pooled.float().cpu().abs() + 1.0), torch.zeros(C), 2).numpy()
    got = out.float().cpu().numpy()
    err = np.abs(got - want)
    print(f"C={C} P={P} {kind} continuous={continuous}: max err/bound {np.max(err / np.maximum(bound, 1e-30)):.3f}, differing share {(got != want).mean():.2e}")
    assert np.all(err <= bound)
    assert (got != want).mean() < 2e-3
    # bit-equal to its own composition: pool alone, then PE + newline alone
    composed = ops.visual_tokens_points(pooled.view(2, 196, C), newline=newline, n_points=P, pool=False, **src)
    assert torch.equal(composed, out)
    if not continuous:
        # integer-valued coordinates through the on-the-fly form give the table form's bits
        assert torch.equal(ops.visual_tokens(feat, newline=newline, n_points=P, pts=vox), out)
        # a row slice of a larger zeroed buffer: the rows before and after stay untouched
        buf = torch.zeros((7 + 420 + 5, C + 8), dtype=dt, device="cuda")[:, :C]
        ops.visual_tokens(feat, newline=newline, n_points=P, out=buf[7:427], **src)
        assert torch.equal(buf[7:427], out) and not buf[:7].any() and not buf[427:].any()


@pytest.mark.parametrize("kind", ["f16", "bf16", "f32"])
@pytest.mark.parametrize("C", [256, 3584])
def test_fused_points_one_point_equals_visual_tokens(ops, C, kind):
    dt = PC.DT[kind]
    gen = torch.Generator().manual_seed(C)
    feat = torch.randn((2, 729, C), generator=gen).to(dt).cuda()
    newline = torch.randn(C, generator=gen).to(dt).cuda()
    avg, vox, ids = ops.coord_pool_voxel(torch.nan_to_num(PC.seeded_coords(kind).float()).to(dt).cuda())
    want = ops.visual_tokens(feat, ids, ops.Sin3DTable(C, 301, dt, "cuda"), newline)
    got = ops.visual_tokens_points(feat, ids=ids, table=ops.Sin3DTable(C, 301, dt, "cuda", points_layout=True), newline=newline)
    assert torch.equal(got, want)
    assert torch.equal(ops.visual_tokens(feat, newline=newline, pts=vox), want)          # avg-sin3d's form on integer-valued coordinates


def test_fused_points_f32(ops):
    C, P = 256, 9
    feat, newline, pts, vox, ids = _fused_inputs(ops, C, P, "f32")
    pooled = ops.visual_tokens(feat, pool=True)
    for src, x in ((dict(ids=ids, table=ops.Sin3DTable(C, 301, torch.float32, "cuda", n_points=P)), vox), (dict(pts=pts), pts)):
        out = ops.visual_tokens(feat, newline=newline, n_points=P, **src)
        want = _with_newline(pooled.cpu() + PC.pe(x.cpu().reshape(-1, P, 3), C, P), newline.cpu(), 2)
        np.testing.assert_allclose(out.cpu().numpy(), want.numpy(), rtol=2e-6, atol=2e-6)


def test_fused_points_refuses_bad_arguments(ops):
    from v3d._native import V3DError
    feat = torch.zeros((1, 729, 64), dtype=torch.float16, device="cuda")
    pts = torch.zeros((1, 14, 14, 9, 3), dtype=torch.float16, device="cuda")
    with pytest.raises(V3DError, match="features per axis"):
        ops.visual_tokens(feat, n_points=9, pts=pts)                                   # 64 // 27 = 2 < 8
    feat = torch.zeros((1, 729, 256), dtype=torch.float16, device="cuda")
    with pytest.raises(V3DError, match="another dtype / width / number of points"):
        ops.visual_tokens(feat, torch.zeros((1, 14, 14, 9, 3), dtype=torch.int32, device="cuda"),
                          ops.Sin3DTable(256, 301, torch.float16, "cuda", n_points=5), n_points=9)


# ------------------------------------------------------------------------------ the four PE sources of the shared token-row body


def _clamped_ids(ops, kind, V):
    """Patch-constant coordinates drawn past both ends of the voxel range, so that the ids include 0 and the last id of an axis."""
    dt = PC.DT[kind]
    gen = torch.Generator().manual_seed(77 + V)
    cell = (torch.rand((V, 14, 14, 3), generator=gen) - 0.5) * torch.tensor([40.0, 40.0, 14.0])
    coords = torch.zeros((V, 384, 384, 3))
    coords[:, :378, :378] = cell.repeat_interleave(27, dim=1).repeat_interleave(27, dim=2)
    _, vox, ids = ops.coord_pool_voxel(coords.to(dt).cuda())
    assert ids.min().item() == 0 and ids[..., :2].max().item() == 300 and ids[..., 2].max().item() == 100
    assert torch.equal(vox.float().to(torch.int32), ids)          # r = rint of a T value: the voxel coordinate IS the id
    return vox, ids


def _four_forms_agree(ops, kind, V, C, pool, newline_on):
    dt, n = PC.DT[kind], 14
    vox, ids = _clamped_ids(ops, kind, V)
    gen = torch.Generator().manual_seed(C + 2 * pool + newline_on)
    feat = torch.randn((V, 729 if pool else n * n, C), generator=gen).to(dt).cuda()
    newline = torch.randn(C, generator=gen).to(dt).cuda() if newline_on else None
    rows, vec = V * n * (n + 1 if newline_on else n), 4 if kind == "f32" else 8
    forms = {
        "axis table": lambda out: ops.visual_tokens(feat, ids, ops.Sin3DTable(C, 301, dt, "cuda"), newline, pool=pool, out=out),
        "points table": lambda out: ops.visual_tokens_points(feat, ids=ids[..., None, :], table=ops.Sin3DTable(C, 301, dt, "cuda", points_layout=True),
                                                             newline=newline, pool=pool, out=out),
        "trig on the fly": lambda out: ops.visual_tokens_points(feat, pts=vox[..., None, :], newline=newline, pool=pool, out=out),
    }
    if kind != "f32":       # v3d_visual_tokens_rows is the 16-bit training form: it refuses f32 (tests/test_gpu_pe_mlp.py)
        forms["PE rows"] = lambda out: ops.visual_tokens_rows(feat, ops.sin3d_pe(vox, C).reshape(-1, C), newline, pool=pool, out=out)
    outs = {}
    for name, run in forms.items():
        buf = torch.zeros((3 + rows + 2, C + vec), dtype=dt, device="cuda")[:, :C]       # `out` is a row slice of a wider buffer
        run(buf[3:3 + rows])
        assert not buf[:3].any() and not buf[3 + rows:].any(), name
        outs[name] = buf[3:3 + rows]
    first = outs["axis table"]
    assert not torch.equal(first, ops.visual_tokens(feat, newline=newline, pool=pool))     # the PE took part
    for name, out in outs.items():
        bad = (out.view(torch.int32 if kind == "f32" else torch.int16) != first.view(torch.int32 if kind == "f32" else torch.int16)).nonzero()
        assert bad.numel() == 0, f"{name} differs from the axis table at (row, channel) {bad[0].tolist()}: {out[tuple(bad[0])].item()} vs {first[tuple(bad[0])].item()}"


@pytest.mark.parametrize("newline_on", [True, False])
@pytest.mark.parametrize("pool", [True, False])
@pytest.mark.parametrize("kind", ["f16", "bf16", "f32"])
def test_one_point_pe_sources_agree(ops, kind, pool, newline_on):
    """With P = 1 the PE sources of the shared token-row body compute the same value - T(pe_value(float(id), dim_t[j], j)) added to the
    pooled value in T - so their outputs are equal bit for bit.  V = 2; 16-bit C = 104 (nf = 34: segments start at vector offsets 0, 2, 4,
    vectors straddle two segments, channels 102-103 get no PE, 13 vectors < 64 lanes), f32 C = 52 (nf = 17)."""
    _four_forms_agree(ops, kind, 2, 52 if kind == "f32" else 104, pool, newline_on)


@pytest.mark.parametrize("kind,C", [("f32", 2060), ("bf16", 4120)])
def test_one_point_pe_sources_agree_past_512_lanes(ops, kind, C):
    """515 vectors per token > 512 lanes: the lane-strided loop runs twice (f32 C = 2060, nf = 686, offset 2; bf16 C = 4120 so that the
    PE-rows form, which has no f32, takes the second trip as well)."""
    _four_forms_agree(ops, kind, 1, C, True, True)
