"""The row-wise kernels of the training path against the f64 references and per-element bounds of tests/rowwise_check.py: v3d_rmsnorm,
v3d_layernorm, v3d_rmsnorm_grad, v3d_layernorm_grad, v3d_swiglu(_grad), v3d_gelu(_grad) and the rotation's transpose, in bf16 and f16.

References are computed on the device in f64.  The kernels are called through the C interface with the wrappers' own helpers, so that every
output buffer is the test's: it starts as NaN, sits in a wider buffer where the interface takes a leading dimension, and afterwards
everything that should be written is finite and inside the bound (bit-identical on the exact family) and the padding is still NaN.  Inputs
are column slices of wider NaN-filled buffers with three different leading dimensions, so nothing outside a row may reach a result.

The last test prints the worst |err| / bound per kernel and dtype seen in this run."""
import json
import os
import sys

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (os.path.join(ROOT, "tests"), ROOT, os.path.join(ROOT, "video-3d-llm_amd")):
    if _p not in sys.path:
        sys.path.insert(0, _p)

import rowwise_check as rc  # noqa: E402

pytestmark = pytest.mark.gpu

DT = {"bf16": torch.bfloat16, "float16": torch.float16}
WIDTHS = (8, 64, 136, 504, 512, 520, 1152, 1536, 1544, 2048, 3584)
ROW_EDGES = (1, 3, 4, 5, 31, 32, 33, 129)
NAN = float("nan")
WORST = {}


def _ops():
    from v3d import ops
    return ops


def note(kernel, dtn, r):
    key = f"{kernel} {dtn}"
    WORST[key] = max(WORST.get(key, 0.0), r)
    return r


def padded(t, ld, off=0):
    """t [rows, cols] -> the same values as a column slice (at column `off`, a multiple of 8) of a NaN-filled [rows, ld] buffer."""
    rows, cols = t.shape
    big = torch.full((rows, ld), NAN, dtype=t.dtype, device="cuda")
    big[:, off:off + cols] = t
    return big[:, off:off + cols]


def nan_out(rows, cols, ld, dtype):
    big = torch.full((rows, ld), NAN, dtype=dtype, device="cuda")
    return big, big[:, :cols]


def untouched(big, cols):
    return bool(torch.isnan(big[:, cols:]).all())


def inputs(family, rows, cols, dt, norm, seed=0, strided=True):
    p = rc.norm_inputs(family, rows, cols, dt, seed=seed, norm=norm, device="cuda")
    if strided:
        p["x"] = padded(p["x"], cols + 24, 8)
        p["dy"] = padded(p["dy"], cols + 8, 0)
        p["add"] = padded(p["add"], 2 * cols + 16, cols + 16)
    return p


def call_norm_grad(norm, p, add, dw_dtype, ldd=None):
    """-> (dx, dw, db or None, padding untouched).  dx is a slice of a NaN buffer with leading dimension ldd."""
    o = _ops()
    x, dy, a = p["x"], p["dy"], (p["add"] if add else None)
    rows, cols = x.shape
    big, dx = nan_out(rows, cols, ldd or cols + 40, x.dtype)
    dw = torch.full((cols,), NAN, dtype=dw_dtype, device="cuda")
    db = torch.full((cols,), NAN, dtype=dw_dtype, device="cuda")
    lda = a.stride(0) if a is not None else 0
    if norm == "rms":
        ws = o._colsum_ws(rows, cols, x.device)
        o.check(o.lib().v3d_rmsnorm_grad(o._p(x), x.stride(0), o._p(p["w"]), o._p(dy), dy.stride(0), o._p(a), lda, o._p(dx), dx.stride(0), o._p(ws),
                                         o._p(dw), o._DT[dw.dtype], rows, cols, p["eps"], o._code(x), o._stream()), "v3d_rmsnorm_grad")
        db = None
    else:
        ws = torch.empty(max(1, 2 * o.lib().v3d_colsum_workspace_bytes(rows, cols) // 4), dtype=torch.float32, device="cuda")
        o.check(o.lib().v3d_layernorm_grad(o._p(x), x.stride(0), o._p(p["w"]), o._p(dy), dy.stride(0), o._p(a), lda, o._p(dx), dx.stride(0), o._p(ws),
                                           o._p(dw), o._p(db), o._DT[dw.dtype], rows, cols, p["eps"], o._code(x), o._stream()), "v3d_layernorm_grad")
    return dx, dw, db, untouched(big, cols)


def check_norm_grad(norm, family, rows, cols, dtn, add, dw_dtype, seed=0, strided=True):
    dt = DT[dtn]
    p = inputs(family, rows, cols, dt, norm, seed, strided)
    dx, dw, db, clean = call_norm_grad(norm, p, add, dw_dtype)
    ref = (rc.rmsnorm_grad if norm == "rms" else rc.layernorm_grad)(p["x"], p["w"], p["dy"], p["eps"], add=p["add"] if add else None, dw_dtype=dw_dtype)
    what = (norm, family, rows, cols, dtn, add, str(dw_dtype))
    assert clean, ("dx padding written", what)
    outs = {"dx": dx, "dw": dw}
    if norm == "ln":
        outs["db"] = db
    for k, got in outs.items():
        assert bool(torch.isfinite(got).all()), (k, "not written / not finite", what)
        if family == "exact":
            want = ref[k][0].to(dt if k == "dx" else dw_dtype)
            assert torch.equal(got, want), (k, "exact family differs", what, int((got != want).sum()), rc.worst_index(got, ref[k]))
        r = note(f"{norm}norm_grad {k}", dtn, rc.ratio(got, ref[k]))
        assert r < 1.0, (k, r, what, rc.worst_index(got, ref[k]))


@pytest.mark.parametrize("dtn", list(DT))
@pytest.mark.parametrize("norm", ["rms", "ln"])
@pytest.mark.parametrize("cols", WIDTHS)
def test_norm_backward_every_width_and_family(norm, cols, dtn):
    """cols <= 1536 take the <T, 3> form, wider rows <T, 7>; 136 / 504 / 520 / 1544 leave a partial 64-vector step; 3584 wide LayerNorm is the
    one launch with 112 KB of dynamic LDS.  70 rows = two whole 32-row blocks and a partial one."""
    dt = DT[dtn]
    for family in rc.FAMILIES:
        for add in (False, True):
            for dw_dtype in (torch.float32, dt):
                check_norm_grad(norm, family, 70, cols, dtn, add, dw_dtype, strided=family != "random" or add)


@pytest.mark.parametrize("dtn", list(DT))
@pytest.mark.parametrize("norm", ["rms", "ln"])
@pytest.mark.parametrize("cols", [136, 3584])
def test_norm_backward_row_edges(norm, cols, dtn):
    """A workgroup takes 32 rows four at a time and leaves the loop with `break`."""
    for rows in ROW_EDGES:
        for family in ("random", "scaled", "exact"):
            check_norm_grad(norm, family, rows, cols, dtn, rows % 2 == 1, torch.float32, seed=rows)


@pytest.mark.parametrize("dtn", list(DT))
@pytest.mark.parametrize("norm,rows,cols", [("rms", 6794, 3584), ("ln", 6794, 3584), ("ln", 23328, 1152)])
def test_norm_backward_training_sizes(norm, rows, cols, dtn):
    """The 7B model's sequence at its width (213 partial rows) and the SigLIP tower's 32 frames of 729 patches (729 partial rows into
    colsum_final): dx, dweight and dbias against the bound, and bit for bit on the exact family."""
    check_norm_grad(norm, "random", rows, cols, dtn, True, torch.float32, seed=11)
    check_norm_grad(norm, "exact", rows, cols, dtn, False, torch.float32, seed=12)
    check_norm_grad(norm, "exact", rows, cols, dtn, True, DT[dtn], seed=13, strided=False)


@pytest.mark.parametrize("dtn", list(DT))
@pytest.mark.parametrize("norm", ["rms", "ln"])
@pytest.mark.parametrize("cols", [520, 3584])
def test_norm_backward_rows_are_independent_and_calls_repeat(norm, cols, dtn):
    """dx of rows [a, b) computed alone equals those rows of the full call bit for bit (cuts that are not multiples of 4 or 32), and two
    calls give identical dx, dweight and dbias - through the public wrappers."""
    o = _ops()
    p = inputs("outlier", 150, cols, DT[dtn], norm, seed=21)
    fn = o.rmsnorm_grad if norm == "rms" else o.layernorm_grad
    full = fn(p["x"], p["w"], p["dy"], p["eps"], add=p["add"], dw_dtype=torch.float32)
    again = fn(p["x"], p["w"], p["dy"], p["eps"], add=p["add"], dw_dtype=torch.float32)
    for a_, b_ in zip(full, again):
        assert torch.equal(a_, b_)
    for a, b in ((5, 71), (33, 150), (1, 2), (0, 149)):
        part = fn(p["x"][a:b], p["w"], p["dy"][a:b], p["eps"], add=p["add"][a:b], dw_dtype=torch.float32)
        assert torch.equal(part[0], full[0][a:b]), (norm, cols, dtn, a, b)


# ------------------------------------------------------------------------------ forward norms


def check_norm_forward(norm, family, rows, cols, dtn, seed=0):
    o = _ops()
    dt = DT[dtn]
    p = inputs(family, rows, cols, dt, "ln", seed)
    big, out = nan_out(rows, cols, cols + 16, dt)
    if norm == "rms":
        o.rmsnorm(p["x"], p["w"], p["eps"], out=out)
        ref = rc.rmsnorm(p["x"], p["w"], p["eps"])
    else:
        o.layernorm(p["x"], p["w"], p["b"], p["eps"], out=out)
        ref = rc.layernorm(p["x"], p["w"], p["b"], p["eps"])
    what = (norm, family, rows, cols, dtn)
    assert untouched(big, cols), ("padding written", what)
    assert bool(torch.isfinite(out).all()), ("not written / not finite", what)
    if family == "exact":
        assert torch.equal(out, ref[0].to(dt)), ("exact family differs", what, rc.worst_index(out, ref))
    r = note(f"{norm}norm", dtn, rc.ratio(out, ref))
    assert r < 1.0, (r, what, rc.worst_index(out, ref))


@pytest.mark.parametrize("dtn", list(DT))
@pytest.mark.parametrize("cols", WIDTHS + (4096,))
def test_norm_forward_every_width_and_family(cols, dtn):
    """4096 is the widest row NORM_MAXV allows.  70 rows: the one-row-per-wave forms."""
    for family in rc.FAMILIES:
        for norm in ("rms", "ln"):
            check_norm_forward(norm, family, 70, cols, dtn)


@pytest.mark.parametrize("dtn", list(DT))
def test_norm_forward_row_edges_and_three_rows_per_wave(dtn):
    """Up to four rows take v3d_rmsnorm's decode kernel; >= 4096 rows of <= 1536 columns take LayerNorm's three-rows-per-wave form (4100 and
    4102 rows leave one and two rows of the last wave's three unused)."""
    for rows in ROW_EDGES:
        for cols in (136, 4096):
            for family in ("random", "exact"):
                for norm in ("rms", "ln"):
                    check_norm_forward(norm, family, rows, cols, dtn, seed=rows)
    for rows, cols in ((4100, 8), (4102, 520), (4096, 1152), (4100, 1536), (4100, 1544)):
        for family in ("random", "offset", "exact"):
            check_norm_forward("ln", family, rows, cols, dtn, seed=3)
    check_norm_forward("ln", "random", 23328, 1152, dtn, seed=4)
    check_norm_forward("rms", "outlier", 6794, 3584, dtn, seed=5)


# ------------------------------------------------------------------------------ activations


def call_swiglu(gu, ldo):
    o = _ops()
    rows, inter = gu.shape[0], gu.shape[1] // 2
    big, out = nan_out(rows, inter, ldo, gu.dtype)
    o.check(o.lib().v3d_swiglu(o._p(gu), gu.stride(0), o._p(out), out.stride(0), rows, inter, o._code(gu), o._stream()), "v3d_swiglu")
    return out, untouched(big, inter)


def call_swiglu_grad(gu, dh, ldg):
    o = _ops()
    rows, two = gu.shape
    big, dgu = nan_out(rows, two, ldg, gu.dtype)
    o.check(o.lib().v3d_swiglu_grad(o._p(gu), gu.stride(0), o._p(dh), dh.stride(0), o._p(dgu), dgu.stride(0), rows, two // 2, o._code(gu), o._stream()),
            "v3d_swiglu_grad")
    return dgu, untouched(big, two)


def call_gelu(z, dy, kind, ldo):
    o = _ops()
    rows, cols = z.shape
    big, out = nan_out(rows, cols, ldo, z.dtype)
    if dy is None:
        o.check(o.lib().v3d_gelu(o._p(z), z.stride(0), o._p(out), out.stride(0), rows, cols, int(kind), o._code(z), o._stream()), "v3d_gelu")
    else:
        o.check(o.lib().v3d_gelu_grad(o._p(z), z.stride(0), o._p(dy), dy.stride(0), o._p(out), out.stride(0), rows, cols, int(kind), o._code(z), o._stream()),
                "v3d_gelu_grad")
    return out, untouched(big, cols)


def blockwise_ratio(ref_fn, got, args, block=1024):
    """Worst ratio with the f64 reference formed `block` rows at a time."""
    worst = 0.0
    for r0 in range(0, got.shape[0], block):
        worst = max(worst, rc.ratio(got[r0:r0 + block], ref_fn(*[a[r0:r0 + block] for a in args])))
    return worst


def swiglu_case(family, rows, inter, dt, seed=0):
    if family == "sweep":
        g, up = rc.sweep_rows(dt, inter, seed=seed, device="cuda")
        dh = torch.roll(up, 3, 1)
    else:
        g, up = rc.act_random(rows, inter, dt, seed=seed, device="cuda")
        dh = rc.act_random(rows, inter, dt, seed=seed + 1, device="cuda")[1]
    gu = padded(torch.cat([g, up], 1), 2 * inter + 24, 16)
    return gu, padded(dh, inter + 8, 8)


@pytest.mark.parametrize("dtn", list(DT))
@pytest.mark.parametrize("inter", [8, 1192, 18944])
def test_swiglu_forward_and_gradient(inter, dtn):
    dt = DT[dtn]
    cases = [("random", r) for r in (1, 5, 77, 300)] + [("sweep", 0)]
    if inter == 18944:
        cases = [("random", 1), ("random", 77), ("random", 6794)]           # the 7B model's MLP at its sequence length, once per dtype
    for family, rows in cases:
        gu, dh = swiglu_case(family, rows, inter, dt, seed=rows)
        h, clean = call_swiglu(gu, inter + 8)
        dgu, clean_g = call_swiglu_grad(gu, dh, 2 * inter + 16)
        what = (family, rows, inter, dtn)
        assert clean and clean_g, ("padding written", what)
        assert bool(torch.isfinite(h).all()) and bool(torch.isfinite(dgu).all()), ("not written / not finite", what)
        r = note("swiglu", dtn, blockwise_ratio(rc.swiglu, h, (gu,)))
        assert r < 1.0, (r, what)
        r = note("swiglu_grad", dtn, blockwise_ratio(rc.swiglu_grad, dgu, (gu, dh)))
        assert r < 1.0, (r, what)


@pytest.mark.parametrize("dtn", list(DT))
@pytest.mark.parametrize("kind", rc.GELU_KINDS)
@pytest.mark.parametrize("cols", [1160, 3584, 4304])
def test_gelu_forward_and_gradient_every_kind(cols, kind, dtn):
    """kind 0 = erf (the projector), 1 = tanh (the SigLIP MLP), 2 = ReLU (the grounding heads); random rows and the sweep of every
    representable value in [-64, 64], zeros of both signs included."""
    dt = DT[dtn]
    for family in ("random", "sweep"):
        z, dy = (rc.act_random(90, cols, dt, seed=cols, device="cuda") if family == "random" else rc.sweep_rows(dt, cols, seed=cols, device="cuda"))
        z, dy = padded(z, cols + 16, 8), padded(dy, cols + 40, 24)
        y, clean = call_gelu(z, None, kind, cols + 8)
        dz, clean_g = call_gelu(z, dy, kind, cols + 24)
        what = (family, cols, kind, dtn)
        assert clean and clean_g, ("padding written", what)
        assert bool(torch.isfinite(y).all()) and bool(torch.isfinite(dz).all()), ("not written / not finite", what)
        name = ("gelu_erf", "gelu_tanh", "relu")[kind]
        ref, refg = rc.gelu(z, kind), rc.gelu_grad(z, dy, kind)
        r = note(name, dtn, rc.ratio(y, ref))
        assert r < 1.0, (r, what, rc.worst_index(y, ref))
        r = note(name + "_grad", dtn, rc.ratio(dz, refg))
        assert r < 1.0, (r, what, rc.worst_index(dz, refg))


# ------------------------------------------------------------------------------ the rotation's transpose


@pytest.mark.parametrize("dtn", list(DT))
def test_rope_inverse_table_is_the_transpose_of_the_forward_rotation(dtn):
    """Training's backward rotates dq | dk by the inverse table (v3d/train.py: attn_block_backward); against the f64 transpose of the
    forward rotation with the forward table's 16-bit cos / sin, at 28 + 4 heads of 128.  The value columns are not touched."""
    from v3d import train
    o = _ops()
    dt = DT[dtn]
    n_q, n_kv, hd, tokens = 28, 4, 128, 333
    rope = train.RopeTables(hd, 512, 1e6, dt, "cuda")
    assert torch.equal(rope.inv.cos, rope.fwd.cos) and torch.equal(rope.inv.sin, -rope.fwd.sin)
    g = torch.Generator().manual_seed(6)
    width = (n_q + 2 * n_kv) * hd
    d = torch.randn(tokens, width, generator=g).to(dt).cuda()
    d[:, (n_q + n_kv) * hd:] = NAN                                   # the value columns: never read, never written
    src = padded(d, width + 64, 32)
    ref = rc.rope_transpose(src, rope.fwd.cos[:tokens], rope.fwd.sin[:tokens], n_q + n_kv, hd)
    o.rope_apply(src, n_q + n_kv, hd, rope.inv)
    got = src[:, :(n_q + n_kv) * hd].reshape(tokens, n_q + n_kv, hd)
    big = src._base if src._base is not None else src
    assert bool(torch.isnan(src[:, (n_q + n_kv) * hd:]).all()) and bool(torch.isnan(big[:, :32]).all()) and bool(torch.isnan(big[:, 32 + width:]).all())
    assert bool(torch.isfinite(got).all())
    r = note("rope_transpose", dtn, rc.ratio(got, ref))
    assert r < 1.0, (r, rc.worst_index(got, ref))


def test_zz_report_worst_ratios():
    """Not a check of its own: prints the worst |err| / bound per kernel and dtype of this run (each was asserted < 1 where it was measured)."""
    print("\nROWWISE_WORST " + json.dumps({k: round(v, 4) for k, v in sorted(WORST.items())}))
    assert all(v < 1.0 for v in WORST.values())
