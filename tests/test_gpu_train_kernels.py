"""First kernels of the training step (BASELINE configs[4]) against torch autograd on the CPU in f32 (a floating-point kernel:
the torch f32 reference is the checker, tolerances stated per test):
  * v3d_cross_entropy / _grad = the shifted CrossEntropyLoss of Qwen2ForCausalLM.forward (modeling_qwen2.py:1195-1205);
  * v3d_visual_tokens_grad = backward of get_2dPool (bilinear 27 -> 14) + PE add (passes through) + image_newline rows,
    composed as prepare_inputs_labels_for_multimodal does (llava_arch.py:191-210, 307-328, 506-517)."""
import math

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ops():
    from v3d import ops as _ops
    return _ops


@pytest.mark.parametrize("dt,tol", [(torch.float32, 2e-6), (torch.bfloat16, 2e-6), (torch.float16, 2e-6)])
@pytest.mark.parametrize("S,V", [(37, 320), (300, 1000), (64, 152064)])
def test_cross_entropy_and_gradient(ops, dt, tol, S, V):
    g = torch.Generator().manual_seed(S + V)
    logits = (torch.randn(S, V, generator=g) * 3).to(dt)
    labels = torch.randint(0, V, (S,), generator=g)
    labels[torch.rand(S, generator=g) < 0.4] = -100                      # prompt / visual rows carry IGNORE_INDEX
    labels[1] = 5                                                         # at least one valid target
    ref_in = logits.float().requires_grad_(True)                          # the reference casts the logits to f32 first (:1190-1192)
    ref = F.cross_entropy(ref_in[:-1], labels[1:], ignore_index=-100)
    ref.backward()
    loss, st = ops.cross_entropy(logits.cuda(), labels.cuda())
    assert abs(loss.item() - ref.item()) <= tol * max(1.0, abs(ref.item()))
    assert int(st[3][1].item()) == int((labels[1:] != -100).sum())
    grad = ops.cross_entropy_grad(st, dtype=torch.float32).cpu()
    assert grad.shape == (S, V) and not bool(grad[-1].any())              # nothing predicts past the last position
    assert torch.allclose(grad, ref_in.grad, rtol=1e-4, atol=1e-7)
    assert not bool(grad[:-1][labels[1:] == -100].any())
    if dt != torch.float32:                                               # gradient written in the logits' dtype
        g16 = ops.cross_entropy_grad(st, upstream=2.0).float().cpu()
        assert torch.allclose(g16, 2 * ref_in.grad, rtol=2e-2 if dt == torch.bfloat16 else 2e-3, atol=1e-6)


def test_cross_entropy_all_rows_ignored_is_nan(ops):
    logits = torch.randn(9, 64).cuda()
    labels = torch.full((9,), -100, dtype=torch.int64).cuda()
    loss, st = ops.cross_entropy(logits, labels)
    assert torch.isnan(loss) and int(st[3][1].item()) == 0               # torch's CrossEntropyLoss(mean) gives nan too


@pytest.mark.parametrize("dt,tol", [(torch.bfloat16, 1.2e-2), (torch.float16, 2e-3)])
def test_visual_tokens_backward(ops, dt, tol):
    V, C, side, n = 3, 256, 27, 14
    g = torch.Generator().manual_seed(7)
    feat = torch.randn(V, side * side, C, generator=g)
    newline = torch.randn(C, generator=g)
    pe = torch.randn(V, n * n, C, generator=g)                            # stands in for PE(voxel ids): no gradient flows into it
    up = torch.randn(V * n * (n + 1), C, generator=g).to(dt)             # upstream gradient d loss / d tokens
    f = feat.clone().requires_grad_(True)
    nl = newline.clone().requires_grad_(True)
    x = f.view(V, side, side, C).permute(0, 3, 1, 2)
    pooled = F.interpolate(x, size=[n, n], mode="bilinear").permute(0, 2, 3, 1)                  # get_2dPool, llava_arch.py:202-204
    tok = pooled + pe.view(V, n, n, C)                                                            # :515
    seq = torch.cat([tok, nl[None, None, None, :].expand(V, n, 1, C)], 2).reshape(-1, C)         # add_token_per_grid, :307-328
    (seq * up.float()).sum().backward()
    dfeat, dnl = ops.visual_tokens_grad(up.cuda(), V, side, n, newline=True)
    want = f.grad
    err = (dfeat.float().cpu() - want).abs()
    assert bool((err <= tol * (want.abs() + 1.0)).all()), err.max()
    assert torch.allclose(dnl.cpu(), nl.grad, rtol=1e-5, atol=1e-4)
    # without newline rows
    f2 = feat.clone().requires_grad_(True)
    pooled2 = F.interpolate(f2.view(V, side, side, C).permute(0, 3, 1, 2), size=[n, n], mode="bilinear").permute(0, 2, 3, 1)
    up2 = torch.randn(V * n * n, C, generator=g).to(dt)
    (pooled2.reshape(-1, C) * up2.float()).sum().backward()
    d2, none = ops.visual_tokens_grad(up2.cuda(), V, side, n, newline=False)
    assert none is None
    assert bool(((d2.float().cpu() - f2.grad).abs() <= tol * (f2.grad.abs() + 1.0)).all())


# ------------------------------------------------------------------------------ direct tests of the row kernels, f64 references

EPS = {torch.bfloat16: 2.0 ** -7, torch.float16: 2.0 ** -10}
SUBNORMAL_ULP = {torch.bfloat16: 2.0 ** -133, torch.float16: 2.0 ** -24}


def ulp_of(a, dt):
    """The spacing of dt's values at |a| (f64)."""
    a = a.double().abs()
    _, e = torch.frexp(a)
    u = torch.ldexp(torch.full_like(a, EPS[dt]), e - 1)
    return torch.where(a > 0, u, torch.zeros_like(a)).clamp_min(SUBNORMAL_ULP[dt])


def assert_ulp_close(got, want, dt, ulps=1.0, what=""):
    """|got - want| <= ulps ulp of dt at |want| + 1/16 ulp at max|want|, element by element (want: f64)."""
    got, want = got.double().cpu(), want.double()
    bound = ulps * ulp_of(want, dt) + ulp_of(want.abs().max(), dt) / 16
    err = (got - want).abs()
    ok = err <= bound
    assert bool(ok.all()), f"{what}: {int((~ok).sum())} elements out of bound, worst ratio {(err / bound).max().item():.3g}"


def infonce_ref(obj, query, positive, tau):
    """llava_qwen.py:298-308 in f64 autograd: normalize, scores, exp(s / tau), -log(sum over positives / sum)."""
    o = obj.double().requires_grad_(True)
    q = query.double().requires_grad_(True)
    s = (F.normalize(o) * F.normalize(q[None])).sum(-1)
    logits = torch.exp(s / tau)
    loss = -torch.log(logits[positive.bool()].sum() / logits.sum())
    loss.backward()
    return loss.detach(), s.detach(), o.grad, q.grad


def positive_sets(n, g):
    one = torch.zeros(n, dtype=torch.uint8)
    one[int(torch.randint(0, n, (1,), generator=g))] = 1
    several = (torch.rand(n, generator=g) < 0.3).to(torch.uint8)
    several[0] = 1
    last = torch.zeros(n, dtype=torch.uint8)
    last[-1] = 1                                                          # the zero-target row: a sample without labels
    return {"one": one, "several": several, "all": torch.ones(n, dtype=torch.uint8), "last": last}


def check_infonce(got, want, dt):
    loss, scores, dobj, dq = got
    wl, ws, wo, wq = want
    assert abs(loss.item() - wl.item()) <= 1e-5 * max(1.0, abs(wl.item())), (loss.item(), wl.item())
    assert (scores.double().cpu() - ws).abs().max().item() <= 1e-5
    assert_ulp_close(dobj, wo, dt, what="dobj")
    assert_ulp_close(dq, wq, dt, what="dquery")


@pytest.mark.parametrize("dt", [torch.bfloat16, torch.float16])
@pytest.mark.parametrize("C", [8, 1000, 1024, 3584])
@pytest.mark.parametrize("n", [1, 2, 5, 257, 1024])
def test_ground_infonce_vs_f64_autograd(ops, dt, C, n):
    """v3d_ground_infonce against the f64 autograd of the reference's loss: one, several, all (loss 0, gradients 0) and only the last
    row positive; the reference's temperature 0.07 and 1.0.  C = 1000 is not a multiple of the 64 lanes."""
    g = torch.Generator().manual_seed(n * 7 + C)
    obj = (torch.randn(n, C, generator=g) * 0.5 + 0.1).to(dt)
    query = torch.randn(C, generator=g).to(dt)
    for name, pos in positive_sets(n, g).items():
        for tau in (0.07, 1.0):
            got = ops.ground_infonce(obj.cuda(), query.cuda(), pos.cuda(), tau)
            want = infonce_ref(obj, query, pos, tau)
            check_infonce(got, want, dt)
            if name == "all" or n == 1:
                assert got[0].item() == 0.0 and not bool(got[2].any()) and not bool(got[3].any())
            again = ops.ground_infonce(obj.cuda(), query.cuda(), pos.cuda(), tau)
            for a, b in zip(got, again):                                  # one workgroup, fixed order: the same bits again
                assert torch.equal(a, b)


@pytest.mark.parametrize("dt", [torch.bfloat16, torch.float16])
def test_ground_infonce_strided_rows_and_limits(ops, dt):
    """obj as a column slice of a wider tensor (ldo > C) and dobj written with a row stride, through the library entry; n = 1025 is
    refused."""
    n, C = 300, 1000
    g = torch.Generator().manual_seed(3)
    wide = torch.randn(n, C + 24, generator=g).to(dt).cuda()
    obj = wide[:, 16:16 + C]
    query = torch.randn(C, generator=g).to(dt).cuda()
    pos = (torch.rand(n, generator=g) < 0.1).to(torch.uint8)
    pos[3] = 1
    loss = torch.empty(1, dtype=torch.float32, device="cuda")
    scores = torch.empty(n, dtype=torch.float32, device="cuda")
    dwide = torch.full((n, C + 40), 7.0, dtype=dt, device="cuda")
    dobj = dwide[:, 8:8 + C]
    dq = torch.empty(C, dtype=dt, device="cuda")
    pos_d = pos.cuda()
    ops.check(ops.lib().v3d_ground_infonce(ops._p(obj), obj.stride(0), n, ops._p(query), C, ops._p(pos_d), 0.07, ops._p(loss), ops._p(scores),
                                           ops._p(dobj), dobj.stride(0), ops._p(dq), ops._code(obj), ops._stream()), "v3d_ground_infonce")
    check_infonce((loss[0], scores, dobj, dq), infonce_ref(obj.cpu(), query.cpu(), pos, 0.07), dt)
    assert bool((dwide[:, :8] == 7).all()) and bool((dwide[:, 8 + C:] == 7).all())       # nothing written outside the rows' C columns
    with pytest.raises(ops.V3DError):
        ops.ground_infonce(torch.zeros(1025, 8, dtype=dt).cuda(), query[:8].contiguous(), torch.ones(1025, dtype=torch.uint8).cuda(), 0.07)


def masked_mean_grad_ref(mask, dobj):
    """dfeat[t] = sum_o mask[o, t] dobj[o] / count[o] in f64 (the gradient of y[rows].mean(0) per object, llava_arch.py:482-501)."""
    m = mask.double()
    count = m.sum(1, keepdim=True)
    return m.t() @ (dobj.double() / count.clamp_min(1))


def masks(n, T, g):
    mask = (torch.rand(n, T, generator=g) < 0.05).to(torch.uint8)
    if n > 1:
        mask[0] = 0                                                       # an object with an empty mask
    if n > 2:
        mask[1, : T // 2] = 1                                             # overlaps every other object's tokens in that half
        mask[2] = 1                                                       # a mask covering every token
    mask[:, T - 7:] = 0                                                   # tokens no object touches
    return mask


@pytest.mark.parametrize("dt", [torch.bfloat16, torch.float16])
@pytest.mark.parametrize("n,T,C", [(1, 1458, 3584), (50, 1458, 3584), (300, 1458, 3584), (50, 32 * 729, 3584), (300, 32 * 729, 8), (50, 1458, 8)])
def test_masked_mean_grad_vs_f64(ops, dt, n, T, C):
    """v3d_masked_mean_grad: accumulate=False overwrites every row (dfeat pre-filled with NaN; untouched rows exactly 0) and is within
    1 ulp of the f64 sum; accumulate=True leaves untouched rows' bits alone and gives T(T(sum) + old) on the others.  32 x 729 tokens at
    C = 3584 make the grid-stride loop run more than once.  Two calls give the same bits (objects added in order)."""
    g = torch.Generator().manual_seed(n + T + C)
    mask = masks(n, T, g)
    dobj = torch.randn(n, C, generator=g).to(dt)
    md, dd = mask.cuda(), dobj.cuda()
    touched = mask.bool().any(0)
    out = ops.masked_mean_grad(md, dd, torch.full((T, C), float("nan"), dtype=dt, device="cuda"), accumulate=False)
    got = out.cpu()
    assert not bool(torch.isnan(got).any())
    assert not bool(got[~touched].any())
    assert_ulp_close(got[touched], masked_mean_grad_ref(mask, dobj)[touched], dt, what="dfeat")
    again = ops.masked_mean_grad(md, dd, torch.empty((T, C), dtype=dt, device="cuda"), accumulate=False)
    assert torch.equal(out.view(torch.int16), again.view(torch.int16))
    old = torch.randn(T, C, generator=g).to(dt)
    acc = ops.masked_mean_grad(md, dd, old.cuda(), accumulate=True).cpu()
    assert torch.equal(acc[~touched].view(torch.int16), old[~touched].view(torch.int16))
    want = (got.float() + old.float()).to(dt)                             # T(T(sum) + old), T(sum) being the checked output above
    assert torch.equal(acc[touched].view(torch.int16), want[touched].view(torch.int16))
    if n == 50 and T == 1458 and C == 8:                                  # the f64 formula is autograd's gradient of the per-object means
        f = torch.randn(T, C, dtype=torch.float64, generator=g).requires_grad_(True)
        objs = torch.stack([f[mask[o].bool()].mean(0) for o in range(1, n)])
        (objs * dobj[1:].double()).sum().backward()
        assert torch.allclose(f.grad, masked_mean_grad_ref(mask[1:], dobj[1:]), rtol=1e-12, atol=1e-14)


def softmax_rows_ref(s, n_keys, scale, offset, dt):
    """causal_softmax_rows' rounding points (train.hip): x = T(s * scale) (the product in f32), p = T(softmax over j <= i + offset,
    j < n_keys), computed in f64; 0 in the other columns."""
    rows, cols = s.shape
    x = (s.float() * scale).to(dt).double()
    i = torch.arange(rows)[:, None]
    j = torch.arange(cols)[None, :]
    vis = (j <= i + offset) & (j < n_keys)
    x = x.masked_fill(~vis, -float("inf"))
    return torch.softmax(x, 1), vis


def softmax_grad_ref(p, dp, scale, dt):
    """ds = T(T(p (dp - sum_j p dp)) * scale), the sum in f64."""
    p64, dp64 = p.double(), dp.double()
    inner = (p64 * (dp64 - (p64 * dp64).sum(1, keepdim=True))).to(dt)
    return inner.double() * float(torch.tensor(scale, dtype=torch.float32))


@pytest.mark.parametrize("dt", [torch.bfloat16, torch.float16])
@pytest.mark.parametrize("cols", [8, 2048, 2056, 8192])
def test_causal_softmax_and_grad_rows_vs_f64(ops, dt, cols):
    """v3d_causal_softmax_rows and v3d_softmax_grad_rows against f64 at their rounding points: up to the 8192-column register limit,
    n_keys < cols, offset 0 and > 0, row strides wider than the row (library entry), and the aliased ds-into-dp call the attention
    backward makes (train.py), which must equal the out-of-place call bit for bit."""
    rows = 37 if cols < 8192 else 19
    scale = 1 / math.sqrt(128)
    g = torch.Generator().manual_seed(cols)
    for n_keys, offset in ((cols, 0), (max(1, cols - 5), 0), (max(1, cols - 13), 9), (cols, cols)):
        s = (torch.randn(rows, cols, generator=g) * 8).to(dt)
        want, vis = softmax_rows_ref(s, n_keys, scale, offset, dt)
        p = ops.causal_softmax_rows(s.cuda(), n_keys, scale, offset)
        assert_ulp_close(p, want, dt, what=f"p n_keys={n_keys} offset={offset}")
        assert not bool(p.cpu()[~vis].any()), "a column past the visible keys is not 0"
        assert torch.equal(p.view(torch.int16), ops.causal_softmax_rows(s.cuda(), n_keys, scale, offset).view(torch.int16))
        dp = torch.randn(rows, cols, generator=g).to(dt)
        ds = ops.softmax_grad_rows(p, dp.cuda(), scale)
        ds_want = softmax_grad_ref(p.cpu(), dp, scale, dt)
        # 2 ulps: ds is rounded twice, and where the f32 row sum and the f64 one put p (dp - sum) on the two sides of a rounding
        # boundary, the inner value moves one ulp - scale * ulp(inner) is up to 1.42 ulp of ds before the outer rounding
        assert_ulp_close(ds, ds_want, dt, ulps=2.0, what="ds")
        assert (ds.double().cpu() - ds_want.to(dt).double()).ne(0).double().mean().item() < 1e-3
        assert torch.equal(ds.view(torch.int16), ops.softmax_grad_rows(p, dp.cuda(), scale).view(torch.int16))
        dpa = dp.cuda()
        ops.softmax_grad_rows(p, dpa, scale, out=dpa)
        assert torch.equal(dpa.view(torch.int16), ds.view(torch.int16)), "in-place ds differs from the out-of-place one"
        # strided rows: s, p, dp and ds as column windows of wider buffers
        ws = torch.zeros(rows, cols + 24, dtype=dt, device="cuda")
        ws[:, 8:8 + cols] = s.cuda()
        wp = torch.full((rows, cols + 16), 3.0, dtype=dt, device="cuda")
        sv, pv = ws[:, 8:8 + cols], wp[:, :cols]
        ops.check(ops.lib().v3d_causal_softmax_rows(ops._p(sv), sv.stride(0), ops._p(pv), pv.stride(0), rows, n_keys, cols, offset, scale,
                                                    ops._code(sv), ops._stream()), "v3d_causal_softmax_rows")
        assert torch.equal(pv.view(torch.int16), p.view(torch.int16)) and bool((wp[:, cols:] == 3).all())
        wd = torch.zeros(rows, cols + 8, dtype=dt, device="cuda")
        wd[:, :cols] = dp.cuda()
        wo = torch.full((rows, cols + 32), 3.0, dtype=dt, device="cuda")
        dv, ov = wd[:, :cols], wo[:, 16:16 + cols]
        ops.check(ops.lib().v3d_softmax_grad_rows(ops._p(pv), pv.stride(0), ops._p(dv), dv.stride(0), ops._p(ov), ov.stride(0), rows, cols, scale,
                                                  ops._code(pv), ops._stream()), "v3d_softmax_grad_rows")
        assert torch.equal(ov.view(torch.int16), ds.view(torch.int16))
        assert bool((wo[:, :16] == 3).all()) and bool((wo[:, 16 + cols:] == 3).all())


def test_softmax_rows_refuse_more_than_8192_columns(ops):
    x = torch.zeros(2, 8200, dtype=torch.bfloat16, device="cuda")
    with pytest.raises(ops.V3DError):
        ops.causal_softmax_rows(x, 8200, 1.0)
    with pytest.raises(ops.V3DError):
        ops.softmax_grad_rows(x, x.clone(), 1.0)
