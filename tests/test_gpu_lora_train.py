"""LoRA on the decoder's frozen linears (v3d/train.py: lora_linear_forward / lora_linear_backward, lora_init, the language model's
step with adapters, AdamW over the trainable sub-tree) on the device.

One linear (S 200, K 256, N 384, r 16): with B = 0 (peft's init) the forward and dx are bit-identical to the base Linear's, dA is
exactly zero and dB is inside the kernel's bound; with a random B every product is inside its own f64 bound on the operands the device
gave it, and y, dx, dA, dB are inside the composed bound of the whole rule against the unrounded f64 chain (tests/lora_check.py).
The language model's step runs at tests/test_gpu_train_dense.py's own shape (H 512, I 1024, 4/2 heads of 128, V 1024, S 200, 2 layers)
with r 16 against f32 autograd of the same rule on the same 16-bit inputs, inside that test's bounds (2 % for the loss, 2.5e-2
norm-wise / 6e-2 element-wise for the gradients; the helpers are restated here).  One true-width layer (H 3584, I 18944, 28/4 heads,
S 512, r 64) checks the adapters' gradients per element against f64 on the activations the device forward itself produced, so that only
the LoRA products are under test.
"""
import math

import pytest
import torch
import torch.nn.functional as F

import gemm_check as gc
import lora_check as lc

pytestmark = pytest.mark.gpu
BF = torch.bfloat16


@pytest.fixture(scope="module")
def ops():
    assert torch.cuda.is_available()
    from v3d import ops as o
    return o


@pytest.fixture(scope="module")
def train():
    from v3d import train as t
    return t


def _close(got, ref, rel, elem, what, floor=1e-30):
    got, ref = got.float().cpu(), ref.float()
    err = (got - ref).norm() / ref.norm().clamp_min(floor)
    worst = (got - ref).abs().max() / ref.abs().max().clamp_min(floor)
    print(f"{what}: norm-wise {err:.3e}, element-wise {worst:.3e} of max |ref|")
    assert err < rel and worst < elem, f"{what}: norm-wise {err:.3e} (bound {rel}), element-wise {worst:.3e} of max |ref| (bound {elem})"
    return float(err), float(worst)


def _chunks(M, R, K, train=None, dtype=BF, x_dtype=BF):
    """Partial slabs of the wgrad kernel for this shape; 1 where the dispatch sends the product to the GEMM (one run over the rows)."""
    from v3d import _native
    if train is not None and not train._wgrad_on_kernel(K, dtype, x_dtype):
        return 1
    return -(-M // _native.lib().v3d_lora_wgrad_chunk(M, R, K))


ROUTES = {"default": {}, "kernels": {"V3D_LORA_DOWN": "kernel", "V3D_LORA_WGRAD": "kernel"}, "gemms": {"V3D_LORA_DOWN": "gemm", "V3D_LORA_WGRAD": "gemm"}}


def _route(monkeypatch, name):
    for k in ("V3D_LORA_DOWN", "V3D_LORA_WGRAD"):
        monkeypatch.delenv(k, raising=False)
    for k, v in ROUTES[name].items():
        monkeypatch.setenv(k, v)


def _one_linear(train, seed, zero_b, dt=BF, S=200, K=256, N=384, r=16, alpha=16):
    g = torch.Generator(device="cuda").manual_seed(seed)
    mk = lambda *shape, s=1.0: (torch.randn(*shape, generator=g, device="cuda") * s).to(dt)
    x, w, dy = mk(S, K), mk(N, K, s=K ** -0.5), mk(S, N)
    leaves = {"A": mk(r, K, s=K ** -0.5), "B": torch.zeros(N, r, dtype=dt, device="cuda") if zero_b else mk(N, r, s=0.3)}
    return x, w, dy, leaves, train.LoraState(leaves, alpha / r)


@pytest.mark.parametrize("route", list(ROUTES))
def test_zero_b_changes_nothing_and_da_is_zero(ops, train, monkeypatch, route):
    _route(monkeypatch, route)
    x, w, dy, leaves, st = _one_linear(train, 1, zero_b=True)
    y, up = train.lora_linear_forward(x, w, leaves, st)
    u = up[:, :st.R]
    assert bool((up[:, st.R:] == 0).all())
    assert torch.equal(y, ops.gemm(x, w)), "B = 0: the forward differs from the base Linear's"
    dx, g = train.lora_linear_backward(x, w, leaves, st, up, dy)
    dx_base, _, _ = train.linear_backward(x, w, dy, need_dw=False)
    assert torch.equal(dx, dx_base), "B = 0: dx differs from linear_backward's"
    assert g["A"].shape == leaves["A"].shape and bool((g["A"] == 0).all()), "B = 0: dA is not exactly zero"
    assert g["B"].shape == leaves["B"].shape
    ref = lc.wgrad_reference(u, dy, st.s, g["B"].dtype, _chunks(*u.shape, dy.shape[1], train))
    v = lc.verdict(g["B"].t(), ref)
    print(f"B = 0: dB worst |err| / bound {v['ratio']:.3f}")
    assert v["ratio"] <= 1.0 and float(g["B"].float().abs().max()) > 0


@pytest.mark.parametrize("dt", [torch.bfloat16, torch.float16], ids=["bf16", "f16"])
@pytest.mark.parametrize("gd", ["f32", "same"])
@pytest.mark.parametrize("route", list(ROUTES))
def test_random_b_every_product_and_the_whole_rule_against_f64(ops, train, monkeypatch, dt, gd, route):
    _route(monkeypatch, route)
    x, w, dy, leaves, st = _one_linear(train, 2, zero_b=False, dt=dt)
    gdt = torch.float32 if gd == "f32" else dt
    A, B, s = leaves["A"], leaves["B"], st.s
    S, K = x.shape
    N, r = B.shape
    y, up = train.lora_linear_forward(x, w, leaves, st)
    dx, g = train.lora_linear_backward(x, w, leaves, st, up, dy, grad_dtype=gdt)
    u = up[:, :r]
    ca, cb = _chunks(S, r, K, train, gdt, dt), _chunks(S, r, N, train, gdt, dt)
    # each product on the operands the device gave it
    assert lc.verdict(u, lc.down_reference(x, A, 1.0))["ratio"] <= 1.0 and bool((up[:, r:] == 0).all())
    assert gc.compare(y, up, st.sB, res=ops.gemm(x, w), epi=gc.EPI_RES)["ratio"] <= 1.0
    dup = train.lora_down(dy, st.Bt, st.sBtp, s, st.R, st.Rp)          # deterministic: the bits the backward used
    du = dup[:, :r]
    assert lc.verdict(du, lc.down_reference(dy, B.t().contiguous(), s))["ratio"] <= 1.0 and bool((dup[:, r:] == 0).all())
    dx_base, _, _ = train.linear_backward(x, w, dy, need_dw=False)
    assert gc.compare(dx, dup, st.At, res=dx_base, epi=gc.EPI_RES)["ratio"] <= 1.0
    assert lc.verdict(g["A"], lc.wgrad_reference(du, x, 1.0, gdt, ca))["ratio"] <= 1.0
    assert lc.verdict(g["B"].t(), lc.wgrad_reference(u, dy, s, gdt, cb))["ratio"] <= 1.0
    # the whole rule against the unrounded f64 chain
    b = lc.linear_bounds(x, w, None, A, B, s, dy, gdt, ca, cb)
    f64 = lc.lora_linear_grads_f64(x, w, A, B, s, dy)
    assert torch.equal(b["dx"][0], f64["dx"]) and torch.equal(b["dA"][0], f64["dA"]) and torch.equal(b["dB"][0], f64["dB"])
    assert torch.allclose(b["y"][0], lc.lora_linear_f64(x, w, None, A, B, s), rtol=1e-13, atol=1e-13)
    worst = {n: lc.worst_ratio(t, *b[n]) for n, t in (("y", y), ("dx", dx), ("dA", g["A"]), ("dB", g["B"]))}
    print(f"whole rule {dt} grads {gdt}: worst |err| / bound {worst}")
    assert all(v <= 1.0 for v in worst.values()), worst
    # the adapter matters: y and dx are NOT the base Linear's
    assert not torch.equal(y, ops.gemm(x, w)) and not torch.equal(dx, dx_base)


# ------------------------------------------------------------------------------ the language model's step


def _rmsnorm_ref(x, w, eps):
    var = x.pow(2).mean(-1, keepdim=True)
    return w * (x * torch.rsqrt(var + eps))


def _rope_ref(x, n_heads, hd, base=1e6):
    S = x.shape[0]
    inv = 1.0 / (base ** (torch.arange(0, hd, 2, dtype=torch.int64).float() / hd))
    ang = torch.arange(S, dtype=torch.float32)[:, None] * inv[None, :]
    cos, sin = torch.cat([ang, ang], -1).cos()[:, None, :], torch.cat([ang, ang], -1).sin()[:, None, :]
    xh = x.view(S, n_heads, hd)
    rot = torch.cat([-xh[..., hd // 2:], xh[..., :hd // 2]], -1)
    return (xh * cos + rot * sin).reshape(S, n_heads * hd)


def _attention_ref(q, k, v, n_q, n_kv, hd):
    S = q.shape[0]
    qh = q.view(S, n_q, hd).transpose(0, 1)
    kh = k.view(S, n_kv, hd).transpose(0, 1).repeat_interleave(n_q // n_kv, 0)
    vh = v.view(S, n_kv, hd).transpose(0, 1).repeat_interleave(n_q // n_kv, 0)
    s = qh @ kh.transpose(1, 2) / hd ** 0.5
    s = s + torch.full((S, S), float("-inf")).triu(1)
    return (torch.softmax(s, -1) @ vh).transpose(0, 1).reshape(S, n_q * hd)


def _lin(x, w, ad, s, bias=None):
    y = x @ w.t() + s * ((x @ ad["A"].t()) @ ad["B"].t())
    return y + bias if bias is not None else y


def _layer_ref(h, p, s, n_q, n_kv, hd, eps):
    n = _rmsnorm_ref(h, p["ln1"], eps)
    qkv = _lin(n, p["qkv"], p["lora"]["qkv"], s, p["qkv_bias"])
    q = _rope_ref(qkv[:, :n_q * hd], n_q, hd)
    k = _rope_ref(qkv[:, n_q * hd:(n_q + n_kv) * hd], n_kv, hd)
    o = _attention_ref(q, k, qkv[:, (n_q + n_kv) * hd:], n_q, n_kv, hd)
    mid = h + _lin(o, p["o"], p["lora"]["o"], s)
    inter = p["gate_up"].shape[0] // 2
    n2 = _rmsnorm_ref(mid, p["ln2"], eps)
    gu = _lin(n2, p["gate_up"], p["lora"]["gate_up"], s)
    a = F.silu(gu[:, :inter]) * gu[:, inter:]
    return mid + _lin(a, p["down"], p["lora"]["down"], s)


SHAPE = dict(H=512, I=1024, n_q=4, n_kv=2, hd=128, V=1024, S=200, L=2, r=16, alpha=16)


def _model(train, seed=21, random_b=True):
    c = SHAPE
    H, I, n_q, n_kv, hd, V, S, L = c["H"], c["I"], c["n_q"], c["n_kv"], c["hd"], c["V"], c["S"], c["L"]
    g = torch.Generator().manual_seed(seed)
    width = (n_q + 2 * n_kv) * hd
    mk = lambda *shape, s=1.0: (torch.randn(*shape, generator=g) * s).to(BF)
    ln = lambda: (1 + 0.1 * torch.randn(H, generator=g)).to(BF)
    layers = [{"ln1": ln(), "qkv": mk(width, H, s=H ** -0.5), "qkv_bias": mk(width, s=0.3), "o": mk(H, n_q * hd, s=(n_q * hd) ** -0.5),
               "ln2": ln(), "gate_up": mk(2 * I, H, s=H ** -0.5), "down": mk(H, I, s=I ** -0.5)} for _ in range(L)]
    params = {"layers": layers, "norm": ln(), "lm_head": mk(V, H, s=H ** -0.5)}
    x = mk(S, H)
    labels = torch.full((S,), -100, dtype=torch.int64)
    labels[150:] = torch.randint(0, V, (50,), generator=g)
    dev = train._tree_map(lambda t: t.cuda(), params)
    for p in dev["layers"]:
        p["qkv_rows"] = (n_q * hd, n_kv * hd, n_kv * hd)
    train.lora_init(dev, r=c["r"], alpha=c["alpha"], seed=seed)
    if random_b:                                   # away from peft's B = 0, where every dA is zero and dx does not see the adapters
        for p in dev["layers"]:
            for name, ad in p["lora"].items():
                st = p["lora_state"][name]
                for r0, r1, c0, c1 in st.blocks:
                    ad["B"][r0:r1, c0:c1] = (torch.randn(r1 - r0, c1 - c0, generator=g) * 0.05).to(BF).cuda()
        train.lora_refresh(dev)
    return dev, x.cuda(), labels.cuda()


def _block_mask(st, like):
    m = torch.zeros(like.shape, dtype=torch.bool)
    for r0, r1, c0, c1 in st.blocks:
        m[r0:r1, c0:c1] = True
    return m


def test_lora_init_is_pefts(train):
    dev, _, _ = _model(train, random_b=False)
    r = SHAPE["r"]
    for p in dev["layers"]:
        assert sorted(p["lora"]) == sorted(train.LORA_LINEARS)
        for name, ad in p["lora"].items():
            n_mod = len(train.LORA_MODULES[name])
            assert ad["A"].shape == (n_mod * r, p[name].shape[1]) and ad["B"].shape == (p[name].shape[0], n_mod * r)
            assert bool((ad["B"] == 0).all())
            bound = 1.0 / math.sqrt(p[name].shape[1])                # kaiming_uniform_(a = sqrt 5): U(-1 / sqrt(fan_in), 1 / sqrt(fan_in))
            a = ad["A"].float()
            assert float(a.abs().max()) <= bound * (1 + 2 ** -8) and float(a.abs().max()) > 0.9 * bound and abs(float(a.mean())) < 0.1 * bound


def test_llm_step_with_adapters_matches_autograd(ops, train):
    c = SHAPE
    n_q, n_kv, hd, L = c["n_q"], c["n_kv"], c["hd"], c["L"]
    s = c["alpha"] / c["r"]
    dev, x, labels = _model(train)
    keep = ("ln1", "qkv", "qkv_bias", "o", "ln2", "gate_up", "down", "lora")
    ref = {"layers": [{k: train._tree_map(lambda t: t.float().cpu().requires_grad_(), p[k]) for k in keep} for p in dev["layers"]],
           "norm": dev["norm"].float().cpu().requires_grad_(), "lm_head": dev["lm_head"].float().cpu().requires_grad_()}
    xr = x.float().cpu().requires_grad_()
    h = xr
    for p in ref["layers"]:
        h = _layer_ref(h, p, s, n_q, n_kv, hd, 1e-6)
    logits = _rmsnorm_ref(h, ref["norm"], 1e-6) @ ref["lm_head"].t()
    ref_loss = F.cross_entropy(logits[:-1], labels.cpu()[1:], ignore_index=-100)
    ref_loss.backward()
    rope = train.RopeTables(hd, 512, 1e6, BF, "cuda")
    frozen_before = [{k: p[k].clone() for k in train.LORA_FROZEN} for p in dev["layers"]]
    loss, dx, grads = train.llm_forward_backward(dev, x, labels, rope, n_q, n_kv, hd)
    rel = abs(float(loss) - float(ref_loss.detach())) / float(ref_loss.detach())
    print(f"loss {float(loss):.5f} vs autograd {float(ref_loss.detach()):.5f}: {rel:.3e} relative")
    assert rel < 2e-2
    worst = [_close(dx, xr.grad, 2.5e-2, 6e-2, "d inputs_embeds")]
    _close(grads["norm"], ref["norm"].grad, 2.5e-2, 6e-2, "d norm")
    _close(grads["lm_head"], ref["lm_head"].grad, 2.5e-2, 6e-2, "d lm_head")
    for i in range(L):
        gl = grads["layers"][i]
        assert sorted(gl) == ["ln1", "ln2", "lora", "qkv_bias"], f"a frozen leaf has a gradient entry: {sorted(gl)}"
        for k in ("ln1", "ln2", "qkv_bias"):
            _close(gl[k], ref["layers"][i][k].grad, 2.5e-2, 6e-2, f"layer {i} d {k}")
        for name in train.LORA_LINEARS:
            st = dev["layers"][i]["lora_state"][name]
            worst.append(_close(gl["lora"][name]["A"], ref["layers"][i]["lora"][name]["A"].grad, 2.5e-2, 6e-2, f"layer {i} d {name}.A"))
            rb = ref["layers"][i]["lora"][name]["B"].grad
            m = _block_mask(st, rb)
            assert bool((gl["lora"][name]["B"].cpu()[~m] == 0).all()), "an off-diagonal block of a stacked B has a gradient"
            worst.append(_close(gl["lora"][name]["B"].cpu() * m, rb * m, 2.5e-2, 6e-2, f"layer {i} d {name}.B"))
    print(f"worst over dx and the adapter gradients: norm-wise {max(w[0] for w in worst):.3e}, element-wise {max(w[1] for w in worst):.3e}")
    # the gradient tree is the trainable tree
    tt = train.trainable_tree(dev)
    assert train._paths(tt) == train._paths(grads)
    # frozen further: no entry, and the result keeps trainable_tree's structure
    fz = ("lm_head", "norm", "ln1", "ln2", "qkv_bias")
    loss2, dx2, g2 = train.llm_forward_backward(dev, x, labels, rope, n_q, n_kv, hd, frozen=fz)
    assert train._paths(g2) == train._paths(train.trainable_tree(dev, fz)) and all(sorted(g) == ["lora"] for g in g2["layers"])
    assert float(loss2) == float(loss) and torch.equal(dx2, dx)
    # recompute=True: bit-identical gradients
    loss3, dx3, g3 = train.llm_forward_backward(dev, x, labels, rope, n_q, n_kv, hd, recompute=True)
    assert float(loss3) == float(loss) and torch.equal(dx3, dx)
    for a, b in zip(train._leaves(grads), train._leaves(g3)):
        assert torch.equal(a, b)
    # three AdamW steps over the trainable tree: the frozen tensors do not move, the off-diagonal blocks stay zero, the loss goes down
    opt = train.AdamW(tt, lr=2e-3)
    losses = [float(loss)]
    for _ in range(3):
        opt.step(tt, grads)
        train.lora_refresh(dev)
        loss, _, grads = train.llm_forward_backward(dev, x, labels, rope, n_q, n_kv, hd)
        losses.append(float(loss))
    print("losses over three AdamW steps:", losses)
    assert losses[-1] < losses[0]
    for p, before in zip(dev["layers"], frozen_before):
        for k in train.LORA_FROZEN:
            assert torch.equal(p[k], before[k]), f"frozen {k} moved"
        for name, ad in p["lora"].items():
            m = _block_mask(p["lora_state"][name], ad["B"])
            assert bool((ad["B"].cpu()[~m] == 0).all()), "an off-diagonal block of a stacked B left zero"
    assert len(train._leaves_of_state(opt.state)) == len(train._paths(tt)), "optimizer state exists for trainable leaves only"


def test_training_loss_with_adapters_agrees_with_the_merged_weights(train):
    """The loss of the step with adapters against the loss of the same model with every adapter merged into its weight by
    lora_merge_weight and no adapters: within the step test's 2 %."""
    c = SHAPE
    dev, x, labels = _model(train, seed=33)
    rope = train.RopeTables(c["hd"], 512, 1e6, BF, "cuda")
    loss, _, _ = train.llm_forward_backward(dev, x, labels, rope, c["n_q"], c["n_kv"], c["hd"])
    merged = {"layers": [], "norm": dev["norm"], "lm_head": dev["lm_head"]}
    for p in dev["layers"]:
        q = {k: p[k] for k in ("ln1", "qkv_bias", "ln2")}
        for name in train.LORA_LINEARS:
            q[name] = train.lora_merge_weight(p[name], p["lora"][name], p["lora_state"][name])
            assert not torch.equal(q[name], p[name])
        merged["layers"].append(q)
    loss_m, _, _ = train.llm_forward_backward(merged, x, labels, rope, c["n_q"], c["n_kv"], c["hd"])
    rel = abs(float(loss) - float(loss_m)) / float(loss_m)
    print(f"loss with adapters {float(loss):.5f}, merged {float(loss_m):.5f}: {rel:.3e} relative")
    assert rel < 2e-2


@pytest.mark.parametrize("N,K,r,stacked", [(512, 256, 16, False), (4608, 3584, 64, True)])
@pytest.mark.parametrize("dt", [torch.bfloat16, torch.float16], ids=["bf16", "f16"])
def test_merged_weights_per_element_against_f64(train, dt, N, K, r, stacked):
    g = torch.Generator(device="cuda").manual_seed(N + r)
    mk = lambda *shape, s=1.0: (torch.randn(*shape, generator=g, device="cuda") * s).to(dt)
    w = mk(N, K, s=K ** -0.5)
    s = 16.0 / r
    if stacked:                                    # q | k | v of the 7B decoder: 3584 + 512 + 512 rows, R = 3 r, B block-diagonal
        rows = (3584, 512, 512)
        A, B, blocks = train.lora_stack([mk(r, K, s=K ** -0.5) for _ in rows], [mk(n, r, s=0.1) for n in rows])
    else:
        A, B, blocks = mk(r, K, s=K ** -0.5), mk(N, r, s=0.1), None
    leaves = {"A": A, "B": B}
    st = train.LoraState(leaves, s, blocks)
    got = train.lora_merge_weight(w, leaves, st)
    exact = w.double() + s * (B.double() @ A.double())
    ratio = lc.worst_ratio(got, exact, lc.merge_bound(w, A, B, s))
    unequal = int((got.double() != lc.merge_f64(w, A, B, s)).sum())
    print(f"merge {dt} {N}x{K} r={r}: worst |err| / bound {ratio:.3f}; {unequal} of {N * K} differ from the f64 rule's rounding")
    assert ratio <= 1.0
    assert unequal <= 1e-3 * N * K                 # the f32 product may sit on the other side of a rounding boundary of s B A, rarely
    if stacked:                                    # the block structure is honoured: row block i only sees its own A rows
        for (r0, r1, c0, c1) in blocks:
            own = w[r0:r1].double() + s * (B[r0:r1, c0:c1].double() @ A[c0:c1].double())
            assert lc.worst_ratio(got[r0:r1], own, lc.merge_bound(w[r0:r1], A[c0:c1], B[r0:r1, c0:c1], s)) <= 1.0
    z = {"A": A, "B": torch.zeros_like(B)}
    assert torch.equal(train.lora_merge_weight(w, z, train.LoraState(z, s, blocks)), w), "a B = 0 adapter changed the weight"


@pytest.mark.parametrize("route", ["default", "kernels"])
def test_true_width_layer_adapter_gradients_against_f64(ops, train, monkeypatch, route):
    """One decoder layer at the 7B widths (H 3584, I 18944, 28 / 4 heads, S 512, r 64): every lora_linear_backward call is recorded
    and its u, dA and dB are held per element to the f64 bound on the operands the device itself passed in."""
    _route(monkeypatch, route)
    H, I, n_q, n_kv, hd, S, r = 3584, 18944, 28, 4, 128, 512, 64
    g = torch.Generator(device="cuda").manual_seed(7)
    width = (n_q + 2 * n_kv) * hd
    mk = lambda *shape, s=1.0: (torch.randn(*shape, generator=g, device="cuda") * s).to(BF)
    ln = lambda: (1 + 0.1 * torch.randn(H, generator=g, device="cuda")).to(BF)
    p = {"ln1": ln(), "qkv": mk(width, H, s=H ** -0.5), "qkv_bias": mk(width, s=0.3), "o": mk(H, n_q * hd, s=(n_q * hd) ** -0.5),
         "ln2": ln(), "gate_up": mk(2 * I, H, s=H ** -0.5), "down": mk(H, I, s=I ** -0.5), "qkv_rows": (n_q * hd, n_kv * hd, n_kv * hd)}
    params = {"layers": [p]}
    train.lora_init(params, r=r, alpha=16, seed=1)
    for name, ad in p["lora"].items():
        for r0, r1, c0, c1 in p["lora_state"][name].blocks:
            ad["B"][r0:r1, c0:c1] = mk(r1 - r0, c1 - c0, s=0.05)
    train.lora_refresh(params)
    calls = []
    real = train.lora_linear_backward

    def recording(x, w, leaves, state, up, dy, **kw):
        out = real(x, w, leaves, state, up, dy, **kw)
        calls.append((x, leaves, state, up, dy, out[1]))
        return out
    monkeypatch.setattr(train, "lora_linear_backward", recording)
    rope = train.RopeTables(hd, 512, 1e6, BF, "cuda")
    h, dout = mk(S, H), mk(S, H)
    out, saved = train.decoder_layer_forward(h, p, rope, n_q, n_kv, hd)
    dh, grads = train.decoder_layer_backward(dout, saved, p, rope, n_q, n_kv, hd)
    assert len(calls) == 4 and sorted(grads) == ["ln1", "ln2", "lora", "qkv_bias"]
    for x, leaves, st, up, dy, gl in calls:
        M, K = x.shape
        N = dy.shape[1]
        u = up[:, :st.R]
        v_u = lc.verdict(u, lc.down_reference(x, leaves["A"], 1.0))
        du = train.lora_down(dy, st.Bt, st.sBtp, st.s, st.R, st.Rp)[:, :st.R]      # deterministic: the bits the backward used
        v_du = lc.verdict(du, lc.down_reference(dy, leaves["B"].t().contiguous(), st.s))
        v_a = lc.verdict(gl["A"], lc.wgrad_reference(du, x, 1.0, gl["A"].dtype, _chunks(M, st.R, K, train)))
        dbt = lc.wgrad_reference(u, dy, st.s, gl["B"].dtype, _chunks(M, st.R, N, train))
        keep = torch.zeros(gl["B"].shape, dtype=torch.bool, device="cuda")
        for r0, r1, c0, c1 in st.blocks:
            keep[r0:r1, c0:c1] = True
        assert bool((gl["B"][~keep] == 0).all())
        err = ((gl["B"].double() - dbt["out"].t()).abs() / dbt["bound"].t())[keep].max().item()
        print(f"true width K={K} N={N} R={st.R}: worst |err| / bound u {v_u['ratio']:.3f}, du {v_du['ratio']:.3f}, dA {v_a['ratio']:.3f}, dB {err:.3f}")
        assert max(v_u["ratio"], v_du["ratio"], v_a["ratio"], err) <= 1.0


def test_dropout_and_bias_are_refused_by_name(train):
    from v3d._native import V3DError
    with pytest.raises(V3DError, match="lora_dropout"):
        train.LoraConfig(r=16, lora_dropout=0.05).validate()
    assert train.LoraConfig(r=16, lora_dropout=0.05).validate(for_merge=True).scaling == 1.0
    with pytest.raises(V3DError, match="lora_bias"):
        train.LoraConfig(r=16, bias="all").validate()
    with pytest.raises(V3DError, match="lora_r"):
        train.LoraConfig(r=24).validate()
    dev, _, _ = _model(train, random_b=False)
    with pytest.raises(V3DError, match="ZeroAdamW: lora"):
        train.ZeroAdamW(dev)


# ------------------------------------------------------------------------------ the trainer-facing module with adapters


def _reference_sd(seed=91):
    """A one-layer tower + one-layer decoder checkpoint in the reference's keys (the shape of tests/test_gpu_train_dense.py's trainer-surface
    test, restated), with an infonce grounding head."""
    from v3d.train_module import VIT
    Hv, inter, H, I, n_q, n_kv, hd, V = 1152, 4304, 512, 768, 4, 2, 128, 512
    g = torch.Generator().manual_seed(seed)
    mk = lambda *shape, s=1.0: (torch.randn(*shape, generator=g) * s).to(BF)
    ln = lambda n_: (1 + 0.1 * torch.randn(n_, generator=g)).to(BF)
    sd = {VIT + "embeddings.patch_embedding.weight": mk(Hv, 3, 14, 14, s=588 ** -0.5), VIT + "embeddings.patch_embedding.bias": mk(Hv, s=0.1),
          VIT + "embeddings.position_embedding.weight": mk(729, Hv, s=0.5)}
    p = VIT + "encoder.layers.0."
    for n_ in ("q_proj", "k_proj", "v_proj", "out_proj"):
        sd[p + f"self_attn.{n_}.weight"], sd[p + f"self_attn.{n_}.bias"] = mk(Hv, Hv, s=Hv ** -0.5), mk(Hv, s=0.2)
    for n_ in ("layer_norm1", "layer_norm2"):
        sd[p + n_ + ".weight"], sd[p + n_ + ".bias"] = ln(Hv), mk(Hv, s=0.1)
    sd[p + "mlp.fc1.weight"], sd[p + "mlp.fc1.bias"] = mk(inter, Hv, s=Hv ** -0.5), mk(inter, s=0.2)
    sd[p + "mlp.fc2.weight"], sd[p + "mlp.fc2.bias"] = mk(Hv, inter, s=inter ** -0.5), mk(Hv, s=0.2)
    sd["model.mm_projector.0.weight"], sd["model.mm_projector.0.bias"] = mk(H, Hv, s=Hv ** -0.5), mk(H, s=0.1)
    sd["model.mm_projector.2.weight"], sd["model.mm_projector.2.bias"] = mk(H, H, s=H ** -0.5), mk(H, s=0.1)
    sd["model.image_newline"], sd["model.embed_tokens.weight"] = mk(H, s=0.5), mk(V, H, s=0.5)
    p = "model.layers.0."
    sd[p + "self_attn.q_proj.weight"], sd[p + "self_attn.q_proj.bias"] = mk(n_q * hd, H, s=H ** -0.5), mk(n_q * hd, s=0.3)
    for n_ in ("k_proj", "v_proj"):
        sd[p + f"self_attn.{n_}.weight"], sd[p + f"self_attn.{n_}.bias"] = mk(n_kv * hd, H, s=H ** -0.5), mk(n_kv * hd, s=0.3)
    sd[p + "self_attn.o_proj.weight"] = mk(H, n_q * hd, s=(n_q * hd) ** -0.5)
    sd[p + "mlp.gate_proj.weight"], sd[p + "mlp.up_proj.weight"], sd[p + "mlp.down_proj.weight"] = mk(I, H, s=H ** -0.5), mk(I, H, s=H ** -0.5), mk(H, I, s=I ** -0.5)
    sd[p + "input_layernorm.weight"], sd[p + "post_attention_layernorm.weight"] = ln(H), ln(H)
    sd["model.norm.weight"], sd["lm_head.weight"] = ln(H), mk(V, H, s=H ** -0.5)
    sd["ground_head_zero_target"] = mk(H)
    for head in ("ground_head_obj", "ground_head_query"):
        sd.update({f"{head}.0.weight": mk(H, H, s=H ** -0.5), f"{head}.0.bias": mk(H, s=0.1), f"{head}.2.weight": 1 + mk(H, s=0.1),
                   f"{head}.2.bias": mk(H, s=0.1), f"{head}.3.weight": mk(H, H, s=H ** -0.5), f"{head}.3.bias": mk(H, s=0.1)})
    frames = 2
    images = torch.randn(frames, 3, 384, 384, generator=g)
    coords = (torch.rand(frames, 384, 384, 3, generator=g) - 0.5) * torch.tensor([20.0, 20.0, 8.0])
    t_ = torch.randint(0, 490, (30,), generator=g)
    input_ids = torch.cat([t_[:9], torch.tensor([-200]), t_[9:]])
    labels = torch.full((31,), -100, dtype=torch.int64)
    labels[20:] = input_ids[20:]
    return sd, (n_q, n_kv, hd, V), (input_ids, labels, images, coords)


def _randomise_b(model, seed=5):
    g = torch.Generator().manual_seed(seed)
    for L in model._full["llm"]["layers"]:
        for name, ad in L["lora"].items():
            for r0, r1, c0, c1 in L["lora_state"][name].blocks:
                ad["B"][r0:r1, c0:c1] = (torch.randn(r1 - r0, c1 - c0, generator=g) * 0.05).to(BF).cuda()


def test_module_with_adapters_backward_fills_only_trainable_grads(ops, train, monkeypatch, tmp_path):
    """LlavaQwenTrainable(lora=LoraConfig(...)): only the adapters and the non-frozen leaves are nn.Parameters, loss.backward() fills their
    .grad alone - bit-identical to train.sample_forward_backward(frozen=) - the frozen tower's backward is not run, a torch optimizer step
    moves no frozen tensor, and save_lora -> load_lora is exact."""
    from v3d import loader as L
    from v3d.train_module import LORA_DEFAULT_FROZEN, LlavaQwenTrainable, _flatten
    sd, (n_q, n_kv, hd, V), (input_ids, labels, images, coords) = _reference_sd()
    model = LlavaQwenTrainable.from_reference_state_dict(sd, n_q, n_kv, max_pos=1024, lora=train.LoraConfig(r=16, lora_alpha=16))
    _randomise_b(model)
    assert model.frozen == LORA_DEFAULT_FROZEN
    want_names = sorted([f"llm.layers.0.lora.{n}.{w}" for n in train.LORA_LINEARS for w in "AB"] +
                        ["projector.w1", "projector.b1", "projector.w2", "projector.b2", "newline"])
    assert sorted(model.names) == want_names and len(list(model.parameters())) == len(want_names)
    before = {k: v.clone() for k, v in model.reference_state_dict().items()}
    assert set(before) == set(sd) and all(torch.equal(before[k].cpu(), sd[k]) for k in sd)      # the base checkpoint, exactly

    def no_tower_backward(*a, **k):
        raise AssertionError("the frozen tower's backward was run")
    monkeypatch.setattr(train, "siglip_tower_backward", no_tower_backward)
    loss = model(input_ids, labels, images, coords)
    assert loss.requires_grad
    loss.backward()
    assert all(p.grad is not None and bool(torch.isfinite(p.grad.float()).all()) for p in model.parameters())
    assert all(float(p.grad.float().abs().max()) > 0 for n, p in zip(model.names, model._params)), "a trainable leaf got a zero gradient"
    # the same gradients as the explicit step on the same tensors
    frames = images.shape[0]
    patches = ops.patchify(images.to(BF).cuda(), 14, 640)
    _, _, vox = ops.coord_pool_voxel(coords.to(BF).cuda(), want_avg=False, want_vox=False)
    full = torch.cat([labels[:9], torch.full((frames * 210,), -100, dtype=torch.int64), labels[10:]]).cuda()
    loss2, grads = train.sample_forward_backward(model.param_tree(), patches, vox, model.pe_table, input_ids[:9].cuda(), input_ids[10:].cuda(), full,
                                                 model.rope, frames, n_q, n_kv, hd, frozen=model.frozen)
    assert float(loss.detach()) == float(loss2)
    by_name = dict(_flatten(grads))
    assert sorted(by_name) == want_names, "the gradient tree has an entry for a frozen leaf"
    for name, prm in zip(model.names, model._params):
        assert torch.equal(prm.grad, by_name[name].to(prm.dtype)), name
    # an optimizer step moves the trainable tensors only, and the next forward sees the new adapters
    torch.optim.SGD(model.parameters(), lr=0.05).step()
    after = model.reference_state_dict()
    moved = sorted(k for k in sd if not torch.equal(before[k], after[k]))
    assert moved and all(k.startswith("model.mm_projector.") or k == "model.image_newline" for k in moved), moved
    loss3 = model(input_ids, labels, images, coords)
    assert float(loss3.detach()) != float(loss2)
    # save_lora -> load_lora: exact, in the reference's per-module keys
    d = str(tmp_path / "adapter")
    model.save_lora(d)
    lora = L.load_lora(d)
    assert lora["r"] == 16 and lora["scaling"] == 1.0 and len(lora["adapters"]) == 7
    layer = model._full["llm"]["layers"][0]
    for name, modules in train.LORA_MODULES.items():
        a_list, b_list = train.lora_unstack(layer["lora"][name]["A"], layer["lora"][name]["B"], layer["lora_state"][name].blocks)
        for m, a, b in zip(modules, a_list, b_list):
            assert torch.equal(lora["adapters"][(0, m)][0], a.cpu()) and torch.equal(lora["adapters"][(0, m)][1], b.cpu()), m
    assert sorted(lora["non_lora"]) == sorted(["model.mm_projector.0.weight", "model.mm_projector.0.bias", "model.mm_projector.2.weight",
                                               "model.mm_projector.2.bias", "model.image_newline"])
    assert all(torch.equal(lora["non_lora"][k], after[k].cpu()) for k in lora["non_lora"])
    # merged into the base checkpoint by the loader, the adapters give the weights the training rule's merge gives
    merged = L.merge_lora({k: v for k, v in sd.items()}, lora, BF, "cuda")
    want_q = train.lora_merge_weight(layer["qkv"], layer["lora"]["qkv"], layer["lora_state"]["qkv"])[: n_q * hd]
    assert torch.equal(merged["model.layers.0.self_attn.q_proj.weight"], want_q)


def test_grounding_sample_with_adapters(train):
    """forward_ground on a module with adapters: the grounding head, the adapters, projector and newline get gradients, nothing else is a
    parameter, and the loss equals the explicit step's."""
    from v3d.train_module import LORA_DEFAULT_FROZEN, LlavaQwenTrainable
    sd, (n_q, n_kv, hd, V), (input_ids, labels, images, coords) = _reference_sd(seed=93)
    frozen = tuple(f for f in LORA_DEFAULT_FROZEN if f != "ground")
    model = LlavaQwenTrainable.from_reference_state_dict(sd, n_q, n_kv, max_pos=1024, lora=train.LoraConfig(r=16, lora_alpha=16), frozen=frozen,
                                                         ground_head_type="infonce", ground_token_ids=[500])
    _randomise_b(model)
    ids = input_ids.clone()
    ids[25] = 500
    lab = torch.full_like(labels, -100)
    lab[25] = 500
    boxes = torch.tensor([[0.0, 0.0, 0.0, 4.0, 4.0, 3.0], [3.0, -2.0, 1.0, 5.0, 5.0, 4.0], [-4.0, 4.0, -1.0, 6.0, 6.0, 4.0]])
    loss = model.forward_ground(ids, lab, images, coords, boxes, [1])
    loss.backward()
    got = {n for n, p in zip(model.names, model._params) if p.grad is not None}
    assert all(n.startswith(("llm.layers.0.lora.", "projector.", "ground.")) or n == "newline" for n in model.names)
    assert got == set(model.names), sorted(set(model.names) - got)
    assert any(n.startswith("ground.") for n in got) and bool(torch.isfinite(loss.detach()))
