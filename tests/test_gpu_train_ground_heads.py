"""Training of the 'mlp' and 'score' grounding heads (llava_qwen.py:59-91, 283-293, 313-322) against torch autograd in f32 over the
reference's formulae, restated, on the same 16-bit inputs:
  * the kernels: v3d_ground_rowdot_bce (the heads' score tail + BCE with positive weighting + its backward, one launch) and
    v3d_mul_rows_grad (backward of `obj_feat * query_feat`);
  * the grounding sample's step (train.ground_sample_forward_backward(head_type='mlp' / 'score')) through the heads, the decoder, the
    projector and the tower, and the heads alone at the 7B model's width;
  * the trainer surface: the heads' reference keys round-trip, forward_ground(...).backward() fills .grad with the functional step's
    gradients, and AdamW steps on one sample lower the loss.
The device side rounds every tensor it stores to 16 bits, so the comparison is by tolerance, stated per tensor: a norm-wise relative
error and an element-wise bound relative to the largest reference magnitude."""
import pytest
import torch
import torch.nn.functional as F

from test_gpu_train_dense import _close, _layer_ref, _rmsnorm_ref, _siglip_layer_ref

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ops():
    from v3d import ops as o
    return o


@pytest.fixture(scope="module")
def train():
    from v3d import train as t
    return t


def _bce_ref(scores, positive, pos_weight):
    # llava_qwen.py:313-322: BCEWithLogitsLoss(reduction='none')(scores, target) * weight, .mean()
    t = positive.float()
    weight = torch.where(positive.bool(), torch.full_like(t, pos_weight), torch.ones_like(t))
    return (F.binary_cross_entropy_with_logits(scores, t, reduction="none") * weight).mean()


def _label_sets(n):
    """P = 0, 1, several (a duplicate among them: P counts it, the target is set once), n."""
    several = sorted({0, n // 3, n // 2, n - 1}) + [n // 2] if n > 1 else [0, 0]
    return [[], [n // 2], several, list(range(n))]


@pytest.mark.parametrize("dt", [torch.bfloat16, torch.float16])
@pytest.mark.parametrize("n", [1, 6, 50, 257, 1024])
@pytest.mark.parametrize("C", [1024, 3584])
@pytest.mark.parametrize("rounded", [True, False])
def test_rowdot_bce_matches_autograd(ops, train, dt, n, C, rounded):
    """Loss, scores, dX, dw and dbias against autograd for P = 0, 1, several, n; logits up to +-80 (the stable form); 'mlp' form
    (products rounded to the dtype, no bias) and 'score' form (a Linear(C, 1) with bias); two calls give identical bits."""
    g = torch.Generator().manual_seed(n * 7 + C + rounded)
    X = torch.randn(n, C, generator=g).to(dt)
    w = (torch.randn(C, generator=g) * 30.0 / C ** 0.5).to(dt)               # scores of magnitude ~30
    X[0] = (torch.sign(w.float()) * (80.0 / w.float().abs().sum())).to(dt)   # row 0 scores ~ +80, the last row ~ -80
    if n > 1:
        X[-1] = -X[0]
    bias = None if rounded else torch.tensor([0.75]).to(dt)
    for labels in _label_sets(n):
        positive, pos_weight = train.ground_bce_targets(labels, n)
        Xr, wr = X.float().requires_grad_(), w.float().requires_grad_()
        br = bias.float().requires_grad_() if bias is not None else None
        prod = Xr * wr
        s = (prod.to(dt).float() if rounded else prod).sum(-1) + (br if br is not None else 0.0)
        ref = _bce_ref(s, positive, pos_weight)
        ref.backward()
        out = ops.ground_rowdot_bce(X.cuda(), w.cuda(), positive.cuda(), pos_weight, bias=bias.cuda() if bias is not None else None,
                                    products_rounded=rounded)
        loss, scores, dX, dw, db = out
        what = f"n={n} C={C} P={len(labels)}"
        assert float(s.detach().abs().max()) > 70.0, what
        assert float((scores.cpu() - s.detach()).abs().max()) <= 1e-5 * float((X.float() * w.float()).abs().sum(-1).max()) + 1e-6, what
        ref = ref.detach()
        assert abs(float(loss) - float(ref)) <= 1e-4 * max(1.0, abs(float(ref))), (what, float(loss), float(ref))
        if len(labels) == n:                                                  # every weight 0
            assert float(loss) == 0.0 and not bool(dX.any()) and not bool(dw.any())
        else:
            _close(dX, Xr.grad, 5e-3, 1e-2, "dX " + what)
            _close(dw, wr.grad, 5e-3, 1e-2, "dw " + what)
        if bias is not None:
            assert abs(float(db.float().cpu()) - float(br.grad)) <= 1e-2 * abs(float(br.grad)) + 1e-6, what
        else:
            assert db is None
        again = ops.ground_rowdot_bce(X.cuda(), w.cuda(), positive.cuda(), pos_weight, bias=bias.cuda() if bias is not None else None,
                                      products_rounded=rounded)
        for a, b in zip(out, again):
            if a is not None:
                assert torch.equal(a, b), what


def test_rowdot_bce_refuses_out_of_bounds_shapes(ops):
    from v3d._native import V3DError
    pos = torch.zeros(1025, dtype=torch.uint8, device="cuda")
    with pytest.raises(V3DError, match="1 to 1024 rows"):
        ops.ground_rowdot_bce(torch.zeros(1025, 64, dtype=torch.bfloat16, device="cuda"), torch.zeros(64, dtype=torch.bfloat16, device="cuda"),
                              pos, 1.0)
    with pytest.raises(V3DError, match=r"x must be \[n, C\]"):
        ops.ground_rowdot_bce(torch.zeros(64, dtype=torch.bfloat16, device="cuda"), torch.zeros(64, dtype=torch.bfloat16, device="cuda"), pos[:1], 1.0)
    with pytest.raises(V3DError, match="multiple of 8"):
        ops.ground_rowdot_bce(torch.zeros(4, 3592, dtype=torch.bfloat16, device="cuda"), torch.zeros(3592, dtype=torch.bfloat16, device="cuda"),
                              pos[:4], 1.0)


@pytest.mark.parametrize("dt", [torch.bfloat16, torch.float16])
@pytest.mark.parametrize("n,C", [(1, 1024), (6, 1024), (50, 1024), (257, 3584), (1024, 1024)])
def test_mul_rows_grad_matches_autograd(ops, dt, n, C):
    g = torch.Generator().manual_seed(n + C)
    o, q, dm = (torch.randn(n, C, generator=g).to(dt), torch.randn(C, generator=g).to(dt), (torch.randn(n, C, generator=g) * 1e-2).to(dt))
    orr, qr = o.float().requires_grad_(), q.float().requires_grad_()
    (orr * qr).backward(dm.float())
    do, dq = ops.mul_rows_grad(dm.cuda(), o.cuda(), q.cuda())
    assert torch.equal(do.cpu(), orr.grad.to(dt))                             # one product, one rounding
    _close(dq, qr.grad, 4e-3, 8e-3, f"dq n={n} C={C}")
    do2, dq2 = ops.mul_rows_grad(dm.cuda(), o.cuda(), q.cuda())
    assert torch.equal(do, do2) and torch.equal(dq, dq2)


def _errs(got, ref, floor=1e-30):
    got, ref = got.float().cpu(), ref.float()
    return float((got - ref).norm() / ref.norm().clamp_min(floor)), float((got - ref).abs().max() / ref.abs().max().clamp_min(floor))


def _check_all(pairs):
    """pairs: [(name, got, ref, (norm-wise bound, element-wise bound))]; every tensor is measured (printed under -s), then all failures
    are reported together."""
    bad = []
    for name, got, ref, (rel, elem) in pairs:
        err, worst = _errs(got, ref)
        print(f"{name:28s} norm-wise {err:.3e} (bound {rel})  element-wise {worst:.3e} (bound {elem})")
        if not (err < rel and worst < elem):
            bad.append(f"{name}: norm-wise {err:.3e} (bound {rel}), element-wise {worst:.3e} of max |ref| (bound {elem})")
    assert not bad, "; ".join(bad)


# ------------------------------------------------------------------------------ the heads (restated in f32)


def _relu_ln(t, hp):
    # ground_head (mlp) / the infonce heads: Linear, ReLU, LayerNorm, Linear (llava_qwen.py:66-71)
    return F.linear(F.layer_norm(F.relu(F.linear(t, hp["w0"], hp["b0"])), (hp["ln_w"].shape[0],), hp["ln_w"], hp["ln_b"], 1e-5), hp["w3"], hp["b3"])


def _ln_relu(t, hp):
    # ground_head_obj / query / score of the 'score' head: Linear, LayerNorm, ReLU, Linear (llava_qwen.py:74-91)
    return F.linear(F.relu(F.layer_norm(F.linear(t, hp["w0"], hp["b0"]), (hp["ln_w"].shape[0],), hp["ln_w"], hp["ln_b"], 1e-5)), hp["w3"], hp["b3"])


def _head_scores_ref(head_type, gr, of, query):
    if head_type == "mlp":
        return (_relu_ln(query, gr["head"])[0] * of).sum(-1)                           # :283-285
    m = _ln_relu(of, gr["obj"]) * _ln_relu(query, gr["query"])                             # :286-290
    return _ln_relu(m, gr["score"]).squeeze(1)                                             # :291-292


def _make_heads(head_type, H, mk, ln):
    """Random heads whose comparison with an f32 reference does not hinge on rounding: every ReLU input is offset by +-3 of its spread
    (b0 for Linear -> ReLU, ln_b for LayerNorm -> ReLU), so that a unit takes the ReLU on both sides or on neither - a unit whose input
    lies within the 16-bit forward's difference of 0 moves a whole row of w0's gradient - and the last Linear is scaled so that the
    scores are O(1), where sigmoid(s) does not saturate and a small score difference stays a small ds difference.  Half of the units
    are on, half off."""
    def margin(o):
        return (3.0 * torch.sign(mk(o))).to(torch.bfloat16)

    def head(i, o, out, relu_first, last_scale=1.0):
        return {"w0": mk(o, i, s=i ** -0.5), "b0": margin(o) if relu_first else mk(o, s=0.1), "ln_w": ln(o),
                "ln_b": mk(o, s=0.1) if relu_first else margin(o), "w3": mk(out, o, s=last_scale * o ** -0.5), "b3": mk(out, s=0.1 * last_scale)}
    if head_type == "mlp":
        return {"head": head(H, H, H, True, last_scale=0.05)}                # q . object features: |s| ~ 1 at H 768 .. 3584
    return {"obj": head(H, 1024, 1024, False), "query": head(H, 1024, 1024, False), "score": head(1024, 1024, 1, False, last_scale=0.5)}


@pytest.mark.parametrize("head_type", ["mlp", "score"])
def test_true_width_head_matches_autograd(train, head_type):
    """The head alone at the 7B model's width: H 3584, 50 proposals, three targets; loss, scores and the gradients of every head tensor,
    the object features and the query row."""
    H, n = 3584, 50
    g = torch.Generator().manual_seed(3584 + len(head_type))
    mk = lambda *shape, s=1.0: (torch.randn(*shape, generator=g) * s).to(torch.bfloat16)     # noqa: E731
    ln = lambda n_: (1 + 0.1 * torch.randn(n_, generator=g)).to(torch.bfloat16)              # noqa: E731
    heads = _make_heads(head_type, H, mk, ln)
    of, query = mk(n, H, s=0.5), mk(1, H)
    positive, pos_weight = train.ground_bce_targets([3, 17, 41], n)
    cu = lambda t: train._tree_map(lambda a: a.cuda(), t)                                      # noqa: E731
    loss, scores, d_of, d_q, grads = train._bce_head_forward_backward(head_type, cu(heads), of.cuda(), query.cuda(), positive.cuda(), pos_weight)
    torch.cuda.synchronize()
    gr = train._tree_map(lambda a: a.float().requires_grad_(), heads)
    ofr, qr = of.float().requires_grad_(), query.float().requires_grad_()
    sc = _head_scores_ref(head_type, gr, ofr, qr)
    ref = _bce_ref(sc, positive, pos_weight)
    ref.backward()
    assert float((scores.cpu() - sc.detach()).abs().max()) <= 2e-2 * max(1.0, float(sc.detach().abs().max()))
    assert abs(float(loss) - float(ref)) <= 2e-2 * max(1.0, float(ref))
    tol = (5e-2, 1.2e-1)                                                       # the infonce step's bound
    pairs = [("d object features", d_of, ofr.grad, tol), ("d query row", d_q, qr.grad, tol)]
    pairs += [(f"d {mod} {k}", grads[mod][k], gr[mod][k].grad, tol) for mod in heads for k in heads[mod]]
    _check_all(pairs)


# ------------------------------------------------------------------------------ the grounding sample's step


def _sample(train, ops, head_type, labels):
    frames, tokens, Hv, heads, inter, kpad = 2, 729, 1152, 16, 4304, 640
    H, I, n_q, n_kv, hd, V, L, n_obj = 768, 1024, 4, 2, 128, 1024, 2, 6
    g = torch.Generator().manual_seed(55)
    mk = lambda *shape, s=1.0: (torch.randn(*shape, generator=g) * s).to(torch.bfloat16)     # noqa: E731
    ln = lambda n_: (1 + 0.1 * torch.randn(n_, generator=g)).to(torch.bfloat16)              # noqa: E731
    vit = {"ln1_w": ln(Hv), "ln1_b": mk(Hv, s=0.1), "ln2_w": ln(Hv), "ln2_b": mk(Hv, s=0.1),
           "q_w": mk(Hv, Hv, s=Hv ** -0.5), "q_b": mk(Hv, s=0.2), "k_w": mk(Hv, Hv, s=Hv ** -0.5), "k_b": mk(Hv, s=0.2),
           "v_w": mk(Hv, Hv, s=Hv ** -0.5), "v_b": mk(Hv, s=0.2), "o_w": mk(Hv, Hv, s=Hv ** -0.5), "o_b": mk(Hv, s=0.2),
           "fc1_w": mk(inter, Hv, s=Hv ** -0.5), "fc1_b": mk(inter, s=0.2), "fc2_w": mk(Hv, inter, s=inter ** -0.5), "fc2_b": mk(Hv, s=0.2)}
    patch_w, patch_b, pos = mk(Hv, kpad, s=588 ** -0.5), mk(Hv, s=0.1), mk(tokens, Hv, s=0.5)
    patch_w[:, 588:] = 0
    proj = {"w1": mk(H, Hv, s=Hv ** -0.5), "b1": mk(H, s=0.1), "w2": mk(H, H, s=H ** -0.5), "b2": mk(H, s=0.1)}
    newline, embed = mk(H, s=0.5), mk(V, H, s=0.5)
    width = (n_q + 2 * n_kv) * hd
    layers = [{"ln1": ln(H), "qkv": mk(width, H, s=H ** -0.5), "qkv_bias": mk(width, s=0.3), "o": mk(H, n_q * hd, s=(n_q * hd) ** -0.5),
               "ln2": ln(H), "gate_up": mk(2 * I, H, s=H ** -0.5), "down": mk(H, I, s=I ** -0.5)} for _ in range(L)]
    llm = {"layers": layers, "norm": ln(H)}
    ground = _make_heads(head_type, H, mk, ln)
    patches = mk(frames * tokens, kpad)
    patches[:, 588:] = 0
    ids = torch.randint(0, 64, (frames, 14, 14, 3), generator=g, dtype=torch.int32)
    pre_ids, post_ids = torch.randint(0, V, (9,), generator=g), torch.randint(0, V, (21,), generator=g)
    n_vis = frames * 14 * 15
    ground_row = 9 + n_vis + 17
    mask = (torch.rand(n_obj, frames * tokens, generator=g) < 0.02).to(torch.uint8)
    mask[4] = 0                                                               # a proposal that covers no patch: its feature is the PE alone
    box_pe = mk(n_obj, H, s=0.5)
    positive, pos_weight = train.ground_bce_targets(labels, n_obj)
    return locals()


@pytest.mark.parametrize("head_type", ["mlp", "score"])
@pytest.mark.parametrize("labels", [[1, 3], []], ids=["P2", "P0"])
def test_bce_grounding_sample_step_matches_autograd(ops, train, head_type, labels):
    """A grounding sample with the 'mlp' / 'score' head: tower -> projector -> splice -> decoder -> predict_box's head and BCE loss
    (llava_qwen.py:239-322, llava_arch.py:479-501) at the widths of test_grounding_sample_step_matches_autograd; loss, scores and the
    gradients of the heads, the decoder, the projector and the tower against autograd in f32; a sample with targets and one without."""
    d = _sample(train, ops, head_type, labels)
    frames, tokens, H, n_q, n_kv, hd, n_obj, heads = d["frames"], d["tokens"], d["H"], d["n_q"], d["n_kv"], d["hd"], d["n_obj"], d["heads"]
    table = ops.Sin3DTable(H, 64, torch.bfloat16, "cuda")
    pe = ops.sin3d_pe(d["ids"].view(frames, 196, 3).to(torch.bfloat16).cuda(), H).float().cpu()
    rope = train.RopeTables(hd, 1024, 1e6, torch.bfloat16, "cuda")
    cu = lambda t: train._tree_map(lambda a: a.cuda(), t)                                      # noqa: E731
    params = {"vision": {"patch_w": d["patch_w"].cuda(), "patch_b": d["patch_b"].cuda(), "pos": d["pos"].cuda(), "layers": [train.siglip_pad_layer(cu(d["vit"]))]},
              "projector": cu(d["proj"]), "newline": d["newline"].cuda(), "embed": d["embed"].cuda(), "llm": cu(d["llm"]), "ground": cu(d["ground"])}
    loss, scores, grads = train.ground_sample_forward_backward(params, d["patches"].cuda(), d["ids"].cuda(), table, d["pre_ids"].cuda(),
                                                               d["post_ids"].cuda(), d["ground_row"], d["mask"].cuda(), d["box_pe"].cuda(),
                                                               d["positive"].cuda(), rope, frames, n_q, n_kv, hd, head_type=head_type,
                                                               pos_weight=d["pos_weight"])
    assert scores.shape == (n_obj,) and set(grads["ground"]) == set(d["ground"])

    f32 = lambda t: train._tree_map(lambda a: a.float().requires_grad_(), t)                  # noqa: E731
    r_vit, r_proj, r_llm, r_gr = f32(d["vit"]), f32(d["proj"]), f32(d["llm"]), f32(d["ground"])
    r_pw, r_nl, r_emb = (t.float().requires_grad_() for t in (d["patch_w"], d["newline"], d["embed"]))
    h = ((d["patches"].float() @ r_pw.t() + d["patch_b"].float()).view(frames, tokens, -1) + d["pos"].float()).view(frames * tokens, -1)
    h = _siglip_layer_ref(h, r_vit, frames, tokens, heads)
    y = F.gelu(h @ r_proj["w1"].t() + r_proj["b1"]) @ r_proj["w2"].t() + r_proj["b2"]
    pooled = F.interpolate(y.view(frames, 27, 27, H).permute(0, 3, 1, 2), size=[14, 14], mode="bilinear").permute(0, 2, 3, 1)
    vis = torch.cat([pooled + pe.view(frames, 14, 14, H), r_nl[None, None, None, :].expand(frames, 14, 1, H)], 2).reshape(-1, H)
    x = torch.cat([r_emb[d["pre_ids"]], vis, r_emb[d["post_ids"]]], 0)
    for p in r_llm["layers"]:
        x = _layer_ref(x, p, n_q, n_kv, hd, 1e-6)
    query = _rmsnorm_ref(x[d["ground_row"]:d["ground_row"] + 1], r_llm["norm"], 1e-6)
    objs = []
    for i in range(n_obj):
        rows = d["mask"][i].bool()
        objs.append((y[rows].mean(0) if bool(rows.any()) else torch.zeros(H)) + d["box_pe"][i].float())
    sc = _head_scores_ref(head_type, r_gr, torch.stack(objs), query)
    ref_loss = _bce_ref(sc, d["positive"], d["pos_weight"])
    ref_loss.backward()

    assert float((scores.cpu() - sc.detach()).abs().max()) < 2e-2 * max(1.0, float(sc.detach().abs().max()))
    assert abs(float(loss) - float(ref_loss.detach())) < 0.02 * max(1.0, float(ref_loss.detach()))
    tol = (5e-2, 1.2e-1)                                                       # the infonce step's bound
    pairs = [(f"d {mod} head {k}", grads["ground"][mod][k], r_gr[mod][k].grad, tol) for mod in d["ground"] for k in d["ground"][mod]]
    pairs.append(("d final norm", grads["llm"]["norm"], r_llm["norm"].grad, tol))
    pairs += [("llm layer 0 d " + k, grads["llm"]["layers"][0][k], r_llm["layers"][0][k].grad, tol) for k in d["layers"][0]]
    pairs += [("d projector " + k, grads["projector"][k], r_proj[k].grad, tol) for k in d["proj"]]
    real = train.siglip_unpad_grads(grads["vision"]["layers"][0])
    pairs += [("vit d " + k, real[k], r_vit[k].grad, tol) for k in ("q_w", "o_w", "fc1_w", "fc2_w", "ln1_w")]
    pairs.append(("d embed", grads["embed"], r_emb.grad, tol))
    _check_all(pairs)


# ------------------------------------------------------------------------------ the trainer surface


def _reference_sd(head_type, H=512, I=768, n_q=4, n_kv=2, hd=128, V=512, seed=91):
    from v3d.train_module import VIT
    Hv, inter = 1152, 4304
    g = torch.Generator().manual_seed(seed)
    mk = lambda *shape, s=1.0: (torch.randn(*shape, generator=g) * s).to(torch.bfloat16)      # noqa: E731
    ln = lambda n_: (1 + 0.1 * torch.randn(n_, generator=g)).to(torch.bfloat16)                 # noqa: E731
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
    sd[VIT + "post_layernorm.weight"], sd[VIT + "post_layernorm.bias"] = ln(Hv), mk(Hv, s=0.1)        # unmodelled, carried through
    # the head's tensors under the reference's keys (llava_qwen.py:57-110)
    width = {"infonce": H, "mlp": H, "score": 1024}[head_type]
    mods = {"infonce": [("ground_head_obj.", 2), ("ground_head_query.", 2)], "mlp": [("ground_head.", 2)],
            "score": [("ground_head_obj.", 1), ("ground_head_query.", 1), ("ground_head_score.", 1)]}[head_type]
    for pfx, li in mods:
        i_, o_ = (1024, 1024) if pfx == "ground_head_score." else (H, width)
        out = 1 if pfx == "ground_head_score." else width
        sd[pfx + "0.weight"], sd[pfx + "0.bias"] = mk(o_, i_, s=i_ ** -0.5), mk(o_, s=0.1)
        sd[pfx + f"{li}.weight"], sd[pfx + f"{li}.bias"] = ln(o_), mk(o_, s=0.1)
        sd[pfx + "3.weight"], sd[pfx + "3.bias"] = mk(out, o_, s=o_ ** -0.5), mk(out, s=0.1)
    if head_type == "infonce":
        sd["ground_head_zero_target"] = mk(H)
    return sd


GROUND_ID = 500                                                              # the <ground> label id of these samples


def _ground_inputs(seed=7, V=512, frames=2):
    g = torch.Generator().manual_seed(seed)
    images = torch.randn(frames, 3, 384, 384, generator=g)
    coords = (torch.rand(frames, 384, 384, 3, generator=g) - 0.5) * torch.tensor([20.0, 20.0, 8.0])
    t_ = torch.randint(0, 400, (30,), generator=g)
    input_ids = torch.cat([t_[:9], torch.tensor([-200]), t_[9:]])
    input_ids[26] = GROUND_ID
    labels = torch.full((31,), -100, dtype=torch.int64)
    labels[26] = GROUND_ID
    centres = (torch.rand(8, 3, generator=g) - 0.5) * torch.tensor([12.0, 12.0, 4.0])
    boxes = torch.cat([centres, 2.0 + 4.0 * torch.rand(8, 3, generator=g)], 1)
    return input_ids, labels, images, coords, boxes


@pytest.mark.parametrize("head_type", ["infonce", "mlp", "score"])
def test_trainer_surface_ground_heads(ops, train, head_type):
    """LlavaQwenTrainable(ground_head_type=...): the head's reference keys round-trip exactly; forward_ground(...).backward() fills .grad
    with train.ground_sample_forward_backward's gradients (the LM head gets none); the LM-sample forward leaves the head's .grad alone;
    AdamW steps on one fixed grounding sample lower its loss."""
    from v3d.train_module import LlavaQwenTrainable, _flatten, ground_key_map
    n_q, n_kv, hd = 4, 2, 128
    sd = _reference_sd(head_type)
    model = LlavaQwenTrainable.from_reference_state_dict(sd, n_q, n_kv, max_pos=1024, ground_head_type=head_type, ground_token_ids=[GROUND_ID])
    back = model.reference_state_dict()
    assert set(back) == set(sd) and all(torch.equal(back[k].cpu(), sd[k]) for k in sd)
    assert all(k not in model._passthrough for k in ground_key_map(head_type))                 # modelled, not carried
    assert any(n.startswith("ground.") for n in model.names)
    input_ids, labels, images, coords, boxes = _ground_inputs()
    box_labels = [2, 5]
    loss = model.forward_ground(input_ids, labels, images, coords, boxes, box_labels)
    assert loss.requires_grad and loss.dtype == torch.float32
    loss.backward()

    tr = model.param_tree()
    dt, H, frames, n_vis = torch.bfloat16, 512, 2, 2 * 210
    patches = ops.patchify(images.to(dt).cuda(), 14, 640)
    cd = coords.to(dt).cuda()
    _, _, vox = ops.coord_pool_voxel(cd, want_avg=False, want_vox=False)
    bx = boxes.to(dt).cuda()
    mask = ops.object_patch_mask(cd, bx).view(8, -1).contiguous()
    box_pe = ops.sin3d_pe(ops.discrete_coords(bx[:, :3].contiguous())[None], H, dim_t=model.pe_table.dim_t)[0].contiguous()
    if head_type == "infonce":
        positive, kw = torch.zeros(9, dtype=torch.uint8), {}
        positive[box_labels] = 1
    else:
        positive, pw = train.ground_bce_targets(box_labels, 8)
        kw = {"pos_weight": pw}
    loss2, _, grads = train.ground_sample_forward_backward(tr, patches, vox, model.pe_table, input_ids[:9].cuda(), input_ids[10:].cuda(),
                                                           26 + n_vis - 1, mask, box_pe, positive.cuda(), model.rope, frames, n_q, n_kv, hd,
                                                           head_type=head_type, **kw)
    assert float(loss.detach()) == float(loss2)
    by_name = dict(_flatten(grads))
    for name, prm in zip(model.names, model._params):
        if name == "llm.lm_head":
            assert prm.grad is None
        else:
            assert prm.grad is not None and torch.equal(prm.grad, by_name[name].to(prm.dtype)), name
    # an LM sample: the head's .grad stays as the grounding sample left it
    head_grads = {n: p.grad.clone() for n, p in zip(model.names, model._params) if n.startswith("ground.")}
    lm_labels = torch.full((31,), -100, dtype=torch.int64)
    lm_labels[20:] = input_ids[20:]
    model(input_ids, lm_labels, images, coords).backward()
    for n, p in zip(model.names, model._params):
        if n.startswith("ground."):
            assert torch.equal(p.grad, head_grads[n]), n
    # AdamW on the tree, three steps on the fixed sample
    opt = train.AdamW(tr, lr=1e-3)
    losses = []
    for _ in range(4):
        model.zero_grad()
        loss = model.forward_ground(input_ids, labels, images, coords, boxes, box_labels)
        losses.append(float(loss.detach()))
        loss.backward()
        if len(losses) == 4:
            break
        it = iter(model._params)
        gtree = train._tree_map(lambda _: (lambda p: p.grad if p.grad is not None else torch.zeros_like(p))(next(it)), model._shape)
        opt.step(tr, gtree)
    assert losses[-1] < losses[0], losses
    assert all(torch.isfinite(p.float()).all() for p in model._params)
