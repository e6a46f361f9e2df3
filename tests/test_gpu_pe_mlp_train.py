"""Training of the learned MLP position encoding (`avg-discrete-mlp`): one LM sample with <coord> rows and one infonce grounding sample of
a small random model (the widths of tests/test_gpu_train_ground_heads.py's trainer tests: SigLIP layer at its true width, one Qwen2 layer
at hidden 512) against torch autograd in f32 over the reference's formulae, restated (tests/pe_mlp_check.restate_f32 for the module), by
the per-tensor rule of tests/test_gpu_train_ground_heads.py: norm-wise 5e-2, element-wise 1.2e-1 of the largest reference magnitude.
All rows that go through the module in a sample - the token coordinates, the box centre of the <coord> rows, the object centres - are one
batch on the device and one in the reference.  Also: re-computation is bit-identical, the MLP gradients are non-zero and move with a
centre, the shipped type's gradients do not change when an unused MLP group is present, and the trainer surface hands out .grad."""
import pytest
import torch
import torch.nn.functional as F

import pe_mlp_check as MC
from test_gpu_train_dense import _layer_ref, _rmsnorm_ref, _siglip_layer_ref
from test_gpu_train_ground_heads import _check_all

pytestmark = pytest.mark.gpu
TOL = (5e-2, 1.2e-1)             # tests/test_gpu_train_ground_heads.py: the infonce step's bound


@pytest.fixture(scope="module")
def ops():
    from v3d import ops as o
    return o


@pytest.fixture(scope="module")
def train():
    from v3d import train as t
    return t


def _model(seed=61):
    frames, tokens, Hv, heads, inter, kpad = 2, 729, 1152, 16, 4304, 640
    H, I, n_q, n_kv, hd, V, n_obj = 512, 768, 4, 2, 128, 512, 6
    g = torch.Generator().manual_seed(seed)
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
               "ln2": ln(H), "gate_up": mk(2 * I, H, s=H ** -0.5), "down": mk(H, I, s=I ** -0.5)}]
    llm = {"layers": layers, "norm": ln(H), "lm_head": mk(V, H, s=H ** -0.5)}
    # every ReLU input is offset by +-3 of its spread (the heads' b0: Linear -> ReLU; the module's ln_b: LayerNorm -> ReLU), as
    # tests/test_gpu_train_ground_heads.py:_make_heads does and for its reason: a grounding sample's gradient sits in a handful of rows (the
    # object proposals), and a unit whose ReLU input lies within the 16-bit forward's rounding of 0 is on in one computation and off in the
    # other, which moves a whole column of ln_b / b0 / w0's gradient - a property of comparing a 16-bit forward with an f32 one, not of the
    # backward under test.  Half of the units are on, half off.
    margin = lambda o: (3.0 * torch.sign(mk(o))).to(torch.bfloat16)                          # noqa: E731
    head = lambda: {"w0": mk(H, H, s=H ** -0.5), "b0": margin(H), "ln_w": ln(H), "ln_b": mk(H, s=0.1), "w3": mk(H, H, s=H ** -0.5), "b3": mk(H, s=0.1)}   # noqa: E731
    ground = {"obj": head(), "query": head(), "zero_target": mk(H)}
    # w3 is scaled so that the PE rows have about the spread of the projector's rows (0.6): the object features, and with them the inputs
    # of the heads' ReLUs, then have a spread of about 0.7, a quarter of the offset
    pe_mlp = MC.seeded_mlp(H, "bf16", seed=MC.SEED + 2, w3_scale=0.5, b3_offset=0.0)
    pe_mlp["ln_b"] = margin(MC.HIDDEN)
    patches = mk(frames * tokens, kpad)
    patches[:, 588:] = 0
    # the module's input under avg-discrete-mlp: integer-VALUED voxel coordinates in the model dtype (ids above 256 are rounded to bf16)
    xyz = torch.randint(0, 301, (frames, 14, 14, 3), generator=g).to(torch.bfloat16)
    pre_ids, post_ids = torch.randint(0, V, (9,), generator=g), torch.randint(0, V, (31,), generator=g)
    n_vis = frames * 14 * 15
    S = 9 + n_vis + 31
    labels = torch.full((S,), -100, dtype=torch.int64)
    labels[S - 20:] = torch.randint(0, V, (20,), generator=g)
    coord_rows = torch.tensor([9 + n_vis + 4, 9 + n_vis + 11])
    box_centre = torch.tensor([[151.0, 88.0, 47.0]]).to(torch.bfloat16)
    ground_row = 9 + n_vis + 17
    mask = (torch.rand(n_obj, frames * tokens, generator=g) < 0.02).to(torch.uint8)
    mask[4] = 0                                                               # a proposal that covers no patch: its feature is the PE alone
    obj_centres = torch.randint(0, 301, (n_obj, 3), generator=g).to(torch.bfloat16)
    positive = torch.zeros(n_obj + 1, dtype=torch.uint8)
    positive[[1, 3]] = 1
    return locals()


def _params(train, d, with_ground, with_mlp=True):
    cu = lambda t: train._tree_map(lambda a: a.cuda(), t)                     # noqa: E731
    llm = d["llm"] if not with_ground else {k: v for k, v in d["llm"].items() if k != "lm_head"}
    p = {"vision": {"patch_w": d["patch_w"].cuda(), "patch_b": d["patch_b"].cuda(), "pos": d["pos"].cuda(), "layers": [train.siglip_pad_layer(cu(d["vit"]))]},
         "projector": cu(d["proj"]), "newline": d["newline"].cuda(), "embed": d["embed"].cuda(), "llm": cu(llm)}
    if with_ground:
        p["ground"] = cu(d["ground"])
    if with_mlp:
        p["pe_mlp"] = cu(d["pe_mlp"])
    return p


def _reference_trunk(train, d, centres):
    """f32 autograd graph up to the decoder's output: returns (leaves, y, x_out, pe rows of the centres)."""
    frames, tokens, H, heads = d["frames"], d["tokens"], d["H"], d["heads"]
    f32 = lambda t: train._tree_map(lambda a: a.float().requires_grad_(), t)  # noqa: E731
    r = {"vit": f32(d["vit"]), "proj": f32(d["proj"]), "llm": f32(d["llm"]), "ground": f32(d["ground"]), "mlp": f32(d["pe_mlp"])}
    r["pw"], r["nl"], r["emb"] = (t.float().requires_grad_() for t in (d["patch_w"], d["newline"], d["embed"]))
    h = ((d["patches"].float() @ r["pw"].t() + d["patch_b"].float()).view(frames, tokens, -1) + d["pos"].float()).view(frames * tokens, -1)
    h = _siglip_layer_ref(h, r["vit"], frames, tokens, heads)
    y = F.gelu(h @ r["proj"]["w1"].t() + r["proj"]["b1"]) @ r["proj"]["w2"].t() + r["proj"]["b2"]
    pooled = F.interpolate(y.view(frames, 27, 27, H).permute(0, 3, 1, 2), size=[14, 14], mode="bilinear").permute(0, 2, 3, 1)
    pe = MC.restate_f32(torch.cat([d["xyz"].reshape(-1, 3), centres], 0), r["mlp"])          # ONE batch through the module
    n_tok = frames * 196
    vis = torch.cat([pooled + pe[:n_tok].view(frames, 14, 14, H), r["nl"][None, None, None, :].expand(frames, 14, 1, H)], 2).reshape(-1, H)
    x = torch.cat([r["emb"][d["pre_ids"]], vis, r["emb"][d["post_ids"]]], 0)
    return r, y, x, pe[n_tok:]


def _mlp_pairs(grads, r):
    return [("d pe_mlp " + k, grads["pe_mlp"][k], r["mlp"][k].grad, TOL) for k in MC.KEYS]


def test_lm_sample_with_coord_rows_matches_autograd(ops, train):
    d = _model()
    frames, n_q, n_kv, hd, H = d["frames"], d["n_q"], d["n_kv"], d["hd"], d["H"]
    rope = train.RopeTables(hd, 1024, 1e6, torch.bfloat16, "cuda")
    params = _params(train, d, with_ground=False)
    args = (d["patches"].cuda(), d["xyz"].cuda(), None, d["pre_ids"].cuda(), d["post_ids"].cuda(), d["labels"].cuda(), rope, frames, n_q, n_kv, hd)
    kw = dict(coord_rows=d["coord_rows"].cuda(), pe_mlp=params["pe_mlp"], pe_centres=d["box_centre"].cuda())
    loss, grads = train.sample_forward_backward(params, *args, **kw)
    assert set(grads["pe_mlp"]) == set(MC.KEYS)
    for k in MC.KEYS:
        assert grads["pe_mlp"][k].shape == params["pe_mlp"][k].shape and bool(torch.isfinite(grads["pe_mlp"][k]).all())
        assert float(grads["pe_mlp"][k].float().abs().max()) > 0, k

    # re-computation: the same loss and gradients, bit for bit
    loss_r, grads_r = train.sample_forward_backward(params, *args, recompute=True, **kw)
    assert float(loss_r) == float(loss)
    for a_, b_ in zip(train._leaves(grads_r), train._leaves(grads)):
        assert torch.equal(a_, b_)
    del grads_r

    # another box centre: the MLP gradients move (the <coord> rows' gradient goes through the module at another point)
    moved = dict(kw, pe_centres=torch.tensor([[20.0, 250.0, 3.0]]).to(torch.bfloat16).cuda())
    _, grads_m = train.sample_forward_backward(params, *args, **moved)
    assert not torch.equal(grads_m["pe_mlp"]["w0"], grads["pe_mlp"]["w0"]) and not torch.equal(grads_m["pe_mlp"]["w3"], grads["pe_mlp"]["w3"])
    del grads_m

    r, y, x, pe_c = _reference_trunk(train, d, d["box_centre"])
    x = x.index_add(0, d["coord_rows"], pe_c.expand(2, H))
    for p in r["llm"]["layers"]:
        x = _layer_ref(x, p, n_q, n_kv, hd, 1e-6)
    logits = _rmsnorm_ref(x, r["llm"]["norm"], 1e-6) @ r["llm"]["lm_head"].t()
    ref_loss = F.cross_entropy(logits[:-1], d["labels"][1:], ignore_index=-100)
    ref_loss.backward()
    assert abs(float(loss) - float(ref_loss.detach())) < 3e-2 * float(ref_loss.detach())
    pairs = _mlp_pairs(grads, r)
    pairs += [("d newline", grads["newline"], r["nl"].grad, TOL), ("d embed", grads["embed"], r["emb"].grad, TOL),
              ("d lm_head", grads["llm"]["lm_head"], r["llm"]["lm_head"].grad, TOL)]
    pairs += [("d projector " + k, grads["projector"][k], r["proj"][k].grad, TOL) for k in d["proj"]]
    pairs += [("llm layer 0 d " + k, grads["llm"]["layers"][0][k], r["llm"]["layers"][0][k].grad, TOL) for k in ("qkv", "down")]
    _check_all(pairs)


def test_grounding_sample_matches_autograd(ops, train):
    d = _model()
    frames, n_q, n_kv, hd, H, n_obj = d["frames"], d["n_q"], d["n_kv"], d["hd"], d["H"], d["n_obj"]
    rope = train.RopeTables(hd, 1024, 1e6, torch.bfloat16, "cuda")
    params = _params(train, d, with_ground=True)
    args = (d["patches"].cuda(), d["xyz"].cuda(), None, d["pre_ids"].cuda(), d["post_ids"].cuda(), d["ground_row"], d["mask"].cuda(), None,
            d["positive"].cuda(), rope, frames, n_q, n_kv, hd)
    kw = dict(pe_mlp=params["pe_mlp"], pe_centres=d["obj_centres"].cuda())
    loss, scores, grads = train.ground_sample_forward_backward(params, *args, **kw)
    assert scores.shape == (n_obj + 1,) and set(grads["pe_mlp"]) == set(MC.KEYS)
    loss_r, _, grads_r = train.ground_sample_forward_backward(params, *args, recompute=True, **kw)
    assert float(loss_r) == float(loss)
    for a_, b_ in zip(train._leaves(grads_r), train._leaves(grads)):
        assert torch.equal(a_, b_)
    del grads_r
    moved_c = d["obj_centres"].clone()
    moved_c[4] = torch.tensor([7.0, 7.0, 290.0]).to(torch.bfloat16)            # the proposal whose feature is the PE alone
    _, _, grads_m = train.ground_sample_forward_backward(params, *args, **dict(kw, pe_centres=moved_c.cuda()))
    assert not torch.equal(grads_m["pe_mlp"]["w0"], grads["pe_mlp"]["w0"])
    del grads_m

    r, y, x, box_pe = _reference_trunk(train, d, d["obj_centres"])
    for p in r["llm"]["layers"]:
        x = _layer_ref(x, p, n_q, n_kv, hd, 1e-6)
    query = _rmsnorm_ref(x[d["ground_row"]:d["ground_row"] + 1], r["llm"]["norm"], 1e-6)
    objs = []
    for i in range(n_obj):                                                    # llava_arch.py:482-501
        rows = d["mask"][i].bool()
        objs.append((y[rows].mean(0) if bool(rows.any()) else torch.zeros(H)) + box_pe[i])
    of = torch.cat([torch.stack(objs), r["ground"]["zero_target"][None]], 0)
    mlp = lambda t, hp: F.linear(F.layer_norm(F.relu(F.linear(t, hp["w0"], hp["b0"])), (H,), hp["ln_w"], hp["ln_b"], 1e-5), hp["w3"], hp["b3"])   # noqa: E731
    sc = (F.normalize(mlp(of, r["ground"]["obj"])) * F.normalize(mlp(query, r["ground"]["query"]))).sum(-1)
    lg = torch.exp(sc / 0.07)
    ref_loss = -torch.log(lg[d["positive"].bool()].sum() / lg.sum())
    ref_loss.backward()
    assert float((scores.cpu() - sc.detach()).abs().max()) < 2e-2
    assert abs(float(loss) - float(ref_loss.detach())) < 0.05 * max(1.0, float(ref_loss.detach()))
    pairs = _mlp_pairs(grads, r)
    pairs += [(f"d {h_} head {k}", grads["ground"][h_][k], r["ground"][h_][k].grad, TOL) for h_ in ("obj", "query") for k in ("w0", "w3")]
    pairs += [("d final norm", grads["llm"]["norm"], r["llm"]["norm"].grad, TOL), ("d embed", grads["embed"], r["emb"].grad, TOL)]
    pairs += [("d projector " + k, grads["projector"][k], r["proj"][k].grad, TOL) for k in d["proj"]]
    _check_all(pairs)


def test_shipped_type_ignores_an_unused_mlp_group(ops, train):
    """The shipped type's step with and without a "pe_mlp" group in the parameter tree: the same loss and gradients bit for bit, and no
    gradient for the group - the sin3d path runs the kernels it ran before."""
    d = _model()
    frames, n_q, n_kv, hd, H = d["frames"], d["n_q"], d["n_kv"], d["hd"], d["H"]
    rope = train.RopeTables(hd, 1024, 1e6, torch.bfloat16, "cuda")
    table = ops.Sin3DTable(H, 301, torch.bfloat16, "cuda")
    ids = d["xyz"].to(torch.int32).cuda()
    coord_pe = ops.sin3d_pe(d["box_centre"][None].cuda(), H)[0, 0]
    out = []
    for with_mlp in (False, True):
        params = _params(train, d, with_ground=False, with_mlp=with_mlp)
        out.append(train.sample_forward_backward(params, d["patches"].cuda(), ids, table, d["pre_ids"].cuda(), d["post_ids"].cuda(), d["labels"].cuda(),
                                                 rope, frames, n_q, n_kv, hd, coord_rows=d["coord_rows"].cuda(), coord_pe=coord_pe))
    (loss0, g0), (loss1, g1) = out
    assert "pe_mlp" not in g0 and "pe_mlp" not in g1
    assert float(loss0) == float(loss1)
    for a_, b_ in zip(train._leaves(g0), train._leaves(g1)):
        assert torch.equal(a_, b_)


def test_trainer_surface_hands_the_mlp_its_grad(ops, train):
    """LlavaQwenTrainable under avg-discrete-mlp: forward(...).backward() and forward_ground(...).backward() fill the six tensors' .grad
    with the functional step's gradients; under the shipped type a carried group gets none and the other gradients do not change."""
    from test_gpu_train_ground_heads import GROUND_ID, _ground_inputs, _reference_sd
    from v3d.train_module import LlavaQwenTrainable, _flatten
    n_q, n_kv, hd, H = 4, 2, 128, 512
    sd = _reference_sd("infonce")
    mlp = MC.seeded_mlp(H, "bf16", seed=MC.SEED + 2, w3_scale=0.5, b3_offset=0.0)
    sd.update({MC.SD_PREFIX + MC.REF_KEYS[k]: v for k, v in mlp.items()})
    model = LlavaQwenTrainable.from_reference_state_dict(sd, n_q, n_kv, max_pos=1024, ground_head_type="infonce", ground_token_ids=[GROUND_ID],
                                                         world_position_embedding_type="avg-discrete-mlp")
    back = model.reference_state_dict()
    assert set(back) == set(sd) and all(torch.equal(back[k].cpu(), sd[k]) for k in sd)
    assert all(MC.SD_PREFIX + k not in model._passthrough for k in MC.REF_KEYS.values())
    input_ids, labels, images, coords, boxes = _ground_inputs()
    lm_ids = input_ids.clone()
    lm_ids[[14, 22]] = 317                                                       # two <coord> tokens
    lm_labels = torch.full((31,), -100, dtype=torch.int64)
    lm_labels[20:] = lm_ids[20:]
    box = torch.tensor([1.5, -2.25, 0.5])
    loss = model(lm_ids, lm_labels, images, coords, coord_token_id=317, box_input=box)
    loss.backward()

    tr = model.param_tree()
    dt, frames, n_vis = torch.bfloat16, 2, 2 * 210
    patches = ops.patchify(images.to(dt).cuda(), 14, 640)
    cd = coords.to(dt).cuda()
    _, vox, _ = ops.coord_pool_voxel(cd, want_avg=False, want_ids=False)
    assert vox.dtype == dt
    centre = ops.discrete_coords(box.reshape(1, 3).to(dt).cuda())
    full = torch.cat([lm_labels[:9], torch.full((n_vis,), -100, dtype=torch.int64), lm_labels[10:]]).cuda()
    rows = torch.tensor([14 + n_vis - 1, 22 + n_vis - 1]).cuda()
    loss2, grads = train.sample_forward_backward(tr, patches, vox, None, lm_ids[:9].cuda(), lm_ids[10:].cuda(), full, model.rope, frames, n_q, n_kv, hd,
                                                 coord_rows=rows, pe_mlp=tr["pe_mlp"], pe_centres=centre)
    assert float(loss.detach()) == float(loss2)
    by_name = dict(_flatten(grads))
    seen = 0
    for name, prm in zip(model.names, model._params):
        if name.startswith("ground."):
            assert prm.grad is None
        else:
            assert prm.grad is not None and torch.equal(prm.grad, by_name[name].to(prm.dtype)), name
            seen += name.startswith("pe_mlp.")
    assert seen == 6
    lm_grads = {n: p.grad.clone() for n, p in zip(model.names, model._params) if n.startswith("pe_mlp.")}

    # a grounding sample accumulates into the same .grad (autograd semantics): the increment is the functional step's gradient
    model.forward_ground(input_ids, labels, images, coords, boxes, [2, 5]).backward()
    bx = boxes.to(dt).cuda()
    mask = ops.object_patch_mask(cd, bx).view(8, -1).contiguous()
    positive = torch.zeros(9, dtype=torch.uint8)
    positive[[2, 5]] = 1
    _, _, ggrads = train.ground_sample_forward_backward(tr, patches, vox, None, input_ids[:9].cuda(), input_ids[10:].cuda(), 26 + n_vis - 1, mask, None,
                                                        positive.cuda(), model.rope, frames, n_q, n_kv, hd, pe_mlp=tr["pe_mlp"],
                                                        pe_centres=ops.discrete_coords(bx[:, :3].contiguous()))
    for name, prm in zip(model.names, model._params):
        if name.startswith("pe_mlp."):
            k = name.split(".")[1]
            assert float(ggrads["pe_mlp"][k].float().abs().max()) > 0
            assert torch.equal(prm.grad, lm_grads[name] + ggrads["pe_mlp"][k].to(prm.dtype)), name

    # the shipped type with the same tensors in the checkpoint: carried, not modelled; and with a group in the tree: no .grad for it
    shipped = LlavaQwenTrainable.from_reference_state_dict(sd, n_q, n_kv, max_pos=1024)
    assert shipped.pe_kind == "sin3d" and all(MC.SD_PREFIX + k in shipped._passthrough for k in MC.REF_KEYS.values())
    tree = shipped.param_tree()
    tree["pe_mlp"] = {k: v.cuda() for k, v in mlp.items()}
    carried = LlavaQwenTrainable(tree, n_q, n_kv, max_pos=1024)
    shipped(lm_ids, lm_labels, images, coords, coord_token_id=317, box_input=box).backward()
    carried(lm_ids, lm_labels, images, coords, coord_token_id=317, box_input=box).backward()
    g_shipped = {n: p.grad for n, p in zip(shipped.names, shipped._params)}
    for n, p in zip(carried.names, carried._params):
        if n.startswith("pe_mlp."):
            assert p.grad is None
        else:
            assert torch.equal(p.grad, g_shipped[n]), n
