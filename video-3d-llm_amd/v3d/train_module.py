"""Trainer-facing surface of the device-side training step (BASELINE configs[4]): what connects `v3d.train` to
`loss.backward()` and to checkpoints in the reference's own key names.

The reference trains `LlavaQwenForCausalLM` under the HF Trainer: `loss = model(input_ids, labels=..., images=..., video_dict=...).loss;
loss.backward(); optimizer.step()` (llava_qwen.py:121-205, llava_trainer.py, train_3d.py:1572).  `LlavaQwenTrainable` is an `nn.Module`
whose parameters are `nn.Parameter`s holding the tensors of `v3d.train`'s layouts (fused q|k|v rows, stacked gate|up rows, the tower's
72-wide heads zero-padded to 128); `forward(...)` returns the loss as a tensor with a `grad_fn`: the explicit device-side
forward + backward (`train.sample_forward_backward`, every operation a C-ABI call) runs inside a `torch.autograd.Function`, and
`loss.backward()` hands its gradients to the parameters' `.grad` - so any torch optimizer (or `train.AdamW` / `train.ZeroAdamW` on
`module.param_tree()`) and a Trainer-style loop work unchanged.  `from_reference_state_dict` / `reference_state_dict` convert between the
checkpoint's keys (`model.layers.N.self_attn.q_proj.weight`, `model.vision_tower...`, `model.mm_projector.{0,2}`, ...) and the training
layouts, exactly (the padding is zeros and is dropped on the way back).

Grounding samples (ScanRefer / Multi3DRefer): built with `ground_head_type` ('infonce', 'mlp' or 'score', the reference's
`config.ground_head_type`, llava_qwen.py:57-110), the module also models that head's parameters under their reference keys
(`ground_head.N.*`, `ground_head_obj/query/score.N.*`, `ground_head_zero_target`) and `forward_ground(...)` returns the grounding loss
(`train.ground_sample_forward_backward`) with a `grad_fn`; an LM sample leaves the head's `.grad` untouched, a grounding sample the LM head's.

Position encodings: the shipped `avg-discrete-sin3d` (no parameters) and the learned `mlp` types (`avg[-discrete]-mlp`,
`sample1[-discrete]-mlp`): the six tensors of `model.world_position_embedding.mlp.{0,1,3}` are parameters of the module (tree["pe_mlp"]) and
take their `.grad` from LM and grounding samples alike.

One sample per call, as the reference trains (`per_device_train_batch_size 1`, train_multi.sh:58).  Not here: DeepSpeed's engine.

LoRA (`lora_enable`, train_3d.py:168-173, 259-274): `LlavaQwenTrainable(tree, ..., lora=train.LoraConfig(r, lora_alpha), frozen=(...))` puts
peft's init on the decoder's seven linears (`train.lora_init`); only the adapters and the leaves not named in `frozen` are `nn.Parameter`s
(default with adapters: the projector and image_newline beside them), `loss.backward()` fills their `.grad` alone, a frozen tower's backward is not
run, and `save_lora(dir)` writes the adapter directory the reference's trainer leaves (`loader.save_lora`; read back by `loader.load_lora`).
"""
import torch
import torch.nn as nn

from . import ops, train
from ._native import V3DError
from .engine import PE_MLP_KEYS, PE_MLP_PREFIX
from .token_ids import IGNORE_INDEX, IMAGE_TOKEN_INDEX

VIT = "model.vision_tower.vision_tower.vision_model."
# with adapters, what is not trained unless the caller says otherwise: everything but the adapters, the projector and image_newline
LORA_DEFAULT_FROZEN = ("vision", "embed", "lm_head", "norm", "ln1", "ln2", "qkv_bias", "ground", "pe_mlp")


# head type -> its modules: (reference prefix, key in the tree's "ground", Sequential index of the LayerNorm); Linear at 0 and 3 throughout
_GROUND_MODULES = {"infonce": (("ground_head_obj.", "obj", 2), ("ground_head_query.", "query", 2)),      # Linear, ReLU, LayerNorm, Linear
                   "mlp": (("ground_head.", "head", 2),),
                   "score": (("ground_head_obj.", "obj", 1), ("ground_head_query.", "query", 1),           # Linear, LayerNorm, ReLU, Linear
                             ("ground_head_score.", "score", 1))}


def ground_key_map(head_type):
    """{reference key: (module key in tree["ground"] or None, leaf)} of a grounding head type (llava_qwen.py:57-110)."""
    if head_type not in _GROUND_MODULES:
        raise V3DError(f"ground_head_type {head_type!r}: the reference has {tuple(_GROUND_MODULES)}")
    out = {}
    for pfx, mod, ln in _GROUND_MODULES[head_type]:
        for key, leaf in (("0.weight", "w0"), ("0.bias", "b0"), (f"{ln}.weight", "ln_w"), (f"{ln}.bias", "ln_b"), ("3.weight", "w3"), ("3.bias", "b3")):
            out[pfx + key] = (mod, leaf)
    if head_type == "infonce":
        out["ground_head_zero_target"] = (None, "zero_target")
    return out


def _flatten(tree, prefix=""):
    out = []
    if isinstance(tree, dict):
        for k in tree:
            out += _flatten(tree[k], f"{prefix}.{k}" if prefix else str(k))
    elif isinstance(tree, list):
        for i, v in enumerate(tree):
            out += _flatten(v, f"{prefix}.{i}")
    else:
        out.append((prefix, tree))
    return out


class _SampleLoss(torch.autograd.Function):
    """forward: the whole sample's forward AND backward on the device (the gradients are a by-product of the one pass that exists);
    backward: hands them over, scaled by the incoming gradient of the loss (1 for a plain loss.backward(), 1 / steps under the
    Trainer's gradient accumulation)."""

    @staticmethod
    def forward(ctx, module, args, *flat_params):
        args, kw = args
        loss, grads = train.sample_forward_backward(module.param_tree(), *args, recompute=module.recompute, frozen=module.frozen, **kw)
        ctx.grads = _match_grads(module, grads, ("ground.",) + module.unused_prefixes)      # the grounding head takes no part in an LM sample
        return loss.detach().clone()

    @staticmethod
    def backward(ctx, grad_loss):
        scale = float(grad_loss)
        out = []
        for g in ctx.grads:
            if g is not None and scale != 1.0:
                if g.dtype in (torch.bfloat16, torch.float16):
                    z = torch.zeros_like(g)
                    ops.axpy(z, g.contiguous(), scale)      # 16-bit scale on the device (v3d_axpy)
                    g = z
                else:
                    g = g * scale                           # the few f32 leaves (image_newline: one row)
            out.append(g)
        ctx.grads = None
        return (None, None, *out)


def _match_grads(module, grads, absent_prefix):
    """The gradient tree in the module's parameter order; parameters under absent_prefix (a prefix or a tuple of them: the part of the
    model a sample does not use) may be missing and get no gradient (None: their .grad stays as it was, as under autograd)."""
    by_name = dict(_flatten(grads))
    missing = set(module.names) - set(by_name)
    if set(by_name) - set(module.names) or any(not n.startswith(absent_prefix) for n in missing):
        raise V3DError("the gradient tree does not match the parameter tree")
    return [by_name.get(n) for n in module.names]


class _GroundLoss(_SampleLoss):
    """_SampleLoss for a grounding sample (train.ground_sample_forward_backward; the LM head gets no gradient)."""

    @staticmethod
    def forward(ctx, module, args, *flat_params):
        args, kw = args
        loss, _, grads = train.ground_sample_forward_backward(module.param_tree(), *args, recompute=module.recompute, frozen=module.frozen, **kw)
        ctx.grads = _match_grads(module, grads, ("llm.lm_head",) + module.unused_prefixes)
        return loss.detach().clone()


def _training_position_type(wtype):
    """-> (pe_kind, aggregation, discrete) of a type training supports: the shipped 'avg-discrete-sin3d', or an `mlp` type
    (avg / sample1, with or without `discrete`); raises for every other string."""
    from .loader import parse_mlp_position_type, parse_position_encoder, parse_position_type
    if parse_position_encoder(wtype) == "mlp":
        aggregation, _, discrete = parse_mlp_position_type(wtype)
        return "mlp", aggregation, discrete
    if parse_position_type(wtype) != ("avg", 1, True):
        raise V3DError(f"world_position_embedding_type {wtype!r}: training supports 'avg-discrete-sin3d' and the 'mlp' types "
                       "('avg[-discrete]-mlp', 'sample1[-discrete]-mlp') only; the sampled-point, min/max and continuous sin3d encodings are "
                       "inference-only (v3d.engine.Engine)")
    return "sin3d", "avg", True


class LlavaQwenTrainable(nn.Module):
    def __init__(self, tree, n_q, n_kv, head_dim=128, vit_heads=16, vit_inter=4304, rope_theta=1e6, max_pos=8192, recompute=False,
                 min_xyz=(-15, -15, -5), max_xyz=(15, 15, 5), voxel_size=0.1, ground_head_type=None, ground_temperature=0.07,
                 ground_token_ids=None, world_position_embedding_type="avg-discrete-sin3d", lora=None, frozen=None, lora_seed=0):
        """world_position_embedding_type: the checkpoint's config value; training runs the shipped 'avg-discrete-sin3d' and the `mlp` types
        (avg / sample1, with or without `discrete`; tree["pe_mlp"] = {w0, b0, ln_w, ln_b, w3, b3} is then required and trained); the other
        sin3d types are inference-only and are refused here, never trained as averages.  A "pe_mlp" group in the tree
        under the sin3d type is carried and gets no gradient.
        ground_head_type: None (no grounding head modelled) or 'infonce' / 'mlp' / 'score' with tree["ground"] in the layout of
        train.ground_sample_forward_backward; ground_temperature: the infonce head's config.ground_head_temperature; ground_token_ids:
        config.ground_token_ids (the label ids whose row is the grounding query, llava_qwen.py:280).
        lora: a train.LoraConfig - adapters on the decoder's seven linears (peft's init from torch's CPU generator seeded with lora_seed);
        frozen: names of the tree whose leaves are not trained (train.trainable_tree; default with adapters LORA_DEFAULT_FROZEN: all but
        the adapters, the projector and image_newline; without adapters nothing).  Frozen leaves are not nn.Parameters."""
        super().__init__()
        self.lora = lora
        self.frozen = tuple(frozen) if frozen is not None else (LORA_DEFAULT_FROZEN if lora is not None else ())
        if lora is not None:
            lora.validate()
            train.lora_init(tree["llm"], r=lora.r, alpha=lora.lora_alpha, seed=lora_seed, qkv_rows=(n_q * head_dim, n_kv * head_dim, n_kv * head_dim))
        self.pe_kind, self.aggregation, self.discrete = _training_position_type(world_position_embedding_type)
        if self.pe_kind == "mlp" and "pe_mlp" not in tree:
            raise V3DError(f"world_position_embedding_type {world_position_embedding_type!r} but the tree has no 'pe_mlp' entry")
        self.unused_prefixes = ("pe_mlp.",) if self.pe_kind != "mlp" and "pe_mlp" in tree else ()
        if ground_head_type is not None:
            ground_key_map(ground_head_type)                        # a known type
            if "ground" not in tree:
                raise V3DError(f"ground_head_type {ground_head_type!r} but the tree has no 'ground' entry")
        self.ground_head_type, self.ground_temperature = ground_head_type, ground_temperature
        self.ground_token_ids = None if ground_token_ids is None else [int(i) for i in ground_token_ids]
        self._full = tree if (lora is not None or self.frozen) else None      # every tensor, frozen ones and the adapters' state included
        flat = _flatten(train.trainable_tree(tree, self.frozen) if self._full is not None else tree)
        self.names = [n for n, _ in flat]
        self._params = nn.ParameterList([nn.Parameter(t, requires_grad=True) for _, t in flat])
        self._shape = tree
        self.n_q, self.n_kv, self.hd, self.vit_heads, self.vit_inter = n_q, n_kv, head_dim, vit_heads, vit_inter
        self.recompute = recompute
        self.min_xyz, self.max_xyz, self.voxel_size = tuple(min_xyz), tuple(max_xyz), voxel_size
        first = tree["newline"]
        self.rope = train.RopeTables(head_dim, max_pos, rope_theta, first.dtype, first.device)
        H = tree["newline"].shape[0]
        n_ids = int(round(max(b - a for a, b in zip(min_xyz, max_xyz)) / voxel_size)) + 1
        self.pe_table = ops.Sin3DTable(H, n_ids, first.dtype, first.device) if self.pe_kind == "sin3d" else None

    # ------------------------------------------------------------------ parameter tree <-> nn.Parameters
    def param_tree(self):
        """The parameters as the dict / list tree `v3d.train` takes (the tensors ARE the nn.Parameters' storage).  With adapters or
        frozen leaves: the whole tree, whose trainable leaves are the nn.Parameters' storage; the adapters' derived copies are brought up
        to date with their leaves (an optimizer may have stepped since)."""
        if self._full is not None:
            if self.lora is not None:
                train.lora_refresh(self._full["llm"])
            return self._full
        it = iter(self._params)

        def build(t):
            if isinstance(t, dict):
                return {k: build(v) for k, v in t.items()}
            if isinstance(t, list):
                return [build(v) for v in t]
            return next(it).data
        return build(self._shape)

    # ------------------------------------------------------------------ checkpoints in the reference's keys
    @classmethod
    def from_reference_state_dict(cls, sd, n_q, n_kv, vit_heads=16, dtype=torch.bfloat16, device="cuda", kpad=640, ground_head_type=None, **kw):
        """sd: the reference's state dict (llava_qwen.py / siglip_encoder.py / builder.py keys) -> the module.  ground_head_type: the
        grounding head to model (its ground_head* keys must be in sd); None carries any ground_head* tensors through unmodelled."""
        t = lambda k: sd[k].to(device=device, dtype=dtype)       # noqa: E731
        n_vit = 1 + max(int(k[len(VIT + "encoder.layers."):].split(".")[0]) for k in sd if k.startswith(VIT + "encoder.layers."))
        n_llm = 1 + max(int(k.split(".")[2]) for k in sd if k.startswith("model.layers."))
        pw = t(VIT + "embeddings.patch_embedding.weight")
        Hv = pw.shape[0]
        patch_w = torch.zeros((Hv, kpad), dtype=dtype, device=device)
        patch_w[:, : pw[0].numel()] = pw.reshape(Hv, -1)
        vit_layers = []
        for i in range(n_vit):
            p = VIT + f"encoder.layers.{i}."
            raw = {"ln1_w": t(p + "layer_norm1.weight"), "ln1_b": t(p + "layer_norm1.bias"), "ln2_w": t(p + "layer_norm2.weight"),
                   "ln2_b": t(p + "layer_norm2.bias"), "o_w": t(p + "self_attn.out_proj.weight"), "o_b": t(p + "self_attn.out_proj.bias"),
                   "fc1_w": t(p + "mlp.fc1.weight"), "fc1_b": t(p + "mlp.fc1.bias"), "fc2_w": t(p + "mlp.fc2.weight"), "fc2_b": t(p + "mlp.fc2.bias")}
            for n in ("q", "k", "v"):
                raw[n + "_w"], raw[n + "_b"] = t(p + f"self_attn.{n}_proj.weight"), t(p + f"self_attn.{n}_proj.bias")
            vit_layers.append(train.siglip_pad_layer(raw, heads=vit_heads, inter_pad=(raw["fc1_w"].shape[0] + 127) // 128 * 128))
        llm_layers = []
        for i in range(n_llm):
            p = f"model.layers.{i}."
            llm_layers.append({
                "ln1": t(p + "input_layernorm.weight"),
                "qkv": torch.cat([t(p + f"self_attn.{n}_proj.weight") for n in ("q", "k", "v")], 0).contiguous(),
                "qkv_bias": torch.cat([t(p + f"self_attn.{n}_proj.bias") for n in ("q", "k", "v")], 0).contiguous(),
                "o": t(p + "self_attn.o_proj.weight").contiguous(), "ln2": t(p + "post_attention_layernorm.weight"),
                "gate_up": torch.cat([t(p + "mlp.gate_proj.weight"), t(p + "mlp.up_proj.weight")], 0).contiguous(),
                "down": t(p + "mlp.down_proj.weight").contiguous()})
        tree = {"vision": {"patch_w": patch_w, "patch_b": t(VIT + "embeddings.patch_embedding.bias"),
                           "pos": t(VIT + "embeddings.position_embedding.weight").contiguous(), "layers": vit_layers},
                "projector": {"w1": t("model.mm_projector.0.weight").contiguous(), "b1": t("model.mm_projector.0.bias"),
                              "w2": t("model.mm_projector.2.weight").contiguous(), "b2": t("model.mm_projector.2.bias")},
                "newline": t("model.image_newline"), "embed": t("model.embed_tokens.weight").contiguous(),
                "llm": {"layers": llm_layers, "norm": t("model.norm.weight"), "lm_head": t("lm_head.weight").contiguous()}}
        if ground_head_type is not None:
            keys = ground_key_map(ground_head_type)
            absent = [k for k in keys if k not in sd]
            if absent:
                raise V3DError(f"ground_head_type {ground_head_type!r} but the state dict has no {absent[0]}")
            ground = {}
            for k, (mod, leaf) in keys.items():
                if mod is None:
                    ground[leaf] = t(k).contiguous()
                else:
                    ground.setdefault(mod, {})[leaf] = t(k).contiguous()
            tree["ground"] = ground
        pe_mlp = "mlp" in kw.get("world_position_embedding_type", "")
        if pe_mlp:
            absent = [PE_MLP_PREFIX + k for k in PE_MLP_KEYS.values() if PE_MLP_PREFIX + k not in sd]
            if absent:
                raise V3DError(f"world_position_embedding_type {kw['world_position_embedding_type']!r} but the state dict has no {absent[0]}")
            tree["pe_mlp"] = {leaf: t(PE_MLP_PREFIX + k).contiguous() for leaf, k in PE_MLP_KEYS.items()}
        hd = tree["llm"]["layers"][0]["qkv"].shape[0] // (n_q + 2 * n_kv)
        m = cls(tree, n_q, n_kv, head_dim=hd, vit_heads=vit_heads, vit_inter=sd[VIT + "encoder.layers.0.mlp.fc1.weight"].shape[0],
                ground_head_type=ground_head_type, **kw)
        m._patch_shape = tuple(pw.shape)
        # tensors a real LlavaQwen checkpoint holds and this module does not train - vision_model.post_layernorm (stays in the tower after
        # siglip_encoder.py:570-571), the vision_model.head.* pooling head, the ground_head* tensors, rotary inv_freq buffers, ...: kept
        # as they came (frozen, on the host) and emitted unchanged by reference_state_dict(), so that a checkpoint saved through this
        # surface loads strictly on the reference's side
        m._passthrough = {k: v.detach().clone().cpu() for k, v in sd.items() if k not in m._modelled_keys(n_vit, n_llm, ground_head_type, pe_mlp)}
        return m

    @staticmethod
    def _modelled_keys(n_vit, n_llm, ground_head_type=None, pe_mlp=False):
        keys = set(ground_key_map(ground_head_type)) if ground_head_type is not None else set()
        if pe_mlp:
            keys |= {PE_MLP_PREFIX + k for k in PE_MLP_KEYS.values()}
        keys |= {VIT + "embeddings.patch_embedding.weight", VIT + "embeddings.patch_embedding.bias", VIT + "embeddings.position_embedding.weight",
                "model.mm_projector.0.weight", "model.mm_projector.0.bias", "model.mm_projector.2.weight", "model.mm_projector.2.bias",
                "model.image_newline", "model.embed_tokens.weight", "model.norm.weight", "lm_head.weight"}
        for i in range(n_vit):
            p = VIT + f"encoder.layers.{i}."
            for n in ("self_attn.q_proj", "self_attn.k_proj", "self_attn.v_proj", "self_attn.out_proj", "mlp.fc1", "mlp.fc2", "layer_norm1", "layer_norm2"):
                keys |= {p + n + ".weight", p + n + ".bias"}
        for i in range(n_llm):
            p = f"model.layers.{i}."
            keys |= {p + f"self_attn.{n}_proj.{w}" for n in ("q", "k", "v") for w in ("weight", "bias")}
            keys |= {p + "self_attn.o_proj.weight", p + "mlp.gate_proj.weight", p + "mlp.up_proj.weight", p + "mlp.down_proj.weight",
                     p + "input_layernorm.weight", p + "post_attention_layernorm.weight"}
        return keys

    def reference_state_dict(self):
        """Back to the reference's keys and shapes (fused / stacked / padded layouts undone; the padding holds zeros)."""
        tr = self.param_tree()
        out = {}
        v = tr["vision"]
        shape = getattr(self, "_patch_shape", None) or (v["patch_w"].shape[0], 3, 14, 14)
        out[VIT + "embeddings.patch_embedding.weight"] = v["patch_w"][:, : shape[1] * shape[2] * shape[3]].reshape(shape).clone()
        out[VIT + "embeddings.patch_embedding.bias"] = v["patch_b"].clone()
        out[VIT + "embeddings.position_embedding.weight"] = v["pos"].clone()
        for i, L in enumerate(v["layers"]):
            raw = train.siglip_unpad_grads(L, heads=self.vit_heads, inter=self.vit_inter)       # (the same un-padding serves weights)
            p = VIT + f"encoder.layers.{i}."
            for n in ("q", "k", "v"):
                out[p + f"self_attn.{n}_proj.weight"], out[p + f"self_attn.{n}_proj.bias"] = raw[n + "_w"].clone(), raw[n + "_b"].clone()
            out[p + "self_attn.out_proj.weight"], out[p + "self_attn.out_proj.bias"] = raw["o_w"].clone(), raw["o_b"].clone()
            out[p + "mlp.fc1.weight"], out[p + "mlp.fc1.bias"] = raw["fc1_w"].clone(), raw["fc1_b"].clone()
            out[p + "mlp.fc2.weight"], out[p + "mlp.fc2.bias"] = raw["fc2_w"].clone(), raw["fc2_b"].clone()
            out[p + "layer_norm1.weight"], out[p + "layer_norm1.bias"] = raw["ln1_w"].clone(), raw["ln1_b"].clone()
            out[p + "layer_norm2.weight"], out[p + "layer_norm2.bias"] = raw["ln2_w"].clone(), raw["ln2_b"].clone()
        pj = tr["projector"]
        out["model.mm_projector.0.weight"], out["model.mm_projector.0.bias"] = pj["w1"].clone(), pj["b1"].clone()
        out["model.mm_projector.2.weight"], out["model.mm_projector.2.bias"] = pj["w2"].clone(), pj["b2"].clone()
        out["model.image_newline"], out["model.embed_tokens.weight"] = tr["newline"].clone(), tr["embed"].clone()
        nq, nkv, hd = self.n_q * self.hd, self.n_kv * self.hd, self.hd
        for i, L in enumerate(tr["llm"]["layers"]):
            p = f"model.layers.{i}."
            for n, a, b in (("q", 0, nq), ("k", nq, nq + nkv), ("v", nq + nkv, nq + 2 * nkv)):
                out[p + f"self_attn.{n}_proj.weight"], out[p + f"self_attn.{n}_proj.bias"] = L["qkv"][a:b].clone(), L["qkv_bias"][a:b].clone()
            out[p + "self_attn.o_proj.weight"] = L["o"].clone()
            inter = L["gate_up"].shape[0] // 2
            out[p + "mlp.gate_proj.weight"], out[p + "mlp.up_proj.weight"] = L["gate_up"][:inter].clone(), L["gate_up"][inter:].clone()
            out[p + "mlp.down_proj.weight"] = L["down"].clone()
            out[p + "input_layernorm.weight"], out[p + "post_attention_layernorm.weight"] = L["ln1"].clone(), L["ln2"].clone()
        out["model.norm.weight"], out["lm_head.weight"] = tr["llm"]["norm"].clone(), tr["llm"]["lm_head"].clone()
        if self.ground_head_type is not None:
            for k, (mod, leaf) in ground_key_map(self.ground_head_type).items():
                out[k] = (tr["ground"][leaf] if mod is None else tr["ground"][mod][leaf]).clone()
        if self.pe_kind == "mlp":
            for leaf, k in PE_MLP_KEYS.items():
                out[PE_MLP_PREFIX + k] = tr["pe_mlp"][leaf].clone()
        for k, v in getattr(self, "_passthrough", {}).items():      # unmodelled tensors of the source checkpoint, unchanged
            out[k] = v.clone()
        return out

    def save_lora(self, lora_dir):
        """The adapter directory of the reference's trainer (train_3d.py:1875-1884): adapter_config.json, adapter_model.bin (per-module
        lora_A / lora_B under peft's keys, the stacked q|k|v and gate|up adapters taken apart exactly) and non_lora_trainables.bin (the
        trained non-adapter tensors under peft's names of the reference's keys)."""
        from . import loader
        if self.lora is None:
            raise V3DError("save_lora: this module was built without lora=")
        adapters = {}
        for i, L in enumerate(self._full["llm"]["layers"]):
            for name, modules in train.LORA_MODULES.items():
                a_list, b_list = train.lora_unstack(L["lora"][name]["A"], L["lora"][name]["B"], L["lora_state"][name].blocks)
                for m, a, b in zip(modules, a_list, b_list):
                    adapters[(i, m)] = (a, b)
        base = ("self_attn.q_proj.weight", "self_attn.k_proj.weight", "self_attn.v_proj.weight", "self_attn.o_proj.weight",
                "mlp.gate_proj.weight", "mlp.up_proj.weight", "mlp.down_proj.weight")
        groups = {"vision": lambda k: k.startswith(VIT), "projector": lambda k: k.startswith("model.mm_projector."),
                  "newline": lambda k: k == "model.image_newline", "embed": lambda k: k == "model.embed_tokens.weight",
                  "lm_head": lambda k: k == "lm_head.weight", "norm": lambda k: k == "model.norm.weight",
                  "ln1": lambda k: k.endswith("input_layernorm.weight"), "ln2": lambda k: k.endswith("post_attention_layernorm.weight"),
                  "qkv_bias": lambda k: k.startswith("model.layers.") and k.endswith("_proj.bias"),
                  "ground": lambda k: k.startswith("ground_head"), "pe_mlp": lambda k: k.startswith(PE_MLP_PREFIX)}
        trained = [f for name, f in groups.items() if name not in self.frozen]
        passthrough = set(getattr(self, "_passthrough", {}))
        non_lora = {"base_model.model." + k: v for k, v in self.reference_state_dict().items()
                    if k not in passthrough and not k.endswith(base) and any(f(k) for f in trained)}
        loader.save_lora(lora_dir, adapters, non_lora, self.lora.r, self.lora.lora_alpha)

    # ------------------------------------------------------------------ forward (llava_qwen.py:121-205 for one video sample with labels)
    def forward(self, input_ids, labels, images, world_coords, coord_token_id=None, box_input=None):
        """input_ids / labels: 1-D, the collator's (one IMAGE_TOKEN_INDEX; labels aligned to input_ids, IGNORE_INDEX where masked -
        train_3d.py:1329-1366); images [F,3,S,S] pixel values; world_coords [F,S,S,3].  The visual rows take IGNORE_INDEX labels
        (llava_arch.py:736-741).  box_input [3] + coord_token_id: Scan2Cap's box-centre PE on the <coord> rows (:416-417, 697-700).
        Returns the loss (f32 scalar with a grad_fn)."""
        tr = self.param_tree()
        dev, dt = tr["newline"].device, tr["newline"].dtype
        ids = input_ids.reshape(-1).cpu()
        lab = labels.reshape(-1).cpu()
        at = (ids == IMAGE_TOKEN_INDEX).nonzero().flatten()
        if at.numel() != 1:
            raise V3DError("exactly one <image> token per sample")
        at = int(at[0])
        frames = images.shape[0]
        n = 14
        n_vis = frames * n * (n + 1)
        pre_ids, post_ids = ids[:at].to(dev), ids[at + 1:].to(dev)
        full_labels = torch.cat([lab[:at], torch.full((n_vis,), IGNORE_INDEX, dtype=torch.int64), lab[at + 1:]]).to(dev)
        patches = ops.patchify(images.to(device=dev, dtype=dt), 14, tr["vision"]["patch_w"].shape[1])
        vox = self._position_input(world_coords.to(device=dev, dtype=dt))
        coord_rows = coord_pe = None
        kw = {}
        if coord_token_id is not None and box_input is not None:
            rows = [r if r < at else r + n_vis - 1 for r, t in enumerate(ids.tolist()) if t == coord_token_id]
            if rows:
                centre = self._centres(torch.as_tensor(box_input, dtype=torch.float32).reshape(1, 3).to(device=dev, dtype=dt))
                if self.pe_kind == "mlp":
                    kw["pe_centres"] = centre          # encoded with the tokens, as one batch
                else:
                    coord_pe = ops.sin3d_pe(centre[None], tr["newline"].shape[0], dim_t=self.pe_table.dim_t)[0, 0]
                coord_rows = torch.tensor(rows, dtype=torch.int64, device=dev)
        if self.pe_kind == "mlp":
            kw["pe_mlp"] = tr["pe_mlp"]
        args = (patches, vox, self.pe_table, pre_ids, post_ids, full_labels, self.rope, frames, self.n_q, self.n_kv, self.hd)
        kw_args = args + (729, 27, 14, coord_rows, coord_pe)
        return _SampleLoss.apply(self, (kw_args, kw), *self._params)

    def _position_input(self, coords):
        """What the PE is taken of, per token (llava_arch.py:395-420): int32 voxel ids for the shipped type; for an `mlp` type the module's
        input in the model dtype - the aggregated coordinates, voxelised (integer-valued) with `discrete`."""
        a = (coords, 27, self.min_xyz, self.max_xyz, self.voxel_size)
        if self.pe_kind == "sin3d":
            return ops.coord_pool_voxel(*a, want_avg=False, want_vox=False)[2]
        if self.aggregation == "avg":
            avg, vox, _ = ops.coord_pool_voxel(*a, want_avg=not self.discrete, want_vox=self.discrete, want_ids=False)
        else:
            avg, vox, _ = ops.coord_points_voxel(coords, self.aggregation, *a[1:], want_pts=not self.discrete, want_vox=self.discrete, want_ids=False)
        return vox if self.discrete else avg

    def _centres(self, xyz):
        """Box / object centres [N, 3] as the module takes them: voxelised when the type is `discrete` (llava_arch.py:416-420)."""
        return ops.discrete_coords(xyz.contiguous(), self.min_xyz, self.max_xyz, self.voxel_size) if self.discrete else xyz.contiguous()

    # ------------------------------------------------------------------ grounding samples (llava_qwen.py:239-322)
    def forward_ground(self, input_ids, labels, images, world_coords, boxes, box_labels, ground_token_ids=None):
        """A ScanRefer / Multi3DRefer training sample with this module's ground_head_type: input_ids / labels / images / world_coords as
        forward(); boxes [n, 6] the object proposals (centre xyz, size xyz; 'patch14' object features, llava_arch.py:351-376, 479-501);
        box_labels: box_labels[0] of the reference, the indices of the target proposals.  The query is the final-norm hidden state of the
        row whose label lies in [ground_token_ids[0], ground_token_ids[-1]] (llava_qwen.py:280-282; default: the module's).
        Returns the grounding loss (f32 scalar with a grad_fn): infonce, or the positive-weighted BCE of 'mlp' / 'score' (:313-322)."""
        if self.ground_head_type is None:
            raise V3DError("forward_ground: this module models no grounding head (build it with ground_head_type)")
        gids = self.ground_token_ids if ground_token_ids is None else [int(i) for i in ground_token_ids]
        if not gids:
            raise V3DError("forward_ground: no ground_token_ids")
        tr = self.param_tree()
        dev, dt = tr["newline"].device, tr["newline"].dtype
        H = tr["newline"].shape[0]
        ids = input_ids.reshape(-1).cpu()
        lab = labels.reshape(-1).cpu()
        at = (ids == IMAGE_TOKEN_INDEX).nonzero().flatten()
        if at.numel() != 1:
            raise V3DError("exactly one <image> token per sample")
        at = int(at[0])
        rows = ((lab >= gids[0]) & (lab <= gids[-1])).nonzero().flatten().tolist()
        if len(rows) != 1 or rows[0] == at:
            raise V3DError(f"forward_ground: {len(rows)} rows carry a <ground> label, the reference's predict_box takes one")
        frames, n = images.shape[0], 14
        n_vis = frames * n * (n + 1)
        ground_row = rows[0] if rows[0] < at else rows[0] + n_vis - 1
        pre_ids, post_ids = ids[:at].to(dev), ids[at + 1:].to(dev)
        patches = ops.patchify(images.to(device=dev, dtype=dt), 14, tr["vision"]["patch_w"].shape[1])
        coords = world_coords.to(device=dev, dtype=dt)
        vox = self._position_input(coords)
        bx = boxes.to(device=dev, dtype=dt).reshape(-1, 6).contiguous()
        n_obj = bx.shape[0]
        if n_obj < 1:
            raise V3DError("forward_ground: no object proposals")
        mask = ops.object_patch_mask(coords, bx).view(n_obj, -1).contiguous()
        centres = self._centres(bx[:, :3])
        if self.pe_kind == "mlp":
            box_pe = None                              # encoded with the tokens, as one batch (train.ground_sample_forward_backward)
        else:
            box_pe = ops.sin3d_pe(centres[None], H, dim_t=self.pe_table.dim_t)[0].contiguous()
        labels0 = [int(i) for i in box_labels]
        kw = {"head_type": self.ground_head_type, "temperature": self.ground_temperature}
        if self.ground_head_type == "infonce":
            positive = torch.zeros(n_obj + 1, dtype=torch.uint8)
            positive[torch.tensor(labels0 or [-1], dtype=torch.int64)] = 1        # no target: the zero-target row (llava_qwen.py:304-305)
        else:
            positive, kw["pos_weight"] = train.ground_bce_targets(labels0, n_obj)
        if self.pe_kind == "mlp":
            kw["pe_mlp"], kw["pe_centres"] = tr["pe_mlp"], centres
        args = (patches, vox, self.pe_table, pre_ids, post_ids, ground_row, mask, box_pe, positive.to(dev), self.rope, frames,
                self.n_q, self.n_kv, self.hd)
        return _GroundLoss.apply(self, (args, kw), *self._params)
