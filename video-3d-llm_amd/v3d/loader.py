"""Checkpoint side of `LlavaQwenForCausalLM.from_pretrained` (reference: llava/model/builder.py:206-228 ->
transformers' from_pretrained): reads the weight shards of a LLaVA-Qwen checkpoint directory into one state dict
under the reference's keys and derives the engine's widths from the HF config + the tensors' shapes.

Only loaders that execute nothing from the file are used: safetensors, or torch.load(weights_only=True) for
pytorch_model*.bin.  Host-side plumbing; nothing here computes on the path."""
import glob
import json
import os

import torch

from ._native import V3DError
from .engine import PE_MLP_KEYS, PE_MLP_PREFIX, EngineConfig, LlmConfig, VitConfig

VIT_PREFIX = "model.vision_tower.vision_tower.vision_model."


def _load_file(path):
    if path.endswith(".safetensors"):
        from safetensors.torch import load_file
        return load_file(path, device="cpu")
    return torch.load(path, map_location="cpu", weights_only=True)


def read_weights(model_dir):
    """All tensors of a checkpoint directory (model.safetensors[.index.json] shards or pytorch_model*.bin)."""
    if not os.path.isdir(model_dir):
        raise V3DError(f"{model_dir} is not a checkpoint directory (hub ids cannot be fetched: there is no network path here)")
    for index in ("model.safetensors.index.json", "pytorch_model.bin.index.json"):
        ip = os.path.join(model_dir, index)
        if os.path.exists(ip):
            with open(ip) as f:
                files = sorted(set(json.load(f)["weight_map"].values()))
            break
    else:
        files = sorted(os.path.basename(p) for p in glob.glob(os.path.join(model_dir, "*.safetensors")))
        if not files:
            files = sorted(os.path.basename(p) for p in glob.glob(os.path.join(model_dir, "pytorch_model*.bin")))
    if not files:
        raise V3DError(f"no *.safetensors / pytorch_model*.bin weights under {model_dir}")
    sd = {}
    for f in files:
        sd.update(_load_file(os.path.join(model_dir, f)))
    return sd


def read_tower_weights(tower_dir):
    """SigLipVisionModel.from_pretrained(vision_tower_name) (siglip_encoder.py:568) for checkpoints that do not carry
    the tower: keys `vision_model.*` of the SigLIP directory, re-prefixed to where the LLaVA state dict keeps them."""
    sd = read_weights(tower_dir)
    out = {}
    for k, v in sd.items():
        if k.startswith("vision_model."):
            out["model.vision_tower.vision_tower." + k] = v
    if not out:
        raise V3DError(f"{tower_dir} holds no vision_model.* tensors")
    return out


_AGGREGATIONS = (("avg", 1), ("sample9", 9), ("sample5", 5), ("sample1", 1), ("minmax", 2))


def _parse_aggregation(wtype):
    """The first of avg / sample9 / sample5 / sample1 / minmax the string contains (llava_arch.py:395-407) and `discrete`."""
    for aggregation, n_points in _AGGREGATIONS:
        if aggregation in wtype:
            return aggregation, n_points, "discrete" in wtype
    raise V3DError(f"world_position_embedding_type {wtype!r} names none of avg / sample9 / sample5 / sample1 / minmax")


def parse_position_type(wtype):
    """world_position_embedding_type -> (aggregation, n_points, discrete), with the reference's precedence (llava_arch.py:395-407,
    :51-58): the first of avg / sample9 / sample5 / sample1 / minmax the string contains; `discrete` = voxelise before the PE.  This is
    the sin3d parser: an `mlp` type (parse_position_encoder, parse_mlp_position_type) needs checkpoint weights, `mrope` another rotary rule
    (DESIGN section 2)."""
    if "mrope" in wtype or "mlp" in wtype:
        raise V3DError(f"world_position_embedding_type {wtype!r}: the 'mlp' and 'mrope' encodings are not on the accelerated path")
    if "sin3d" not in wtype:
        raise V3DError(f"world_position_embedding_type {wtype!r}: only 'sin3d' encodings are on the accelerated path")
    return _parse_aggregation(wtype)


def parse_position_encoder(wtype):
    """world_position_embedding_type -> 'sin3d' | 'mlp': which module encodes the coordinates.  `mlp` in the string selects
    PositionEmbeddingMLP and wins over `sin3d` (llava_arch.py:60-63); it is accepted with the one-point aggregations only (avg, sample1,
    each with or without `discrete`): with sample9 / sample5 / minmax the reference's module names an undefined `num_feats`
    (position_encoding.py:79) and cannot run.  `mrope` is refused: the reference tests its flag before it sets it (llava_arch.py:415-423)
    and defines no decode positions."""
    if "mrope" in wtype:
        raise V3DError(f"world_position_embedding_type {wtype!r}: 'mrope' does not run in the reference (its flag is tested before it is set, "
                       "llava_arch.py:415-423, and decode positions are undefined); it is not on the accelerated path")
    if "mlp" in wtype:
        aggregation, n_points, _ = _parse_aggregation(wtype)
        if n_points != 1:
            raise V3DError(f"world_position_embedding_type {wtype!r}: the 'mlp' encoding takes one point per patch (avg, sample1); with "
                           f"{aggregation!r} the reference module names an undefined `num_feats` (position_encoding.py:79) and cannot run")
        return "mlp"
    parse_position_type(wtype)
    return "sin3d"


def parse_mlp_position_type(wtype):
    """(aggregation, n_points, discrete) of an `mlp` type; raises for every other string."""
    if parse_position_encoder(wtype) != "mlp":
        raise V3DError(f"world_position_embedding_type {wtype!r} is not an 'mlp' type")
    return _parse_aggregation(wtype)


def engine_config(hf_config, sd, max_positions=None):
    """EngineConfig from the HF config (Qwen2 fields, llava_qwen.py:37-38 + the 3-D keys train_3d.py:1429-1459 persists)
    and the SigLIP tensors' shapes.  The tower keeps every layer the checkpoint has except the one the reference deletes
    (siglip_encoder.py:570): a checkpoint saved AFTER that deletion (the tower was trained / saved with the model) has it
    gone already, a raw SigLIP directory still has all 27."""
    c = hf_config
    wtype = getattr(c, "world_position_embedding_type", "avg-discrete-sin3d")
    pe_kind = "mlp" if "mlp" in wtype and "mrope" not in wtype else "sin3d"
    if pe_kind == "mlp":       # accepted only with the module's six tensors; a state dict that has them under a sin3d type ignores them
        missing = [PE_MLP_PREFIX + k for k in PE_MLP_KEYS.values() if PE_MLP_PREFIX + k not in sd]
        if missing:
            raise V3DError(f"world_position_embedding_type {wtype!r} needs the PositionEmbeddingMLP weights, the state dict has no {missing[0]}")
        aggregation, n_points, discrete = parse_mlp_position_type(wtype)
    else:
        aggregation, n_points, discrete = parse_position_type(wtype)
    for key, want in (("mm_spatial_pool_mode", "bilinear"), ("mm_newline_position", "grid"), ("mm_projector_type", "mlp2x_gelu")):
        got = getattr(c, key, want)
        if got != want:
            raise V3DError(f"config.{key} = {got!r}: only {want!r} is on the accelerated path")
    if int(getattr(c, "mm_spatial_pool_stride", 2)) != 2:
        raise V3DError("only mm_spatial_pool_stride 2 (27x27 -> 14x14) is on the accelerated path")
    pe_w = sd.get(VIT_PREFIX + "embeddings.patch_embedding.weight")
    if pe_w is None:
        raise V3DError("the state dict has no SigLIP tower (model.vision_tower.vision_tower.vision_model.*)")
    layers = 1 + max(int(k[len(VIT_PREFIX + "encoder.layers."):].split(".")[0]) for k in sd if k.startswith(VIT_PREFIX + "encoder.layers."))
    v_hidden, patch = pe_w.shape[0], pe_w.shape[-1]
    n_pos = sd[VIT_PREFIX + "embeddings.position_embedding.weight"].shape[0]
    side = int(round(n_pos ** 0.5))
    vit = VitConfig(hidden=v_hidden, inter=sd[VIT_PREFIX + "encoder.layers.0.mlp.fc1.weight"].shape[0], layers=layers,
                    heads=v_hidden // 72, image=side * patch, patch=patch, eps=1e-6)
    cap = max_positions or getattr(c, "v3d_max_positions", None) or min(int(getattr(c, "max_position_embeddings", 8192)), 8192)
    llm = LlmConfig(hidden=c.hidden_size, inter=c.intermediate_size, layers=c.num_hidden_layers, heads=c.num_attention_heads,
                    kv_heads=c.num_key_value_heads, vocab=sd["lm_head.weight"].shape[0], eps=float(c.rms_norm_eps),
                    rope_theta=float(getattr(c, "rope_theta", None) or (getattr(c, "rope_parameters", None) or {}).get("rope_theta", 1e6)),
                    max_pos=int(cap))
    return EngineConfig(vit=vit, llm=llm, min_xyz=tuple(getattr(c, "min_xyz_range", (-15, -15, -5))),
                        max_xyz=tuple(getattr(c, "max_xyz_range", (15, 15, 5))), voxel_size=float(getattr(c, "voxel_size", 0.1)),
                        ground_head_type=getattr(c, "ground_head_type", None) or "infonce",
                        object_feature_type=getattr(c, "object_feature_type", None) or "patch14-pe",
                        aggregation=aggregation, n_points=n_points, discrete=discrete, pe_kind=pe_kind)


def drop_deleted_tower_layer(sd, tower_from_raw_siglip):
    """siglip_encoder.py:570 `del encoder.layers[-1:]` for weights that come from a raw SigLIP directory."""
    if not tower_from_raw_siglip:
        return sd
    pfx = VIT_PREFIX + "encoder.layers."
    last = max(int(k[len(pfx):].split(".")[0]) for k in sd if k.startswith(pfx))
    return {k: v for k, v in sd.items() if not k.startswith(f"{pfx}{last}.")}


# ------------------------------------------------------------------------------ LoRA adapter directories (--lora-path)

LORA_TARGETS = ("q_proj", "k_proj", "v_proj", "o_proj", "gate_proj", "up_proj", "down_proj")     # find_all_linear_names for this model
_LORA_PARENT = {"q_proj": "self_attn", "k_proj": "self_attn", "v_proj": "self_attn", "o_proj": "self_attn", "gate_proj": "mlp",
                "up_proj": "mlp", "down_proj": "mlp"}


def strip_peft_prefix(key):
    """builder.py:104-106: `base_model.` off, then `model.` off a key that starts `model.model.` - peft's wrapper names down to the
    state dict's."""
    if key.startswith("base_model."):
        key = key[len("base_model."):]
    if key.startswith("model.model."):
        key = key[len("model."):]
    return key


def lora_key(layer, module, which, adapter_name=None):
    """The reference's key of one adapter matrix: base_model.model.model.layers.{i}.{self_attn|mlp}.{module}.lora_{A|B}[.name].weight."""
    mid = f".{adapter_name}" if adapter_name else ""
    return f"base_model.model.model.layers.{layer}.{_LORA_PARENT[module]}.{module}.lora_{which}{mid}.weight"


def save_lora(lora_dir, adapters, non_lora_trainables, r, lora_alpha):
    """An adapter directory as the reference's trainer leaves it (train_3d.py:1875-1884): adapter_config.json, adapter_model.bin
    (torch.save; keys lora_key(...)) and non_lora_trainables.bin (the trained non-adapter tensors under the reference's keys).
    adapters: {(layer, module): (A [r, K], B [N, r])}."""
    os.makedirs(lora_dir, exist_ok=True)
    cfg = {"peft_type": "LORA", "r": int(r), "lora_alpha": lora_alpha, "target_modules": list(LORA_TARGETS), "lora_dropout": 0.0,
           "bias": "none", "task_type": "CAUSAL_LM"}
    with open(os.path.join(lora_dir, "adapter_config.json"), "w") as f:
        json.dump(cfg, f, indent=1)
    sd = {}
    for (layer, module), (a, b) in sorted(adapters.items()):
        sd[lora_key(layer, module, "A")] = a.detach().cpu().contiguous()
        sd[lora_key(layer, module, "B")] = b.detach().cpu().contiguous()
    torch.save(sd, os.path.join(lora_dir, "adapter_model.bin"))
    torch.save({k: v.detach().cpu().contiguous() for k, v in non_lora_trainables.items()}, os.path.join(lora_dir, "non_lora_trainables.bin"))


def load_lora(lora_dir):
    """Reads an adapter directory -> {"r", "lora_alpha", "scaling", "adapters": {(layer, module): (A, B)}, "non_lora": {key: tensor}}.
    Keys in either form peft writes (`.lora_A.weight`, or `.lora_A.<adapter name>.weight` as the drivers' adapter_name="lora" gives),
    prefixes stripped as builder.py:104-106 does.  lora_dropout is accepted whatever it is (it plays no part in a merge); bias must be
    "none"."""
    import re
    cp = os.path.join(lora_dir, "adapter_config.json")
    if not os.path.exists(cp):
        raise V3DError(f"{lora_dir} holds no adapter_config.json: not a LoRA adapter directory")
    with open(cp) as f:
        cfg = json.load(f)
    if cfg.get("peft_type", "LORA") != "LORA":
        raise V3DError(f"adapter_config.peft_type = {cfg.get('peft_type')!r}: only LORA adapters can be merged")
    if cfg.get("bias", "none") != "none":
        raise V3DError(f"adapter_config.bias = {cfg.get('bias')!r}: adapter biases are not built, lora_bias must be 'none'")
    r, alpha = int(cfg["r"]), float(cfg["lora_alpha"])
    for name in ("adapter_model.safetensors", "adapter_model.bin"):
        if os.path.exists(os.path.join(lora_dir, name)):
            raw = _load_file(os.path.join(lora_dir, name))
            break
    else:
        raise V3DError(f"{lora_dir} holds no adapter_model.safetensors / adapter_model.bin")
    pat = re.compile(r"^model\.layers\.(\d+)\.(?:self_attn|mlp)\.([a-z_]+)\.lora_([AB])(?:\.[^.]+)?\.weight$")
    parts = {}
    for k, v in raw.items():
        m = pat.match(strip_peft_prefix(k))
        if m is None or m.group(2) not in LORA_TARGETS:
            raise V3DError(f"adapter key {k!r}: adapters are merged on the decoder's {', '.join(LORA_TARGETS)} only")
        parts.setdefault((int(m.group(1)), m.group(2)), {})[m.group(3)] = v
    adapters = {}
    for key, ab in parts.items():
        if sorted(ab) != ["A", "B"] or ab["A"].shape[0] != r or ab["B"].shape[1] != r:
            raise V3DError(f"adapter of layer {key[0]} {key[1]}: needs lora_A [r, in] and lora_B [out, r] with r = {r}")
        adapters[key] = (ab["A"], ab["B"])
    nl = os.path.join(lora_dir, "non_lora_trainables.bin")
    non_lora = {strip_peft_prefix(k): v for k, v in _load_file(nl).items()} if os.path.exists(nl) else {}
    return {"r": r, "lora_alpha": alpha, "scaling": alpha / r, "adapters": adapters, "non_lora": non_lora}


def merge_lora(sd, lora, dtype, device):
    """Merges every adapter of load_lora's result into the state dict's 16-bit weight on the device, W' = round(W + round(s B A))
    (v3d.train.lora_merge: one v3d_gemm with EPI_RES per linear), then overlays the non-adapter tensors.  Runs before the
    engine lays the weights out and before any e4m3 / MXFP4 quantisation; the merged tensors stay in HBM."""
    from . import train
    out = dict(sd)
    for (layer, module), (a, b) in sorted(lora["adapters"].items()):
        key = f"model.layers.{layer}.{_LORA_PARENT[module]}.{module}.weight"
        if key not in out:
            raise V3DError(f"the adapter names {key}, which the checkpoint does not have")
        w = out[key].to(device=device, dtype=dtype).contiguous()
        if tuple(w.shape) != (b.shape[0], a.shape[1]):
            raise V3DError(f"adapter of {key}: A {tuple(a.shape)} / B {tuple(b.shape)} do not fit the weight {tuple(w.shape)}")
        out[key] = train.lora_merge(w, _pad_rank(a.to(device=device, dtype=dtype), 0), _pad_rank(b.to(device=device, dtype=dtype), 1), lora["scaling"])
    for k, v in lora["non_lora"].items():
        out[k] = v
    return out


def _pad_rank(t, dim):
    """Zero rows (A) / columns (B) up to the next multiple of 16 (v3d_transpose takes columns in eights); zeros add nothing to B A."""
    r = t.shape[dim]
    rp = (r + 15) // 16 * 16
    if rp == r:
        return t.contiguous()
    shape = list(t.shape)
    shape[dim] = rp
    out = torch.zeros(shape, dtype=t.dtype, device=t.device)
    out.narrow(dim, 0, r).copy_(t)
    return out


def load_pretrained_model(model_path, model_base=None, model_name=None, device_map="auto", torch_dtype="float16",
                          attn_implementation="flash_attention_2", overwrite_config=None, llm_weights="bf16", lora_path=None, **kwargs):
    """The LLaVA-Qwen branch of llava.model.builder.load_pretrained_model (builder.py:26-36, 206-228, 266-292) for callers that
    run without the reference checkout on the path: tokenizer, LlavaQwenForCausalLM.from_pretrained with the same keyword
    arguments, resize_token_embeddings, the tower's image processor, the context length.  Same return tuple.  llm_weights "fp8" / "fp4":
    e4m3 / MXFP4 decoder linears (Engine(llm_fp8=) / Engine(llm_fp4=)); the reference has neither.  lora_path: an adapter directory
    (model_scanqa.py:91-112): its config.json (when it has one) overwrites the checkpoint's config and its tokenizer (when it has one)
    replaces the checkpoint's; inside from_pretrained the adapters are merged on the device and non_lora_trainables.bin is overlaid, then
    llm_weights quantises the merged 16-bit weights; the token tables are resized to the tokenizer last (the reference's drivers resize
    before they merge: the merge touches only the decoder's linears, which a resize does not)."""
    from transformers import AutoTokenizer

    from llava.model import LlavaQwenConfig, LlavaQwenForCausalLM
    if model_base is not None or kwargs:
        raise NotImplementedError(f"only a full LLaVA-Qwen checkpoint directory is supported here (model_base / {sorted(kwargs)} given)")
    dt = {"float16": torch.float16, "bfloat16": torch.bfloat16}[torch_dtype] if isinstance(torch_dtype, str) else torch_dtype
    tok_dir = model_path
    if lora_path is not None:
        lora_path = os.fspath(lora_path)
        cj = os.path.join(lora_path, "config.json")
        if os.path.exists(cj):
            with open(cj) as f:
                from_lora = {k: v for k, v in json.load(f).items() if not k.startswith("_") and k not in ("transformers_version", "architectures")}
            overwrite_config = {**from_lora, **(overwrite_config or {})}
        if os.path.exists(os.path.join(lora_path, "tokenizer_config.json")):
            tok_dir = lora_path
    tokenizer = AutoTokenizer.from_pretrained(tok_dir)
    cfg = None
    if overwrite_config:
        cfg = LlavaQwenConfig.from_pretrained(model_path)
        for k, v in overwrite_config.items():
            setattr(cfg, k, v)
    model = LlavaQwenForCausalLM.from_pretrained(model_path, low_cpu_mem_usage=True, attn_implementation=attn_implementation, config=cfg,
                                                 device_map=device_map, torch_dtype=dt, llm_fp8=llm_weights == "fp8",
                                                 llm_fp4=llm_weights == "fp4", lora_path=lora_path)
    # builder.py:266-275: the image patch / start / end tokens join the tokenizer before the tables are resized to len(tokenizer)
    # (mm_use_im_patch_token defaults to True upstream) - mirrored so that both loaders see the same vocabulary size
    if getattr(model.config, "mm_use_im_patch_token", True):
        tokenizer.add_tokens(["<im_patch>"], special_tokens=True)
    if getattr(model.config, "mm_use_im_start_end", False):
        tokenizer.add_tokens(["<im_start>", "<im_end>"], special_tokens=True)
    model.resize_token_embeddings(len(tokenizer))
    tower = model.get_vision_tower()
    if not tower.is_loaded:
        tower.load_model(device_map=device_map)
    for key in ("max_sequence_length", "max_position_embeddings", "tokenizer_model_max_length"):
        if hasattr(model.config, key):
            return tokenizer, model, tower.image_processor, getattr(model.config, key)
    return tokenizer, model, tower.image_processor, 2048
