#!/usr/bin/env python3
"""Golden vectors for the P-point position encodings (sample9 / sample5 / sample1 / minmax, with and without `discrete`).

TEST INFRASTRUCTURE ONLY, in the manner of oracle/gen_golden.py: runs where a checkout of the reference exists (V3D_REFERENCE), imports
its modules from where they lie, calls its own `sample_n_points`, `minmax_coordinate_in_patch`, `discrete_coords`,
`PositionEmbeddingSine3D(E, n_points=P)` and `LlavaQwenForCausalLM`, and stores OUTPUTS only:

  tests/golden/pe_points.npz               coordinates and PE values; the inputs are regenerated from a seed (tests/pe_points_check.py)
  tests/golden/tiny_model_pe_variants.npz  the tiny model of tests/golden/tiny_model.npz (its weights and F2 inputs, read from that
                                           file) under four other world_position_embedding_type strings

Usage: python tools/gen_pe_points_golden.py [coords] [model]"""
import sys
sys.dont_write_bytecode = True
import os
import types

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
from oracle import gen_golden as GG          # noqa: E402  (_import_reference, make_arch, DEFAULT_CFG, save)
import pe_points_check as PC                 # noqa: E402  (the seeded inputs only)

MODEL_CASES = (("sample9-discrete-sin3d", ("f16", "bf16")), ("minmax-discrete-sin3d", ("f16",)), ("sample5-sin3d", ("f16",)),
               ("sample1-discrete-sin3d", ("f16",)))


def g_coords():
    from llava.model.position_encoding import PositionEmbeddingSine3D
    arch = GG.make_arch(GG.DEFAULT_CFG)
    out = {}
    for kind in ("f32", "f16", "bf16"):
        x = PC.seeded_coords(kind)
        for mode, P in PC.MODES.items():
            pts = arch.minmax_coordinate_in_patch(x) if mode == "minmax" else arch.sample_n_points(x, n_points=P)
            vox = arch.discrete_coords(pts, None)
            out[f"{mode}_pts_{kind}"] = PC.bits(pts)
            out[f"{mode}_vox_{kind}"] = PC.bits(vox)
            ids = torch.nan_to_num(vox.float(), nan=-1.0).to(torch.int16)        # NaN positions are in vox; -1 marks them here
            out[f"{mode}_ids_{kind}"] = ids.numpy()
    for E, P in PC.PE_CASES:
        mod = PositionEmbeddingSine3D(E, n_points=P)
        for src, cont in (("ids", False), ("cont", True)):
            for kind in ("f16", "bf16") + (("f32",) if E == 256 else ()):
                x = PC.pe_inputs(E, P, kind, cont)
                out[f"pe_E{E}_P{P}_{src}_{kind}"] = PC.bits(mod(x[None])[0])
    GG.save("pe_points", **out)


def _tiny_model(wtype, weights):
    """g_tiny_model's construction (oracle/gen_golden.py) with another type string and the stored weights."""
    from llava.model.language_model import llava_qwen as lq
    from llava.model.multimodal_encoder import siglip_encoder as se
    from llava.model.multimodal_projector.builder import build_vision_projector
    H, VH = 256, 144
    cfg = lq.LlavaQwenConfig(vocab_size=320, hidden_size=H, intermediate_size=384, num_hidden_layers=2, num_attention_heads=2,
                             num_key_value_heads=1, max_position_embeddings=4096, rms_norm_eps=1e-6, rope_theta=1000000.0,
                             use_sliding_window=False, attention_dropout=0.0)
    cfg.rope_theta = 1000000.0
    cfg._attn_implementation = "eager"
    for k, v in dict(world_position_embedding_type=wtype, mm_spatial_pool_mode="bilinear", mm_spatial_pool_stride=2,
                     voxel_size=0.1, min_xyz_range=[-15, -15, -5], max_xyz_range=[15, 15, 5], mm_patch_merge_type="spatial_unpad",
                     mm_newline_position="grid", ground_head_type="infonce", ground_head_temperature=0.07,
                     object_feature_type="patch14-pe", ground_token_ids=[318], coord_token_ids=[317]).items():
        setattr(cfg, k, v)
    m = lq.LlavaQwenForCausalLM(cfg)
    vcfg = se.SigLipVisionConfig(hidden_size=VH, intermediate_size=272, num_hidden_layers=3, num_attention_heads=2, image_size=384, patch_size=14)
    tower = object.__new__(se.SigLipVisionTower)
    torch.nn.Module.__init__(tower)
    tower.is_loaded, tower.config, tower.vision_tower_name = True, vcfg, "tiny-random"
    tower.vision_tower = se.SigLipVisionModel(vcfg)
    del tower.vision_tower.vision_model.encoder.layers[-1:]
    tower.vision_tower.vision_model.head = torch.nn.Identity()
    m.model.vision_tower = tower
    m.model.mm_projector = build_vision_projector(types.SimpleNamespace(mm_projector_type="mlp2x_gelu", mm_hidden_size=VH, hidden_size=H))
    m.model.image_newline = torch.nn.Parameter(torch.zeros(H))
    m.eval()
    res = m.load_state_dict(weights, strict=False)
    assert not res.unexpected_keys, res.unexpected_keys
    assert all("post_layernorm" in k or "position_ids" in k or "inv_freq" in k for k in res.missing_keys), res.missing_keys
    inv = {k: v.detach().clone() for k, v in m.named_buffers() if "inv_freq" in k}
    return m, inv


def g_model():
    g = np.load(os.path.join(GG.OUT, "tiny_model.npz"))
    weights = {k[2:]: torch.from_numpy(g[k].view(np.int16)).view(torch.bfloat16).float() for k in g.files if k.startswith("w.")}

    def up8(x, dims):
        for d in dims:
            x = x.repeat_interleave(8, dim=d)
        return x

    images = up8(torch.from_numpy(g["F2_img_lo"]), (2, 3))[None]
    wc = up8(torch.from_numpy(g["F2_wc_lo"]), (1, 2))[None]
    boxes = torch.from_numpy(g["F2_boxes"])
    ids, gids, glabels, cids = (torch.from_numpy(g["F2_" + k])[None] for k in ("ids", "gids", "glabels", "cids"))
    box_in = torch.from_numpy(g["F2_box_in"])
    out = {}
    for wtype, kinds in MODEL_CASES:
        m, inv = _tiny_model(wtype, weights)
        tag = wtype.replace("-", "_")
        for kind in kinds:
            dt = PC.DT[kind]
            m.to(dt)
            for mod_name, b in inv.items():                       # from_pretrained(torch_dtype=...) keeps inv_freq f32
                m.get_submodule(mod_name.rsplit(".", 1)[0]).inv_freq = b.float().clone()
            vd = {"world_coords": wc.to(dt), "box_input": [], "objects": boxes.to(dt)[None]}
            with torch.no_grad():
                _, _, _, _, emb, _, _, _ = m.prepare_inputs_labels_for_multimodal(ids, None, None, None, None, images.to(dt), ["video"], None, vd)
                logits = m(input_ids=ids, images=images.to(dt), modalities=["video"], video_dict=vd, use_cache=False).logits
                seq, toks, steps, lg = emb, [], [], logits[0, -1]
                for _ in range(4):
                    toks.append(int(torch.argmax(lg)))
                    if len(toks) == 4:
                        break
                    seq = torch.cat([seq, m.get_model().embed_tokens(torch.tensor([[toks[-1]]]))], 1)
                    lg = m(inputs_embeds=seq, use_cache=False).logits[0, -1]
                    steps.append(lg)
                out[f"{tag}_embeds_{kind}"] = PC.bits(emb[0])
                out[f"{tag}_logits_{kind}"] = logits[0, -1].float().numpy()
                out[f"{tag}_tokens_{kind}"] = np.array(toks, np.int64)
                out[f"{tag}_step_logits_{kind}"] = torch.stack(steps).float().numpy()
                if wtype == "sample9-discrete-sin3d":
                    vdc = dict(vd, box_input=box_in.to(dt))
                    _, _, _, _, emb_c, _, _, _ = m.prepare_inputs_labels_for_multimodal(cids, None, None, None, None, images.to(dt), ["video"], None, vdc)
                    out[f"{tag}_coord_rows_{kind}"] = PC.bits(emb_c[0, [8 + 2 * 210 - 1, 11 + 2 * 210 - 1]])
                    out[f"{tag}_coord_logits_{kind}"] = m(input_ids=cids, images=images.to(dt), modalities=["video"], video_dict=vdc,
                                                          use_cache=False).logits[0, -1].float().numpy()
                    _, scores = m(input_ids=gids, images=images.to(dt), modalities=["video"], video_dict=vd, labels=glabels,
                                  use_object_proposals=True, use_cache=False)
                    out[f"{tag}_scores_{kind}"] = PC.bits(scores)
            m.float()
    GG.save("tiny_model_pe_variants", **out)


if __name__ == "__main__":
    GG._import_reference()
    what = sys.argv[1:] or ["coords", "model"]
    if "coords" in what:
        g_coords()
    if "model" in what:
        g_model()
