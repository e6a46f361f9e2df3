#!/usr/bin/env python3
"""Golden vectors for the learned MLP position encoding (`mlp` in world_position_embedding_type).

TEST INFRASTRUCTURE ONLY, in the manner of tools/gen_pe_points_golden.py: runs where a checkout of the reference exists (V3D_REFERENCE),
imports its modules from where they lie, calls its own `PositionEmbeddingMLP` and `LlavaQwenForCausalLM`, and stores OUTPUTS only:

  tests/golden/pe_mlp.npz             module outputs at E = 256 and 3584, f16 / bf16, integer-valued and continuous inputs; the weights
                                      and inputs are regenerated from a seed (tests/pe_mlp_check.py)
  tests/golden/pe_mlp_stages.npz      the module's z, h and pe with the weights as drawn (no b3 offset), fewer rows
  tests/golden/tiny_model_pe_mlp.npz  the tiny model of tests/golden/tiny_model.npz (its weights and F2 inputs, read from that file) under
                                      four `mlp` type strings, plus the six seeded MLP tensors as bf16 bits

Usage: python tools/gen_pe_mlp_golden.py [module] [stages] [model]"""
import sys
sys.dont_write_bytecode = True
import os

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "tools")]
from oracle import gen_golden as GG          # noqa: E402  (_import_reference, save)
import pe_mlp_check as MC                    # noqa: E402  (the seeded weights and inputs only)
import gen_pe_points_golden as GP            # noqa: E402  (_tiny_model: the tiny model's construction)

MODEL_CASES = (("avg-discrete-mlp", ("f16", "bf16")), ("avg-mlp", ("f16",)), ("sample1-discrete-mlp", ("f16",)))
MODEL_SEED, MODEL_W3_SCALE = MC.SEED + 1, 2.0      # the second Linear scaled so that the PE is not negligible beside the features


def g_module():
    from llava.model.position_encoding import PositionEmbeddingMLP
    out = {}
    for E, kind, src in MC.MODULE_CASES:
        p = MC.seeded_mlp(E, kind)
        mod = PositionEmbeddingMLP(E)
        mod.load_state_dict({MC.REF_KEYS[k]: v.float() for k, v in p.items()}, strict=True)
        mod.to(MC.DT[kind]).eval()
        x = MC.seeded_inputs(kind, src, MC.ROWS[E])
        with torch.no_grad():
            pe = mod(x[None])[0]
        assert pe.dtype == MC.DT[kind] and tuple(pe.shape) == (MC.ROWS[E], E)
        out[f"pe_E{E}_{src}_{kind}"] = MC.bits(pe)
        share, worst = MC.ulp_shares(MC.restate(x, p), out[f"pe_E{E}_{src}_{kind}"])
        print(f"  E={E} {kind} {src}: restatement differs in {100 * share:.3f} % of the elements, at most {worst} ulp")
    GG.save("pe_mlp", **out)


def g_stages():
    """The reference module's three stage outputs with the weights as drawn (no b3 offset): z and h at E = 256's weights, pe at both widths."""
    from llava.model.position_encoding import PositionEmbeddingMLP
    out = {}
    for E in (256, 3584):
        for kind, src in MC.STAGE_CASES:
            p = MC.seeded_mlp(E, kind, b3_offset=0.0)
            mod = PositionEmbeddingMLP(E)
            mod.load_state_dict({MC.REF_KEYS[k]: v.float() for k, v in p.items()}, strict=True)
            mod.to(MC.DT[kind]).eval()
            x = MC.seeded_inputs(kind, src, MC.STAGE_ROWS[E])
            with torch.no_grad():
                z = mod.mlp[0](x)
                h = mod.mlp[2](mod.mlp[1](z))
                pe = mod(x[None])[0]
                assert torch.equal(pe, mod.mlp[3](h))
            if E == 256:
                out[f"z_{src}_{kind}"], out[f"h_{src}_{kind}"] = MC.bits(z), MC.bits(h)
            else:
                out[f"h_E{E}_{src}_{kind}"] = MC.bits(h)
            out[f"pe_E{E}_{src}_{kind}"] = MC.bits(pe)
    GG.save("pe_mlp_stages", **out)


def g_model():
    g = np.load(os.path.join(GG.OUT, "tiny_model.npz"))
    weights = {k[2:]: torch.from_numpy(g[k].view(np.int16)).view(torch.bfloat16).float() for k in g.files if k.startswith("w.")}
    mlp = MC.seeded_mlp(256, "bf16", seed=MODEL_SEED, w3_scale=MODEL_W3_SCALE, b3_offset=0.0)
    weights.update({MC.SD_PREFIX + MC.REF_KEYS[k]: v.float() for k, v in mlp.items()})

    def up8(x, dims):
        for d in dims:
            x = x.repeat_interleave(8, dim=d)
        return x

    images = up8(torch.from_numpy(g["F2_img_lo"]), (2, 3))[None]
    wc = up8(torch.from_numpy(g["F2_wc_lo"]), (1, 2))[None]
    boxes = torch.from_numpy(g["F2_boxes"])
    ids, gids, glabels, cids = (torch.from_numpy(g["F2_" + k])[None] for k in ("ids", "gids", "glabels", "cids"))
    box_in = torch.from_numpy(g["F2_box_in"])
    out = {"mlp." + k: MC.bits(v) for k, v in mlp.items()}
    for wtype, kinds in MODEL_CASES:
        m, inv = GP._tiny_model(wtype, weights)
        assert type(m.get_model().world_position_embedding).__name__ == "PositionEmbeddingMLP"
        tag = wtype.replace("-", "_")
        for kind in kinds:
            dt = MC.DT[kind]
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
                out[f"{tag}_embeds_{kind}"] = MC.bits(emb[0])
                out[f"{tag}_logits_{kind}"] = logits[0, -1].float().numpy()
                out[f"{tag}_tokens_{kind}"] = np.array(toks, np.int64)
                out[f"{tag}_step_logits_{kind}"] = torch.stack(steps).float().numpy()
                shipped = torch.from_numpy(g[f"F2_embeds_{kind}"].astype(np.uint32) << 16).view(torch.float32) if kind == "bf16" \
                    else torch.from_numpy(g[f"F2_embeds_{kind}"]).float()
                print(f"  {wtype} {kind}: tokens {toks}; rel L2 to the shipped type's embeds {((emb[0].float() - shipped).norm() / emb[0].float().norm()).item():.3f}")
                if wtype == "avg-discrete-mlp":
                    vdc = dict(vd, box_input=box_in.to(dt))
                    _, _, _, _, emb_c, _, _, _ = m.prepare_inputs_labels_for_multimodal(cids, None, None, None, None, images.to(dt), ["video"], None, vdc)
                    out[f"{tag}_coord_rows_{kind}"] = MC.bits(emb_c[0, [8 + 2 * 210 - 1, 11 + 2 * 210 - 1]])
                    out[f"{tag}_coord_logits_{kind}"] = m(input_ids=cids, images=images.to(dt), modalities=["video"], video_dict=vdc,
                                                          use_cache=False).logits[0, -1].float().numpy()
                    _, scores = m(input_ids=gids, images=images.to(dt), modalities=["video"], video_dict=vd, labels=glabels,
                                  use_object_proposals=True, use_cache=False)
                    out[f"{tag}_scores_{kind}"] = MC.bits(scores)
            m.float()
    GG.save("tiny_model_pe_mlp", **out)


if __name__ == "__main__":
    GG._import_reference()
    what = sys.argv[1:] or ["module", "stages", "model"]
    if "stages" in what:
        g_stages()
    if "module" in what:
        g_module()
    if "model" in what:
        g_model()
