"""--lora-path: a LoRA adapter directory merged into the decoder's linears at load (v3d.loader.load_lora / merge_lora,
LlavaQwenForCausalLM.from_pretrained(lora_path=), load_pretrained_model(lora_path=), v3d.eval_scanqa --lora-path), on the tiny model of
tests/tiny_model_fixture.py with the dataset files of tests/test_gpu_eval_harness.py.

  * a B = 0 adapter directory leaves every weight bit-identical and every generated token identical;
  * a random adapter against a checkpoint whose state dict THIS TEST merged (f64 -> 16 bit by the rule W' = round(W + round(s B A)),
    tests/lora_check.py): every merged element is inside the merge bound, each one that differs from the rule's rounding sits at a
    rounding boundary of the rule, the last-token logits are within the merge bound propagated to the logits (_logit_tolerance), and the
    greedy tokens are equal unless the top-2 margin is below 2.5 times that (the form of tests/test_gpu_engine.py); the CPU oracle shows
    that the rule-merged model of this seed has no such near-tie;
  * with llm_weights "fp8" / "fp4" the merge comes first: the engine's quantised bytes and scales equal the quantiser applied to the
    merged 16-bit weights, bit for bit;
  * the training forward with adapters agrees with the engine's loss on the merged weights within the step test's 2 %;
  * v3d.eval_scanqa --lora-path writes the answer file the pre-merged checkpoint writes, record for record.
(The per-element check of merged weights at 512 x 256 and at the stacked 4608 x 3584 is tests/test_gpu_lora_train.py's.)
"""
import json
import os
import shutil

import pytest
import torch

import lora_check as lc
import tiny_model_fixture as TM

pytestmark = pytest.mark.gpu
R, ALPHA, N_NEW = 16, 16, 5
DT = torch.float16                                  # load_pretrained_model's default, the eval drivers' dtype (builder.py:27)


def _shapes():
    # the tiny decoder: hidden 256, MLP 384, 2 / 1 heads of 128
    return {"q_proj": (256, 256), "k_proj": (128, 256), "v_proj": (128, 256), "o_proj": (256, 256), "gate_proj": (384, 256),
            "up_proj": (384, 256), "down_proj": (256, 384)}


def _adapters(zero_b, seed=3):
    g = torch.Generator().manual_seed(seed)
    out = {}
    for layer in range(2):
        for module, (n, k) in _shapes().items():
            a = (torch.randn(R, k, generator=g) * 0.05).to(DT)
            b = torch.zeros(n, R, dtype=DT) if zero_b else (torch.randn(n, R, generator=g) * 0.05).to(DT)
            out[(layer, module)] = (a, b)
    return out


def _rewrite(src, dst, tensors):
    """A copy of checkpoint directory src in which the named tensors are replaced."""
    from safetensors.torch import load_file, save_file
    shutil.copytree(src, dst)
    idx = json.load(open(os.path.join(dst, "model.safetensors.index.json")))
    for shard in sorted(set(idx["weight_map"].values())):
        sd = load_file(os.path.join(dst, shard))
        for k in list(sd):
            if k in tensors:
                sd[k] = tensors[k].detach().cpu().contiguous()
        save_file(sd, os.path.join(dst, shard), metadata={"format": "pt"})
    return dst


@pytest.fixture(scope="module")
def g():
    return TM.load()


@pytest.fixture(scope="module")
def dirs(g, tmp_path_factory):
    from v3d import loader as L
    root = tmp_path_factory.mktemp("lora")
    base = TM.write_checkpoint(str(root / "base" / "llava_qwen_tiny"), g)
    zero, rand = str(root / "adapter_zero"), str(root / "adapter_rand")
    L.save_lora(zero, _adapters(True), {}, R, ALPHA)
    L.save_lora(rand, _adapters(False), {}, R, ALPHA)
    sd = {k: v.to(DT) for k, v in L.read_weights(base).items()}
    lora = L.load_lora(rand)
    by_rule, by_device = {}, {}
    dev = L.merge_lora(sd, lora, DT, "cuda")
    for (layer, module), (a, b) in lora["adapters"].items():
        key = f"model.layers.{layer}.{'self_attn' if module in ('q_proj', 'k_proj', 'v_proj', 'o_proj') else 'mlp'}.{module}.weight"
        by_rule[key] = lc.merge_f64(sd[key], a, b, lora["scaling"]).to(DT)
        by_device[key] = dev[key]
    rule_dir = _rewrite(base, str(root / "rule" / "llava_qwen_tiny"), by_rule)
    dev_dir = _rewrite(base, str(root / "device" / "llava_qwen_tiny"), by_device)
    return dict(base=base, zero=zero, rand=rand, rule=rule_dir, device=dev_dir, by_rule=by_rule, by_device=by_device, sd=sd)


def _load(path, **kw):
    from v3d import loader as L
    return L.load_pretrained_model(path, None, "llava_qwen_tiny", **kw)[1]


def _run(model, g, n_new=5):
    inp = TM.case_inputs(g, "F2")
    images = inp["images"][None].to(DT).cuda()
    vd = {"world_coords": inp["world_coords"][None].to(DT).cuda(), "box_input": torch.Tensor([]), "objects": inp["boxes"][None].to(DT).cuda()}
    logits = model(inp["ids"][None].cuda(), images=images, modalities="video", video_dict=vd).logits[0, -1].float().cpu()
    toks = model.generate(inp["ids"][None].cuda(), images=images, modalities="video", do_sample=False, num_beams=1, max_new_tokens=n_new,
                          use_cache=True, video_dict=vd)[0].tolist()
    return logits, toks


def test_adapter_directory_has_the_references_files_and_keys(dirs):
    from v3d import loader as L
    cfg = json.load(open(os.path.join(dirs["rand"], "adapter_config.json")))
    assert cfg["peft_type"] == "LORA" and cfg["r"] == R and cfg["lora_alpha"] == ALPHA and cfg["lora_dropout"] == 0.0 and cfg["bias"] == "none"
    assert sorted(cfg["target_modules"]) == sorted(L.LORA_TARGETS)
    raw = torch.load(os.path.join(dirs["rand"], "adapter_model.bin"), weights_only=True)
    assert "base_model.model.model.layers.0.self_attn.q_proj.lora_A.weight" in raw and len(raw) == 2 * 2 * 7
    assert os.path.exists(os.path.join(dirs["rand"], "non_lora_trainables.bin"))
    lora = L.load_lora(dirs["rand"])
    want = _adapters(False)
    assert sorted(lora["adapters"]) == sorted(want) and lora["scaling"] == ALPHA / R
    assert all(torch.equal(lora["adapters"][k][0], want[k][0]) and torch.equal(lora["adapters"][k][1], want[k][1]) for k in want)


def test_zero_b_adapter_changes_no_weight_and_no_token(dirs, g):
    from v3d import loader as L
    merged = L.merge_lora(dirs["sd"], L.load_lora(dirs["zero"]), DT, "cuda")
    assert sorted(merged) == sorted(dirs["sd"])
    for k, v in dirs["sd"].items():
        assert torch.equal(merged[k].cpu(), v), f"{k} changed under a B = 0 adapter"
    base = _run(_load(dirs["base"]), g)
    zero = _run(_load(dirs["base"], lora_path=dirs["zero"]), g)
    assert torch.equal(base[0], zero[0]) and base[1] == zero[1]


def _key(layer, module):
    return f"model.layers.{layer}.{'self_attn' if module in ('q_proj', 'k_proj', 'v_proj', 'o_proj') else 'mlp'}.{module}.weight"


def _logit_tolerance(dirs):
    """The merge bound propagated to the logits the way tests/test_gpu_engine.py states its tolerances (one relative L2 figure for the
    logits, 2.5 times it, of the largest |logit|, as the margin below which a differing greedy token is a near-tie): the two models
    differ only in the 14 merged linears, linear k by at most merge_bound_k per element, i.e. by rho_k = |bound_k|_F / |W'_k|_F
    relatively; to first order each perturbed linear moves what follows it by rho_k of its size (the norms and the softmax do not
    amplify a relative change), so the logits move by at most the sum of the rho_k.  From reference quantities only."""
    s, tol = ALPHA / R, 0.0
    for (layer, module), (a, b) in _adapters(False).items():
        w = dirs["sd"][_key(layer, module)]
        exact = w.double() + s * (b.double() @ a.double())
        tol += (lc.merge_bound(w, a, b, s).norm() / exact.norm()).item()
    return tol


def test_the_rule_merged_model_has_no_near_tie_on_the_cpu_oracle(dirs, g):
    """The seed of _adapters: the model merged by the f64 rule, evaluated by the CPU oracle alone (no device code), shows no top-2
    near-tie at any of the greedy steps the device tests compare - so a differing token below is a finding, not an excuse."""
    from oracle import pipeline_oracle as PO
    sd = dict(TM.state_dict(g))
    sd.update({k: v.float() for k, v in dirs["by_rule"].items()})
    inp = TM.case_inputs(g, "F2")
    out = PO.scene_forward(sd, TM.ORACLE_CFG, inp["ids"], inp["images"], inp["world_coords"], DT, max_new_tokens=N_NEW)
    noise = 2.5 * _logit_tolerance(dirs)
    margins = []
    for lg in [out["logits_last"]] + list(out["step_logits"])[: N_NEW - 1]:
        top2 = torch.topk(lg.float(), 2).values
        margins.append(((top2[0] - top2[1]) / lg.float().abs().max()).item())
    print(f"CPU oracle, rule-merged model: top-2 margins / max |logit| {[round(m, 4) for m in margins]}, noise level {noise:.4f}")
    assert min(margins) > noise, (margins, noise)


def test_random_adapter_equals_the_checkpoint_merged_by_the_rule(dirs, g):
    s = ALPHA / R
    h = lc.H[DT]
    differ = total = moved = 0
    for (layer, module), (a, b) in _adapters(False).items():
        k = _key(layer, module)
        w, dev, rule = dirs["sd"][k], dirs["by_device"][k].cpu(), dirs["by_rule"][k]
        total += w.numel()
        moved += int((rule != w).sum())
        exact = w.double() + s * (b.double() @ a.double())
        assert lc.worst_ratio(dev, exact, lc.merge_bound(w, a, b, s)) <= 1.0, k          # every element inside the merge bound
        # every element that differs from the f64 rule sits at a rounding boundary of one of the rule's two roundings: the f32 product
        # (error at most acc) lies within acc of a midpoint between two 16-bit neighbours of s B A, or the sum W + delta does with the
        # delta one ulp apart
        bad = (dev.double() != rule.double()).nonzero()
        differ += bad.shape[0]
        prod = s * (b.double() @ a.double())
        acc = lc.C_ACC * (128 / 32.0 + lc.C0) * lc.ULP32 * (abs(s) * (b.double().abs() @ a.double().abs()))
        for i, j in bad.tolist():
            lo, hi = lc.rnd(prod[i, j] - acc[i, j], DT), lc.rnd(prod[i, j] + acc[i, j], DT)
            sums = {float(lc.rnd(w[i, j].double() + d, DT)) for d in (lo, hi)}
            assert lo != hi and float(dev[i, j]) in sums, f"{k}[{i}, {j}]: {float(dev[i, j])} vs the rule's {float(rule[i, j])}, not a rounding boundary"
    print(f"device merge vs the f64 rule: {differ} of {total} elements differ, each at a rounding boundary; the adapter moved {moved}")
    assert moved > 0.5 * total
    tol = _logit_tolerance(dirs)
    got = _run(_load(dirs["base"], lora_path=dirs["rand"]), g)
    want = _run(_load(dirs["rule"]), g)
    same = _run(_load(dirs["device"]), g)
    base = _run(_load(dirs["base"]), g)
    assert torch.equal(got[0], same[0]) and got[1] == same[1], "merged at load differs from the checkpoint that stores the same merged weights"
    rel = ((got[0] - want[0]).norm() / want[0].norm()).item()
    print(f"last-token logits, merged at load vs merged by the rule: rel L2 {rel:.2e} (propagated merge bound {tol:.2e}); "
          f"vs the base model {((base[0] - want[0]).norm() / want[0].norm()).item():.2e}")
    assert rel <= tol
    assert not torch.equal(base[0], want[0]), "the adapter does not change the logits: the comparison shows nothing"
    if got[1] != want[1]:
        t = next(i for i, (x, y) in enumerate(zip(got[1], want[1])) if x != y)
        assert t == 0, f"tokens differ at step {t} ({got[1]} vs {want[1]}): only the first step's logits are held here"
        top2 = torch.topk(want[0], 2).values
        margin = ((top2[0] - top2[1]) / want[0].abs().max()).item()
        print(f"tokens differ ({got[1]} vs {want[1]}); top-2 margin of the first step {margin:.4f} of max |logit|")
        assert margin < 2.5 * tol, (got[1], want[1], margin)


def _engine_linears(by_key, layer, quant):
    """The four decoder linears of one layer in the engine's layouts, from per-module 16-bit weights (v3d/engine.py _prep_llm)."""
    from v3d import ops
    from v3d.engine import _pad2, _up
    p = f"model.layers.{layer}."
    w = lambda n: by_key[p + n + ".weight"].cuda()
    wqkv = torch.cat([w("self_attn.q_proj"), w("self_attn.k_proj"), w("self_attn.v_proj")], 0)
    return {"wqkv": _pad2(wqkv, _up(wqkv.shape[0], 256 if quant else 128), wqkv.shape[1]), "wo": w("self_attn.o_proj").contiguous(),
            "wgu": ops.interleave_gate_up(w("mlp.gate_proj"), w("mlp.up_proj")), "wd": w("mlp.down_proj").contiguous()}


@pytest.mark.parametrize("llm_weights", ["fp8", "fp4"])
def test_quantisation_comes_after_the_merge(dirs, g, llm_weights):
    """The engine's quantised bytes and scales of every decoder linear equal the quantiser applied to the merged 16-bit weights, bit
    for bit; logits and tokens equal those of the checkpoint that stores the merged weights."""
    from v3d import ops
    model = _load(dirs["base"], lora_path=dirs["rand"], llm_weights=llm_weights)
    quantise, tag = (ops.quantize_fp8_rows, "8") if llm_weights == "fp8" else (ops.quantize_mxfp4_rows, "4")
    unmerged = 0
    for layer in range(2):
        merged = _engine_linears(dirs["by_device"], layer, True)
        plain = _engine_linears(dirs["sd"], layer, True)
        for name, w16 in merged.items():
            have = model.engine.l_layers[layer][name + tag]
            want = quantise(w16)
            assert len(have) == len(want) == 2
            assert torch.equal(have[0], want[0]), f"layer {layer} {name}: quantised bytes differ from the quantiser on the merged weights"
            assert torch.equal(have[1], want[1]), f"layer {layer} {name}: scales differ from the quantiser on the merged weights"
            unmerged += int(not torch.equal(have[0], quantise(plain[name])[0]))
    assert unmerged == 8, "the quantised weights equal those of the UNMERGED checkpoint: the comparison shows nothing"
    got = _run(model, g)
    want = _run(_load(dirs["device"], llm_weights=llm_weights), g)
    assert torch.equal(got[0], want[0]) and got[1] == want[1], "the quantised model differs from quantising the merged 16-bit weights"
    plain = _run(_load(dirs["device"]), g)
    assert not torch.equal(plain[0], want[0]), "llm_weights had no effect: the comparison shows nothing"


def test_training_forward_loss_agrees_with_the_engines_loss_on_the_merged_weights(dirs, g):
    """The training forward with adapters (v3d.train's LoRA rule on unmerged weights) against the ENGINE's loss on the weights
    loader.merge_lora merged: the language model of the tiny checkpoint on the engine's own inputs_embeds and labels, within the step
    test's 2 %."""
    from v3d import loader as L
    from v3d import ops, train
    model = _load(dirs["base"], lora_path=dirs["rand"], torch_dtype=torch.bfloat16)
    inp = TM.case_inputs(g, "F2")
    bf = torch.bfloat16
    images = inp["images"][None].to(bf).cuda()
    vd = {"world_coords": inp["world_coords"][None].to(bf).cuda(), "box_input": torch.Tensor([]), "objects": inp["boxes"][None].to(bf).cuda()}
    lab = torch.full_like(inp["ids"], -100)
    lab[-4:] = inp["ids"][-4:]
    out = model(inp["ids"][None].cuda(), images=images, modalities="video", video_dict=vd, labels=lab[None].cuda())
    tup = model.prepare_inputs_labels_for_multimodal(inp["ids"][None].cuda(), None, None, None, lab[None].cuda(), images, ["video"], None, vd)
    x, labels = tup[4][0].to(bf).contiguous(), tup[5][0].contiguous()
    sd = {k: v.to(bf).cuda() for k, v in dirs["sd"].items()}
    lora = L.load_lora(dirs["rand"])
    layers = []
    for i in range(2):
        p = f"model.layers.{i}."
        t = lambda n: sd[p + n].contiguous()
        layers.append({"ln1": t("input_layernorm.weight"),
                       "qkv": torch.cat([t(f"self_attn.{n}_proj.weight") for n in "qkv"], 0).contiguous(),
                       "qkv_bias": torch.cat([t(f"self_attn.{n}_proj.bias") for n in "qkv"], 0).contiguous(),
                       "o": t("self_attn.o_proj.weight"), "ln2": t("post_attention_layernorm.weight"),
                       "gate_up": torch.cat([t("mlp.gate_proj.weight"), t("mlp.up_proj.weight")], 0).contiguous(), "down": t("mlp.down_proj.weight")})
    params = {"layers": layers, "norm": sd["model.norm.weight"], "lm_head": sd["lm_head.weight"].contiguous()}
    train.lora_init(params, r=R, alpha=ALPHA, seed=0, qkv_rows=(256, 128, 128))
    for i, p in enumerate(params["layers"]):                       # the directory's adapters in the stacked training form
        for name, modules in train.LORA_MODULES.items():
            a_list = [lora["adapters"][(i, m)][0].to(bf).cuda() for m in modules]
            b_list = [lora["adapters"][(i, m)][1].to(bf).cuda() for m in modules]
            A, B, _ = train.lora_stack(a_list, b_list)
            p["lora"][name]["A"].copy_(A)
            p["lora"][name]["B"].copy_(B)
    train.lora_refresh(params)
    rope = train.RopeTables(128, 2048, 1e6, bf, "cuda")
    # the training forward of v3d.train (llm_layers_forward with adapters, final norm, LM head, shifted cross-entropy); the 320-row head
    # is padded to the GEMM's 128-row tiles with zero rows and the padding columns are cut before the loss
    h, _ = train.llm_layers_forward(params, x, rope, 2, 1, 128)
    head = torch.zeros((384, 256), dtype=bf, device="cuda")
    head[:320] = params["lm_head"]
    logits = ops.gemm(ops.rmsnorm(h, params["norm"], 1e-6), head)[:, :320]
    loss, _ = ops.cross_entropy(logits, labels)
    rel = abs(float(loss) - float(out.loss)) / float(out.loss)
    print(f"training forward with adapters {float(loss):.5f}, engine on the merged weights {float(out.loss):.5f}: {rel:.3e} relative")
    assert rel < 2e-2


def test_eval_scanqa_lora_path_writes_the_premerged_answers(dirs, tmp_path):
    from test_gpu_eval_harness import _dataset
    from v3d import eval_scanqa as E
    root = str(tmp_path)
    _dataset(root)

    def argv(ckpt, out, *extra):
        return ["--model-path", ckpt, "--video-folder", root, "--embodiedscan-folder", os.path.join(root, "embodiedscan"),
                "--metadata-folder", os.path.join(root, "metadata"), "--question-file", os.path.join(root, "questions.json"),
                "--max_frame_num", "4", "--max-new-tokens", "5", "--no-pipeline", "--answer-file", os.path.join(root, "out", out), *extra]
    assert E.main(argv(dirs["base"], "lora.jsonl", "--lora-path", dirs["rand"])) == 0
    assert E.main(argv(dirs["device"], "merged.jsonl")) == 0
    assert E.main(argv(dirs["base"], "base.jsonl")) == 0
    lora = [json.loads(l) for l in open(os.path.join(root, "out", "lora.jsonl"))]
    merged = [json.loads(l) for l in open(os.path.join(root, "out", "merged.jsonl"))]
    base = [json.loads(l) for l in open(os.path.join(root, "out", "base.jsonl"))]
    assert len(lora) == 7 and lora == merged
    assert lora != base, "the adapter changes no answer: the comparison shows nothing"


def test_refusals_name_the_field(dirs, tmp_path):
    from v3d import loader as L
    from v3d._native import V3DError
    bad = str(tmp_path / "bias")
    shutil.copytree(dirs["rand"], bad)
    cfg = json.load(open(os.path.join(bad, "adapter_config.json")))
    cfg["bias"], cfg["lora_dropout"] = "all", 0.05
    json.dump(cfg, open(os.path.join(bad, "adapter_config.json"), "w"))
    with pytest.raises(V3DError, match="lora_bias"):
        L.load_lora(bad)
    cfg["bias"] = "none"                             # the config default of 0.05 dropout is accepted at merge time
    json.dump(cfg, open(os.path.join(bad, "adapter_config.json"), "w"))
    assert L.load_lora(bad)["r"] == R
    with pytest.raises(V3DError, match="adapter_config.json"):
        L.load_lora(str(tmp_path))
