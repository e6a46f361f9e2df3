"""The LoRA checker (tests/lora_check.py) is neither loose nor wrong.  No GPU: -m "not gpu".

An f32 emulation of the two kernels' summation (csrc/lora.hip: 32-wide blocks in one accumulator; for wgrad chunks of rows, their
slabs added in order) passes the bound on random inputs and is bit-equal on exact ones; emulations with one thing wrong fail one of the
two.  The f64 rule of a LoRA linear is held against torch autograd in f64, and the merge rule against its definition.

Worst |err| / bound of the emulation (C_ACC = 2, C0 = 32 are gemm_check's constants; they were NOT tuned here or on the kernels):
    down   (M 48, R 64)      K     64     320    3584   18944
           bf16                 0.979   0.951   0.877   0.548
           f16                  0.922   0.945   0.652   0.145
    wgrad  (R 32, K 64)      M      7     129    1000    6794      chunk 32 / 64 / 128 / 704 rows
           bf16 -> bf16         0.963   0.975   0.920   0.818
           f16  -> f16          0.945   0.941   0.785   0.372
           bf16 -> f32          0.017   0.008   0.002   0.0004
           f16  -> f32          0.042   0.020   0.003   0.0004
An f32 output has no 16-bit rounding to fill the bound with, only the accumulation term, and that term is a worst case (every rounding
of a depth-long chain in one direction) where a random sum's error grows like its square root: on f32 outputs the bound catches what
is structurally wrong (a dropped block or chunk is hundreds of bounds away, below) and the exact family carries the bit-level claims.
"""
import pytest
import torch

import lora_check as lc

DT = {"bf16": torch.bfloat16, "f16": torch.float16}


@pytest.mark.parametrize("kind", ["bf16", "f16"])
@pytest.mark.parametrize("K", [64, 320, 3584, 18944])
def test_down_emulation_is_inside_the_bound_and_exact_on_exact_inputs(kind, K):
    dt = DT[kind]
    M, R = 48, 64
    x, p, scale, _ = lc.down_inputs("random", M, K, R, dt, seed=K)
    v = lc.verdict(lc.emulate_down(x, p, scale), lc.down_reference(x, p, scale))
    print(f"down emulation {kind} K={K}: ratio {v['ratio']:.3f}")
    assert 0.1 < v["ratio"] <= 1.0, v
    x, p, scale, _ = lc.down_inputs("exact", M, K, R, dt, seed=K)
    ref = lc.down_reference(x, p, scale)
    v = lc.verdict(lc.emulate_down(x, p, scale), ref)
    assert v["unequal"] == 0 and v["ratio"] <= 1.0, v
    assert (ref["rounded"] != ref["out"]).double().mean().item() > 0.1, "an exact case in which almost nothing needs rounding sees little"
    x, p, scale, want = lc.down_inputs("gather", M, K, R, dt)
    assert torch.equal(lc.emulate_down(x, p, scale), want)


@pytest.mark.parametrize("kind", ["bf16", "f16"])
@pytest.mark.parametrize("M,chunk", [(7, 32), (129, 64), (1000, 128), (6794, 704)])
def test_wgrad_emulation_is_inside_the_bound_and_exact_on_exact_inputs(kind, M, chunk):
    dt = DT[kind]
    R, K = 32, 64
    n_chunks = -(-M // chunk)
    for gd in (dt, torch.float32):
        u, x, scale, _, _ = lc.wgrad_inputs("random", M, R, K, dt, seed=M)
        v = lc.verdict(lc.emulate_wgrad(u, x, scale, gd, chunk), lc.wgrad_reference(u, x, scale, gd, n_chunks))
        print(f"wgrad emulation {kind} -> {gd} M={M}: ratio {v['ratio']:.3f}")
        assert v["ratio"] <= 1.0 and (v["ratio"] > 0.1 or gd == torch.float32), v
        u, x, scale, _, _ = lc.wgrad_inputs("exact", M, R, K, dt, seed=M)
        v = lc.verdict(lc.emulate_wgrad(u, x, scale, gd, chunk), lc.wgrad_reference(u, x, scale, gd, n_chunks))
        assert v["unequal"] == 0 and v["ratio"] <= 1.0, v
    u, x, scale, want, _ = lc.wgrad_inputs("gather", M, R, K, dt)
    assert torch.equal(lc.emulate_wgrad(u, x, scale, dt, chunk), want)


@pytest.mark.parametrize("kind", ["bf16", "f16"])
def test_mutants_are_rejected(kind):
    """One thing wrong each: structural mutants fail the bound on random inputs AND the bit test on exact ones; the rounding mutants
    (a second rounding, 16-bit slabs) are within a rounding of the truth and are carried by the exact family."""
    dt = DT[kind]
    M, K, R = 48, 320, 64
    for mut, by_bound in (("drop_block", True), ("kstep_twice", True), ("double_round", False)):
        x, p, scale, _ = lc.down_inputs("random", M, K, R, dt, seed=1)
        vr = lc.verdict(lc.emulate_down(x, p, scale, mut), lc.down_reference(x, p, scale))
        x, p, scale, _ = lc.down_inputs("exact", M, K, R, dt, seed=1)
        if mut == "double_round":
            scale = 1.0 / 3.0            # a product with scale that rounds: the second rounding can show
            ve = lc.verdict(lc.emulate_down(x, p, scale, mut), lc.down_reference(x, p, scale))
            honest = lc.verdict(lc.emulate_down(x, p, scale), lc.down_reference(x, p, scale))
            assert ve["unequal"] > honest["unequal"], (mut, ve, honest)
        else:
            ve = lc.verdict(lc.emulate_down(x, p, scale, mut), lc.down_reference(x, p, scale))
            assert ve["unequal"] > 0, (mut, ve)
        assert (vr["ratio"] > 1.0) or not by_bound, (mut, vr)
    M, R, K, chunk = 200, 32, 64, 64
    for mut in ("tail_rows_dropped", "last_chunk_dropped", "slabs16"):
        u, x, scale, _, _ = lc.wgrad_inputs("random", M, R, K, dt, seed=2)
        vr = lc.verdict(lc.emulate_wgrad(u, x, scale, torch.float32, chunk, mut), lc.wgrad_reference(u, x, scale, torch.float32, 4))
        u, x, scale, _, _ = lc.wgrad_inputs("exact", M, R, K, dt, seed=2)
        ve = lc.verdict(lc.emulate_wgrad(u, x, scale, torch.float32, chunk, mut), lc.wgrad_reference(u, x, scale, torch.float32, 4))
        assert vr["ratio"] > 1.0 and ve["unequal"] > 0, (mut, vr, ve)


def test_gather_mismatch_names_the_row_that_was_read():
    dt = torch.bfloat16
    u, x, scale, want, (a, w) = lc.wgrad_inputs("gather", 200, 32, 64, dt)
    bad = lc.emulate_wgrad(torch.roll(u, 1, 0), x, scale, dt, 64)               # every output row reads the token row before its own
    assert not torch.equal(bad, want)
    text = lc.gather_explain(bad, a, w, want)
    assert "outputs differ" in text and "k = " in text


def test_rule_of_a_lora_linear_against_autograd_f64():
    g = torch.Generator().manual_seed(0)
    S, K, N, r, s = 37, 64, 48, 16, 16.0 / 16
    x = torch.randn(S, K, generator=g, dtype=torch.float64, requires_grad=True)
    w = torch.randn(N, K, generator=g, dtype=torch.float64, requires_grad=True)
    bias = torch.randn(N, generator=g, dtype=torch.float64)
    a = torch.randn(r, K, generator=g, dtype=torch.float64, requires_grad=True)
    b = torch.randn(N, r, generator=g, dtype=torch.float64, requires_grad=True)
    dy = torch.randn(S, N, generator=g, dtype=torch.float64)
    y = torch.nn.functional.linear(x, w, bias) + s * torch.nn.functional.linear(torch.nn.functional.linear(x, a), b)
    assert torch.allclose(lc.lora_linear_f64(x.detach(), w.detach(), bias, a.detach(), b.detach(), s), y.detach(), rtol=1e-13, atol=1e-13)
    y.backward(dy)
    got = lc.lora_linear_grads_f64(x.detach(), w.detach(), a.detach(), b.detach(), s, dy)
    for name, t in (("dx", x), ("dA", a), ("dB", b)):
        assert torch.allclose(got[name], t.grad, rtol=1e-12, atol=1e-12), name
    # B = 0 (peft's init): the adapter changes neither y nor dx, and dA is exactly zero
    z = torch.zeros_like(b.detach())
    assert torch.equal(lc.lora_linear_f64(x.detach(), w.detach(), bias, a.detach(), z, s), (x.detach() @ w.detach().T + bias))
    g0 = lc.lora_linear_grads_f64(x.detach(), w.detach(), a.detach(), z, s, dy)
    assert torch.equal(g0["dA"], torch.zeros_like(a.detach())) and torch.equal(g0["dx"], dy @ w.detach())


@pytest.mark.parametrize("kind", ["bf16", "f16"])
def test_merge_rule_against_f64(kind):
    """W' = round(W + round(s B A)): equal to applying W' for every input (to the two roundings), inside merge_bound of the unrounded
    sum, and the identity for B = 0."""
    dt = DT[kind]
    g = torch.Generator().manual_seed(3)
    N, K, r, s = 96, 128, 16, 16.0 / 16
    w = (torch.randn(N, K, generator=g) * 0.05).to(dt)
    a = (torch.randn(r, K, generator=g) * 0.05).to(dt)
    b = (torch.randn(N, r, generator=g) * 0.05).to(dt)
    m = lc.merge_f64(w, a, b, s)
    assert torch.equal(m.to(dt).double(), m)                                  # 16-bit numbers
    exact = w.double() + s * (b.double() @ a.double())
    assert bool(((m - exact).abs() <= lc.merge_bound(w, a, b, s)).all())
    assert ((m - exact).abs() / lc.merge_bound(w, a, b, s)).max().item() > 0.2, "the merge bound is far from the rule's own roundings"
    assert torch.equal(lc.merge_f64(w, a, torch.zeros_like(b), s), w.double())
    # the f32 accumulation the device uses stays inside the bound as well
    dev = (w.float() + ((s * b.float()).to(dt).float() @ a.float()).to(dt).float()).to(dt).double()
    assert bool(((dev - exact).abs() <= lc.merge_bound(w, a, b, s)).all())


def test_stacked_and_per_module_forms_convert_exactly_both_ways():
    """q | k | v and gate | up are fused rows in the training layouts: A's rows concatenated, B block-diagonal.  Stacking and unstacking
    are exact, the off-diagonal blocks are identically zero, the stacked adapter computes what the per-module adapters compute, and a
    stacked B with anything outside its blocks is refused."""
    from v3d import train
    from v3d._native import V3DError
    g = torch.Generator().manual_seed(4)
    K, r, rows = 64, 16, (48, 16, 16)
    a_list = [torch.randn(r, K, generator=g).to(torch.bfloat16) for _ in rows]
    b_list = [torch.randn(n, r, generator=g).to(torch.bfloat16) for n in rows]
    A, B, blocks = train.lora_stack(a_list, b_list)
    assert A.shape == (3 * r, K) and B.shape == (sum(rows), 3 * r) and blocks == [(0, 48, 0, 16), (48, 64, 16, 32), (64, 80, 32, 48)]
    mask = torch.zeros(B.shape, dtype=torch.bool)
    for r0, r1, c0, c1 in blocks:
        mask[r0:r1, c0:c1] = True
    assert bool((B[~mask] == 0).all()) and int(mask.sum()) == sum(rows) * r
    a2, b2 = train.lora_unstack(A, B, blocks)
    assert all(torch.equal(x, y) for x, y in zip(a_list + b_list, a2 + b2))
    x = torch.randn(5, K, generator=g, dtype=torch.float64)
    fused = (x @ A.double().T) @ B.double().T
    per_module = torch.cat([(x @ a.double().T) @ b.double().T for a, b in zip(a_list, b_list)], 1)
    assert torch.equal(fused, per_module)           # the zero blocks add exact zeros
    B[0, 20] = 1
    with pytest.raises(V3DError, match="off-diagonal"):
        train.lora_unstack(A, B, blocks)


def test_adapter_directory_round_trip_and_key_forms(tmp_path):
    """save_lora -> load_lora is exact; the `.lora_A.<adapter name>.weight` form the drivers' adapter_name="lora" produces and the
    prefixes peft adds are read alike (builder.py:104-106); a key outside the decoder's seven linears is refused."""
    import json
    import os

    from v3d import loader as L
    from v3d._native import V3DError
    g = torch.Generator().manual_seed(5)
    adapters = {(i, m): (torch.randn(16, 32, generator=g).to(torch.bfloat16), torch.randn(24, 16, generator=g).to(torch.bfloat16))
                for i in range(2) for m in L.LORA_TARGETS}
    extra = {"base_model.model.model.mm_projector.0.weight": torch.randn(4, 4, generator=g), "model.image_newline": torch.randn(4, generator=g)}
    d = str(tmp_path / "a")
    L.save_lora(d, adapters, extra, r=16, lora_alpha=16)
    assert sorted(os.listdir(d)) == ["adapter_config.json", "adapter_model.bin", "non_lora_trainables.bin"]
    lora = L.load_lora(d)
    assert lora["r"] == 16 and lora["scaling"] == 1.0 and sorted(lora["adapters"]) == sorted(adapters)
    assert all(torch.equal(lora["adapters"][k][0], adapters[k][0]) and torch.equal(lora["adapters"][k][1], adapters[k][1]) for k in adapters)
    assert sorted(lora["non_lora"]) == ["model.image_newline", "model.mm_projector.0.weight"]
    assert torch.equal(lora["non_lora"]["model.mm_projector.0.weight"], extra["base_model.model.model.mm_projector.0.weight"])
    named = {L.lora_key(i, m, w, adapter_name="lora"): t for (i, m), ab in adapters.items() for w, t in zip("AB", ab)}
    assert "base_model.model.model.layers.1.mlp.down_proj.lora_B.lora.weight" in named
    torch.save(named, os.path.join(d, "adapter_model.bin"))
    again = L.load_lora(d)
    assert all(torch.equal(again["adapters"][k][0], adapters[k][0]) and torch.equal(again["adapters"][k][1], adapters[k][1]) for k in adapters)
    assert L.strip_peft_prefix("base_model.model.model.layers.0.x") == "model.layers.0.x" and L.strip_peft_prefix("lm_head.weight") == "lm_head.weight"
    named["base_model.model.lm_head.lora_A.weight"] = torch.zeros(16, 32)
    torch.save(named, os.path.join(d, "adapter_model.bin"))
    with pytest.raises(V3DError, match="lm_head"):
        L.load_lora(d)
    cfg = json.load(open(os.path.join(d, "adapter_config.json")))
    assert cfg["lora_dropout"] == 0.0 and cfg["bias"] == "none" and cfg["peft_type"] == "LORA"
