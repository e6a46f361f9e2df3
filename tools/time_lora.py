"""The LoRA rank products (csrc/lora.hip) against the same products through the routes that existed before them, and the language
   model's training step with and without adapters.  Same process, device events, the forms alternating round by round (clock and
   neighbour drift hit all alike); bf16, S = 6794 decoder rows, r = 64 (train_3d.py:168-173).
     kernel table   v3d_lora_down   u = x A^T at K = 3584 / 18944 and du = s dy B at dy widths 4608 / 3584 / 37888
                                    against v3d_gemm with the rank zero-padded to N = 128
                    v3d_lora_wgrad  dA = du^T x at K = 3584 / 18944 and dB^T = s u^T dy at the three dy widths
                                    against v3d_gemm_layout(1, 1) with the rank zero-padded to 128 rows
                    per product: median us over the rounds (min .. max), the bytes the product has to move (operands once, output
                    once) and that over the time as a fraction of 8 TB/s, and new / existing.
     step           llm_forward_backward + AdamW on --layers decoder layers of the 7B widths (H 3584, I 18944, 28 / 4 heads, V 152064):
                    lora   adapters on the seven linears, every base tensor frozen (optimizer over the adapters only), the rank
                           products on the routes v3d.train dispatches them to by default
                    full   no adapters, every tensor trained: the path as it was
                    gemm   the lora step with every rank product forced onto the existing GEMMs (V3D_LORA_DOWN / _WGRAD = gemm)
                    kernel the lora step with every rank product forced onto the new kernels (= kernel)
                    each in turn (--step-rounds times): one warm-up step, then the median of two timed steps and the peak allocated
                    memory of those steps (the model's own tensors included, the other forms' optimizer states freed).
       python tools/time_lora.py [--rounds 7] [--layers 28] [--no-step] [--out profiles/lora.txt]
   Recorded, not gated: profiles/lora.txt holds the unedited output of one run on one MI355X; DESIGN.md section 7 quotes it."""
import argparse
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "video-3d-llm_amd"))
from v3d import ops, train  # noqa: E402

S, R, DT = 6794, 64, torch.bfloat16
HBM = 8e12


def time_alternating(forms, rounds, inner, lines, label, nbytes):
    names = list(forms)
    for fn in forms.values():
        for _ in range(2):
            fn()
    torch.cuda.synchronize()
    us = {n: [] for n in names}
    for r in range(rounds):
        for n in names[r % len(names):] + names[: r % len(names)]:
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(inner):
                forms[n]()
            e1.record()
            torch.cuda.synchronize()
            us[n].append(e0.elapsed_time(e1) * 1e3 / inner)
    med = {n: statistics.median(v) for n, v in us.items()}
    for n in names:
        lines.append(f"{label:40s} {n:9s} {med[n]:9.1f} us  (min {min(us[n]):8.1f}  max {max(us[n]):8.1f})  {nbytes / 1e6:8.1f} MB  "
                     f"{nbytes / (med[n] * 1e-6) / HBM:6.1%} of 8 TB/s   x existing {med[n] / med['existing']:.3f}")
        print(lines[-1], flush=True)


def kernel_table(rounds, lines):
    mk = lambda *shape, s=1.0: torch.randn(*shape, device="cuda", dtype=DT) * s
    for K in (3584, 18944):
        x, A = mk(S, K), mk(R, K, s=K ** -0.5)
        Ap = torch.zeros(128, K, dtype=DT, device="cuda")
        Ap[:R] = A
        nb = (S * K + R * K + S * R) * 2
        time_alternating({"existing": lambda: ops.gemm(x, Ap), "lora_down": lambda: ops.lora_down(x, A)}, rounds, 6, lines,
                         f"down  u = x A^T      {S} x {K} x {R}", nb)
        du = mk(S, R)
        dup = torch.zeros(S, 128, dtype=DT, device="cuda")
        dup[:, :R] = du
        ws = ops.lora_wgrad_workspace(S, R, K, "cuda")
        nb = (S * R + S * K) * 2 + R * K * 4
        time_alternating({"existing": lambda: ops.gemm_layout(dup, x, a_kmajor=True, b_kmajor=True),
                          "lora_wgrad": lambda: ops.lora_wgrad(du, x, 1.0, workspace=ws)}, rounds, 6, lines,
                         f"wgrad dA = du^T x    {R} x {K} x {S}", nb)
        del x, A, Ap, du, dup, ws
        torch.cuda.empty_cache()
    for N in (4608, 3584, 37888):
        dy, Bt, u = mk(S, N), mk(R, N, s=0.05), mk(S, R)
        Btp = torch.zeros(128, N, dtype=DT, device="cuda")
        Btp[:R] = Bt
        nb = (S * N + R * N + S * R) * 2
        time_alternating({"existing": lambda: ops.gemm(dy, Btp), "lora_down": lambda: ops.lora_down(dy, Bt, 0.25)}, rounds, 4, lines,
                         f"down  du = s dy B    {S} x {N} x {R}", nb)
        up = torch.zeros(S, 128, dtype=DT, device="cuda")
        up[:, :R] = u
        ws = ops.lora_wgrad_workspace(S, R, N, "cuda")
        nb = (S * R + S * N) * 2 + R * N * 4
        time_alternating({"existing": lambda: ops.gemm_layout(up, dy, a_kmajor=True, b_kmajor=True),
                          "lora_wgrad": lambda: ops.lora_wgrad(u, dy, 0.25, workspace=ws)}, rounds, 4, lines,
                         f"wgrad dB^T = s u^T dy {R} x {N} x {S}", nb)
        del dy, Bt, Btp, u, up, ws
        torch.cuda.empty_cache()


def build_model(layers):
    H, I, n_q, n_kv, hd, V = 3584, 18944, 28, 4, 128, 152064
    g = torch.Generator(device="cuda").manual_seed(0)
    mk = lambda *shape, s=1.0: (torch.randn(*shape, generator=g, device="cuda", dtype=torch.float32) * s).to(DT)
    width = (n_q + 2 * n_kv) * hd
    ls = [{"ln1": torch.ones(H, dtype=DT, device="cuda"), "qkv": mk(width, H, s=H ** -0.5), "qkv_bias": mk(width, s=0.02),
           "o": mk(H, n_q * hd, s=(n_q * hd) ** -0.5), "ln2": torch.ones(H, dtype=DT, device="cuda"), "gate_up": mk(2 * I, H, s=H ** -0.5),
           "down": mk(H, I, s=I ** -0.5)} for _ in range(layers)]
    params = {"layers": ls, "norm": torch.ones(H, dtype=DT, device="cuda"), "lm_head": mk(V, H, s=H ** -0.5)}
    x = mk(S, H)
    labels = torch.full((S,), -100, dtype=torch.int64, device="cuda")
    labels[-200:] = torch.randint(0, V, (200,), generator=g, device="cuda")
    rope = train.RopeTables(hd, 8192, 1e6, DT, "cuda")
    return params, x, labels, rope, (n_q, n_kv, hd)


def step_table(layers, rounds, lines):
    params, x, labels, rope, heads = build_model(layers)
    with_lora = {"layers": [dict(p, qkv_rows=(28 * 128, 4 * 128, 4 * 128)) for p in params["layers"]], "norm": params["norm"],
                 "lm_head": params["lm_head"]}                      # shares the base tensors with `params`
    train.lora_init(with_lora, r=R, alpha=16, seed=0)
    g = torch.Generator(device="cuda").manual_seed(1)
    for p in with_lora["layers"]:                                    # away from B = 0: zeros run at another clock than data
        for name, ad in p["lora"].items():
            for r0, r1, c0, c1 in p["lora_state"][name].blocks:
                ad["B"][r0:r1, c0:c1] = (torch.randn(r1 - r0, c1 - c0, generator=g, device="cuda") * 0.02).to(DT)
    train.lora_refresh(with_lora)
    frozen = ("lm_head", "norm", "ln1", "ln2", "qkv_bias")
    env = {"lora": {}, "kernel": {"V3D_LORA_DOWN": "kernel", "V3D_LORA_WGRAD": "kernel"}, "gemm": {"V3D_LORA_DOWN": "gemm", "V3D_LORA_WGRAD": "gemm"}}

    def run(form):
        for k in ("V3D_LORA_DOWN", "V3D_LORA_WGRAD"):
            os.environ.pop(k, None)
        os.environ.update(env.get(form, {}))
        if form == "full":
            opt = train.AdamW(params, lr=1e-6)
            one = lambda: opt.step(params, train.llm_forward_backward(params, x, labels, rope, *heads)[2])
        else:
            tt = train.trainable_tree(with_lora, frozen)
            opt = train.AdamW(tt, lr=1e-6)

            def one():
                opt.step(tt, train.llm_forward_backward(with_lora, x, labels, rope, *heads, frozen=frozen)[2])
                train.lora_refresh(with_lora)
        one()
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        ms = []
        for _ in range(2):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            one()
            e1.record()
            torch.cuda.synchronize()
            ms.append(e0.elapsed_time(e1))
        peak = torch.cuda.max_memory_allocated() / 2 ** 30
        del opt
        torch.cuda.empty_cache()
        return statistics.median(ms), peak
    forms = ["lora", "full", "gemm", "kernel"]
    res = {f: [] for f in forms}
    for r in range(rounds):
        for f in forms[r % 4:] + forms[: r % 4]:
            res[f].append(run(f))
    for f in forms:
        t = [a for a, _ in res[f]]
        lines.append(f"step {layers} layers S {S}  {f:5s} {statistics.median(t):9.1f} ms  (min {min(t):8.1f}  max {max(t):8.1f})   "
                     f"peak allocated {max(b for _, b in res[f]):7.2f} GiB   x full {statistics.median(t) / statistics.median([a for a, _ in res['full']]):.3f}")
        print(lines[-1], flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--step-rounds", type=int, default=2)
    ap.add_argument("--layers", type=int, default=28)
    ap.add_argument("--no-step", action="store_true")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    torch.manual_seed(0)
    lines = [f"# {torch.cuda.get_device_name(0)}; bf16; S = {S}, r = {R}; {a.rounds} alternating rounds, median us per product; "
             "MB = operands once + output once"]
    print(lines[0], flush=True)
    kernel_table(a.rounds, lines)
    if not a.no_step:
        step_table(a.layers, a.step_rounds, lines)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
