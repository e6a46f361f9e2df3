"""What the device sampler costs beside v3d_argmax_rows, in one process on one MI355X, alternating in blocks:

  1. v3d_sample_rows against v3d_argmax_rows on the same bf16 logits at the model's vocabulary (V = 152064), M = 1 and M = 32 rows, for
     temperature alone (1.0, 0, 1.0: no threshold pass, every token gets a key) and for (0.7, 50, 0.9) (both bisections, few keys);
     us per call, its ratio to argmax, and the threshold / draw + merge split of the sampler (the draw timed alone through top_k = 0,
     top_p = 1).
  2. Engine.answer_group at 32 questions behind the bench scene's prompt at the 7B widths, sampled (0.7, 50, 0.9) against greedy: ms per
     decode step of the group as (time of 17 new tokens - time of 1) / 16, and the sampler's and argmax's share of that step.

    timeout -k 10 900 python tools/time_sampling.py > profiles/sampling.txt"""
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "video-3d-llm_amd"))
import bench  # noqa: E402
from v3d import ops  # noqa: E402
from v3d.engine import Engine, EngineConfig, random_state_dict  # noqa: E402

dt, dev = torch.bfloat16, torch.device("cuda:0")
V, CALLS, ROUNDS = 152064, 40, 5
SETTINGS = [("temperature only (1.0, 0, 1.0)", (1.0, 0, 1.0)), ("(0.7, 50, 0.9)", (0.7, 50, 0.9)), ("(0.7, 50, 1.0)", (0.7, 50, 1.0)),
            ("(1.0, 0, 0.9)", (1.0, 0, 0.9))]


def _block(fn, n):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for i in range(n):
        fn(i)
    b.record()
    return a, b


def kernels():
    g = torch.Generator().manual_seed(3)
    x = (torch.randn(32, V, generator=g) * 2.5).to(dt).to(dev)
    out = torch.zeros(32, dtype=torch.int64, device=dev)
    amax_ws = torch.empty(256 * 32, dtype=torch.float32, device=dev)
    ws = ops.sample_workspace(32, V, dev)
    print(f"v3d_sample_rows against v3d_argmax_rows, V = {V}, bf16, {ROUNDS} alternating blocks of {CALLS} back-to-back calls each (us per call)")
    for M in (1, 32):
        xm = x[:M]
        runs = {"argmax": lambda i: ops.argmax_rows(xm, out[:M], amax_ws)}
        for name, (T, k, p) in SETTINGS:
            runs[name] = (lambda i, T=T, k=k, p=p: ops.sample_rows(xm, out[:M], ws, T, k, p, 1, i))
        for fn in runs.values():
            fn(0)                                              # warm-up
        spans = {name: [] for name in runs}
        for _ in range(ROUNDS):
            for name, fn in runs.items():
                spans[name].append(_block(fn, CALLS))
        torch.cuda.synchronize()
        us = {name: 1e3 * min(a.elapsed_time(b) for a, b in v) / CALLS for name, v in spans.items()}
        print(f"  M = {M}")
        print(f"    v3d_argmax_rows                               : {us['argmax']:8.1f} us")
        draw = us[SETTINGS[0][0]]
        for name, _ in SETTINGS:
            extra = "" if name == SETTINGS[0][0] else f"   (threshold pass about {us[name] - draw:7.1f} us: the rest is at most the temperature-only draw)"
            print(f"    v3d_sample_rows {name:30s}: {us[name]:8.1f} us   = {us[name] / us['argmax']:6.2f} x argmax{extra}")
    return us


def group():
    cfg = EngineConfig()
    eng = Engine(cfg, random_state_dict(cfg, dt, dev, seed=0), dtype=dt, device=dev, max_frames=bench.FRAMES)
    inp = bench.synth_inputs(dev, dt, seed=1000)
    images, coords = ops.preprocess_rgb(inp["frames"], dt), ops.unproject_sampled(inp["depth"], inp["K"], inp["P"], 384, dt)
    ids = inp["input_ids"].cpu()
    at = int((ids == -200).nonzero()[0])
    P = eng.prefill_scene(ids[: at + 1], images, coords)
    g = torch.Generator().manual_seed(5)
    questions = [torch.randint(0, 150000, (int(n),), generator=g) for n in torch.randint(12, 28, (32,), generator=g)]
    draw = dict(do_sample=True, temperature=0.7, top_k=50, top_p=0.9, seed=1)

    def run(n_new, **kw):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        eng.answer_group(questions, max_new_tokens=n_new, **kw)
        torch.cuda.synchronize()
        return 1e3 * (time.perf_counter() - t0)

    for kw in ({}, draw):
        run(17, **kw)
        run(1, **kw)
    t = {k: [] for k in ("g17", "g1", "s17", "s1")}
    for _ in range(4):
        t["g17"].append(run(17)); t["s17"].append(run(17, **draw)); t["g1"].append(run(1)); t["s1"].append(run(1, **draw))
    best = {k: min(v) for k, v in t.items()}
    greedy, sampled = (best["g17"] - best["g1"]) / 16, (best["s17"] - best["s1"]) / 16
    print(f"Engine.answer_group, 32 questions behind the bench scene's prefix (P = {P}), 7B widths, bf16; best of 4, alternating")
    print(f"  greedy  : 17 new tokens {best['g17']:8.2f} ms, 1 new token {best['g1']:8.2f} ms -> {greedy:6.3f} ms per 32-row decode step")
    print(f"  sampled : 17 new tokens {best['s17']:8.2f} ms, 1 new token {best['s1']:8.2f} ms -> {sampled:6.3f} ms per 32-row decode step   "
          f"ratio {sampled / greedy:.3f}")
    return greedy


def main():
    us = kernels()
    step = group()
    print("share of the 32-row decode step (greedy, measured above):")
    print(f"  v3d_argmax_rows, 32 rows                : {100 * us['argmax'] / (1e3 * step):5.2f} %")
    for name, _ in SETTINGS:
        print(f"  v3d_sample_rows {name:24s}: {100 * us[name] / (1e3 * step):5.2f} %")


if __name__ == "__main__":
    with torch.no_grad():
        main()
