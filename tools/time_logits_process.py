"""What the logits processors cost, in one process on one MI355X, alternating in blocks:

  1. v3d_logits_process_rows (repetition_penalty 1.3, no_repeat_ngram_size 3, min_new_tokens above the history, one EOS id: all three on)
     against v3d_argmax_rows on the same 32 bf16 rows at the model's vocabulary (V = 152064), for histories of 16 and of 512 tokens drawn
     from 2000 ids (so n-grams recur); us per call and its ratio to argmax.  The launch works in place, so the rows it is timed on are the
     rows it has already processed: the addresses and the work are those of a first call.
  2. Engine.answer_group at 32 questions behind the bench scene's prompt at the 7B widths, with the three controls against without: ms per
     decode step of the group as (time of 17 new tokens - time of 1) / 16.

    timeout -k 10 900 python tools/time_logits_process.py > profiles/logits_process.txt"""
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
V, M, CALLS, ROUNDS = 152064, 32, 40, 5
CONTROLS = dict(repetition_penalty=1.3, no_repeat_ngram_size=3, min_new_tokens=600)


def _block(fn, n):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for i in range(n):
        fn(i)
    b.record()
    return a, b


def kernels():
    g = torch.Generator().manual_seed(3)
    x = (torch.randn(M, V, generator=g) * 2.5).to(dt).to(dev)
    out = torch.zeros(M, dtype=torch.int64, device=dev)
    amax_ws = torch.empty(256 * M, dtype=torch.float32, device=dev)
    hist = torch.randint(0, 2000, (512, M), generator=g).to(dev)
    eos = torch.tensor([151645], dtype=torch.int64, device=dev)
    runs = {"argmax": lambda i: ops.argmax_rows(x, out, amax_ws)}
    for L in (16, 512):
        runs[f"process L={L}"] = (lambda i, L=L: ops.logits_process_rows(x, hist, L, eos_ids=eos, **CONTROLS))
    for fn in runs.values():
        fn(0)                                              # warm-up
    spans = {name: [] for name in runs}
    for _ in range(ROUNDS):
        for name, fn in runs.items():
            spans[name].append(_block(fn, CALLS))
    torch.cuda.synchronize()
    us = {name: 1e3 * min(a.elapsed_time(b) for a, b in v) / CALLS for name, v in spans.items()}
    print(f"v3d_logits_process_rows against v3d_argmax_rows, V = {V}, {M} rows, bf16, penalty 1.3 + 3-gram ban + min-new-tokens (one EOS id), "
          f"{ROUNDS} alternating blocks of {CALLS} back-to-back calls each (us per call)")
    print(f"    v3d_argmax_rows                      : {us['argmax']:8.1f} us")
    for L in (16, 512):
        k = f"process L={L}"
        print(f"    v3d_logits_process_rows, history {L:4d} : {us[k]:8.1f} us   = {us[k] / us['argmax']:6.2f} x argmax")
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
    off = dict(eos_token_id=151645)                        # both runs carry the device stop test; random weights never emit the id
    on = dict(off, repetition_penalty=1.3, no_repeat_ngram_size=3, min_new_tokens=17)

    def run(n_new, **kw):
        if "min_new_tokens" in kw:
            kw = dict(kw, min_new_tokens=min(kw["min_new_tokens"], n_new))
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        eng.answer_group(questions, max_new_tokens=n_new, **kw)
        torch.cuda.synchronize()
        return 1e3 * (time.perf_counter() - t0)

    for kw in (off, on):
        run(17, **kw)
        run(1, **kw)
    t = {k: [] for k in ("g17", "g1", "p17", "p1")}
    for _ in range(4):
        t["g17"].append(run(17, **off)); t["p17"].append(run(17, **on)); t["g1"].append(run(1, **off)); t["p1"].append(run(1, **on))
    best = {k: min(v) for k, v in t.items()}
    plain, processed = (best["g17"] - best["g1"]) / 16, (best["p17"] - best["p1"]) / 16
    print(f"Engine.answer_group, 32 questions behind the bench scene's prefix (P = {P}), 7B widths, bf16, greedy; best of 4, alternating")
    print(f"  controls off : 17 new tokens {best['g17']:8.2f} ms, 1 new token {best['g1']:8.2f} ms -> {plain:6.3f} ms per 32-row decode step")
    print(f"  controls on  : 17 new tokens {best['p17']:8.2f} ms, 1 new token {best['p1']:8.2f} ms -> {processed:6.3f} ms per 32-row decode step   "
          f"ratio {processed / plain:.3f}")
    return plain


def main():
    us = kernels()
    step = group()
    print("share of the 32-row decode step (controls off, measured above):")
    print(f"  v3d_argmax_rows, 32 rows                   : {100 * us['argmax'] / (1e3 * step):5.2f} %")
    for L in (16, 512):
        print(f"  v3d_logits_process_rows, history {L:4d}      : {100 * us[f'process L={L}'] / (1e3 * step):5.2f} %")


if __name__ == "__main__":
    with torch.no_grad():
        main()
