"""dx and dW of the seven training linears (BASELINE configs[4]: S = 6794 decoder rows, 23 328 SigLIP rows, bf16), the transposing path
   against v3d_gemm_layout, same process, the two forms alternating round by round (clock and neighbour drift hit both alike):
     parent  what linear_backward issues with V3D_TRAIN_GEMM_LAYOUTS unset, on one stream: dx = transpose(w), gemm(dy, w^T);
             dW = train._weight_grads (transposes of dy and x with the token rows padded to 128, gemm; the tower's 1152-wide dW padded
             to 1280 columns for the split-K tail)
     layout  dx = gemm_layout(dy, w, b_kmajor=True); dW = gemm_layout(dy, x, a_kmajor=True, b_kmajor=True) - timed for every shape, also
             where linear_backward keeps the transposing path under the switch (marked `kept`: the tower's dW, which relies on that tail)
   Per product: median over the rounds of the time per call (each round = `inner` calls between two device events), min..max, and
   layout / parent.  Then bench.py's train_config4 measurement in two fresh child processes, switch off and on.
       python tools/time_gemm_layouts.py [--rounds 7] [--no-step] [--out profiles/gemm_layouts.txt]
   Recorded, not gated: profiles/gemm_layouts.txt holds the unedited output of one run on one MI355X; DESIGN.md section 7 quotes it."""
import argparse
import os
import statistics
import subprocess
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "video-3d-llm_amd"))
from v3d import ops, train  # noqa: E402

S, SV = 6794, 23328
DT = torch.bfloat16
# name, out-features N, in-features K, token rows
SHAPES = [("qkv", 4608, 3584, S), ("o", 3584, 3584, S), ("gate_up", 37888, 3584, S), ("down", 3584, 18944, S), ("lm_head", 152064, 3584, S),
          ("siglip_fc1", 4352, 1152, SV), ("siglip_fc2", 1152, 4352, SV)]


def time_alternating(forms, rounds, inner, lines, label, note=""):
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
        lines.append(f"{label:44s} {n:6s} {med[n]:9.1f} us  (min {min(us[n]):8.1f}  max {max(us[n]):8.1f})   x parent {med[n] / med['parent']:.3f} {note if n == 'layout' else ''}")
        print(lines[-1], flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--no-step", action="store_true")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    os.environ.pop("V3D_TRAIN_GEMM_LAYOUTS", None)
    torch.manual_seed(0)
    lines = [f"# {torch.cuda.get_device_name(0)}; bf16; dx [rows, K] = dy . W and dW [N, K] = dy^T . x of a linear W [N, K]; {a.rounds} alternating rounds, median us per product"]
    print(lines[0], flush=True)
    for name, N, K, rows in SHAPES:
        x = torch.randn(rows, K, device="cuda", dtype=DT)
        w = torch.randn(N, K, device="cuda", dtype=DT) * K ** -0.5
        dy = torch.randn(rows, N, device="cuda", dtype=DT)
        inner = 3 if N > 100000 else 6

        def dx_parent():
            return ops.gemm(dy, ops.transpose(w))

        kept_dx = "" if train._layout_fits(dy, w, False, True) else "(kept: the ABI refuses the shape)"
        forms = {"parent": dx_parent}
        if not kept_dx:
            forms["layout"] = lambda: ops.gemm_layout(dy, w, b_kmajor=True)
        time_alternating(forms, a.rounds, inner, lines, f"{name} dx {rows} x {K} x {N} (M N K)", kept_dx)
        Kp = (K + 255) // 256 * 256
        kept = "(kept: split-K tail branch)" if Kp != K and rows >= 8192 and (Kp - K) * 8 <= K else ""
        forms = {"parent": lambda: train._weight_grads(x, dy, True, False)[0],
                 "layout": lambda: ops.gemm_layout(dy, x, a_kmajor=True, b_kmajor=True)}
        time_alternating(forms, a.rounds, inner, lines, f"{name} dW {N} x {K} x {rows} (M N K)", kept)
        del x, w, dy
        torch.cuda.empty_cache()
    if not a.no_step:
        torch.cuda.synchronize()
        torch.cuda.empty_cache()
        for flag in ("0", "1"):
            env = dict(os.environ, V3D_TRAIN_GEMM_LAYOUTS=flag)
            r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "time_train_step.py")], env=env, capture_output=True, text=True, timeout=900)
            last = r.stdout.strip().splitlines()[-1] if r.stdout.strip() else "no output; " + r.stderr.strip()[-300:]
            lines.append(f"train_config4 V3D_TRAIN_GEMM_LAYOUTS={flag} (exit {r.returncode}): {last}")
            print(lines[-1], flush=True)
            if r.returncode != 0:
                break
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
