#!/usr/bin/env python3
"""Same-call timing of the learned MLP position encoding's path at full size (V = 32 frames, 729 -> 196 tokens, C = 3584, bf16) beside
the shipped kernel:

  v3d_visual_tokens        the shipped `avg-discrete-sin3d` fused kernel (ids + table), re-measured here
  v3d_pe_mlp_hidden        Linear(3, 512) + LayerNorm + ReLU on the 6272 token coordinates
  PE GEMM                  v3d_gemm 6272 x 3584 x 512 with the bias epilogue -> the PE rows
  v3d_visual_tokens_rows   the fused kernel reading those rows
  the mlp path             the three launches back to back, as Engine.build_inputs_embeds issues them

Every variant is launched once per round, the rounds alternate the variants, each launch sits between two device events; the figure is
the median over the rounds and the spread is the 10th..90th percentile.  Ratios are to the shipped kernel, same call.

Usage: python tools/time_pe_mlp.py [--rounds 50] [--warmup 5] [--out profiles/pe_mlp.txt]"""
import argparse
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "video-3d-llm_amd"), os.path.join(ROOT, "tools")]
from time_pe_points import report, timed_rounds          # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--frames", type=int, default=32)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "pe_mlp.txt"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("time_pe_mlp.py measures on the GPU; there is none here")
    from v3d import ops
    V, C, Hh, dt = a.frames, 3584, ops.PE_MLP_HIDDEN, torch.bfloat16
    g = torch.Generator().manual_seed(5)
    feat = torch.randn((V, 729, C), generator=g).to(dt).cuda()
    newline = torch.randn(C, generator=g).to(dt).cuda()
    coords = ((torch.rand((V, 384, 384, 3), generator=g) - 0.5) * torch.tensor([30.0, 30.0, 10.0])).to(dt).cuda()
    out = torch.empty((V * 210, C), dtype=dt, device="cuda")
    p = {"w0": torch.randn((Hh, 3), generator=g) * 3 ** -0.5, "b0": torch.randn(Hh, generator=g) * 0.3, "ln_w": 1 + 0.1 * torch.randn(Hh, generator=g),
         "ln_b": 0.1 * torch.randn(Hh, generator=g), "w3": torch.randn((C, Hh), generator=g) * Hh ** -0.5, "b3": torch.randn(C, generator=g) * 0.1}
    p = {k: v.to(dt).cuda() for k, v in p.items()}
    _, vox, ids = ops.coord_pool_voxel(coords, want_avg=False)
    table = ops.Sin3DTable(C, 301, dt, "cuda")
    N = V * 196
    h = ops.pe_mlp_hidden(vox, p["w0"], p["b0"], p["ln_w"], p["ln_b"], 1e-5)
    pe = torch.empty((N, C), dtype=dt, device="cuda")
    ops.gemm(h, p["w3"], bias=p["b3"], epilogue=ops.EPI_BIAS, out=pe)

    def path():
        hh = ops.pe_mlp_hidden(vox, p["w0"], p["b0"], p["ln_w"], p["ln_b"], 1e-5)
        ops.gemm(hh, p["w3"], bias=p["b3"], epilogue=ops.EPI_BIAS, out=pe)
        ops.visual_tokens_rows(feat, pe, newline, out=out)

    variants = [("v3d_visual_tokens (shipped, table)", lambda: ops.visual_tokens(feat, ids, table, newline, out=out)),
                ("v3d_pe_mlp_hidden", lambda: ops.pe_mlp_hidden(vox, p["w0"], p["b0"], p["ln_w"], p["ln_b"], 1e-5)),
                (f"PE GEMM {N} x {C} x {Hh} + bias", lambda: ops.gemm(h, p["w3"], bias=p["b3"], epilogue=ops.EPI_BIAS, out=pe)),
                ("v3d_visual_tokens_rows", lambda: ops.visual_tokens_rows(feat, pe, newline, out=out)),
                ("the mlp path (three launches)", path)]
    times = timed_rounds(variants, a.rounds, a.warmup)
    fused = (feat.numel() + out.numel()) * 2
    nbytes = {variants[0][0]: fused, variants[1][0]: (N * 3 + N * Hh) * 2, variants[2][0]: (N * Hh + C * Hh + N * C) * 2,
              variants[3][0]: fused + N * C * 2, variants[4][0]: None}
    lines = [f"tools/time_pe_mlp.py: V={V} frames, 729 -> 196 tokens, C={C}, hidden {Hh}, bf16, {a.rounds} alternating rounds after {a.warmup} warm-up rounds",
             f"device: {torch.cuda.get_device_name(0)}", ""]
    report(f"GB/s over each launch's algorithmic traffic (fused kernels: feat + out = {fused / 1e6:.0f} MB, the rows form + {N * C * 2 / 1e6:.0f} MB of PE rows); "
           f"the hidden launch includes its output allocation", times, nbytes, lines)
    med = {n: t[len(t) // 2] * 1e3 for n, t in times.items()}
    parts = med[variants[1][0]] + med[variants[2][0]] + med[variants[3][0]]
    flops = 2.0 * N * C * Hh
    lines += [f"sum of the three launches' medians: {parts:.1f} us = {parts / med[variants[0][0]]:.2f} x the shipped kernel's {med[variants[0][0]]:.1f} us "
              f"(back to back: {med[variants[4][0]]:.1f} us)",
              f"shares of that sum: hidden {med[variants[1][0]] / parts:.0%}, GEMM {med[variants[2][0]] / parts:.0%} "
              f"({flops / (med[variants[2][0]] * 1e-6) / 1e12:.0f} TFLOP/s), fused rows kernel {med[variants[3][0]] / parts:.0%}", ""]
    text = "\n".join(lines)
    print(text)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
