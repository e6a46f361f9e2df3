"""The four LLM linears of the 7B decoder with bf16 / e4m3 / MXFP4 weights, same process, the three forms alternating round by round
   (so that clock and neighbour drift hit all three alike): the prefill GEMMs at M = 6794 (v3d_gemm / v3d_gemm_fp8 / v3d_gemm_mxfp4)
   and the 32-row decode linears (v3d_linear_decode_rows / _fp8_rows / _mxfp4_rows).  Per form: median over the rounds of the time per
   launch (each round = `inner` launches between two device events), min..max, and the ratios to bf16 and to e4m3.
       python tools/time_gemm_fp4.py [--rounds 7] [--out profiles/NAME.txt]
   Recorded, not gated: profiles/fp4_linears.txt holds the unedited output of one run on one MI355X (the runtime reports that card as
   "AMD Radeon Graphics"); DESIGN.md section 2 quotes it."""
import argparse
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "video-3d-llm_amd"))
from v3d import ops  # noqa: E402

S, ROWS = 6794, 32
DT = torch.bfloat16
SHAPES = [("gate_up+swiglu", 37888, 3584, "swiglu"), ("down+res", 3584, 18944, "res"), ("qkv+bias", 4608, 3584, "bias"), ("o+res", 3584, 3584, "res")]
PRE = {"swiglu": ops.EPI_SWIGLU, "res": ops.EPI_RES, "bias": ops.EPI_BIAS}
DEC = {"swiglu": ops.DEC_SWIGLU, "res": ops.DEC_RES, "bias": ops.DEC_BIAS}


def time_alternating(forms, rounds, inner, lines, label):
    """forms: {name: fn}.  One round = every form once, `inner` launches each, in rotating order."""
    names = list(forms)
    for fn in forms.values():
        for _ in range(3):
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
        lines.append(f"{label:34s} {n:5s} {med[n]:9.1f} us  (min {min(us[n]):8.1f}  max {max(us[n]):8.1f})   x bf16 {med[n] / med['bf16']:.3f}   x fp8 {med[n] / med['fp8']:.3f}")
        print(lines[-1], flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    torch.manual_seed(0)
    lines = [f"# {torch.cuda.get_device_name(0)}; M = {S} prefill, {ROWS}-row decode; bf16 activations; {a.rounds} alternating rounds, median us per launch"]
    print(lines[0], flush=True)
    for name, N, K, epi in SHAPES:
        w = torch.randn(N, K, device="cuda", dtype=DT) * K ** -0.5
        if epi == "swiglu":
            w = ops.interleave_gate_up(w[: N // 2].contiguous(), w[N // 2:].contiguous())
        w8, s8 = ops.quantize_fp8_rows(w)
        w4, e4 = ops.quantize_mxfp4_rows(w)
        n_out = N // 2 if epi == "swiglu" else N
        bias = torch.randn(N, device="cuda", dtype=DT) if epi == "bias" else None
        for M, table, inner in ((S, PRE, 10), (ROWS, DEC, 50)):
            x = torch.randn(M, K, device="cuda", dtype=DT)
            res = torch.randn(M, N, device="cuda", dtype=DT) if epi == "res" else None
            out = torch.empty(M, n_out, device="cuda", dtype=DT)
            kw = dict(bias=bias, res=res, epilogue=table[epi])
            if M == S:
                qa, sa = ops.quantize_fp8_rows(x)
                forms = {"bf16": lambda: ops.gemm(x, w, out=out, **kw),
                         "fp8": lambda: ops.gemm_fp8(qa, sa, w8, s8, DT, out=out, **kw),
                         "fp4": lambda: ops.gemm_mxfp4(qa, sa, w4, e4, DT, out=out, **kw)}
            else:
                forms = {"bf16": lambda: ops.linear_decode_rows(x, w, out, **kw),
                         "fp8": lambda: ops.linear_decode_fp8_rows(x, w8, s8, out, **kw),
                         "fp4": lambda: ops.linear_decode_mxfp4_rows(x, w4, e4, out, **kw)}
            time_alternating(forms, a.rounds, inner, lines, f"{name} M={M} N={N} K={K}")
        del w, w8, s8, w4, e4
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
