#!/usr/bin/env python3
"""Same-call timing of the position path's variants at full size (V = 32 frames, 729 -> 196 tokens, C = 3584, bf16):

  fused   v3d_visual_tokens (P = 1, the shipped kernel) against v3d_visual_tokens_points at P = 9, 5, 2, with the table and with
          trig on the fly; GB/s over the algorithmic traffic feat + out
  coords  v3d_coord_pool_voxel against v3d_coord_points_voxel for sample9 and minmax; GB/s over the 378 rows of each frame that the
          patches cover (the sample modes read 9 pixels per patch: no rate is given for them)

Every variant is launched once per round, the rounds alternate the variants, each launch sits between two device events; the figure is
the median over the rounds and the spread is the 10th..90th percentile.  Ratios are to the first variant of the group, same call.

Usage: python tools/time_pe_points.py [--rounds 50] [--warmup 5] [--out profiles/pe_points.txt]"""
import argparse
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "video-3d-llm_amd")]


def timed_rounds(variants, rounds, warmup):
    """variants: [(name, fn)] -> {name: sorted list of milliseconds}"""
    for _ in range(warmup):
        for _, fn in variants:
            fn()
    torch.cuda.synchronize()
    ev = {name: [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(rounds)] for name, _ in variants}
    for r in range(rounds):
        for name, fn in variants:
            a, b = ev[name][r]
            a.record()
            fn()
            b.record()
    torch.cuda.synchronize()
    return {name: sorted(a.elapsed_time(b) for a, b in pairs) for name, pairs in ev.items()}


def report(title, times, nbytes, lines):
    lines.append(title)
    lines.append(f"  {'variant':34s} {'median us':>10s} {'p10..p90 us':>17s} {'GB/s':>8s} {'ratio':>7s}")
    base = None
    for name, t in times.items():
        med, lo, hi = t[len(t) // 2], t[len(t) // 10], t[(9 * len(t)) // 10]
        base = base or med
        rate = f"{nbytes[name] / (med * 1e-3) / 1e9:8.0f}" if nbytes.get(name) else f"{'-':>8s}"
        lines.append(f"  {name:34s} {med * 1e3:10.1f} {lo * 1e3:8.1f}..{hi * 1e3:<7.1f} {rate} {med / base:7.2f}")
    lines.append("")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--frames", type=int, default=32)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "pe_points.txt"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("time_pe_points.py measures on the GPU; there is none here")
    from v3d import ops
    V, C, dt = a.frames, 3584, torch.bfloat16
    g = torch.Generator().manual_seed(5)
    feat = torch.randn((V, 729, C), generator=g).to(dt).cuda()
    newline = torch.randn(C, generator=g).to(dt).cuda()
    coords = ((torch.rand((V, 384, 384, 3), generator=g) - 0.5) * torch.tensor([30.0, 30.0, 10.0])).to(dt).cuda()
    out = torch.empty((V * 210, C), dtype=dt, device="cuda")
    lines = [f"tools/time_pe_points.py: V={V} frames, 729 -> 196 tokens, C={C}, bf16, {a.rounds} alternating rounds after {a.warmup} warm-up rounds",
             f"device: {torch.cuda.get_device_name(0)}", ""]

    fused_bytes = (feat.numel() + out.numel()) * 2
    _, _, ids1 = ops.coord_pool_voxel(coords, want_avg=False, want_vox=False)
    table1 = ops.Sin3DTable(C, 301, dt, "cuda")
    variants = [("v3d_visual_tokens P=1 (table)", lambda: ops.visual_tokens(feat, ids1, table1, newline, out=out))]
    keep = []
    for P, mode in ((9, "sample9"), (5, "sample5"), (2, "minmax")):
        pts, _, ids = ops.coord_points_voxel(coords, mode, want_vox=False)
        table = ops.Sin3DTable(C, 301, dt, "cuda", n_points=P)
        dim_t = ops.reference_dim_t(C // (3 * P)).cuda()
        keep.append((pts, ids, table, dim_t))
        variants.append((f"points P={P} table ({len(table.shifts)} copies)",
                         lambda P=P, ids=ids, table=table: ops.visual_tokens_points(feat, ids=ids, table=table, n_points=P, newline=newline, out=out)))
    for (P, _), (pts, ids, table, dim_t) in zip(((9, 0), (5, 0), (2, 0)), keep):
        variants.append((f"points P={P} trig on the fly",
                         lambda P=P, pts=pts, dim_t=dim_t: ops.visual_tokens_points(feat, pts=pts, dim_t=dim_t, n_points=P, newline=newline, out=out)))
    times = timed_rounds(variants, a.rounds, a.warmup)
    report(f"fused visual tokens; GB/s over feat + out = {fused_bytes / 1e6:.0f} MB", times, {n: fused_bytes for n, _ in variants}, lines)

    strip_bytes = V * 378 * 384 * 3 * 2
    variants = [("v3d_coord_pool_voxel (avg)", lambda: ops.coord_pool_voxel(coords, want_avg=False, want_vox=False)),
                ("v3d_coord_points_voxel minmax", lambda: ops.coord_points_voxel(coords, "minmax", want_pts=False, want_vox=False)),
                ("v3d_coord_points_voxel sample9", lambda: ops.coord_points_voxel(coords, "sample9", want_pts=False, want_vox=False))]
    times = timed_rounds(variants, a.rounds, a.warmup)
    report(f"coordinates -> voxel ids (the launch with its output allocation); GB/s over the {strip_bytes / 1e6:.0f} MB of rows the patches cover",
           times, {variants[0][0]: strip_bytes, variants[1][0]: strip_bytes}, lines)

    text = "\n".join(lines)
    print(text)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
