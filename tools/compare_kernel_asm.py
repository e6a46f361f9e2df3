#!/usr/bin/env python3
"""Compare two builds of one .hip file, kernel by kernel, from what the compiler wrote:

    hipcc -S --cuda-device-only -O3 --offload-arch=gfx950 -Rpass-analysis=kernel-resource-usage FILE.hip -o X.s 2> X.rpt
    python tools/compare_kernel_asm.py old.s old.rpt new.s new.rpt

Prints, per kernel family (the name before the template arguments): how many kernels, how many have the identical instruction
stream (local labels .LBB<function>_<block> renumbered by function, comments and directives dropped), and for the others the
VGPR range, spills, scratch, occupancy and instruction counts of both builds.  Exit status 1 when the symbols differ or a kernel
of the new build has more VGPRs, more spills, more scratch or another occupancy than its twin."""
import collections
import re
import sys


def kernels(path):
    """{symbol: [instruction lines]} of the functions an assembly file defines"""
    out, name, body = {}, None, []
    for line in open(path):
        m = re.match(r"^(_Z\w+):", line)
        if m:
            name, body = m.group(1), []
            continue
        if name is None:
            continue
        if line.startswith(".Lfunc_end"):
            out[name], name = body, None
            continue
        t = line.split(";")[0].strip()
        if not t or (t.startswith(".") and not t.startswith(".LBB")):
            continue
        body.append(re.sub(r"\.LBB\d+_", ".LBB_", t))
    return out


def resources(path):
    """{symbol: {field: value}} of a -Rpass-analysis=kernel-resource-usage report"""
    out, cur = {}, None
    for line in open(path):
        m = re.search(r"remark: Function Name: (\S+)", line)
        if m:
            cur = out.setdefault(m.group(1), {})
            continue
        m = re.search(r"remark:\s+([A-Za-z ]+?)(?: \[[^\]]*\])?: (\d+) \[-Rpass", line)
        if m and cur is not None:
            cur[m.group(1)] = int(m.group(2))
    return out


def family(sym):
    m = re.match(r"_ZN3v3d(\d+)", sym)
    return sym[len(m.group(0)):][:int(m.group(1))] if m else sym


def main():
    old_s, old_r, new_s, new_r = sys.argv[1:5]
    ka, kb, ra, rb = kernels(old_s), kernels(new_s), resources(old_r), resources(new_r)
    bad = 0
    if set(ra) != set(rb):
        print("kernel symbols differ:", sorted(set(ra) ^ set(rb)))
        bad = 1
    fams = collections.defaultdict(list)
    for sym in sorted(set(ra) & set(rb)):
        fams[family(sym)].append(sym)
    print(f"{len(ra)} kernel symbols in the old build, {len(rb)} in the new")
    rng = lambda v: f"{min(v)}" if min(v) == max(v) else f"{min(v)}-{max(v)}"
    for fam, syms in fams.items():
        same = [s for s in syms if ka.get(s) == kb.get(s)]
        print(f"{fam}: {len(syms)} kernels, {len(same)} with identical instruction streams")
        for s in syms:
            a, b = ra[s], rb[s]
            worse = (b["VGPRs"] > a["VGPRs"] or b["VGPRs Spill"] > a["VGPRs Spill"] or b["SGPRs Spill"] > a["SGPRs Spill"] or
                     b["ScratchSize"] > a["ScratchSize"] or b["Occupancy"] != a["Occupancy"])
            if worse:
                bad = 1
                print(f"  WORSE {s}: {a} -> {b}")
        diff = [s for s in syms if s not in same]
        if diff:
            f = lambda r, k: rng([r[s][k] for s in diff])
            n = lambda k: rng([len(k[s]) for s in diff])
            print(f"  the {len(diff)} others, old -> new: VGPRs {f(ra, 'VGPRs')} -> {f(rb, 'VGPRs')}, VGPR spills {f(ra, 'VGPRs Spill')} -> "
                  f"{f(rb, 'VGPRs Spill')}, SGPR spills {f(ra, 'SGPRs Spill')} -> {f(rb, 'SGPRs Spill')}, scratch {f(ra, 'ScratchSize')} -> "
                  f"{f(rb, 'ScratchSize')}, occupancy {f(ra, 'Occupancy')} -> {f(rb, 'Occupancy')}, instructions {n(ka)} -> {n(kb)}")
            for s in diff:
                print(f"    {s}: VGPRs {ra[s]['VGPRs']} -> {rb[s]['VGPRs']}, instructions {len(ka[s])} -> {len(kb[s])}")
    return bad


if __name__ == "__main__":
    sys.exit(main())
