"""Register spills of the hot kernels (hipcc -Rpass-analysis=kernel-resource-usage, device code only, no GPU needed).
Round 2's largest single step (gate/up 1.43 -> 1.35 ms, scene step 111 -> 107 ms) was the removal of accumulator spills that a
rarely executed code path had induced in EVERY tile of the ping-pong GEMM; nothing functional fails when they come back, so the
compiler's own report is held to it here."""
import os
import re
import shutil
import subprocess
from concurrent.futures import ThreadPoolExecutor

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "video-3d-llm_amd", "csrc")
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")


def _report(src, extra=()):
    cmd = [HIPCC, "-O3", "-std=c++17", "--offload-arch=gfx950", *extra, "-I" + os.path.join(ROOT, "include"), "-I" + CSRC, "-S", "--cuda-device-only",
           os.path.join(CSRC, src), "-o", os.devnull, "-Rpass-analysis=kernel-resource-usage"]
    out = subprocess.run(cmd, capture_output=True, text=True, timeout=900)
    assert out.returncode == 0, out.stderr[-2000:]
    spills, name = {}, None
    for line in out.stderr.splitlines():
        m = re.search(r"Function Name: (\S+)", line)
        if m:
            name = m.group(1)
        m = re.search(r"VGPRs Spill: (\d+)", line)
        if m and name:
            spills[name] = int(m.group(1))
    return spills


@pytest.fixture(scope="module")
def reports():
    if not shutil.which(HIPCC):
        pytest.skip("hipcc not available")
    jobs = {"gemm.hip": (), "gemm_fp8.hip": (), "attention.hip": ("-fno-slp-vectorize",), "decode.hip": (), "attention_bwd.hip": ()}
    with ThreadPoolExecutor(max_workers=5) as ex:
        futs = {k: ex.submit(_report, k, v) for k, v in jobs.items()}
        return {k: f.result() for k, f in futs.items()}


def test_gemm_kernels_without_the_split_k_exchange_do_not_spill(reports):
    pp = {k: v for k, v in reports["gemm.hip"].items() if "gemm256pp_kernel" in k}
    assert len(pp) >= 48
    assert all(v == 0 for v in pp.values()), {k: v for k, v in pp.items() if v}      # with and without the split-K exchange (SKT)
    others = {k: v for k, v in reports["gemm.hip"].items() if "gemm256pp_kernel" not in k}
    assert all(v <= 20 for v in others.values()), {k: v for k, v in others.items() if v > 20}      # v3 / 128 x 128 / skinny kernels
    assert all(v == 0 for v in reports["gemm_fp8.hip"].values()), reports["gemm_fp8.hip"]


def _inner_loop_spills(asm_text, kernel_substr):
    """scratch (= spill) instructions inside the first innermost loop (the steady-state tile loop) of the kernels whose mangled name contains kernel_substr, not counting
    those between the `; V3D_RARE_BEGIN` / `; V3D_RARE_END` markers the source puts around its rarely executed blocks."""
    bad, n_kernels = [], 0
    for m in re.finditer(r"^(_ZN3v3d\S*%s\S*):[^\n]*\n(.*?)s_endpgm" % kernel_substr, asm_text, re.S | re.M):
        n_kernels += 1
        lines = m.group(2).split("\n")
        in_loop, rare, seen = False, 0, 0
        for i, ln in enumerate(lines):
            if "Inner Loop Header" in ln:
                seen += 1
                if seen > 1:                 # only the FIRST inner loop is the steady-state tile loop (the second walks the last <= 3 tiles)
                    break
                in_loop = True
                header = re.match(r"^(\.LBB\d+_\d+):", lines[i - 1] if not ln.startswith(".LBB") else ln)
                label = header.group(1) if header else None
            if "V3D_RARE_BEGIN" in ln:
                rare += 1
            if "V3D_RARE_END" in ln:
                rare -= 1
            if in_loop and rare == 0 and re.search(r"\bscratch_(load|store)", ln):
                bad.append((m.group(1)[:60], i, ln.strip()))
            if in_loop and label and re.search(r"s_c?branch\S*\s+%s\b" % re.escape(label), ln):
                in_loop = False
    return n_kernels, bad


def test_attention_and_decode_kernels_do_not_spill_in_their_loops(reports):
    att = reports["attention.hip"]
    # r03: the prefill kernel's rarely taken raise-of-the-maximum block (and code outside the tile loop) may spill; its steady-state
    # tile loop must not - checked on the generated code below.  The totals stay bounded so that a regression is noticed.
    prefill = {k: v for k, v in att.items() if "attn_prefill_kernel" in k or "attn_prefill16_kernel" in k}      # (r04: + the 16x16x32 form)
    assert prefill and all(v <= 24 for v in prefill.values()), prefill
    att = {k: v for k, v in att.items() if k not in prefill}
    assert all(v == 0 for v in reports["attention_bwd.hip"].values()), reports["attention_bwd.hip"]
    assert all(v <= 2 for v in att.values()), att
    assert all(v == 0 for v in reports["decode.hip"].values()), reports["decode.hip"]
    out = subprocess.run([HIPCC, "-O3", "-std=c++17", "--offload-arch=gfx950", "-I" + os.path.join(ROOT, "include"), "-I" + CSRC, "-fno-slp-vectorize",
                          "-Wno-inline-asm", "-S", "--cuda-device-only", os.path.join(CSRC, "attention.hip"), "-o", "-"], capture_output=True, text=True, timeout=900)
    assert out.returncode == 0, out.stderr[-2000:]
    n, bad = _inner_loop_spills(out.stdout, "attn_prefill_kernel")
    assert n >= 14 and not bad, bad[:10]
    n, bad = _inner_loop_spills(out.stdout, "attn_prefill16_kernel")
    assert n >= 8 and not bad, bad[:10]
