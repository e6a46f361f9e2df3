"""v3d_logits_process_rows against tests/logits_check.py's restatement, bit for bit over the whole padded row, for f16 and bf16, on the case
list of logits_check.kernel_cases: V = 1000 of ld 1024 (the pad columns hold a sentinel) and V = 152064; 1, 5 and 32 rows with different
histories at a step stride larger than M; history lengths 0, 1, n-2, n-1, n, 2n, 300 and 1100 (the last two wrap the kernel's 256-thread
loops); an id repeated at positions 3, 3 + 256 and 1030; zero, -inf, positive and negative logits under the penalty; ids outside [0, V);
each control alone and all three together.  The number of changed entries per row is compared as well, and must be positive where the rule
certainly rewrites something: a kernel that writes nothing cannot pass."""
import pytest
import torch

import logits_check as lc
from v3d import ops
from v3d._native import V3DError

pytestmark = pytest.mark.gpu

DTYPES = {"bf16": torch.bfloat16, "f16": torch.float16}
_CASES = {}


def _cases(name):
    """the cases and their expected rows, computed once per dtype and left unchanged"""
    if name not in _CASES:
        _CASES[name] = [(c, *lc.expected(c)) for c in lc.kernel_cases(DTYPES[name])]
    return _CASES[name]


@pytest.mark.parametrize("name", sorted(DTYPES))
def test_kernel_is_the_restatement_bit_for_bit(name):
    seen_change = 0
    for case, want, count in _cases(name):
        x = case["logits"].cuda()
        hist = case["history"].cuda()
        eos = torch.tensor(case["eos"], dtype=torch.int64, device="cuda") if case["eos"] else None
        out = ops.logits_process_rows(x, hist, case["L"], case["p"], case["n"], case["k"], eos, V=case["V"])
        assert out is x
        got = x.cpu()
        diff = lc.bits(got) != lc.bits(want)
        assert not bool(diff.any()), (f"{name} {case['name']}: {int(diff.sum())} entries differ, first at {diff.nonzero()[0].tolist()}: "
                                      f"got {float(got[tuple(diff.nonzero()[0])])} want {float(want[tuple(diff.nonzero()[0])])}")
        changed = (lc.bits(got) != lc.bits(case["logits"])).sum(1)
        assert torch.equal(changed, count), (name, case["name"], changed.tolist(), count.tolist())
        if lc.must_change(case):
            assert int(changed[0]) > 0, f"{name} {case['name']}: nothing was written to row 0"
            seen_change += 1
        assert torch.equal(hist.cpu(), case["history"]), "the history was written"
    assert seen_change >= 30


@pytest.mark.parametrize("name", sorted(DTYPES))
def test_a_repeated_id_is_penalised_once_and_bans_win(name):
    dt = DTYPES[name]
    case = lc.make_case("repeat", dt, 5, 1100, p=1.3)
    x = case["logits"].cuda()
    ops.logits_process_rows(x, case["history"].cuda(), 1100, 1.3, V=case["V"])
    once = (torch.tensor(3.0) / torch.tensor(1.3)).to(dt)
    assert torch.equal(lc.bits(x[:, lc.REPEAT_ID].cpu()), lc.bits(once.expand(5))), x[:, lc.REPEAT_ID].tolist()
    # one row of the engine's own layout: a 1-D history, one row of logits; the ban lands behind the penalty's store to the same entry
    row = torch.full((1, 64), 2.0, dtype=dt, device="cuda")
    hist = torch.tensor([5, 9, 5, 9, 5], dtype=torch.int64, device="cuda")
    ops.logits_process_rows(row[0], hist, 5, 2.0, 2, 6, torch.tensor([63], dtype=torch.int64, device="cuda"))
    want = torch.full((64,), 2.0)
    want[5], want[9], want[63] = 1.0, -float("inf"), -float("inf")
    assert torch.equal(row[0].float().cpu(), want)


def test_refusals():
    x = torch.zeros(2, 32, dtype=torch.bfloat16, device="cuda")
    h = torch.zeros(4, 2, dtype=torch.int64, device="cuda")
    for kw in (dict(repetition_penalty=0.0), dict(repetition_penalty=float("inf")), dict(no_repeat_ngram_size=-2), dict(min_new_tokens=-1)):
        with pytest.raises(V3DError):
            ops.logits_process_rows(x, h, 4, **kw)
    with pytest.raises(V3DError):
        ops.logits_process_rows(x, h, 5)                                       # more steps than the history holds
    with pytest.raises(V3DError):
        ops.logits_process_rows(x, h[:, :1], 4)                                # fewer columns than rows
    with pytest.raises(V3DError):
        ops.logits_process_rows(x.float(), h, 4, 1.3)                          # 16-bit logits only
    with pytest.raises(V3DError, match="LOGITS_MAX_HISTORY"):
        ops.logits_process_rows(x, torch.zeros(ops.LOGITS_MAX_HISTORY + 1, 2, dtype=torch.int64, device="cuda"), ops.LOGITS_MAX_HISTORY + 1, 1.3)
    with pytest.raises(V3DError):
        ops.logits_process_rows(torch.zeros(33, 32, dtype=torch.bfloat16, device="cuda"), torch.zeros(4, 33, dtype=torch.int64, device="cuda"), 4, 1.3)
    # the longest history the engine can hold runs
    big = torch.randint(0, 32, (ops.LOGITS_MAX_HISTORY, 2), dtype=torch.int64)
    x = torch.ones(2, 32, dtype=torch.bfloat16, device="cuda")
    ops.logits_process_rows(x, big.cuda(), ops.LOGITS_MAX_HISTORY, 2.0, 0, 0)
    want = lc.process_rows(torch.ones(2, 32, dtype=torch.bfloat16), big, ops.LOGITS_MAX_HISTORY, 2.0)
    assert torch.equal(lc.bits(x.cpu()), lc.bits(want))
