"""CPU checks of the beam-search specification and its checker (tests/beam_check.py): BeamRef is what the installed transformers'
generate(num_beams=B, do_sample=False) does, token for token; the host twin v3d_beam_step_host equals BeamRef.step bit for bit over scripted
candidate streams; and eight planted faults in a torch model of the whole loop (top-K, step, K/V gather by parent) are each rejected by
check_topk or by the state comparison - the two rules tests/test_gpu_beam_search.py applies to the engine."""
import itertools

import pytest
import torch

import beam_check as bc
from v3d import ops

PROMPT = torch.tensor([[5, 17, 42, 7, 100, 3, 250]])
NEW = 10


@pytest.fixture(scope="module")
def tiny_lm():
    tf = pytest.importorskip("transformers")
    torch.manual_seed(15)                         # of the seeds tried, one whose greedy tokens are all distinct and whose cases end in all three ways
    cfg = tf.Qwen2Config(vocab_size=300, hidden_size=64, intermediate_size=128, num_hidden_layers=2, num_attention_heads=4, num_key_value_heads=2,
                         max_position_embeddings=128, tie_word_embeddings=False)
    m = tf.Qwen2ForCausalLM(cfg).float().eval()
    with torch.no_grad():
        for p in m.parameters():
            if p.dim() > 1:
                p.mul_(4.0)                        # logits that are not flat
        greedy = m.generate(PROMPT, max_new_tokens=NEW, do_sample=False, num_beams=1, pad_token_id=0)[0, PROMPT.shape[1]:].tolist()
    return m, greedy


def _ref_search(m, B, eos, lp):
    """BeamRef driven by the model's own logits (full forward over [prompt | running sequence], f32)."""
    ref = bc.BeamRef(B, 300, NEW, eos, lp)
    with torch.no_grad():
        while not ref.done:
            if ref.steps == 0:
                ids = PROMPT
            else:
                ids = torch.cat([PROMPT.expand(B, -1), torch.tensor(ref.run_seq)], 1)
            lp32 = torch.log_softmax(m(ids).logits[:, -1].float(), -1)
            ref.step(*bc.BeamRef.topk(lp32, ref.run_score, ref.K))
    return ref


def test_beamref_is_transformers_beam_search(tiny_lm):
    m, greedy = tiny_lm
    seen = dict(eos_early=0, heuristic=0, length=0)
    eos_sets = [(greedy[3],), (greedy[2], greedy[6])]
    for B, lp, eos in itertools.product((1, 2, 4, 5), (1.0, 0.6), eos_sets):
        with torch.no_grad():
            want = m.generate(PROMPT, max_new_tokens=NEW, do_sample=False, num_beams=B, length_penalty=lp, early_stopping=False,
                              eos_token_id=list(eos), pad_token_id=0, num_return_sequences=1)[0, PROMPT.shape[1]:].tolist()
        ref = _ref_search(m, B, eos, lp)
        toks, score, n = ref.result()
        assert toks == want[: len(toks)] and all(t == 0 for t in want[len(toks):]), (B, lp, eos, toks, want)
        seen["eos_early"] += int(n < NEW and toks[-1] in eos)
        seen["heuristic"] += int(ref.steps < NEW)
        seen["length"] += int(ref.steps == NEW)
    assert all(v > 0 for v in seen.values()), seen


# ------------------------------------------------------------------ the host twin


def _drive_twin(B, K, V, L, eos, lp, stream, extra_calls=2):
    """The twin and BeamRef side by side; -> number of compared steps.  After done, further calls must change nothing."""
    ref = bc.BeamRef(B, V, L, eos, lp)
    assert ref.K == K
    words = torch.zeros(int(ops.lib().v3d_beam_state_bytes(B, L)) // 4, dtype=torch.int32)
    words[1] = 1
    f = words.view(torch.float32)
    f[4: 4 + 2 * B] = ops.BEAM_NEG
    f[4] = 0.0                                           # (ops.BeamState's initial words, without its device buffers)
    div = torch.tensor([0.0] + [float(n) ** lp for n in range(1, L + 1)], dtype=torch.float64).to(torch.float32)
    ts, tf_ = torch.zeros((L, K)), torch.zeros((L, K), dtype=torch.int32)
    flags = dict(done_at=None)
    for t, (sc, flat) in enumerate(stream):
        was_done = ref.done
        before = words.clone()
        nxt, par = ops.beam_step_host(words, sc, flat, B, V, L, t, eos, div, ts, tf_)
        ref.step(sc, flat)
        if was_done:
            assert torch.equal(words, before), "a step after done changed the state"
            continue
        got = bc.views_snapshot(ops.beam_state_views(words, B, L))
        assert got == ref.snapshot(), (B, K, t, got, ref.snapshot())
        assert nxt.tolist() == ref.next_tokens.tolist() and par.tolist() == ref.parents.tolist()
        assert torch.equal(ts[t].view(torch.int32), sc.view(torch.int32)) and torch.equal(tf_[t], flat)
        if ref.done and flags["done_at"] is None:
            flags["done_at"] = t
    return ref, flags


@pytest.mark.parametrize("B", [1, 2, 4, 5, 16])
@pytest.mark.parametrize("n_eos", [1, 2])
def test_host_twin_equals_beamref_bit_for_bit(B, n_eos):
    V, L = 23, 12
    eos = (3,) if n_eos == 1 else (3, 11)
    K = bc.beams_to_keep(B, n_eos)                       # 2 B and 3 B
    assert K == (2 if n_eos == 1 else 3) * B
    seen_done_early = 0
    for lp, seed in itertools.product((1.0, 0.6), range(6)):
        plant = bc.PLANTS[seed % 2]
        stream = bc.scripted_stream(B, K, V, L, eos, 100 * B + seed, plant)
        ref, flags = _drive_twin(B, K, V, L, eos, lp, stream)
        assert ref.done
        seen_done_early += int(flags["done_at"] is not None and flags["done_at"] < L - 1)
        if seed % 2 == 0:                                 # the planted cases did what they were planted for
            chk = bc.BeamRef(B, V, L, eos, lp)
            chk.step(*stream[0])
            assert not bool(chk.fin_flag.any())           # step 0: an EOS at rank >= B does not finish
            before = [list(r) for r in chk.run_seq]
            chk.step(*stream[1])
            if B >= 2:                                    # step 1: two hypotheses finish with one score, the earlier candidate first
                assert chk.fin_score[0] == chk.fin_score[1] and chk.fin_len[:2] == [2, 2] and bool(chk.fin_flag[:2].all())
                assert chk.fin_seq[0] == before[0] + [eos[0]] and chk.fin_seq[1] == before[1] + [eos[0]]
            else:                                         # (one beam: nothing was planted at step 1; step 2 has the EOS at rank 0 < B)
                assert not bool(chk.fin_flag.any())
                chk.step(*stream[2])
                assert bool(chk.fin_flag[0]) and chk.fin_len[0] == 3
    assert seen_done_early > 0                            # the "done, then further calls change nothing" branch ran


def test_twin_rejects_bad_shapes():
    from v3d._native import V3DError
    w = torch.zeros(4096, dtype=torch.int32)
    z = lambda k, dt=torch.float32: torch.zeros(k, dtype=dt)      # noqa: E731
    with pytest.raises(V3DError):
        ops.beam_step_host(w, z(34), z(34, torch.int32), 17, 10, 4, 0, (), z(5), z(4 * 34), z(4 * 34, torch.int32))
    with pytest.raises(V3DError):
        ops.beam_step_host(w, z(4), z(4, torch.int32), 2, 10, 4, 4, (), z(5), z(16), z(16, torch.int32))       # step == max_new_tokens
    with pytest.raises(V3DError):
        ops.beam_step_host(w[:8], z(4), z(4, torch.int32), 2, 10, 4, 0, (), z(5), z(16), z(16, torch.int32))   # state too small


# ------------------------------------------------------------------ planted faults in a model of the whole loop


class ToyLoop:
    """Engine.beam_search in torch: 'logits' of a beam are a fixed function of its OWN cache rows (one row per generated token, weighted by
    position, so order and content both matter), rounded to bf16; the rows live in two sets of B slices; step t decodes in set t & 1 after
    the chosen parents' rows were gathered into it.  mutant: one planted fault."""

    D = 16

    def __init__(self, B, V, L, eos, lp, seed, mutant=None):
        g = torch.Generator().manual_seed(seed)
        self.B, self.V, self.L, self.mutant = B, V, L, mutant
        self.emb = torch.randn(V, self.D, generator=g, dtype=torch.float64)
        self.W = torch.randn(V, self.D, generator=g, dtype=torch.float64) * 1.5
        self.W[9] = self.W[7]                               # two tokens with identical logits in every beam: exact ties
        self.bias = torch.zeros(V, dtype=torch.float64)
        self.bias[7] = self.bias[9] = 2.0
        for e in eos:
            self.bias[e] = 2.5
        self.p = torch.randn(self.D, generator=g, dtype=torch.float64)
        self.a = 1.0 / (1.0 + torch.arange(L, dtype=torch.float64))
        step_mut = mutant if mutant in ("eos_any_rank", "running_as_finished", "wrong_n") else None
        self.state = bc.BeamRef(B, V, L, eos, lp, mutant=step_mut)
        self.cache = torch.zeros(2, B, L, self.D, dtype=torch.float64)

    def logits16(self, rows, n):
        """rows [M, L, D] (the first n valid) -> bf16-rounded logits [M, V] as f64"""
        h = torch.tanh(self.p + (rows[:, :n] * self.a[:n, None]).sum(1))
        return (h @ self.W.T + self.bias).to(torch.bfloat16).double()

    def true_logits16(self, seqs):
        rows = torch.zeros(len(seqs), self.L, self.D, dtype=torch.float64)
        for b, s in enumerate(seqs):
            for j, t in enumerate(s):
                rows[b, j] = self.emb[t]
        return self.logits16(rows, len(seqs[0]))

    def run(self):
        """-> per step dict(cand_score, cand_flat, running (before the step), run_seq (before the step), snapshot (after it))"""
        st, B, trace = self.state, self.B, []
        x = self.logits16(self.cache[0, :1], 0)
        for t in range(self.L):
            running = st.run_score.clone()
            seqs = [list(s) for s in st.run_seq]
            lp32 = torch.log_softmax(x.float(), -1)
            add = torch.zeros_like(running) if (self.mutant == "no_running" and t > 0) else running
            dead = running[: x.shape[0]] <= bc.NEG
            cs, cf = bc.BeamRef.topk(lp32.masked_fill(dead[:, None], float("-inf")), add, st.K, reverse_ties=self.mutant == "reverse_ties")
            st.step(cs, cf)
            trace.append(dict(cand_score=cs, cand_flat=cf, running=running, run_seq=seqs, snapshot=st.snapshot()))
            if st.done:
                break
            cur, src = t & 1, (t & 1) ^ 1
            par = st.parents.long()
            if t >= 1 and self.mutant != "gather_skipped":
                n = t - 1 if self.mutant == "newest_not_moved" else t
                for b in range(B):
                    pb = (int(par[b]) + 1) % B if self.mutant == "parent_off_by_one" else int(par[b])
                    self.cache[cur, b, :n] = self.cache[src, pb, :n]
            for b in range(B):
                self.cache[cur, b, t] = self.emb[int(st.next_tokens[b])]
            x = self.logits16(self.cache[cur], t + 1)
        return trace


def check_loop(loop, trace, eos, lp):
    """The two rules of tests/test_gpu_beam_search.py on a ToyLoop run: check_topk against f64 scores of the TRUE model teacher-forced with the
    loop's running sequences, and the loop's state against BeamRef fed with the loop's own candidates.  -> number of exact ties seen."""
    B, V = loop.B, loop.V
    clean = bc.BeamRef(B, V, loop.L, eos, lp)
    ties = 0
    for t, rec in enumerate(trace):
        x = loop.true_logits16(rec["run_seq"][:1] if t == 0 else rec["run_seq"])
        lp64 = torch.log_softmax(x, -1)
        alive = rec["running"][: x.shape[0]] > bc.NEG
        s64 = torch.where(alive[:, None], rec["running"][: x.shape[0], None].double() + lp64, torch.tensor(float("-inf"), dtype=torch.float64))
        e_ref = bc.e_ref_log_softmax(x)
        own = s64.reshape(-1)[rec["cand_flat"].long()]
        bc.check_topk(rec["cand_score"], rec["cand_flat"], s64, bc.kernel_bound(e_ref, own.abs().clamp(max=1e6)), label=f"step {t}")
        ties += int((rec["cand_score"][1:] == rec["cand_score"][:-1]).sum())
        clean.step(rec["cand_score"], rec["cand_flat"])
        assert clean.snapshot() == rec["snapshot"], f"state after step {t} differs from BeamRef on the same candidates"
    return ties


TOY = dict(B=4, V=40, L=8, eos=(3, 5), lp=0.6, seed=3)
MUTANTS = ["parent_off_by_one", "gather_skipped", "newest_not_moved", "no_running", "wrong_n", "eos_any_rank", "running_as_finished", "reverse_ties"]


def test_the_clean_loop_passes_and_has_ties():
    loop = ToyLoop(**TOY)
    trace = loop.run()
    assert len(trace) >= 4
    assert check_loop(loop, trace, TOY["eos"], TOY["lp"]) > 0, "no exact tie among the candidates: the tie rule would go unchecked"


@pytest.mark.parametrize("mutant", MUTANTS)
def test_planted_faults_are_rejected(mutant):
    loop = ToyLoop(**TOY, mutant=mutant)
    trace = loop.run()
    with pytest.raises(AssertionError):
        check_loop(loop, trace, TOY["eos"], TOY["lp"])
