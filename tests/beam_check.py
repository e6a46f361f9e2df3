"""Beam search (v3d_beam_topk / v3d_beam_step / v3d_beam_kv_gather, Engine.beam_search) against its specification.  A helper, not a test:
tests/test_beam_check_cpu.py proves that BeamRef is what transformers' generate(num_beams=B) does, that the host twin equals it bit for
bit and that the rules below reject eight planted faults; tests/test_gpu_beam_kernels.py and tests/test_gpu_beam_search.py apply them.

The rule ("Beam search, stated once").  B beams, vocab V, K = max(2, 1 + n_eos) * B candidates per step.  Step t
(n = t + 1 tokens after it): candidate scores = running score + f32 log_softmax of the beam's logits; the K largest of the B * V sums,
descending, EQUAL SCORES IN ASCENDING FLAT ORDER (flat = beam * V + token); a candidate stops on an EOS id or at n = max_new_tokens; the
next running beams are the B largest of (score - 1e9 if stopping); a candidate may enter the finished set with score / float32(n **
length_penalty) only if it stops, ranks below B and the heuristic flag of the previous step is set; finished = the B largest of [old
finished | candidates], the earlier position first among equals; improvable &= any(running[0] / float32(n ** lp) > worst finished (or
-1e9 where the flag is clear)); the search ends when improvable is false or every candidate stopped.  BeamRef states it in torch f32
with the operations of GenerationMixin._beam_search (transformers 5.x); ties by a stable sort.

check_topk.  A returned top-K (scores f32, flats) against f64 scores of ALL B * V candidates passes only if (1) the flats are distinct and
in range, (2) every returned score is within `bound` of the f64 score of its own flat, (3) scores descend and flats ascend among equal
scores, (4) no candidate left out has an f64 score above the smallest returned f64 score + 2 * bound.  For the kernel alone, bound =
4 * e_ref + 2^-22 * |score|, e_ref = max |torch-CPU f32 log_softmax - f64| on the test's inputs (the same arithmetic in another summation
order: the project's 4 x e_ref convention, tests/answer_check.py); for the engine, bound = 2 * e_ref[logits] * max|logit| as the token rule
of answer_check has it.  No bound comes from the code under test."""
import torch

NEG = -1.0e9


def beams_to_keep(B, n_eos):
    return max(2, 1 + n_eos) * B


class BeamRef:
    """The specification.  State as host values: run_seq / fin_seq (lists of token lists), run_score / fin_score (f32 tensors), fin_flag (bool
    tensor), fin_len, improvable, done, steps.  mutant: one of the planted faults of tests/test_beam_check_cpu.py (None = the rule)."""

    def __init__(self, B, V, L, eos=(), length_penalty=1.0, mutant=None):
        self.B, self.V, self.L, self.lp, self.mutant = B, V, L, float(length_penalty), mutant
        self.eos = torch.tensor([int(e) for e in eos], dtype=torch.int64)
        self.K = beams_to_keep(B, len(self.eos))
        self.run_seq = [[] for _ in range(B)]
        self.run_score = torch.full((B,), NEG, dtype=torch.float32)
        self.run_score[0] = 0.0
        self.fin_seq = [[] for _ in range(B)]
        self.fin_score = torch.full((B,), NEG, dtype=torch.float32)
        self.fin_flag = torch.zeros(B, dtype=torch.bool)
        self.fin_len = [0] * B
        self.improvable, self.done, self.steps = True, False, 0
        self.next_tokens = self.parents = None

    @staticmethod
    def topk(logprobs, running, K, reverse_ties=False):
        """logprobs [M, V] (any float type; rounded to f32 first), running f32 [>= M] -> (scores f32 [K], flats int64 [K]): the K largest
        f32 sums, equal ones in ascending flat order (a stable descending sort)."""
        s = (logprobs.to(torch.float32) + running[: logprobs.shape[0], None].to(torch.float32)).reshape(-1)
        if reverse_ties:
            order = (s.numel() - 1) - torch.sort(s.flip(0), descending=True, stable=True).indices
        else:
            order = torch.sort(s, descending=True, stable=True).indices
        return s[order[:K]], order[:K]

    def step(self, cand_score, cand_flat):
        """One step over K candidates (f32 scores, flat indices).  A no-op once done."""
        if self.done:
            return self
        B, V, K = self.B, self.V, self.K
        cs = cand_score.to(torch.float32).clone()
        flat = cand_flat.to(torch.int64)
        assert cs.numel() == K and flat.numel() == K
        n = self.steps + 1
        tok, par = flat % V, flat // V
        stop = torch.isin(tok, self.eos) | torch.tensor(n >= self.L)
        # e. the running beams of the next iteration
        adj = cs + stop.to(torch.float32) * NEG
        order = torch.sort(adj, descending=True, stable=True).indices[:B]
        cont = [self.run_seq[int(par[k])] + [int(tok[k])] for k in range(K)]
        # f. the finished set
        top_b = torch.arange(K) < (K if self.mutant == "eos_any_rank" else B)
        did = stop & top_b
        if self.mutant == "running_as_finished":
            did = top_b.clone()
        d = torch.tensor(float(n + 1 if self.mutant == "wrong_n" else n) ** self.lp, dtype=torch.float32)
        fs = cs / d
        fs = fs + torch.tensor(not self.improvable).to(torch.float32) * NEG
        fs = fs + (~did).to(torch.float32) * NEG
        merged = torch.cat([self.fin_score, fs])
        midx = torch.sort(merged, descending=True, stable=True).indices[:B]
        mseq = self.fin_seq + cont
        mflag = torch.cat([self.fin_flag, did])
        mlen = self.fin_len + [n] * K
        self.fin_seq = [mseq[int(i)] for i in midx]
        self.fin_len = [mlen[int(i)] for i in midx]
        self.fin_score, self.fin_flag = merged[midx], mflag[midx]
        self.run_seq = [cont[int(k)] for k in order]
        self.run_score = adj[order]
        self.next_tokens, self.parents = tok[order], par[order].to(torch.int32)
        # g. the heuristic and the end of the loop
        hope = self.run_score[:1] / torch.tensor(float(n) ** self.lp, dtype=torch.float32)
        worst = torch.where(self.fin_flag, self.fin_score.min(), torch.tensor(NEG, dtype=torch.float32))
        self.improvable = self.improvable and bool(torch.any(hope > worst))
        self.steps = n
        self.done = (not self.improvable) or bool(stop.all())
        return self

    def result(self):
        """(tokens of finished entry 0 cut after its first EOS, its score, its length)"""
        seq = self.fin_seq[0][: self.fin_len[0]]
        eos = set(self.eos.tolist())
        for i, t in enumerate(seq):
            if t in eos:
                seq = seq[: i + 1]
                break
        return seq, float(self.fin_score[0]), self.fin_len[0]

    def snapshot(self):
        """Everything comparable, scores as int32 bit patterns."""
        return dict(done=int(self.done), improvable=int(self.improvable), steps=self.steps, run_score=self.run_score.view(torch.int32).tolist(),
                    fin_score=self.fin_score.view(torch.int32).tolist(), fin_flag=self.fin_flag.int().tolist(), fin_len=list(self.fin_len),
                    run_seq=[list(s) for s in self.run_seq], fin_seq=[list(s[:n]) for s, n in zip(self.fin_seq, self.fin_len)])


def views_snapshot(v):
    """ops.beam_state_views(...) in BeamRef.snapshot()'s form."""
    T = v["steps"]
    lens = v["fin_len"].tolist()
    return dict(done=v["done"], improvable=v["improvable"], steps=T, run_score=v["run_score"].view(torch.int32).tolist(),
                fin_score=v["fin_score"].view(torch.int32).tolist(), fin_flag=v["fin_flag"].tolist(), fin_len=lens,
                run_seq=[r[:T].tolist() for r in v["run_seq"]], fin_seq=[r[:n].tolist() for r, n in zip(v["fin_seq"], lens)])


def e_ref_log_softmax(logits):
    """max |torch-CPU f32 log_softmax - f64| over the rows of `logits` (16-bit or f32 values, taken as exact)."""
    x = logits.detach().cpu()
    return (torch.log_softmax(x.float(), -1).double() - torch.log_softmax(x.double(), -1)).abs().max().item()


def kernel_bound(e_ref, score64):
    return 4.0 * e_ref + 2.0 ** -22 * score64.abs()


def check_topk(scores, flats, f64_scores, bound, label=""):
    """scores f32 [K], flats [K]: the returned candidates; f64_scores [B * V] (f64; -inf for candidates that may not be chosen); bound: a
    float or a tensor broadcastable to [K].  Returns the worst |score - f64| seen; raises AssertionError naming every miss."""
    s = scores.detach().cpu().to(torch.float32)
    f = flats.detach().cpu().to(torch.int64)
    ref = f64_scores.detach().cpu().double().reshape(-1)
    N, K = ref.numel(), f.numel()
    miss = []
    if not bool(((f >= 0) & (f < N)).all()):
        raise AssertionError(f"top-K {label}: a flat index is outside [0, {N}): {f.tolist()}")
    if len(set(f.tolist())) != K:
        miss.append(f"flat indices are not distinct: {f.tolist()}")
    own = ref[f]
    b = torch.as_tensor(bound).detach().cpu().double().reshape(-1)
    b = b.expand(K) if b.numel() == 1 else b
    assert b.numel() == K
    err = (s.double() - own).abs()
    if not bool(torch.isfinite(s).all()):
        miss.append("a returned score is not finite")
    elif bool((err > b).any()):
        k = int((err - b).argmax())
        miss.append(f"score {float(s[k])!r} of flat {int(f[k])} (rank {k}) is {err[k].item():.3e} from its f64 score {own[k].item()!r}, bound {b[k].item():.3e}")
    for k in range(1, K):
        if s[k] > s[k - 1]:
            miss.append(f"scores do not descend at rank {k}: {float(s[k - 1])!r} then {float(s[k])!r}")
            break
        if s[k] == s[k - 1] and f[k] <= f[k - 1]:
            miss.append(f"equal scores at ranks {k - 1}, {k} are not in ascending flat order: {int(f[k - 1])}, {int(f[k])}")
            break
    rest = ref.clone()
    rest[f] = float("-inf")
    best_out = rest.max().item()
    floor = own.min().item()
    slack = 2.0 * b.max().item()
    if best_out > floor + slack:
        miss.append(f"candidate {int(rest.argmax())} with f64 score {best_out!r} was left out; the smallest returned has {floor!r} (+ 2 x bound {slack:.3e})")
    assert not miss, f"top-K {label}: " + "; ".join(miss)
    return err.max().item()


def scripted_stream(B, K, V, L, eos, seed, plant):
    """A scripted candidate stream: per step K (score, flat) pairs in the order v3d_beam_topk returns them (scores descend on a coarse grid, so
    equal scores are common; flats ascend among equals).  plant: step -> what to force there."""
    g = torch.Generator().manual_seed(seed)
    steps = []
    base = 0.0
    for t in range(L):
        kind = plant.get(t)
        # strictly descending where something is planted (the planted ranks then survive the ordering below)
        sc = base - torch.cumsum(torch.randint(0 if kind is None else 1, 3, (K,), generator=g).float() * 0.25, 0)
        flat = torch.randperm(B * V, generator=g)[:K].to(torch.int32)
        if kind == "eos_low_rank":                      # an EOS among the first B
            flat[0] = (flat[0] // V) * V + eos[0]
        elif kind == "eos_high_rank":                   # the only EOS at rank >= B: must not finish
            for k in range(K):
                while int(flat[k]) % V in eos:
                    flat[k] = (flat[k] // V) * V + (int(flat[k]) % V + 1) % V
            flat[K - 1] = (flat[K - 1] // V) * V + eos[-1]
        elif kind == "all_top_eos":                     # every candidate of rank < B is an EOS
            for k in range(B):
                flat[k] = (k % B) * V + eos[k % len(eos)]
        elif kind == "equal_finished" and B >= 2:       # two hypotheses finish with one score
            sc[1] = sc[0]
            flat[0], flat[1] = 0 * V + eos[0], 1 * V + eos[0]
        # equal scores in ascending flat order, as the kernel returns them
        key = sorted(range(K), key=lambda k: (-float(sc[k]), int(flat[k])))
        steps.append((sc[key].contiguous(), flat[key].contiguous()))
        base = float(sc[min(B, K) - 1])
    return steps


PLANTS = ({0: "eos_high_rank", 1: "equal_finished", 2: "eos_low_rank", 4: "all_top_eos"}, {1: "all_top_eos", 3: "eos_high_rank"})
