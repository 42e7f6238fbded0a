"""A plain restatement of the beam search's bookkeeping -- one step, and the whole search -- over a logits callback
f(sentence, history) -> row [vocab], with no transformer in it.  The rules are those of oracle/text_decoder.py::beam_search (the
fairseq2 defaults); on top of them it states what the device defines beyond them:

  * per-sentence prompts and caps: sentence s has its own prompt, max_len_s = min(plen_s + gen_cap, model_max) and
    min_len_s = min(plen_s + min_gen, max_len_s);
  * the order of equal candidates: score descending, then row ascending, then token ascending;
  * the decision margins: the smallest gap between neighbours of a free step's sorted candidate list (its first 2 * beam entries)
    from the best one to the first candidate the rules do not consume, and best minus second finished score;
  * -inf is never a candidate: a sentence with fewer finite candidates than `beam` continues with fewer rows.

Everything is a flat, sorted candidate list; arithmetic is float64 unless `dtype` says otherwise (float32 reproduces the oracle's
bits).  Also here: the synthetic logits of the kernel tests (a hash of sentence and history) and the gap condition on them."""
from __future__ import annotations

import math
from dataclasses import dataclass, field
from typing import Callable, List, Optional, Sequence, Tuple

import numpy as np
import torch

NEG_INF = -math.inf


@dataclass(frozen=True)
class BeamParams:
    beam: int
    pad_idx: int = 0
    unk_idx: int = 1
    eos_idx: int = 3
    temperature: float = 1.0
    unk_penalty: float = 0.0
    len_penalty: float = 1.0
    normalize: bool = True


@dataclass(frozen=True)
class Plan:
    """One sentence's prompt and length limits."""
    prompt: Tuple[int, ...]
    gen_cap: int
    min_gen: int = 1
    model_max: int = 1 << 30

    @property
    def plen(self) -> int:
        return len(self.prompt)

    @property
    def max_len(self) -> int:
        return min(self.plen + self.gen_cap, self.model_max)

    @property
    def min_len(self) -> int:
        return min(self.plen + self.min_gen, self.max_len)

    def mode(self, step_nr: int) -> str:
        """what the sentence does at the step that chooses token step_nr: 'prompt', 'eos' (forced), 'free' or 'past'"""
        if step_nr < self.plen:
            return "prompt"
        if step_nr == self.max_len - 1:
            return "eos"
        return "free" if step_nr < self.max_len - 1 else "past"


@dataclass
class Row:
    hist: List[int]
    cum: float


@dataclass
class Gap:
    """two neighbours of a sorted list whose order decides something"""
    gap: float
    by_construction: bool  # a gap of exactly 0 between candidates of identical cum bits and identical logits rows
    where: str


@dataclass
class StepOut:
    kind: str                                                      # 'prompt', 'eos' or 'free'
    lists: List[Tuple[List[float], List[int]]] = field(default_factory=list)   # free: per live row, its best 2 * beam (value, token)
    row_max: List[float] = field(default_factory=list)            # per live row: maximum of the scaled row
    lse: List[float] = field(default_factory=list)                # per live row: log-sum-exp of the scaled row
    ranked: List[Tuple[float, int, int]] = field(default_factory=list)   # the sorted candidates (score, row, token), first 2 * beam
    cont: List[Tuple[int, int, float]] = field(default_factory=list)     # (parent row, token, cum) of the rows that continue
    fin: List[tuple] = field(default_factory=list)   # (row, raw score, final score, tie key), in finishing order
    done: bool = False
    margin: float = math.inf                                       # free steps only
    events: set = field(default_factory=set)                       # what the EOS rules met at this step
    gaps: List[Gap] = field(default_factory=list)


def _final_score(P: BeamParams, raw: float, step_nr: int) -> float:
    # the finished sequence has step_nr + 1 tokens, the prompt's first one included; fairseq2 divides by (seq_len - 1) ^ len_penalty
    return raw / float(step_nr) ** P.len_penalty if P.normalize else raw


def step(P: BeamParams, plan: Plan, step_nr: int, rows: Sequence[Row], logits: torch.Tensor, nfin: int,
         dtype: torch.dtype = torch.float64) -> StepOut:
    """One position of one sentence that is not done.  rows: its live rows; logits [len(rows), vocab] (any float dtype, converted to
    `dtype`); nfin: hypotheses it has finished so far."""
    kind = plan.mode(step_nr)
    assert kind != "past" and len(rows) >= 1 and logits.shape[0] == len(rows)
    beam, vocab = P.beam, logits.shape[1]
    scaled = logits.to(dtype) / P.temperature
    lprobs = torch.log_softmax(scaled, dim=-1)
    cum = torch.tensor([r.cum for r in rows], dtype=dtype)
    out = StepOut(kind, row_max=scaled.max(dim=1).values.tolist(), lse=torch.logsumexp(scaled, dim=1).tolist())
    if kind == "prompt":
        tok = plan.prompt[step_nr]
        out.cont = [(r, tok, float(lprobs[r, tok] + cum[r])) for r in range(len(rows))]
        return out
    if kind == "eos":
        cand = sorted(((float(lprobs[r, P.eos_idx] + cum[r]), r) for r in range(len(rows))), key=lambda c: (-c[0], c[1]))
        take = max(beam - nfin, 0)
        for a, b in list(zip(cand, cand[1:]))[:take]:   # the order of those that finish, and the first one that does not
            out.gaps.append(_gap(a[0], b[0], rows[a[1]], rows[b[1]], logits[a[1]], logits[b[1]], f"forced EOS step {step_nr}"))
        for sc, r in cand[:take]:
            out.fin.append((r, sc, _final_score(P, sc, step_nr), _tie_key(step_nr, rows[r], logits[r])))
        out.done = True
        return out
    # ---- a free step: the masks, then one flat list
    masked = lprobs.clone()
    if P.unk_idx >= 0:
        masked[:, P.unk_idx] -= P.unk_penalty
    if P.pad_idx >= 0:
        masked[:, P.pad_idx] = NEG_INF
    if step_nr < plan.min_len:
        masked[:, P.eos_idx] = NEG_INF
    # what the selection leaves per row, in the scaled-logit domain: value desc, token asc, -inf dropped
    val = scaled.clone()
    val[torch.isinf(masked) & (masked < 0)] = NEG_INF
    if P.unk_idx >= 0:
        val[:, P.unk_idx] -= P.unk_penalty
    for r in range(len(rows)):
        v, t = torch.sort(val[r], descending=True, stable=True)
        keep = int((v[:2 * beam] > NEG_INF).sum())
        out.lists.append((v[:keep].tolist(), t[:keep].tolist()))
    flat = (masked + cum[:, None]).reshape(-1)
    sv, si = torch.sort(flat, descending=True, stable=True)   # stable over row * vocab + token: row asc, then token asc
    nfinite = int((sv > NEG_INF).sum())
    top = [(float(sv[i]), int(si[i]) // vocab, int(si[i]) % vocab) for i in range(min(nfinite, 2 * beam + 1))]
    beyond = top[2 * beam:]       # the best candidate that is NOT on the list, if one exists
    top = top[:2 * beam]
    out.ranked = top
    last = len(top) - 1
    for i, (sc, r, t) in enumerate(top[:beam]):
        if t == P.eos_idx:
            out.fin.append((r, sc, _final_score(P, sc, step_nr), _tie_key(step_nr, rows[r], logits[r])))
            if nfin + len(out.fin) == beam:
                out.done, last = True, i
                break
    eos_at = [i for i, c in enumerate(top) if c[2] == P.eos_idx]
    if len({top[i][1] for i in eos_at if i < beam}) >= 2:
        out.events.add("several rows finish")
    if out.done and last < len(top) - 1:
        out.events.add("beam completed mid-list")
    if any(i >= beam for i in eos_at) and not out.done:
        out.events.add("EOS between beam and 2 beam")
    if not out.done:
        for i, (sc, r, t) in enumerate(top):
            if t != P.eos_idx:
                out.cont.append((r, t, sc))
                if len(out.cont) == beam:
                    last = i
                    break
    # the decision range: neighbours (i, i + 1) for i <= last; the margin sees the list only, the gap condition also what follows it
    seq = top + beyond
    for i in range(min(last + 1, len(seq) - 1)):
        a, b = seq[i], seq[i + 1]
        if i + 1 < len(top):
            out.margin = min(out.margin, a[0] - b[0])
        out.gaps.append(_gap(a[0], b[0], rows[a[1]], rows[b[1]], logits[a[1]], logits[b[1]], f"step {step_nr} rank {i}"))
    return out


def _tie_key(step_nr: int, row: Row, logits_row: torch.Tensor) -> tuple:
    """equal keys and equal scores: two finished hypotheses that any arithmetic ties"""
    return (step_nr, row.cum, logits_row.numpy().tobytes())


def _gap(a: float, b: float, ra: Row, rb: Row, la: torch.Tensor, lb: torch.Tensor, where: str) -> Gap:
    same = a == b and ra.cum == rb.cum and torch.equal(la, lb)
    return Gap(a - b, same, where)


@dataclass
class SearchOut:
    hyps: List[List[Tuple[List[int], float]]]   # per sentence: (generated tokens with the final EOS, score), best first
    margins: List[Tuple[float, float]]          # per sentence: (steps, final ranking)
    gaps: List[List[Gap]]                       # per sentence: every gap inside a decision range, the final ranking's included
    max_abs_cum: float = 0.0
    events: set = field(default_factory=set)
    nactive: List[List[int]] = field(default_factory=list)   # per sentence: live rows after each step


def search(P: BeamParams, plans: Sequence[Plan], f: Callable[[int, List[int]], torch.Tensor],
           dtype: torch.dtype = torch.float64) -> SearchOut:
    """The whole search, every sentence on its own.  A callback with a `batch(sentence, histories) -> [rows, vocab]` method is asked
    for a step's rows in one call (a transformer's bits depend on the batch it runs in)."""
    res = SearchOut([], [], [])
    for s, plan in enumerate(plans):
        rows = [Row([plan.prompt[0]], 0.0)]
        fin: List[tuple] = []   # (tokens, score, tie key)
        gaps: List[Gap] = []
        margin = math.inf
        step_nr = 1
        live: List[int] = []
        res.nactive.append(live)
        while True:
            batch = getattr(f, "batch", None)
            logits = batch(s, [r.hist for r in rows]) if batch else torch.stack([f(s, r.hist) for r in rows])
            o = step(P, plan, step_nr, rows, logits, len(fin), dtype)
            gaps += o.gaps
            res.events |= o.events
            margin = min(margin, o.margin)
            for r, _, score, key in o.fin:
                fin.append((rows[r].hist[plan.plen:] + [P.eos_idx], score, key))
            if o.done:
                break
            assert o.cont, "a sentence ran out of candidates before it was done: not a case the tests drive"
            live.append(len(o.cont))
            rows = [Row(rows[p].hist + [t], c) for p, t, c in o.cont]
            res.max_abs_cum = max(res.max_abs_cum, max(abs(r.cum) for r in rows))
            step_nr += 1
        order = sorted(range(len(fin)), key=lambda i: -fin[i][1])   # stable: equal scores keep their finishing order
        ranked = [fin[i] for i in order]
        for a, b in zip(ranked, ranked[1:]):
            gaps.append(Gap(a[1] - b[1], a[1] == b[1] and a[2] == b[2], "final ranking"))
        res.hyps.append([(t, sc) for t, sc, _ in ranked])
        res.margins.append((margin, ranked[0][1] - ranked[1][1] if len(ranked) >= 2 else math.inf))
        res.gaps.append(gaps)
    return res


def gap_violations(gaps: Sequence[Gap], G: float) -> List[Gap]:
    """The gap condition: every gap inside a decision range is 0 by construction or at least G."""
    return [g for g in gaps if not (g.by_construction and g.gap == 0.0) and not g.gap >= G]


# ------------------------------------------------------------------------------------------------- synthetic logits
_M64 = (1 << 64) - 1


def _mix(x: int) -> int:
    x = (x + 0x9E3779B97F4A7C15) & _M64
    x = ((x ^ (x >> 30)) * 0xBF58476D1CE4E5B9) & _M64
    x = ((x ^ (x >> 27)) * 0x94D049BB133111EB) & _M64
    return x ^ (x >> 31)


def _mix_np(x: np.ndarray) -> np.ndarray:
    with np.errstate(over="ignore"):
        x = x + np.uint64(0x9E3779B97F4A7C15)
        x = (x ^ (x >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        x = (x ^ (x >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
        return x ^ (x >> np.uint64(31))


def hash_row(seed: int, key: Sequence[int], vocab: int) -> torch.Tensor:
    """float32 [vocab]: multiples of 1/4 in [-8, 8] (fp16-exact), a deterministic hash of (seed, key, token).  Level 64 - k (value
    8 - k / 4) has probability (2k + 1) / 4096: a row of 1000 has its best ten tokens on about six levels, so a row's candidates
    both tie (within a level) and differ by multiples of 1/4."""
    h = _mix(seed)
    for t in key:
        h = _mix(h ^ (int(t) & _M64))
    with np.errstate(over="ignore"):
        x = _mix_np(np.uint64(h) + np.arange(vocab, dtype=np.uint64) * np.uint64(0xD1342543DE82EF95))
    u = (x >> np.uint64(11)).astype(np.float64) / float(1 << 53)
    level = 64 - np.minimum(np.floor(64.0 * np.sqrt(u)), 64.0)
    return torch.from_numpy((-8.0 + level / 4.0).astype(np.float32))


@dataclass(frozen=True)
class Synthetic:
    """The logits callback of the kernel tests: hash_row of (sentence, history), then
      by_position: of (sentence, position) only, so sibling rows tie exactly;
      eos_bias[len(history)] (its last entry beyond its end) is added to the EOS logit (multiples of 1/4);
      dup: these tokens get the value of the row's best one (duplicates inside a row, across tiles);
      unk_offset: the UNK logit becomes the row maximum plus this;
      descending: only PAD, EOS and the ids j with 4 <= j < last are finite, last = the row's previous token (4 + descending at the
        first step): most logits are -inf, the rows run out of continuations and the sentence's live rows shrink."""
    seed: int
    vocab: int
    eos_idx: int = 3
    unk_idx: int = 1
    by_position: bool = False
    eos_bias: Tuple[float, ...] = ()
    dup: Tuple[int, ...] = ()
    unk_offset: Optional[float] = None
    descending: int = 0
    eos_tie_at: int = 0    # > 0: at len(history) == eos_tie_at the EOS logit equals the row's best ...
    eos_top_from: int = 0  # ... and from len(history) == eos_top_from + sentence % 3 on it is the best by 1/4

    def __call__(self, s: int, hist: Sequence[int]) -> torch.Tensor:
        key = (s, len(hist)) if self.by_position else (s, *hist)
        row = hash_row(self.seed, key, self.vocab)
        if self.eos_bias:
            row[self.eos_idx] += self.eos_bias[min(len(hist), len(self.eos_bias) - 1)]
        if self.dup:
            row[list(self.dup)] = row.max()
        if self.unk_offset is not None:
            row[self.unk_idx] = row.max() + self.unk_offset
        if self.eos_tie_at and len(hist) == self.eos_tie_at:
            row[self.eos_idx] = row.max()
        if self.eos_top_from and len(hist) >= self.eos_top_from + s % 3:
            row[self.eos_idx] = row.max() + 0.25
        if self.descending:
            last = hist[-1] if len(hist) > 1 and hist[-1] >= 4 else 4 + self.descending
            keep = torch.zeros(self.vocab, dtype=torch.bool)
            keep[[0, self.eos_idx]] = True
            keep[4:last] = True
            row[~keep] = NEG_INF
        return row


# ------------------------------------------------------------------------------------------------- the cases of the kernel tests
# Error model of one step, new_cum = (cum + v) - (pmax + __logf(psum)) in fp32 (tests/test_gpu_beam_kernels.py measures L_LOG):
#   three roundings of at most half an ulp of a value below 128 (the tests assert |cum| <= 64; |v|, |pmax| < 16, lse < 32): 1.5 * 2^-17;
#   v, pmax and the tile statistics carry the fp32 scaling logits * (1 / temperature) where the reference divides exactly: two
#     roundings of 2^-24 relative on values below 16, three times: 3 * 2^-23 * 16;
#   L_LOG: the fast log and the fast exp of the normaliser's tile merge, on 1 <= psum <= vocab.
L_LOG = 4e-6   # 4 x the worst value measured on an MI355X (9.8e-7); tests/test_gpu_beam_kernels.py states the measurement
B_STEP = 1.5 * 2.0 ** -17 + 3 * 2.0 ** -23 * 16 + L_LOG
G_GAP = 16 * B_STEP
CUM_MAX = 64.0


@dataclass(frozen=True)
class Case:
    P: BeamParams
    plans: Tuple[Plan, ...]
    logits: Synthetic
    table: bool = False          # drive the device through the per-sentence prompt table


def _same(n: int, prompt: Tuple[int, ...], gen_cap: int, min_gen: int = 1, model_max: int = 1 << 20) -> Tuple[Plan, ...]:
    return tuple(Plan(prompt, gen_cap, min_gen, model_max) for _ in range(n))


_RAMP = (0.0, 0.0, 0.0, 3.0, 4.0, 5.0, 6.0, 7.0)   # the EOS logit rises with the position: hypotheses finish at different lengths


def _cases() -> dict:
    c = {}
    for beam, seed in ((1, 1), (2, 1), (3, 1), (5, 1), (8, 1)):
        vocab = 5000 if beam == 8 else 1000
        c[f"general_beam{beam}"] = Case(BeamParams(beam), _same(6, (3,), 10), Synthetic(seed, vocab, eos_bias=_RAMP))
    # EOS pressure: the EOS logit near the row's best from the third position on
    c["eos_pressure_beam5"] = Case(BeamParams(5), _same(8, (3,), 10), Synthetic(1, 1000, eos_bias=(0.0, 0.0, 7.25, 7.5, 7.75)))
    c["eos_pressure_beam3"] = Case(BeamParams(3), _same(8, (3,), 10), Synthetic(1, 1000, eos_bias=(0.0, 0.0, 7.25, 7.5, 7.75)))
    for beam in (3, 5):
        c[f"ties_beam{beam}"] = Case(BeamParams(beam), _same(4, (3,), 8),
                                     Synthetic(1, 1000, by_position=True, dup=(10, 300, 301, 700), eos_tie_at=2, eos_top_from=4))
    c["few_finite_beam5"] = Case(BeamParams(5), _same(8, (3,), 5), Synthetic(1, 1000, descending=4))
    c["few_finite_beam8"] = Case(BeamParams(8), _same(4, (3,), 7), Synthetic(3, 5000, descending=6))
    c["prompt3_beam3"] = Case(BeamParams(3), _same(4, (3, 300, 700), 6), Synthetic(1, 1000, eos_bias=_RAMP))
    lens = (1, 2, 4, 4, 2, 1)
    toks = (3, 400, 257, 900)
    c["table_beam3"] = Case(BeamParams(3), tuple(Plan(toks[:n], 6, 2, 9) for n in lens), Synthetic(1, 1000, eos_bias=_RAMP), table=True)
    c["table_equal_lengths_beam2"] = Case(BeamParams(2), tuple(Plan((3, 256 + 100 * s), 6, 2, 64) for s in range(4)),
                                          Synthetic(1, 1000, eos_bias=_RAMP), table=True)
    for name, kw, lg in (("temp07", dict(temperature=0.7), {}), ("temp16", dict(temperature=1.6), {}),
                         ("unk_plus2", dict(unk_penalty=2.0), dict(unk_offset=-0.25)),
                         ("unk_minus2", dict(unk_penalty=-2.0), dict(unk_offset=-1.75)),
                         ("lenpen05", dict(len_penalty=0.5), {}), ("lenpen2", dict(len_penalty=2.0), {}),
                         ("unnormalized", dict(normalize=False), {})):
        c[name] = Case(BeamParams(3, **kw), _same(4, (3,), 8), Synthetic(1, 1000, eos_bias=_RAMP, **lg))
    return c


CASES = _cases()
