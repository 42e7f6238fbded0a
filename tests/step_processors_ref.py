"""CPU restatement of the two step processors (fairseq2's NGramRepeatBlockProcessor / BannedSequenceProcessor, as the
engine states them in include/sonar_mi355.h) and an incremental beam search with a processor hook, built on the oracle's
`_decoder_step_cached` / `_IncrementalState` / `Hypothesis` and the `margins_out` convention of
`oracle.text_decoder.beam_search_incremental` (which it equals exactly without processors).  Not collected by pytest."""
from __future__ import annotations

from typing import List, Optional, Sequence, Set, Tuple

import torch


def ngram_bans(seq: Sequence[int], n: int) -> Set[int]:
    """Ids that would repeat an n-gram of `seq`: for every window start i in [0, L - n] whose first n - 1 tokens equal the
    last n - 1 tokens of seq, seq[i + n - 1]."""
    s, L = list(seq), len(seq)
    if n < 1 or L < n:
        return set()
    tail = s[L - n + 1:] if n > 1 else []
    return {s[i + n - 1] for i in range(L - n + 1) if s[i:i + n - 1] == tail}


def banned_seq_bans(seq: Sequence[int], banned_seqs: Sequence[Sequence[int]]) -> Set[int]:
    s, L = list(seq), len(seq)
    out = set()
    for b in banned_seqs:
        b = list(b)
        pl = len(b) - 1
        if pl <= L and (pl == 0 or s[L - pl:] == b[:-1]):
            out.add(b[-1])
    return out


def bans(seq: Sequence[int], ngram: int = 0, banned_seqs: Sequence[Sequence[int]] = ()) -> Set[int]:
    return (ngram_bans(seq, ngram) if ngram else set()) | banned_seq_bans(seq, banned_seqs)


def repeated_ngrams(seq: Sequence[int], n: int) -> int:
    grams = [tuple(seq[i:i + n]) for i in range(len(seq) - n + 1)]
    return len(grams) - len(set(grams))


@torch.inference_mode()
def beam_search_with_bans(params, cfg, embeddings: torch.Tensor, prompt: Sequence[int], beam_size: int = 5,
                          min_gen_len: int = 1, max_gen_len: Tuple[int, int] = (1, 128), max_seq_len: Optional[int] = None,
                          normalize_scores: bool = True, len_penalty: float = 1.0, pad_idx: int = 0, eos_idx: int = 3,
                          source_len: Optional[int] = None, margins_out: Optional[list] = None, ngram: int = 0,
                          banned_seqs: Sequence[Sequence[int]] = ()):
    """oracle.text_decoder.beam_search_incremental with the step processors applied on the free steps: a banned id's
    log-probability becomes -inf after log_softmax, on the row's sequence so far (prompt included)."""
    from oracle.text_decoder import Hypothesis, _decoder_step_cached, _IncrementalState

    model_max = max_seq_len if max_seq_len is not None else cfg.max_seq_len
    plen = len(prompt)
    if source_len is None:
        source_len = cfg.cond_dim
    max_len = min(plen + int(max_gen_len[0] * source_len + max_gen_len[1]), model_max)
    min_len = min(plen + min_gen_len, max_len)
    results: List[List[Hypothesis]] = []
    for e in embeddings:
        emb = e.unsqueeze(0)
        st = _IncrementalState(cfg.num_layers)
        seqs = torch.tensor([list(prompt)], dtype=torch.int64)
        cum = torch.zeros(1, plen, dtype=torch.float32)
        for pos in range(plen - 1):
            lp = torch.log_softmax(_decoder_step_cached(params, cfg, emb, seqs[:, pos], pos, st), dim=-1, dtype=torch.float32)
            cum[0, pos + 1] = cum[0, pos] + lp[0, seqs[0, pos + 1]]
        finished: List[Hypothesis] = []
        step_nr = plen
        dec_margin = dec_margin_free = float("inf")
        while True:
            b = seqs.shape[0]
            logits = _decoder_step_cached(params, cfg, emb.expand(b, -1), seqs[:, -1], step_nr - 1, st)
            lprobs = torch.log_softmax(logits, dim=-1, dtype=torch.float32)
            if step_nr == max_len - 1:
                lprobs[:, :eos_idx] = -torch.inf
                lprobs[:, eos_idx + 1:] = -torch.inf
            else:
                lprobs[:, pad_idx] = -torch.inf
                if step_nr < min_len:
                    lprobs[:, eos_idx] = -torch.inf
                for r in range(b):   # the processors: free steps only
                    banned = bans(seqs[r].tolist(), ngram, banned_seqs)
                    if banned:
                        lprobs[r, sorted(banned)] = -torch.inf
            v = lprobs.shape[1]
            cand = (lprobs + cum[:, -1:]).view(-1)
            top_scores, top_idx = torch.topk(cand, min(2 * beam_size, v - 1))
            seq_idx, vocab_idx = top_idx // v, top_idx % v
            eos_mask = vocab_idx == eos_idx
            done = False
            head = eos_mask[:beam_size]
            completing = -1
            head_pos = torch.nonzero(head).view(-1).tolist()
            for hp, si, sc in zip(head_pos, seq_idx[:beam_size][head].tolist(), top_scores[:beam_size][head].tolist()):
                seq = torch.cat([seqs[si], torch.tensor([eos_idx])])
                steps = torch.cat([cum[si], torch.tensor([sc])])
                seq_len = step_nr + 1
                out_steps = steps[plen:seq_len] - steps[plen - 1:seq_len - 1]
                score = sc / (seq_len - 1) ** len_penalty if normalize_scores else sc
                finished.append(Hypothesis(seq[plen:], float(score), out_steps))
                if len(finished) == beam_size:
                    done = True
                    completing = hp
                    break
            if margins_out is not None:
                last = completing
                if not done:
                    non_eos = torch.nonzero(~eos_mask).view(-1)
                    last = int(non_eos[min(beam_size, non_eos.numel()) - 1]) if non_eos.numel() else top_scores.numel() - 1
                upto = min(last + 1, top_scores.numel() - 1)
                if upto >= 1:
                    gaps = top_scores[:upto] - top_scores[1:upto + 1]
                    gaps = gaps[torch.isfinite(gaps)]
                    if gaps.numel():
                        dec_margin = min(dec_margin, float(gaps.min()))
                        if step_nr != max_len - 1:
                            dec_margin_free = min(dec_margin_free, float(gaps.min()))
            if done:
                break
            keep = ~eos_mask
            seq_idx, vocab_idx, top_scores = seq_idx[keep][:beam_size], vocab_idx[keep][:beam_size], top_scores[keep][:beam_size]
            seqs = torch.cat([seqs[seq_idx], vocab_idx.unsqueeze(1)], dim=1)
            cum = torch.cat([cum[seq_idx], top_scores.unsqueeze(1)], dim=1)
            st.reorder(seq_idx)
            step_nr += 1
            if step_nr >= max_len:
                break
        finished.sort(key=lambda h: h.score, reverse=True)
        results.append(finished)
        if margins_out is not None:
            fin = finished[0].score - finished[1].score if len(finished) > 1 else float("inf")
            margins_out.append((dec_margin, fin, dec_margin_free))
    return results


def rescore(OD, params, ocfg, e: torch.Tensor, prompt: Sequence[int], toks: Sequence[int]) -> torch.Tensor:
    """Teacher-forced fp32 log-probabilities [len(toks)] of the generated tokens after the prompt."""
    full = torch.tensor([list(prompt) + list(toks)])
    lp = torch.log_softmax(OD.decoder_logits(params, ocfg, e.unsqueeze(0), full[:, :-1]), dim=-1)
    p = len(prompt)
    return lp[0, torch.arange(p - 1, full.shape[1] - 1), full[0, p:]]
