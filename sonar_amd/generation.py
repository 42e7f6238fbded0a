"""Samplers and step processors accepted by `EmbeddingToTextModelPipeline.predict(sampler=..., step_processors=...)`.

The reference passes a fairseq2 `Sampler` to `SamplingSeq2SeqGenerator`
(sonar/inference_pipelines/text.py:315-320); fairseq2.generation ships `TopKSampler(k)` and
`TopPSampler(p=0.9)`.  These classes carry the same constructor arguments; the filtering and the draw
run on the device (`smi_text_decoder_sample`, csrc/sampling.hip).  Objects with the same class names
from fairseq2 itself are accepted too (duck-typed on `k` / `p`, see `resolve_sampler`).
"""
from __future__ import annotations

from dataclasses import dataclass
from typing import List, Optional, Sequence, Tuple

from . import _lib


@dataclass(frozen=True)
class TopKSampler:
    """Sample among the `k` most probable tokens (fairseq2.generation.TopKSampler)."""

    k: int

    def __post_init__(self):
        if self.k < 1:
            raise ValueError(f"`k` must be greater than or equal to 1, but is {self.k} instead.")


@dataclass(frozen=True)
class TopPSampler:
    """Nucleus sampling: the smallest set of most probable tokens whose cumulative probability
    exceeds `p` (fairseq2.generation.TopPSampler)."""

    p: float = 0.9

    def __post_init__(self):
        if not 0.0 < self.p <= 1.0:
            raise ValueError(f"`p` must be in (0, 1], but is {self.p} instead.")


def resolve_sampler(sampler) -> Tuple[int, int, float]:
    """-> (SMI_SAMPLER_*, k, p) for one of the classes above or a fairseq2 object of the same kind."""
    name = type(sampler).__name__
    if isinstance(sampler, TopKSampler) or name == "TopKSampler":
        k = int(getattr(sampler, "k", getattr(sampler, "_k", 0)))
        if k < 1:
            raise ValueError("TopKSampler: k must be >= 1")
        return _lib.SMI_SAMPLER_TOP_K, k, 1.0
    if isinstance(sampler, TopPSampler) or name == "TopPSampler":
        p = float(getattr(sampler, "p", getattr(sampler, "_p", 0.0)))
        if not 0.0 < p <= 1.0:
            raise ValueError("TopPSampler: p must be in (0, 1]")
        return _lib.SMI_SAMPLER_TOP_P, 1, p
    raise NotImplementedError(f"sampler {name!r} is not covered by the MI355X engine (TopKSampler, TopPSampler)")


# ---------------------------------------------------------------- step processors
# fairseq2's generators take `step_processors=`; the two it ships are restated here (their published behaviour, [fs2-recall]
# in DESIGN.md 5).  They run on the device inside the token selection (smi_text_decoder_set_step_processors): on the free
# steps only, on the row's sequence so far with the prompt.


@dataclass(frozen=True)
class NGramRepeatBlockProcessor:
    """Ban every token that would repeat an n-gram of the sequence so far, prompt included
    (fairseq2.generation.NGramRepeatBlockProcessor).  n = 1 bans every token already present, the prompt's `</s>` too:
    generation then runs to the length cap."""

    ngram_size: int

    def __post_init__(self):
        if int(self.ngram_size) < 1:
            raise ValueError(f"`ngram_size` must be greater than 0, but is {self.ngram_size} instead.")


@dataclass(frozen=True)
class BannedSequenceProcessor:
    """Ban the last token of each sequence when the sequence so far ends with the rest of it
    (fairseq2.generation.BannedSequenceProcessor); a length-1 sequence bans its token at every free step."""

    banned_seqs: Tuple[Tuple[int, ...], ...]

    def __init__(self, banned_seqs: Sequence[Sequence[int]]):
        if not banned_seqs:
            raise ValueError("`banned_seqs` must contain at least one element.")
        seqs = tuple(tuple(int(t) for t in _as_list(b)) for b in banned_seqs)
        if any(len(b) == 0 for b in seqs):
            raise ValueError("`banned_seqs` must not contain empty sequences.")
        object.__setattr__(self, "banned_seqs", seqs)


def _as_list(x) -> List[int]:
    return x.reshape(-1).tolist() if hasattr(x, "reshape") and hasattr(x, "tolist") else list(x)


def _banned_seqs_of(proc) -> List[List[int]]:
    """Banned sequences of a BannedSequenceProcessor-like object: `banned_seqs`, or fairseq2's own tensors (prefixes
    right-aligned in `banned_prefix` where `banned_prefix_mask` is set, last tokens in `banned_tokens`)."""
    for name in ("banned_seqs", "_banned_seqs"):
        if hasattr(proc, name):
            return [_as_list(b) for b in getattr(proc, name)]
    get = lambda n: getattr(proc, n, getattr(proc, "_" + n, None))  # noqa: E731
    toks, prefix, mask = get("banned_tokens"), get("banned_prefix"), get("banned_prefix_mask")
    if toks is None:
        raise NotImplementedError(f"{type(proc).__name__}: no banned sequences found on the object")
    toks = _as_list(toks)
    out = []
    for i, t in enumerate(toks):
        pre = []
        if prefix is not None and mask is not None:
            pre = [int(p) for p, m in zip(_as_list(prefix[i]), _as_list(mask[i])) if m]
        out.append(pre + [int(t)])
    return out


def resolve_step_processors(step_processors) -> Tuple[int, List[List[int]]]:
    """-> (ngram_size (0 = off), banned sequences) for a list of the classes above or fairseq2 objects of the same names.
    Several n-gram processors resolve to the smallest n (blocking n also blocks every longer repeat); banned sequences
    concatenate.  Any other processor raises NotImplementedError: arbitrary Python processors would need a host round trip
    every step."""
    ngram: Optional[int] = None
    banned: List[List[int]] = []
    for proc in step_processors or ():
        name = type(proc).__name__
        if isinstance(proc, NGramRepeatBlockProcessor) or name == "NGramRepeatBlockProcessor":
            n = int(getattr(proc, "ngram_size", getattr(proc, "_ngram_size", 0)))
            if n < 1:
                raise ValueError("NGramRepeatBlockProcessor: ngram_size must be >= 1")
            ngram = n if ngram is None else min(ngram, n)
        elif isinstance(proc, BannedSequenceProcessor) or name == "BannedSequenceProcessor":
            seqs = _banned_seqs_of(proc)
            if not seqs or any(len(b) == 0 for b in seqs):
                raise ValueError("BannedSequenceProcessor: every banned sequence must be non-empty")
            banned.extend(seqs)
        else:
            raise NotImplementedError(f"step processor {name!r} is not covered by the MI355X engine "
                                      "(NGramRepeatBlockProcessor, BannedSequenceProcessor)")
    return (ngram or 0), banned
