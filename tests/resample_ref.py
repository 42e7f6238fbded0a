"""CPU restatement of the sample-rate conversion the engine states in include/sonar_mi355.h (smi_resample_*): the
windowed-sinc polyphase resampler of torchaudio.functional.resample with its default arguments (sinc_interp_hann,
lowpass_filter_width 6, rolloff 0.99).  torchaudio is not installed next to this engine, so the procedure is written from
torchaudio's published algorithm and is NOT pinned to torchaudio's output.  Everything is torch float64 and literal: the
full (2 width + o)-tap table, cast to fp32 and back, zero padding (width, width + o), conv1d with stride o, transpose,
reshape, cut to ceil(n L / o).  Also here: the compact table the engine keeps (the S-tap support of every phase and its
first tap index), a direct sum over that support, and the sum of |k||x| the GPU tolerance is built on.
Not collected by pytest."""
from __future__ import annotations

import math
from typing import List, Tuple

import torch
import torch.nn.functional as F

LOWPASS_FILTER_WIDTH = 6
ROLLOFF = 0.99


def shape(orig: int, new: int) -> Tuple[int, int, int, int, float]:
    """-> (o, n, width, S, base) of a rate pair."""
    g = math.gcd(orig, new)
    o, n = orig // g, new // g
    base = min(o, n) * ROLLOFF
    width = math.ceil(LOWPASS_FILTER_WIDTH * o / base)
    support = math.floor(2 * LOWPASS_FILTER_WIDTH * o / base) + 1
    return o, n, width, support, base


def num_samples(length: int, orig: int, new: int) -> int:
    o, n = shape(orig, new)[:2]
    return -(-n * length // o)


def _table64(orig: int, new: int) -> Tuple[torch.Tensor, torch.Tensor]:
    """-> (coefficients float64 [n, 2 width + o] before the fp32 cast, the unclamped t of every tap)."""
    o, n, width, _, base = shape(orig, new)
    idx = torch.arange(-width, width + o, dtype=torch.float64)[None, :] / o
    t = torch.arange(0, -n, -1, dtype=torch.float64)[:, None] / n + idx
    t = t * base
    raw = t.clone()
    t = t.clamp(-LOWPASS_FILTER_WIDTH, LOWPASS_FILTER_WIDTH)
    window = torch.cos(t * math.pi / (2 * LOWPASS_FILTER_WIDTH)) ** 2
    t = t * math.pi
    scale = base / o
    k = torch.where(t == 0, torch.ones_like(t), t.sin() / t)
    return k * (window * scale), raw


def full_table(orig: int, new: int) -> torch.Tensor:
    """The filter as it is applied: float64 [n, 2 width + o] holding fp32 values."""
    return _table64(orig, new)[0].float().double()


def compact_table(orig: int, new: int) -> Tuple[torch.Tensor, List[int]]:
    """-> (fp32 [n, S], first tap index per phase): the S-tap run that starts at the first tap whose window is not the
    clamped cos(pi/2)^2 (moved back where it would run past the table)."""
    o, n, width, support, _ = shape(orig, new)
    k64, raw = _table64(orig, new)
    total = 2 * width + o
    inside = raw > -LOWPASS_FILTER_WIDTH
    first = []
    for p in range(n):
        nz = torch.nonzero(inside[p])
        i = int(nz[0]) if len(nz) else total - 1
        first.append(max(0, min(i, total - support)))
    cols = torch.tensor(first)[:, None] + torch.arange(support)[None, :]
    return torch.gather(k64.float(), 1, cols), first


def resample(x: torch.Tensor, orig: int, new: int) -> torch.Tensor:
    """The literal procedure on one clip (1-D) -> float64 [ceil(n L / o)]."""
    x = x.double().reshape(-1)
    if orig == new:
        return x
    o, n, width, _, _ = shape(orig, new)
    k = full_table(orig, new)
    xpad = F.pad(x[None, None], (width, width + o))
    y = F.conv1d(xpad, k[:, None, :], stride=o)          # [1, n, frames]
    return y.transpose(1, 2).reshape(-1)[: num_samples(x.numel(), orig, new)]


def _support_products(x: torch.Tensor, orig: int, new: int) -> torch.Tensor:
    """float64 [outputs, S]: k[p][first[p] + s] * xpad[m o + first[p] + s] for output j = m n + p."""
    x = x.double().reshape(-1)
    o, n, width, support, _ = shape(orig, new)
    taps, first = compact_table(orig, new)
    xpad = F.pad(x, (width, width + o))
    j = torch.arange(num_samples(x.numel(), orig, new))
    m, p = j // n, j % n
    start = m * o + torch.tensor(first)[p]
    cols = start[:, None] + torch.arange(support)[None, :]
    return taps.double()[p] * xpad[cols]


def resample_compact(x: torch.Tensor, orig: int, new: int) -> torch.Tensor:
    """The same outputs as a direct sum over the compact support."""
    if orig == new:
        return x.double().reshape(-1)
    return _support_products(x, orig, new).sum(dim=1)


def abs_products(x: torch.Tensor, orig: int, new: int) -> torch.Tensor:
    """sum_i |k_i| |x_i| per output: the scale of the fp32 dot-product error bound."""
    return _support_products(x, orig, new).abs().sum(dim=1)
