"""Sample-rate conversion on the MI355X (`smi_resample_batch`): the windowed-sinc polyphase resampler that
`torchaudio.functional.resample` applies by default (sinc_interp_hann, lowpass_filter_width 6, rolloff 0.99), one launch
for a ragged batch of clips that may each have their own source rate.  Device only, like `waveform_to_fbank`."""
from __future__ import annotations

import ctypes as C
from typing import List, Sequence, Tuple, Union

import torch

from . import _lib


def resample_num_samples(nsamples: int, orig_freq: int, new_freq: int = 16000) -> int:
    """ceil(new * nsamples / orig) on the reduced rates; bad rates raise SmiError."""
    lib = _lib.load()
    n = int(lib.smi_resample_num_samples(int(nsamples), int(orig_freq), int(new_freq)))
    if n < 0:
        raise _lib.SmiError(-2, lib.smi_last_error().decode("utf-8", "replace"))
    return n


def resample_filter(orig_freq: int, new_freq: int = 16000) -> Tuple[torch.Tensor, torch.Tensor, int]:
    """The engine's filter of a rate pair -> (taps fp32 [phases, support], first tap index int32 [phases], width).  Host only."""
    lib = _lib.load()
    ph, sup, width = C.c_int32(0), C.c_int32(0), C.c_int32(0)
    _lib.check(lib.smi_resample_filter(int(orig_freq), int(new_freq), C.byref(ph), C.byref(sup), C.byref(width), None, None))
    taps = torch.empty((ph.value, sup.value), dtype=torch.float32)
    first = torch.empty(ph.value, dtype=torch.int32)
    _lib.check(lib.smi_resample_filter(int(orig_freq), int(new_freq), C.byref(ph), C.byref(sup), C.byref(width),
                                       taps.data_ptr(), first.data_ptr()))
    return taps, first, int(width.value)


def resample_batch_flat(cat: torch.Tensor, offsets: Sequence[int], rates: Union[int, Sequence[int]],
                        new_freq: int = 16000) -> Tuple[torch.Tensor, List[int]]:
    """Clips that are already concatenated on the device: `cat` fp32 1-D, clip i = cat[offsets[i]:offsets[i+1]] sampled at
    rates[i] (one int = every clip).  Returns (the clips at `new_freq`, concatenated, their offsets).  A clip already at
    `new_freq` is copied bit for bit; every output sample depends on its own clip alone."""
    if cat.device.type != "cuda":
        raise RuntimeError("resampling runs on a HIP device only (no CPU path)")
    if cat.dim() != 1 or cat.dtype != torch.float32:
        raise ValueError("`cat` must be a 1-D float32 tensor")
    n = len(offsets) - 1
    if n <= 0:
        raise ValueError("empty batch")
    offs = [int(o) for o in offsets]
    rates = [int(rates)] * n if isinstance(rates, int) else [int(r) for r in rates]
    if len(rates) != n:
        raise ValueError(f"{n} clips but {len(rates)} sample rates")
    if offs[0] < 0 or offs[-1] > cat.numel() or any(b < a for a, b in zip(offs, offs[1:])):
        raise ValueError("offsets must be non-decreasing and lie inside `cat`")
    out_offs = [0]
    for i in range(n):
        out_offs.append(out_offs[-1] + resample_num_samples(offs[i + 1] - offs[i], rates[i], new_freq))
    cat = cat.contiguous()
    out = torch.empty(out_offs[-1], dtype=torch.float32, device=cat.device)
    if out_offs[-1] == 0:
        return out, out_offs
    lib = _lib.load()
    with torch.cuda.device(cat.device):
        _lib.check(lib.smi_resample_batch(cat.data_ptr(), (C.c_int64 * (n + 1))(*offs), (C.c_int32 * n)(*rates), n,
                                          int(new_freq), out.data_ptr(), (C.c_int64 * (n + 1))(*out_offs),
                                          _lib.current_stream_ptr()))
    return out, out_offs


def resample(waveform: torch.Tensor, orig_freq: int, new_freq: int = 16000) -> torch.Tensor:
    """`torchaudio.functional.resample(waveform, orig_freq, new_freq)` with its default filter, on the GPU.
    waveform: 1-D or [channels, samples] fp32 on a HIP device; every channel is resampled as a clip of its own."""
    if not waveform.is_cuda:
        raise RuntimeError("resample runs on a HIP device only (no CPU path)")
    if waveform.dim() not in (1, 2):
        raise ValueError("waveform tensors must be [samples] or [channels, samples]")
    w = waveform.to(torch.float32).contiguous()
    ch, t = (1, w.shape[0]) if w.dim() == 1 else w.shape
    if ch == 0:
        return w.new_empty((0, resample_num_samples(t, orig_freq, new_freq)))
    out, offs = resample_batch_flat(w.reshape(-1), [i * t for i in range(ch + 1)], int(orig_freq), new_freq)
    return out if w.dim() == 1 else out.reshape(ch, offs[1])
