"""CPU: the sample-rate conversion's restatement (tests/resample_ref.py) against itself, the engine's host-built filter
table and length rule against the restatement, every refusal of the C ABI, and the host half of `predict(resample=True)`.
The library cross-compiles and loads without a device; the launch itself is tested in tests/test_gpu_resample.py."""
import ctypes as C
import math
import wave

import pytest
import torch

from tests import flac_writer as FW
from tests import resample_ref as R

PAIRS = [(44100, 16000), (48000, 16000), (8000, 16000), (22050, 16000), (16000, 8000)]


@pytest.fixture(scope="module")
def lib():
    from sonar_amd import _lib, build

    build.build(verbose=False)
    return _lib.load()


def _err(lib):
    return lib.smi_last_error().decode()


@pytest.mark.parametrize("orig,new", PAIRS)
def test_restatement_conv_form_equals_compact_sum(orig, new):
    o, n, width, support, _ = R.shape(orig, new)
    g = torch.Generator().manual_seed(orig + new)
    for length in (0, 1, o - 1, o, o + 1, 4001):
        x = torch.rand(length, generator=g, dtype=torch.float64) * 2 - 1
        y = R.resample(x, orig, new)
        assert y.dtype == torch.float64 and y.numel() == math.ceil(n * length / o) == R.num_samples(length, orig, new)
        z = R.resample_compact(x, orig, new)
        assert z.shape == y.shape
        if y.numel():
            assert (y - z).abs().max().item() <= 1e-12
    # what the compact table leaves out is exactly zero in fp32
    full = R.full_table(orig, new)
    taps, first = R.compact_table(orig, new)
    assert taps.shape == (n, support) and full.shape == (n, 2 * width + o)
    for p in range(n):
        rest = full[p].clone()
        rest[first[p]: first[p] + support] = 0
        assert not rest.any()


def test_restatement_equal_rates_return_the_input():
    x = torch.rand(777, dtype=torch.float64)
    assert torch.equal(R.resample(x, 16000, 16000), x) and torch.equal(R.resample_compact(x, 22050, 22050), x)
    assert R.num_samples(777, 16000, 16000) == 777


def test_filter_shapes_of_the_common_rates():
    assert R.shape(44100, 16000)[:4] == (441, 160, 17, 34)
    assert R.shape(48000, 16000)[:4] == (3, 1, 19, 37)
    assert R.shape(8000, 16000)[:4] == (1, 2, 7, 13)


@pytest.mark.parametrize("orig,new", PAIRS + [(11025, 16000), (44056, 16000)])
def test_engine_filter_table_matches_restatement(lib, orig, new):
    from sonar_amd.resample import resample_filter

    o, n, width, support, _ = R.shape(orig, new)
    ref_taps, ref_first = R.compact_table(orig, new)
    taps, first, w = resample_filter(orig, new)
    assert taps.shape == (n, support) and w == width
    assert first.tolist() == ref_first
    # two correct double evaluations may round to neighbouring fp32 values; near the sinc's zero crossings only the
    # absolute error of sin is bounded
    err = (taps.double() - ref_taps.double()).abs()
    tol = 2.0 ** -23 * ref_taps.double().abs() + 1e-12
    assert bool((err <= tol).all()), (err - tol).max().item()
    # sizes alone, and a second call (the cached table) gives the same bits
    ph, sup, wd = C.c_int32(0), C.c_int32(0), C.c_int32(0)
    assert lib.smi_resample_filter(orig, new, C.byref(ph), C.byref(sup), C.byref(wd), None, None) == 0
    assert (ph.value, sup.value, wd.value) == (n, support, width)
    assert torch.equal(resample_filter(orig, new)[0], taps)


def test_num_samples_matches_the_length_rule(lib):
    for orig, new in PAIRS + [(11025, 16000), (44056, 16000), (16000, 16000), (16001, 16000)]:
        o, n = R.shape(orig, new)[:2]
        for length in (0, 1, o - 1, o, o + 1, 4001, 2 ** 31 + 12345, 2 ** 40 + 1):
            assert lib.smi_resample_num_samples(length, orig, new) == -(-n * length // o), (orig, new, length)
    assert lib.smi_resample_num_samples(3 * 2 ** 31, 48000, 16000) == 2 ** 31


def test_bad_rates_are_refused_with_both_rates_in_the_text(lib):
    from sonar_amd import _lib
    from sonar_amd.resample import resample_filter, resample_num_samples

    for orig, new, what in ((0, 16000, "positive"), (16000, 0, "positive"), (-8000, 16000, "positive"),
                            (2 ** 20 + 1, 16000, "above"), (16000, 2 ** 20 + 1, "above")):
        assert lib.smi_resample_num_samples(100, orig, new) < 0
        assert str(orig) in _err(lib) and str(new) in _err(lib) and what in _err(lib)
        assert lib.smi_resample_filter(orig, new, None, None, None, None, None) == -2
        assert str(orig) in _err(lib) and str(new) in _err(lib) and what in _err(lib)
        with pytest.raises(_lib.SmiError, match="SMI_ERR_UNSUPPORTED"):
            resample_num_samples(100, orig, new)
    # 2^20 itself is a rate like any other
    assert lib.smi_resample_num_samples(2 ** 20, 2 ** 20, 16000) == 16000
    # a pair whose compact table exceeds 16 MiB: 1048573 (prime) -> 16000 has 16000 phases of 795 taps
    assert lib.smi_resample_num_samples(100, 1048573, 16000) == 2
    assert lib.smi_resample_filter(1048573, 16000, None, None, None, None, None) == -2
    assert "1048573" in _err(lib) and "16000" in _err(lib) and "exceeds 16777216 bytes" in _err(lib)
    with pytest.raises(_lib.SmiError, match="filter table"):
        resample_filter(1048573, 16000)
    # 16001 -> 16000 (813 KB) is the largest table of the documented cases and is served
    assert lib.smi_resample_filter(16001, 16000, None, None, None, None, None) == 0


def test_batch_arguments_are_validated_before_any_device_work(lib):
    i64, i32 = C.c_int64, C.c_int32
    buf = (C.c_float * 64)()
    ptr = C.addressof(buf)
    ins, rates, outs = (i64 * 3)(0, 30, 36), (i32 * 2)(48000, 8000), (i64 * 3)(5, 15, 27)

    def call(waves=ptr, in_offsets=ins, rates=rates, n=2, new=16000, out=ptr, out_offsets=outs):
        return lib.smi_resample_batch(waves, in_offsets, rates, n, new, out, out_offsets, None)

    for kw in (dict(waves=None), dict(in_offsets=None), dict(rates=None), dict(out=None), dict(out_offsets=None)):
        assert call(**kw) == -1 and "null argument" in _err(lib)
    assert call(n=0) == -1
    assert call(in_offsets=(i64 * 3)(0, 30, 24)) == -1 and "non-decreasing" in _err(lib)
    assert call(out_offsets=(i64 * 3)(5, 15, 10)) == -1 and "non-decreasing" in _err(lib)
    assert call(out_offsets=(i64 * 3)(5, 15, 26)) == -1 and "clip 1" in _err(lib) and "12" in _err(lib)
    assert call(out_offsets=(i64 * 3)(5, 16, 28)) == -1 and "clip 0" in _err(lib)
    assert call(rates=(i32 * 2)(48000, 0)) == -2 and "0 Hz -> 16000 Hz" in _err(lib)
    assert call(rates=(i32 * 2)(-1, 8000)) == -2 and "-1 Hz" in _err(lib)
    assert call(new=2 ** 20 + 1) == -2 and "above" in _err(lib)
    assert call(rates=(i32 * 2)(1048573, 8000), out_offsets=(i64 * 3)(5, 6, 18)) == -2 and "filter table" in _err(lib)


@pytest.mark.skipif(torch.cuda.is_available(), reason="checks the no-device behaviour")
def test_batch_without_a_device_fails_loudly(lib):
    from sonar_amd import _lib
    from sonar_amd.resample import resample, resample_batch_flat

    buf = (C.c_float * 64)()
    ptr = C.addressof(buf)
    rc = lib.smi_resample_batch(ptr, (C.c_int64 * 3)(0, 30, 36), (C.c_int32 * 2)(48000, 8000), 2, 16000, ptr,
                                (C.c_int64 * 3)(5, 15, 27), None)
    assert rc == -3 and "no HIP device" in _err(lib)
    with pytest.raises(_lib.SmiError, match="SMI_ERR_NO_DEVICE"):
        _lib.check(rc)
    with pytest.raises(RuntimeError, match="HIP device only"):
        resample(torch.zeros(100), 48000)
    with pytest.raises(RuntimeError, match="HIP device only"):
        resample_batch_flat(torch.zeros(100), [0, 100], 48000)


def test_abi_revision_is_unchanged(lib):
    from sonar_amd import _lib

    assert _lib.ABI_VERSION == 7 and lib.smi_abi_version() == 7
    for name in ("smi_resample_num_samples", "smi_resample_filter", "smi_resample_batch"):
        assert name in _lib.SYMBOLS


def _write_wav(path, pcm: torch.Tensor, rate: int):
    with wave.open(str(path), "wb") as w:
        w.setnchannels(1)
        w.setsampwidth(2)
        w.setframerate(rate)
        w.writeframes(pcm.to(torch.int16).numpy().tobytes())


def test_host_half_carries_the_source_rates(lib, tmp_path):
    from sonar_amd.inference_pipelines.speech import SpeechModelPipelineInterface, read_audio, read_wav

    g = torch.Generator().manual_seed(4)
    pcm44 = torch.randint(-20000, 20000, (4410,), generator=g)
    flac = tmp_path / "clip44.flac"
    flac.write_bytes(FW.encode([pcm44.tolist()], 16, 44100, [dict(n=4096, sub=[dict(kind="fixed", order=2, porder=4)]),
                                                              dict(n=4410 - 4096, sub=[dict(kind="fixed", order=1)])]))
    pcm48 = torch.randint(-20000, 20000, (4800,), generator=g)
    wav48 = tmp_path / "clip48.wav"
    _write_wav(wav48, pcm48, 48000)
    t8 = torch.rand(2, 801, generator=g) * 2 - 1

    w, rate = read_audio(flac)
    assert rate == 44100 and w.shape == (1, 4410) and torch.equal(w[0], pcm44.float() / 32768.0)
    w, rate = read_audio(wav48)
    assert rate == 48000 and w.shape == (1, 4800) and torch.equal(w[0], pcm48.float() / 32768.0)

    host = SpeechModelPipelineInterface()
    host.device = torch.device("cpu")
    items = [str(flac), wav48, (t8, 8000), t8[1]]
    hbs = list(host._host_batches(items, 3, 2, resample=True))
    assert [hb.rates for hb in hbs] == [[44100, 48000, 8000], [16000]]
    assert hbs[0].offsets == [0, 4410, 9210, 10011] and hbs[1].offsets == [0, 801]
    assert torch.equal(hbs[0].cat[:4410], pcm44.float() / 32768.0)
    assert torch.equal(hbs[0].cat[4410:9210], pcm48.float() / 32768.0)
    assert torch.equal(hbs[0].cat[9210:], t8[0]) and torch.equal(hbs[1].cat, t8[1])   # channel 0, as ever
    assert [hb.rates for hb in host._prefetched(items, 4, 1, 2, resample=True)] == [[44100, 48000, 8000, 16000]]

    # the default is what it was: other rates raise, pairs are not an input, and the batch carries no rates
    for item in (str(flac), wav48):
        with pytest.raises(ValueError, match="16 kHz"):
            read_wav(item)
        with pytest.raises(ValueError, match="16 kHz"):
            list(host._host_batches([item], 1, 1))
    with pytest.raises(ValueError, match="resample=True"):
        list(host._host_batches([(t8, 8000)], 1, 1))
    with pytest.raises(ValueError, match="resample=True"):
        list(host._prefetched([(t8, 8000)], 1, 1, 2))
    assert [hb.rates for hb in host._host_batches([t8], 1, 1)] == [None]
    with pytest.raises(ValueError, match="pair"):
        list(host._host_batches([(8000, t8)], 1, 1, resample=True))
