"""GPU: the one-launch sample-rate conversion (smi_resample_batch) against the CPU restatement (tests/resample_ref.py),
its independence of the batch around a clip, and `predict(..., resample=True)` of the speech pipelines.

Tolerance of every output sample: |y - y_ref| <= (S + 4) * 2^-24 * sum_i |k_i||x_i| + 1e-10 with k, x from the restatement:
the standard bound of an S-term fp32 dot product in any order, with or without FMA, one output rounding, and the one-ulp
allowance of the filter table (tests/test_resample_cpu.py).  It is derived, not tuned: a sequential fp32 emulation on the
CPU and the kernel itself reach at most 0.31 of it on these cases (each test prints its figure)."""
import ctypes as C
import os
import wave

import pytest
import torch

from tests import resample_ref as R

pytestmark = pytest.mark.gpu

GOLD = os.path.join(os.path.dirname(__file__), "golden", "heads_reference.pt")


def _uniform(n, seed):
    return torch.rand(n, generator=torch.Generator().manual_seed(seed)) * 2 - 1


def _check_against_restatement(x, orig, new):
    from sonar_amd.resample import resample

    y = resample(x.cuda(), orig, new)
    torch.cuda.synchronize()
    ref = R.resample(x, orig, new)
    assert y.dtype == torch.float32 and y.shape == ref.shape, (y.shape, ref.shape)
    if not ref.numel():
        return 0.0
    support = R.shape(orig, new)[3]
    bound = (support + 4) * 2.0 ** -24 * R.abs_products(x, orig, new) + 1e-10
    err = (y.cpu().double() - ref).abs()
    worst = (err / bound).max().item()
    print(f"resample {orig} -> {new}, {x.numel()} samples: max |err| {err.max().item():.3e}, max err / bound {worst:.3f}")
    assert bool((err <= bound).all()), (orig, new, x.numel(), worst)
    return worst


@pytest.mark.parametrize("orig,new", [(48000, 16000), (44100, 16000), (22050, 16000), (11025, 16000), (8000, 16000),
                                      (16000, 8000)])
def test_single_clips_against_restatement(orig, new):
    o, _, _, support, _ = R.shape(orig, new)
    for length in (1, 2, support - 1, o - 1, o, o + 1, 4001, 70001):   # 70 001 samples span many workgroup tiles
        _check_against_restatement(_uniform(length, seed=orig + length), orig, new)


@pytest.mark.parametrize("orig,new,length", [
    (44056, 16000, 30001),   # a 266 KB table: read through L2, the input span staged in LDS with a shorter tile
    (44800, 64, 70001),      # o = 700, n = 1: the table staged in LDS, the 8 485-tap input span read from memory
    (16000, 3, 70001),       # neither fits
])
def test_pairs_whose_table_or_span_does_not_fit_lds(orig, new, length):
    _check_against_restatement(_uniform(length, seed=orig), orig, new)


def test_channels_are_clips_and_equal_rates_copy():
    from sonar_amd.resample import resample

    x = _uniform(3 * 5000, seed=1).reshape(3, 5000).cuda()
    y = resample(x, 44100)
    assert y.shape == (3, R.num_samples(5000, 44100, 16000))
    for c in range(3):
        assert torch.equal(y[c], resample(x[c].clone(), 44100, 16000))
    assert torch.equal(resample(x, 16000, 16000), x) and torch.equal(resample(x[1], 8000, 8000), x[1])
    assert resample(x[:, :0], 48000).shape == (3, 0)


def test_ragged_mixed_rate_batch_is_the_single_clip_results():
    from sonar_amd import _lib
    from sonar_amd.resample import resample, resample_batch_flat

    lib = _lib.load()
    # (rate, samples, loud): lengths 0, 1 and o - 1 (440 at 44.1 kHz, 2 at 48 kHz), two 44.1 kHz neighbours, and every
    # other clip filled with +-1000 so that a read across a clip boundary moves the quiet clips far outside any rounding
    spec = [(48000, 5001, False), (16000, 1237, True), (44100, 440, False), (44100, 9001, True), (8000, 0, False),
            (8000, 1, False), (22050, 3333, True), (48000, 2, False), (22050, 6151, True)]
    clips = []
    for i, (rate, length, loud) in enumerate(spec):
        x = _uniform(length, seed=100 + i)
        clips.append(torch.where(x < 0, -1000.0, 1000.0) if loud else x)
    front, back = 3, 5                                   # odd, unaligned offsets; the pads are loud as well
    cat = torch.cat([torch.full((front,), 1000.0)] + clips + [torch.full((back,), -1000.0)]).cuda()
    offs = [front]
    for x in clips:
        offs.append(offs[-1] + x.numel())
    rates = [s[0] for s in spec]
    n = len(spec)
    lens = [R.num_samples(s[1], s[0], 16000) for s in spec]
    out_offs = [7]
    for length in lens:
        out_offs.append(out_offs[-1] + length)
    sentinel = -12345.5
    singles = [resample(x.cuda(), rate, 16000) for x, rate in zip(clips, rates)]

    def launch():
        out = torch.full((out_offs[-1] + 9,), sentinel, device="cuda")
        _lib.check(lib.smi_resample_batch(cat.data_ptr(), (C.c_int64 * (n + 1))(*offs), (C.c_int32 * n)(*rates), n, 16000,
                                          out.data_ptr(), (C.c_int64 * (n + 1))(*out_offs), _lib.current_stream_ptr()))
        torch.cuda.synchronize()
        return out

    out = launch()
    assert bool((out[:7] == sentinel).all()) and bool((out[out_offs[-1]:] == sentinel).all())
    for i in range(n):
        got = out[out_offs[i]:out_offs[i + 1]]
        assert got.numel() == lens[i]
        assert torch.equal(got, singles[i]), (i, spec[i])
    assert torch.equal(out[out_offs[1]:out_offs[2]], clips[1].cuda())       # the 16 kHz clip is its input
    assert torch.equal(launch(), out)
    # the quiet clips also stand against the restatement from inside the batch
    for i in (0, 2, 7):
        ref = R.resample(clips[i], rates[i], 16000)
        bound = (R.shape(rates[i], 16000)[3] + 4) * 2.0 ** -24 * R.abs_products(clips[i], rates[i], 16000) + 1e-10
        assert bool(((out[out_offs[i]:out_offs[i + 1]].cpu().double() - ref).abs() <= bound).all()), i
    # the same batch through the Python entry point, which packs the outputs from 0
    flat, flat_offs = resample_batch_flat(cat, offs, rates)
    assert flat_offs == [o - 7 for o in out_offs] and torch.equal(flat, out[7:out_offs[-1]])


def _write_wav(path, pcm, rate):
    with wave.open(str(path), "wb") as w:
        w.setnchannels(1)
        w.setsampwidth(2)
        w.setframerate(rate)
        w.writeframes(pcm.numpy().tobytes())


def test_pipelines_resample_files_and_pairs(tmp_path):
    from oracle import speech_encoder as OS
    from oracle.speech_encoder import OracleSpeechEncoderConfig
    from sonar_amd.heads import MutoxClassifier, MutoxConfig
    from sonar_amd.inference_pipelines import MutoxSpeechClassifierPipeline, SpeechToEmbeddingModelPipeline
    from sonar_amd.resample import resample
    from sonar_amd.speech_encoder import SonarSpeechEncoderConfig, SonarSpeechEncoderModel

    ocfg = OracleSpeechEncoderConfig(model_dim=256, num_layers=1, num_heads=4, ffn_inner_dim=512, conv_kernel=7,
                                     pooler_layers=1, pooler_heads=4, pooler_ffn_dim=384, pooler_vocab=64)
    cfg = SonarSpeechEncoderConfig(model_dim=256, num_encoder_layers=1, num_encoder_attn_heads=4, ffn_inner_dim=512,
                                   depthwise_conv_kernel_size=7, num_decoder_layers=1, num_decoder_attn_heads=4,
                                   decoder_ffn_inner_dim=384, max_frames=512)
    model = SonarSpeechEncoderModel(cfg, OS.make_synthetic_params(ocfg, seed=5, std=0.06), device="cuda:0", dtype=torch.float32)
    pipe = SpeechToEmbeddingModelPipeline(model, device=torch.device("cuda:0"))
    files, waves, rates = [], [], [48000, 8000, 16000]
    for i, (rate, length) in enumerate(zip(rates, (52001, 9000, 17777))):
        pcm = (_uniform(length, seed=40 + i) * 32767).round().clamp(-32768, 32767).to(torch.int16)
        files.append(str(tmp_path / f"clip{rate}.wav"))
        _write_wav(files[-1], pcm, rate)
        waves.append((pcm.float() / 32768.0).unsqueeze(0))
    at16k = [resample(w.cuda(), r, 16000) for w, r in zip(waves, rates)]
    assert torch.equal(at16k[2], waves[2].cuda())

    want = pipe.predict(at16k, batch_size=2)
    got = pipe.predict(files, resample=True, batch_size=2)
    assert got.shape == (3, 256) and torch.equal(got, want)
    pairs = [(w, r) for w, r in zip(waves, rates)]
    assert torch.equal(pipe.predict(pairs, resample=True, batch_size=2), want)
    assert torch.equal(pipe.predict([pairs[0], files[1], waves[2]], resample=True, batch_size=2), want)
    # a batch that is at 16 kHz already skips the launch and is what it was without the keyword
    assert torch.equal(pipe.predict(at16k, resample=True, batch_size=2), want)
    with pytest.raises(ValueError, match="16 kHz"):
        pipe.predict(files, batch_size=2)
    with pytest.raises(ValueError, match="16 kHz"):
        pipe.predict(files[:1], resample=False)

    clf = MutoxClassifier(MutoxConfig(256), torch.load(GOLD)["mutox"][0]["state_dict"], device="cuda:0")
    mutox = MutoxSpeechClassifierPipeline(clf, model, device=torch.device("cuda:0"))
    tox = mutox.predict(files, batch_size=2, resample=True)
    assert tox.shape == (3, 1) and torch.equal(tox, mutox.predict(at16k, batch_size=2))
    with pytest.raises(ValueError, match="16 kHz"):
        mutox.predict(files, batch_size=2)
