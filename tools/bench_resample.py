"""Sample-rate conversion in front of the speech encoder: 64 clips x 10 s at 48 kHz and at 44.1 kHz -> 16 kHz in one launch
(`smi_resample_batch`), timed with device events next to the filterbank and the encoder forward of the same batch
(sonar_speech_encoder_eng on synthetic weights, fp16), plus 1 - cos between the embedding of a synthetic 16 kHz clip and of
the same signal sampled at 48 kHz and sent through `predict(..., resample=True)`.

    python tools/bench_resample.py [--n 64] [--seconds 10] [--reps 20] [--out profiles/resample_bench.json]

Times are device-event times around `reps` back-to-back calls, per call: for the resample and filterbank entries that is the
kernel plus the call's own upload of offsets / clip descriptors, which the host waits for -- a floor of about 68 us per call
on the box of profiles/resample_experiments.txt, above the 48 kHz kernel's 42 us.  Run the tool under `rocprofv3
--kernel-trace --stats` for the bare kernels (`resample_batch_kernel`, `fbank_batch_kernel`).  GB/s counts the samples read
once and the samples written once, over the call time."""
import argparse
import ctypes as C
import json
import math
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from sonar_amd import _lib  # noqa: E402
from sonar_amd.resample import resample_batch_flat  # noqa: E402
from sonar_amd.speech_encoder import SonarSpeechEncoderModel, fbank_batch_flat, get_speech_encoder_config  # noqa: E402


def timed(fn, reps):
    fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / reps * 1e3  # us


def synthetic_speech(rate, seconds, seed=7):
    """A band-limited signal (40 partials below 7 kHz under a slow envelope) evaluated at `rate`: the same waveform at any
    sample rate above 14 kHz."""
    g = torch.Generator().manual_seed(seed)
    freqs = torch.rand(40, generator=g, dtype=torch.float64) * 6900 + 80
    amps = torch.rand(40, generator=g, dtype=torch.float64) / (1 + freqs / 500)
    phases = torch.rand(40, generator=g, dtype=torch.float64) * 2 * math.pi
    t = torch.arange(int(rate * seconds), dtype=torch.float64) / rate
    x = (amps[:, None] * torch.sin(2 * math.pi * freqs[:, None] * t[None, :] + phases[:, None])).sum(0)
    x = x * (0.6 + 0.4 * torch.sin(2 * math.pi * 3.1 * t))
    return (x / 8).float()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=64)
    ap.add_argument("--seconds", type=float, default=10.0)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out", default=os.path.join("profiles", "resample_bench.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise RuntimeError("bench_resample needs an MI355X: nothing here is measured on a CPU")
    dev = "cuda:0"
    from tools.synth import speech_encoder_state_dict

    model = SonarSpeechEncoderModel(get_speech_encoder_config("english"), speech_encoder_state_dict(dev), device=dev,
                                    dtype=torch.float16)
    eng = model.engine
    lib = _lib.load()
    n = args.n
    result = {"clips": n, "seconds": args.seconds, "reps": args.reps, "device": torch.cuda.get_device_name(0), "rates": {}}
    for rate in (48000, 44100):
        per = int(rate * args.seconds)
        cat = torch.rand(n * per, device=dev, generator=torch.Generator(device=dev).manual_seed(rate)) * 2 - 1
        offs = [i * per for i in range(n + 1)]
        out, out_offs = resample_batch_flat(cat, offs, rate)
        t_rs = timed(lambda: resample_batch_flat(cat, offs, rate), args.reps)
        feats, lens = fbank_batch_flat(out, out_offs)
        t_fb = timed(lambda: fbank_batch_flat(out, out_offs), args.reps)
        raw = torch.empty_like(feats)
        arr = (C.c_int64 * (n + 1))(*out_offs)

        def fbank_kernel_only():
            _lib.check(lib.smi_fbank_batch(out.data_ptr(), arr, n, 2.0 ** 15, 0, raw.data_ptr(), feats.shape[1],
                                           _lib.current_stream_ptr()))

        t_fk = timed(fbank_kernel_only, args.reps)
        t_enc = timed(lambda: eng.forward(feats, None, torch.float16), max(3, args.reps // 4))
        nbytes = 4 * (cat.numel() + out.numel())
        result["rates"][str(rate)] = {
            "samples_in": cat.numel(), "samples_out": out.numel(), "bytes_moved": nbytes,
            "resample_call_us": round(t_rs, 1), "resample_gb_per_s": round(nbytes / t_rs * 1e-3, 1),
            "fbank_batch_kernel_call_us": round(t_fk, 1), "fbank_with_standardize_call_us": round(t_fb, 1),
            "encoder_forward_us": round(t_enc, 1), "frames_per_clip": lens[0],
        }
        print(f"{rate} Hz -> 16 kHz, {n} x {args.seconds:g} s: resample {t_rs:.1f} us ({nbytes / t_rs * 1e-3:.0f} GB/s), "
              f"fbank_batch_kernel {t_fk:.1f} us, fbank + standardise {t_fb:.1f} us, encoder forward {t_enc / 1e3:.2f} ms")
        del cat, out, feats, raw

    # the same signal at 16 kHz and at 48 kHz through the pipeline
    from sonar_amd.inference_pipelines import SpeechToEmbeddingModelPipeline

    pipe = SpeechToEmbeddingModelPipeline(model, device=torch.device(dev), fbank_dtype=torch.float16)
    e16 = pipe.predict([synthetic_speech(16000, args.seconds)], batch_size=1).float()
    e48 = pipe.predict([(synthetic_speech(48000, args.seconds), 48000)], batch_size=1, resample=True).float()
    cos = torch.nn.functional.cosine_similarity(e16, e48, dim=-1).item()
    result["one_minus_cos_16k_vs_48k_resampled"] = 1 - cos
    print(f"1 - cos(embedding of the 16 kHz clip, embedding of its 48 kHz rendition through resample=True) = {1 - cos:.3e}")
    print(json.dumps(result))
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        json.dump(result, fh, indent=1)
        fh.write("\n")


if __name__ == "__main__":
    main()
