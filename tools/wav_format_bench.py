#!/usr/bin/env python
"""Timing of the codec's device output stage (include/neutts_hip.h ntts_wav_format) at NeuCodec geometry (profiles/wav_format_bench.txt): one
codec pass over `--utts` utterances of `--frames` frames per output format, GPU milliseconds of ntts_codec_last_timing (hipEvents around the
pass, output stage included, H2D / D2H excluded), median of `--repeats` passes with the spread next to it.

    python tools/wav_format_bench.py [--utts 256] [--frames 250] [--repeats 7]
    python tools/wav_format_bench.py --plain-only [--root <another checkout>]

The F32 / 24 kHz row goes through the plain entry point and launches exactly what an engine without the output stage launches; --plain-only
prints that row alone and touches nothing the output stage added, so that with --root it runs on a checkout from before it (the parent commit's
figure on the first line of the profile).  Every other row is the same pass plus wav_format_kernel.  The stage is also timed ALONE, through
CodecEngine.convert_array on `--utts` host waveforms of `--frames` x hop samples (the same events, around the one kernel): that figure, as a share of
the pass, is the stage's cost -- the difference between two whole passes is smaller than their run-to-run spread -- next to the bytes the D2H copy
moves in that format."""
import argparse
import os
import sys

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

ROWS = [("f32", 24000, 6), ("pcm16", 24000, 6), ("pcm16", 16000, 6), ("mulaw", 8000, 6), ("f32", 48000, 6), ("mulaw", 8000, 16)]
ESIZE = {"f32": 4, "pcm16": 2, "mulaw": 1}


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--utts", type=int, default=256)
    ap.add_argument("--frames", type=int, default=250)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--plain-only", action="store_true", help="the F32 / 24 kHz row alone, through the plain entry point")
    ap.add_argument("--root", default=HERE, help="checkout whose package and library are measured (default: this one)")
    a = ap.parse_args()
    root = os.path.abspath(a.root)
    for p in (root, os.path.join(root, "neutts-air_amd")):
        sys.path.insert(0, p)
    import importlib.util
    import numpy as np
    import synthetic as syn
    from neutts import _hip
    spec = importlib.util.spec_from_file_location("ntts_build", os.path.join(root, "neutts-air_amd", "build.py"))
    bmod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(bmod)
    lib = bmod.build(verbose=False)
    ccfg = syn.CodecConfig.neucodec()
    n, T, hop = a.utts, a.frames, ccfg.hop_length
    eng = _hip.CodecEngine(dict(hidden_size=ccfg.hidden_size, intermediate_size=ccfg.intermediate_size, num_layers=ccfg.num_layers,
                                num_heads=ccfg.num_heads, quantization_dim=ccfg.quantization_dim, levels=list(ccfg.levels), hop_length=hop,
                                rms_eps=ccfg.rms_eps, max_frames=max(T, 256), max_rows=n * (T + 6)), 0, lib)
    eng.load_state_dict({k: v.numpy() for k, v in syn.make_codec_weights(ccfg, 0).items()})
    codes = np.random.default_rng(0).integers(0, int(np.prod(ccfg.levels)), size=(n, T)).astype(np.int32)

    def measure(**fmt):
        ms = []
        for i in range(a.warmup + a.repeats):
            wav = eng.decode_array(codes, reuse_output=True, **fmt)
            if i >= a.warmup:
                ms.append(eng.last_timing())
        return float(np.median(ms)), min(ms), max(ms), wav

    print(f"# {n} utterances x {T} frames ({n * T * hop / 1e6:.1f} M samples at 24 kHz), NeuCodec geometry, fp16 operands; GPU ms of one codec pass "
          f"(ntts_codec_last_timing), median of {a.repeats} [min .. max]")
    base, lo, hi, wav = measure()
    tag = "plain entry point" + (f", checkout {os.path.basename(root)}" if a.plain_only else "")
    print(f"f32   24000 Hz W  6 ({tag}): {base:8.3f} ms [{lo:.3f} .. {hi:.3f}]   D2H {wav.nbytes / 1e6:7.1f} MB")
    if a.plain_only:
        return
    x = np.random.default_rng(1).uniform(-1, 1, size=(n, T * hop)).astype(np.float32)
    n_samples = np.full(n, T * hop, dtype=np.int32)

    def stage_alone(**fmt):
        ms = []
        for i in range(a.warmup + a.repeats):
            eng.convert_array(x, n_samples, **fmt)
            if i >= a.warmup:
                ms.append(eng.last_timing())
        return float(np.median(ms)), min(ms), max(ms)

    for enc, rate, W in ROWS[1:]:
        fmt = dict(sample_rate=rate, encoding=enc, filter_width=W)
        med, lo, hi, wav = measure(**fmt)
        st, slo, shi = stage_alone(**fmt)
        samples = n * _hip.wav_out_len(T * hop, rate)
        assert wav.nbytes == samples * ESIZE[enc]
        print(f"{enc:5s} {rate:5d} Hz W {W:2d}: {med:8.3f} ms [{lo:.3f} .. {hi:.3f}]   output stage alone {st:6.3f} ms [{slo:.3f} .. {shi:.3f}] = "
              f"{100 * st / med:4.2f} % of the pass, {samples / st / 1e6:6.1f} G output samples/s   D2H {wav.nbytes / 1e6:7.1f} MB")
    again, lo, hi, _ = measure()
    print(f"f32   24000 Hz W  6 (plain entry point, measured again at the end): {again:8.3f} ms [{lo:.3f} .. {hi:.3f}]")


if __name__ == "__main__":
    main()
