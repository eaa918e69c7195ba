#!/usr/bin/env python
"""Timing of loudness= (the codec's BS.1770 loudness normalisation, include/neutts_hip.h ntts_codec_decode_loud) at NeuCodec geometry
(profiles/loudness_bench.txt): one codec pass over `--utts` utterances of `--frames` frames on the synthetic workload, GPU milliseconds of
ntts_codec_last_timing (hipEvents around the pass, the loudness stage included, H2D / D2H excluded), median of `--repeats` passes with the spread
next to it.

    python tools/bench_loudness.py [--utts 256] [--frames 250] [--repeats 7]
    python tools/bench_loudness.py --plain-only [--root <another checkout>]

--plain-only prints the pass with the option off alone, through the plain entry point, and touches nothing this stage added, so that with --root it
runs on a checkout from before it: run it on this commit and on the parent in turn, a fresh process each, three runs each, and compare the default
with the parent's own run-to-run spread.  Without it: that row, then the pass with loudness=-16 and the two kernels' own times
(ntts_codec_last_loudness_timing: hipEvents around wav_loud_measure_kernel and around wav_loud_apply_kernel), their share of the pass, and the
measure kernel's time over its byte floor.  The floor: one read of the waveform, utterances x frames x hop x 4 bytes, at --hbm-tbs TB/s (the
kernel itself reads every sample twice, once to warm the filters of the next sub-block: the second read is expected to come from the cache)."""
import argparse
import os
import sys

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--utts", type=int, default=256)
    ap.add_argument("--frames", type=int, default=250)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--target", type=float, default=-16.0)
    ap.add_argument("--hbm-tbs", type=float, default=8.0, help="memory bandwidth the byte floor is taken at, TB/s (MI355X: 8)")
    ap.add_argument("--plain-only", action="store_true", help="the pass with the option off alone, through the plain entry point")
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
    rows = [codes[i] for i in range(n)]

    def measure(loud):
        ms, parts = [], []
        for i in range(a.warmup + a.repeats):
            if loud:
                eng.decode(rows, reuse_output=True, loudness=a.target)
            else:
                eng.decode_array(codes, reuse_output=True)
            if i >= a.warmup:
                ms.append(eng.last_timing())
                if loud:
                    parts.append(eng.last_loudness_timing())
        return float(np.median(ms)), min(ms), max(ms), parts

    print(f"# {n} utterances x {T} frames ({n * T * hop / 1e6:.1f} M samples at 24 kHz), NeuCodec geometry, fp16 operands; GPU ms of one codec pass "
          f"(ntts_codec_last_timing), median of {a.repeats} [min .. max]")
    base, lo, hi, _ = measure(False)
    tag = "plain entry point" + (f", checkout {os.path.basename(root)}" if a.plain_only else "")
    print(f"loudness off ({tag}): {base:8.3f} ms [{lo:.3f} .. {hi:.3f}]")
    if a.plain_only:
        return
    via, lo, hi, _ = measure_list_off(eng, rows, a, np)
    print(f"loudness off (decode() of a list, the call the next row makes): {via:8.3f} ms [{lo:.3f} .. {hi:.3f}]")
    med, lo, hi, parts = measure(True)
    me = float(np.median([p[0] for p in parts]))
    ap_ = float(np.median([p[1] for p in parts]))
    floor = n * T * hop * 4 / (a.hbm_tbs * 1e12) * 1e3
    g = eng.decode(rows[:4], loudness=a.target)
    m = eng.measure_loudness(g)
    print(f"loudness {a.target:g}: {med:8.3f} ms [{lo:.3f} .. {hi:.3f}]   measure {me:7.3f} ms [{min(p[0] for p in parts):.3f} .. {max(p[0] for p in parts):.3f}]"
          f" = {100 * me / med:5.2f} % of the pass, apply {ap_:6.3f} ms [{min(p[1] for p in parts):.3f} .. {max(p[1] for p in parts):.3f}]"
          f" = {100 * ap_ / med:5.2f} %   measure byte floor {floor:6.4f} ms: {me / floor:6.1f} x the floor")
    print(f"# (the first four utterances, measured again behind the gain: {', '.join(f'{v:.2f}' for v in m[:, 0])} LUFS, peaks {', '.join(f'{v:.3f}' for v in m[:, 1])})")
    again, lo, hi, _ = measure(False)
    print(f"loudness off (plain entry point, measured again at the end): {again:8.3f} ms [{lo:.3f} .. {hi:.3f}]")


def measure_list_off(eng, rows, a, np):
    ms = []
    for i in range(a.warmup + a.repeats):
        eng.decode(rows, reuse_output=True)
        if i >= a.warmup:
            ms.append(eng.last_timing())
    return float(np.median(ms)), min(ms), max(ms), None


if __name__ == "__main__":
    main()
