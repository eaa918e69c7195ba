#!/usr/bin/env python
"""Timing of speed= (the codec's pitch-preserving time stretch, include/neutts_hip.h ntts_codec_decode_speed) at NeuCodec geometry
(profiles/speed_bench.txt): one codec pass over `--utts` utterances of `--frames` frames, GPU milliseconds of ntts_codec_last_timing (hipEvents
around the pass, the stretch and the output stage included, H2D / D2H excluded), median of `--repeats` passes with the spread next to it.

    python tools/bench_speed.py [--utts 256] [--frames 250] [--repeats 7]
    python tools/bench_speed.py --plain-only [--root <another checkout>]

--plain-only prints the speed-1.0 pass alone, through the plain entry point, and touches nothing this stage added, so that with --root it runs on a
checkout from before it: run it on this commit and on the parent in turn, a fresh process each, and compare the default with the parent's own
run-to-run spread.  Without it: that row, then the pass at 0.8 and 1.25 with the two kernels' own times (ntts_codec_last_stretch_timing: hipEvents
around wav_stretch_search_kernel and wav_stretch_render_kernel), and the search's time over its operation floor.  The floor: K - 1 searched frames per
utterance x candidates x 360 absolute differences, counted from the shapes, on one CU per utterance (one workgroup walks an utterance's frames in
order) at 256 absolute differences per clock per CU -- 4 SIMDs x 32 lanes per clock x the 2 differences of one v_sad_u16 -- at 2.4 GHz."""
import argparse
import os
import sys

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HS, DELTA, WIN = 360, 240, 720


def search_floor_ms(n_in: int, pm: int) -> float:
    """Operation floor of one utterance's search (utterances run side by side, one CU each, while there are CUs)."""
    n_out = -(-n_in * 1000 // pm)
    frames = -(-n_out // HS)
    pmax = max(0, n_in - WIN)
    diffs = 0
    for k in range(1, frames):
        a = (k * HS * pm + 500) // 1000
        lo, hi = min(max(a - DELTA, 0), pmax), min(max(a + DELTA, 0), pmax)
        diffs += (hi - lo + 1) * HS
    return diffs / 256.0 / 2.4e9 * 1e3


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--utts", type=int, default=256)
    ap.add_argument("--frames", type=int, default=250)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--plain-only", action="store_true", help="the speed-1.0 pass alone, through the plain entry point")
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

    def measure(**kw):
        ms, parts = [], []
        for i in range(a.warmup + a.repeats):
            eng.decode_array(codes, reuse_output=True, **kw)
            if i >= a.warmup:
                ms.append(eng.last_timing())
                if kw:
                    parts.append(eng.last_stretch_timing())
        return float(np.median(ms)), min(ms), max(ms), parts

    print(f"# {n} utterances x {T} frames ({n * T * hop / 1e6:.1f} M samples at 24 kHz), NeuCodec geometry, fp16 operands; GPU ms of one codec pass "
          f"(ntts_codec_last_timing), median of {a.repeats} [min .. max]")
    base, lo, hi, _ = measure()
    tag = "plain entry point" + (f", checkout {os.path.basename(root)}" if a.plain_only else "")
    print(f"speed 1.00 ({tag}): {base:8.3f} ms [{lo:.3f} .. {hi:.3f}]")
    if a.plain_only:
        return
    for speed in (0.8, 1.25):
        med, lo, hi, parts = measure(speed=speed)
        se = float(np.median([p[0] for p in parts]))
        re = float(np.median([p[1] for p in parts]))
        floor = search_floor_ms(T * hop, int(round(speed * 1000)))
        print(f"speed {speed:4.2f}: {med:8.3f} ms [{lo:.3f} .. {hi:.3f}]   search {se:7.3f} ms [{min(p[0] for p in parts):.3f} .. {max(p[0] for p in parts):.3f}]"
              f" = {100 * se / med:5.2f} % of the pass, render {re:6.3f} ms [{min(p[1] for p in parts):.3f} .. {max(p[1] for p in parts):.3f}]"
              f"   search floor {floor:6.3f} ms: {se / floor:5.1f} x the floor")
    again, lo, hi, _ = measure()
    print(f"speed 1.00 (plain entry point, measured again at the end): {again:8.3f} ms [{lo:.3f} .. {hi:.3f}]")


if __name__ == "__main__":
    main()
