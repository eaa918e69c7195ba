#!/usr/bin/env python
"""The streaming workload of `bench.py --config nano-fp8 --mode stream` (512 concurrent streams of the fp8 Nano-sized model, 500 prompt + 250
generated tokens each, NeuCodec geometry) through NeuTTS._infer_stream_batch_hip at several stream speeds (profiles/stream_speed_bench.txt): 1.0 (the
launches of an instance without the stage) and, by default, 0.8 and 1.25 (the chunked time stretch, kernels/codec.h wav_stretch_stream_kernel, behind
the cross-fade: one more launch per pump round, two when streams finish in it).

    python tools/bench_stream_speed.py [--speeds 1.0 0.8 1.25] [--batch 512] [--prefill 500] [--decode 250] [--repeats 3] [--tiny]

Per speed: codec tokens/s over the whole pass, time to first audio (first / median / last stream; a chunk without samples is not audio), the samples a
stream received, the frames the search walked and the v_sad_u16 operation floor of that search on the whole device.  The kernel's own time comes from
a run of its own under the profiler, which this tool does not start:

    rocprofv3 --kernel-trace --stats -d <dir> -- python tools/bench_stream_speed.py --speeds 0.8 --repeats 1 --warmup 0

(wav_stretch_stream_kernel's row of the kernel statistics: calls = pump launches, average = time per launch)."""
import argparse
import contextlib
import os
import sys
import time

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOP, CAND = 360, 481                   # kernels/codec.h kStretchHop, kStretchCand
CUS, DIFFS_PER_CLOCK, GHZ = 256, 256, 2.4      # MI355X; per CU 4 SIMDs x 32 lanes per clock x the 2 differences of one v_sad_u16


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--speeds", type=float, nargs="+", default=[1.0, 0.8, 1.25])
    ap.add_argument("--batch", type=int, default=512)
    ap.add_argument("--prefill", type=int, default=500)
    ap.add_argument("--decode", type=int, default=250)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--tiny", action="store_true", help="tiny models (a plumbing check, not a measurement)")
    a = ap.parse_args()
    for p in (HERE, os.path.join(HERE, "neutts-air_amd")):
        sys.path.insert(0, p)
    import importlib.util
    import numpy as np
    import torch
    import synthetic as syn
    from neutts import NeuTTS
    spec = importlib.util.spec_from_file_location("ntts_build", os.path.join(HERE, "neutts-air_amd", "build.py"))
    bmod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(bmod)
    lib = bmod.build(verbose=False)
    B, S, N = a.batch, a.prefill, a.decode
    cfg = syn.BackboneConfig.tiny(vocab_size=512, num_layers=1) if a.tiny else syn.BackboneConfig.neutts_nano_like(142080)
    ccfg = syn.CodecConfig.tiny() if a.tiny else syn.CodecConfig.neucodec()
    fp8 = not a.tiny
    n_codes = int(np.prod(ccfg.levels))
    eos = cfg.vocab_size - 1
    w, cw = syn.make_weights(cfg, 0), syn.make_codec_weights(ccfg, 0)
    with contextlib.redirect_stdout(sys.stderr):
        tts = NeuTTS(
            backbone_repo={"config": dict(vocab_size=cfg.vocab_size, hidden_size=cfg.hidden_size, intermediate_size=cfg.intermediate_size,
                                          num_layers=cfg.num_layers, num_heads=cfg.num_heads, num_kv_heads=cfg.num_kv_heads, rms_eps=cfg.rms_eps,
                                          max_context=((S + N + 31) // 32) * 32, max_prefill_tokens=64 * S, weight_dtype="fp8" if fp8 else "bf16"),
                           "state_dict": {k: v.numpy() for k, v in w.items()}, "inv_freq": syn.rope_inv_freq(cfg).numpy(),
                           "input_scales": syn.default_fp8_input_scales(cfg) if fp8 else None, "tokenizer": None, "speech_base": 0, "eos_token_id": eos},
            backbone_device="cuda:0",
            codec_repo={"config": dict(hidden_size=ccfg.hidden_size, intermediate_size=ccfg.intermediate_size, num_layers=ccfg.num_layers,
                                       num_heads=ccfg.num_heads, quantization_dim=ccfg.quantization_dim, levels=list(ccfg.levels),
                                       hop_length=ccfg.hop_length, rms_eps=ccfg.rms_eps, max_frames=128, max_rows=B * 96),
                        "state_dict": {k: v.numpy() for k, v in cw.items()}},
            codec_device="cuda:0", do_sample=False, max_batch=B, lib_path=lib)
    tts.watermarker = None
    tts._ids_to_codes = lambda ids: [int(i) % n_codes for i in ids]          # random weights do not stay in the speech range (as bench.py)
    tts._stream_modulo = n_codes
    tts._ids_to_codes_array = lambda ids: (np.asarray(ids, dtype=np.int64) % n_codes).astype(np.int32)
    tts.min_new_tokens, tts.max_context = N, S + N
    prompts = [syn.synthetic_prompt(cfg, 1234 + i, S) for i in range(B)]
    refs = [[int(t) % n_codes for t in p[-372:]] for p in prompts]

    def one_pass(spd):
        torch.cuda.synchronize()
        t1 = time.time()
        first, n_chunks, n_empty, n_samp = {}, 0, 0, 0
        for i, chunk in tts._infer_stream_batch_hip([list(p) for p in prompts], refs, None, None, spd):
            if len(chunk):
                first.setdefault(i, (time.time() - t1) * 1e3)
            n_chunks += 1
            n_empty += 0 if len(chunk) else 1
            n_samp += len(chunk)
        total = time.time() - t1
        tt = np.array(sorted(first.values()))
        return B * N / total, (float(tt[0]), float(np.median(tt)), float(tt[-1])), n_chunks, n_empty, n_samp

    print(f"# {B} streams x ({S} prompt + {N} generated tokens), {'tiny models' if a.tiny else 'fp8 Nano-sized backbone, NeuCodec geometry'}, one engine, "
          f"device stream path, 24 kHz float32 chunks; {a.repeats} passes per speed after {a.warmup} warm-up")
    for speed in a.speeds:
        spd = None if round(speed * 1000) == 1000 else [float(speed)] * B
        runs = [one_pass(spd) for _ in range(a.warmup + a.repeats)][a.warmup:]
        tps = [r[0] for r in runs]
        ttfa = np.median(np.array([r[1] for r in runs]), axis=0)
        n_chunks, n_empty, n_samp = runs[-1][2:]
        line = (f"stream_speed {speed:4.2f}: {np.mean(tps) / 1e3:7.1f} k codec-tokens/s [{min(tps) / 1e3:.1f} .. {max(tps) / 1e3:.1f}]   first audio "
                f"{ttfa[0]:6.1f} / {ttfa[1]:6.1f} / {ttfa[2]:6.1f} ms (first / median / last stream)   {n_samp / B:9.1f} samples per stream in "
                f"{n_chunks} chunks ({n_empty} empty)")
        if spd is not None:
            frames = (n_samp / B + HOP - 1) // HOP - 1                    # searched frames per stream: every frame but the first
            floor_ms = B * frames * CAND * HOP / (CUS * DIFFS_PER_CLOCK * GHZ * 1e9) * 1e3
            line += f"   search: {int(frames)} frames per stream, operation floor {floor_ms:.4f} ms per pass on {CUS} CUs"
        print(line, flush=True)


if __name__ == "__main__":
    main()
