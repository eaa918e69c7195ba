#!/usr/bin/env python
"""The streaming workload of `bench.py --config nano-fp8 --mode stream` (512 concurrent streams of the fp8 Nano-sized model, 500 prompt + 250
generated tokens each, NeuCodec geometry) through NeuTTS._infer_stream_batch_hip in three chunk formats (profiles/stream_format_bench.txt):
24 kHz float32 (the native format: the launches of an instance without the stage), 16 kHz PCM16 and 8 kHz mu-law (the chunked output stage,
kernels/codec.h wav_stream_kernel, behind the cross-fade: one more launch per pump round, two when streams finish in it).

    python tools/bench_stream_format.py [--batch 512] [--prefill 500] [--decode 250] [--repeats 3] [--tiny]

Per format: codec tokens/s over the whole pass, time to first audio (first / median / last stream), and the bytes a chunk costs on the D2H copy
(its row of the page-locked buffer) next to the bytes it holds."""
import argparse
import contextlib
import math
import os
import sys
import time

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

FORMATS = [(24000, "f32"), (16000, "pcm16"), (8000, "mulaw")]
ESIZE = {"f32": 4, "pcm16": 2, "mulaw": 1}


def row_elements(longest_chunk: int, rate: int, W: int) -> int:
    """Elements of one chunk's row in the set's output buffer (csrc/codec.cpp wav_core_create)."""
    if rate == 24000:
        return longest_chunk
    g = math.gcd(24000, rate)
    orig, new = 24000 // g, rate // g
    width = math.ceil(W * orig / (min(orig, new) * 0.99))
    return -(-(longest_chunk + 2 * width + orig) * new // orig) + new


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--batch", type=int, default=512)
    ap.add_argument("--prefill", type=int, default=500)
    ap.add_argument("--decode", type=int, default=250)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--filter-width", type=int, default=6)
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
    hop = ccfg.hop_length
    longest = (tts.streaming_frames_per_chunk + tts.streaming_lookforward + tts.streaming_overlap_frames) * hop      # csrc/stream.cpp out_stride

    def one_pass(fmt):
        torch.cuda.synchronize()
        t1 = time.time()
        first, n_chunks, n_elem = {}, 0, 0
        for i, chunk in tts._infer_stream_batch_hip([list(p) for p in prompts], refs, None, fmt):
            first.setdefault(i, (time.time() - t1) * 1e3)
            n_chunks += 1
            n_elem += len(chunk)
        total = time.time() - t1
        tt = np.array(sorted(first.values()))
        return B * N / total, (float(tt[0]), float(np.median(tt)), float(tt[-1])), n_chunks, n_elem

    print(f"# {B} streams x ({S} prompt + {N} generated tokens), {'tiny models' if a.tiny else 'fp8 Nano-sized backbone, NeuCodec geometry'}, one engine, "
          f"device stream path; {a.repeats} passes per format after {a.warmup} warm-up, filter width {a.filter_width}")
    for rate, enc in FORMATS:
        fmt = None if (rate == 24000 and enc == "f32") else (rate, enc, a.filter_width)
        runs = [one_pass(fmt) for _ in range(a.warmup + a.repeats)][a.warmup:]
        tps = [r[0] for r in runs]
        ttfa = np.median(np.array([r[1] for r in runs]), axis=0)
        n_chunks, n_elem = runs[-1][2], runs[-1][3]
        row = row_elements(longest, rate, a.filter_width) * ESIZE[enc]
        print(f"{enc:5s} {rate:5d} Hz: {np.mean(tps) / 1e3:7.1f} k codec-tokens/s [{min(tps) / 1e3:.1f} .. {max(tps) / 1e3:.1f}]   first audio "
              f"{ttfa[0]:6.1f} / {ttfa[1]:6.1f} / {ttfa[2]:6.1f} ms (first / median / last stream)   D2H {row:6d} bytes per chunk row, "
              f"{n_elem * ESIZE[enc] / n_chunks:8.1f} bytes of samples per chunk ({n_chunks} chunks)   "
              f"launches added per pump round: {0 if fmt is None else '1 (2 in a round with final windows)'}")


if __name__ == "__main__":
    main()
