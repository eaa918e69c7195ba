#!/usr/bin/env python
"""Timing of BackboneEngine.score at NeuTTS-Air geometry (profiles/score_bench.txt): `--seqs` sequences of `--len` tokens scored from `--from`,
next to the plain prompt pass over the same tokens on the same engine, the lm_head share of it and the scratch the first score call allocates.

    python tools/score_bench.py [--seqs 256] [--len 750] [--from 500] [--slots 64] [--repeats 3]

The lm_head part (final norm over the scored rows, the chunked lm_head launches, the merge) is taken as the difference between scoring from `--from`
and scoring the last token only (one row per sequence), same prompt pass: rows x V x H x 2 FLOP over that time.  Host clocks around blocking calls."""
import argparse
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "neutts-air_amd")):
    sys.path.insert(0, p)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--seqs", type=int, default=256)
    ap.add_argument("--len", type=int, default=750)
    ap.add_argument("--from", dest="score_from", type=int, default=500)
    ap.add_argument("--slots", type=int, default=64, help="decode slots of the engine = sequences per score call")
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--chunk-rows", type=int, default=0)
    ap.add_argument("--fp8", action="store_true")
    a = ap.parse_args()
    import importlib.util
    import torch
    import synthetic as syn
    from neutts import _hip
    spec = importlib.util.spec_from_file_location("ntts_build", os.path.join(ROOT, "neutts-air_amd", "build.py"))
    bmod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(bmod)
    lib = bmod.build(verbose=False)
    cfg = syn.BackboneConfig.neutts_air()
    V, H = cfg.vocab_size, cfg.hidden_size
    eng = _hip.BackboneEngine(dict(vocab_size=V, hidden_size=H, intermediate_size=cfg.intermediate_size, num_layers=cfg.num_layers,
                                   num_heads=cfg.num_heads, num_kv_heads=cfg.num_kv_heads, rms_eps=cfg.rms_eps,
                                   max_context=((a.len + 1 + 31) // 32) * 32, max_batch=a.slots, max_prefill_tokens=a.slots * a.len,
                                   weight_dtype="fp8" if a.fp8 else "bf16"), 0, lib)
    eng.load_state_dict({k: v.numpy() for k, v in syn.make_weights(cfg, 0).items()}, inv_freq=syn.rope_inv_freq(cfg).numpy(),
                        input_scales=syn.default_fp8_input_scales(cfg) if a.fp8 else None)
    seqs = [syn.synthetic_prompt(cfg, i, a.len) for i in range(a.seqs)]
    rows = a.seqs * (a.len - a.score_from)

    def prompt_pass():
        for i in range(0, a.seqs, a.slots):
            part = seqs[i:i + a.slots]
            slots = list(range(len(part)))
            eng.prefill(part, slots, [_hip.Sampling(max_length=a.len + 1, min_new_tokens=1, eos_token_id=V - 1, do_sample=False) for _ in part])
            eng.sync()
            eng.release_many(slots)
        eng.sync()

    def timed(fn):
        ts = []
        for _ in range(a.repeats):
            t0 = time.perf_counter()
            fn()
            ts.append(time.perf_counter() - t0)
        return ts

    prompt_pass()                                                    # warm-up of the prompt-pass kernels
    free0 = torch.cuda.mem_get_info()[0]
    eng.score(seqs[:a.slots], a.score_from, a.chunk_rows)            # first call: allocates the scratch, loads the scoring kernels
    scratch = free0 - torch.cuda.mem_get_info()[0]
    t_pp = timed(prompt_pass)
    t_full = timed(lambda: eng.score(seqs, a.score_from, a.chunk_rows))
    t_last = timed(lambda: eng.score(seqs, a.len - 1, a.chunk_rows))
    eng.close()
    fmt = lambda ts: f"min {min(ts) * 1e3:9.1f} ms  (all: " + ", ".join(f"{t * 1e3:.1f}" for t in ts) + ")"
    head = min(t_full) - min(t_last)
    print(f"# NeuTTS-Air geometry {'fp8' if a.fp8 else 'bf16'}: {a.seqs} sequences x {a.len} tokens scored from {a.score_from} = {rows} scored rows; "
          f"{a.slots} sequences ({a.slots * a.len} tokens) per call, chunk_rows = {a.chunk_rows or 'default (2048)'}")
    print(f"plain prompt pass over the same tokens (prefill + first token, {a.slots} prompts per call): {fmt(t_pp)}")
    print(f"score from {a.score_from} ({rows} rows):                         {fmt(t_full)}")
    print(f"score of the last token only ({a.seqs} rows):                {fmt(t_last)}")
    print(f"lm_head part (difference of the two minima): {head * 1e3:.1f} ms for {rows - a.seqs} rows x V {V} x H {H} x 2 FLOP = "
          f"{(rows - a.seqs) * V * H * 2 / head / 1e15:.3f} PFLOP/s")
    print(f"device memory taken by the first score call (partials of one chunk, row lists, outputs): {scratch / 2 ** 20:.1f} MiB")


if __name__ == "__main__":
    main()
