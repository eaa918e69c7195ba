#!/usr/bin/env python
"""What the nucleus / min-p stage of the device sampler costs per decode step: a 256-slot engine at NeuTTS-Air geometry stepped with
(a) the default sampling call (top_k 50, temperature 1.0), (b) top_p 0.95 / min_p 0.05 behind top_k 50, (c) top_k 512 alone and (d) with
top_p 0.95 / min_p 0.05 behind it (the candidate list full: the worst case of the stage's one-thread walk, next to what top_k 512 costs by itself).  Meant to run under the profiler, once:

    rocprofv3 --kernel-trace --stats -f csv -d DIR -o nucleus -- python tools/probe_nucleus_cost.py
    python tools/probe_nucleus_cost.py --summarise DIR        # sample_greedy_kernel's average per setting, from the kernel trace

Every setting launches the sampling kernel the same number of times (prompt passes + decode steps), in order; the summary splits the
kernel's dispatches of the trace into that many equal runs and averages the decode-step launches of each."""
import argparse
import csv
import glob
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "neutts-air_amd")):
    sys.path.insert(0, p)

SETTINGS = [("default top_k 50", dict(top_k=50)), ("top_k 50, top_p 0.95, min_p 0.05", dict(top_k=50, top_p=0.95, min_p=0.05)),
            ("top_k 512", dict(top_k=512)), ("top_k 512, top_p 0.95, min_p 0.05", dict(top_k=512, top_p=0.95, min_p=0.05))]
CHUNK = 64          # prompts per prompt pass


def summarise(d, batch, steps):
    rows = []
    for f in glob.glob(os.path.join(d, "**", "*kernel_trace.csv"), recursive=True):
        with open(f) as fh:
            for row in csv.DictReader(fh):
                if "sample_greedy_kernel" in row.get("Kernel_Name", ""):
                    rows.append((int(row["Start_Timestamp"]), int(row["End_Timestamp"])))
    rows.sort()
    per = (batch + CHUNK - 1) // CHUNK + steps
    if len(rows) != per * len(SETTINGS):
        raise SystemExit(f"{len(rows)} sample_greedy_kernel dispatches in the trace, expected {per * len(SETTINGS)}")
    base = None
    for i, (name, _) in enumerate(SETTINGS):
        dec = rows[i * per + per - steps:(i + 1) * per]              # the decode steps of this setting: all `batch` rows draw
        us = sum(b - a for a, b in dec) / len(dec) / 1e3
        base = base or us
        print(f"sample_greedy_kernel, {batch} rows, {name}: {us:.2f} us average over {len(dec)} decode steps ({us / base:.3f} x default)")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--prefill", type=int, default=64)
    ap.add_argument("--steps", type=int, default=40)
    ap.add_argument("--summarise", metavar="DIR", default=None)
    a = ap.parse_args()
    if a.summarise:
        return summarise(a.summarise, a.batch, a.steps)
    import torch
    from neutts import _hip
    import synthetic as syn
    cfg = syn.BackboneConfig.neutts_air(217488)
    w = {k: v.to(torch.bfloat16).cuda() for k, v in syn.make_weights(cfg, 0).items()}
    B, S, N = a.batch, a.prefill, a.steps
    eng = _hip.BackboneEngine(dict(vocab_size=cfg.vocab_size, hidden_size=cfg.hidden_size, intermediate_size=cfg.intermediate_size,
                                   num_layers=cfg.num_layers, num_heads=cfg.num_heads, num_kv_heads=cfg.num_kv_heads, rms_eps=cfg.rms_eps,
                                   max_context=256, max_batch=B, max_prefill_tokens=CHUNK * S), 0)
    eng.load_state_dict(w, inv_freq=syn.rope_inv_freq(cfg).numpy())
    prompts = [syn.synthetic_prompt(cfg, i, S) for i in range(B)]
    for name, kw in SETTINGS:
        sp = [_hip.Sampling(max_length=S + N + 1, min_new_tokens=N + 1, eos_token_id=cfg.vocab_size - 1, do_sample=True, temperature=1.0,
                            seed=1 + i, **kw) for i in range(B)]
        for c in range(0, B, CHUNK):
            eng.prefill(prompts[c:c + CHUNK], list(range(c, min(c + CHUNK, B))), sp[c:c + CHUNK])
        eng.decode(N)
        eng.sync()
        print(f"[nucleus] {name}: {N} decode steps, {eng.last_timing()[1] / N:.3f} ms per step", flush=True)
        eng.release_many(list(range(B)))
        eng.sync()
    eng.close()


if __name__ == "__main__":
    main()
