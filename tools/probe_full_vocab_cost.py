#!/usr/bin/env python
"""What sampling over the whole vocabulary (top_k = -1) costs per decode step: a 256-slot engine at NeuTTS-Air geometry stepped with
(a) the default sampling call (top_k 50, temperature 1.0), (b) top_k -1 alone, (c) with min_p 0.05, (d) with top_p 0.95 and (e) with both.
Meant to run under the profiler, once:

    rocprofv3 --kernel-trace --stats -f csv -d DIR -o full -- python tools/probe_full_vocab_cost.py
    python tools/probe_full_vocab_cost.py --summarise DIR --gbps RATE     # sample_greedy_kernel's average per setting, from the kernel trace

Every setting launches the sampling kernel the same number of times (prompt passes + decode steps), in order; the summary splits the
kernel's dispatches of the trace into that many equal runs and averages the decode-step launches of each.  Each whole-vocabulary setting is
reported against its byte floor: (passes over the row) x V x 2 bytes x rows at RATE GB/s, the copy rate ntts_k_membw measures (the run
prints it).  Passes (csrc/kernels/sample.h sample_full_row): one for the draw's per-slot sums, four more for the nucleus threshold's 16-ary
search when top_p < 1; the row's maximum comes from the lm_head's partials, and the re-read of one 2048-column tile is not counted."""
import argparse
import csv
import glob
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "neutts-air_amd")):
    sys.path.insert(0, p)

VOCAB = 217488
# (name, Sampling keywords, passes over the whole row -- None: the grouped top-k scan reads ~1/45 of it)
SETTINGS = [("default top_k 50", dict(top_k=50), None), ("top_k -1", dict(top_k=-1), 1), ("top_k -1, min_p 0.05", dict(top_k=-1, min_p=0.05), 1),
            ("top_k -1, top_p 0.95", dict(top_k=-1, top_p=0.95), 5), ("top_k -1, top_p 0.95, min_p 0.05", dict(top_k=-1, top_p=0.95, min_p=0.05), 5)]
CHUNK = 64          # prompts per prompt pass


def summarise(d, batch, steps, gbps):
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
    for i, (name, _, passes) in enumerate(SETTINGS):
        dec = rows[i * per + per - steps:(i + 1) * per]              # the decode steps of this setting: all `batch` rows draw
        us = sum(b - a for a, b in dec) / len(dec) / 1e3
        base = base or us
        line = f"sample_greedy_kernel, {batch} rows, {name}: {us:.2f} us average over {len(dec)} decode steps ({us / base:.3f} x default)"
        if passes and gbps:
            floor = passes * VOCAB * 2 * batch / (gbps * 1e9) * 1e6
            line += f"; byte floor {passes} x {VOCAB} x 2 B x {batch} rows at {gbps:.0f} GB/s = {floor:.2f} us ({us / floor:.2f} x floor)"
        print(line)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--prefill", type=int, default=64)
    ap.add_argument("--steps", type=int, default=40)
    ap.add_argument("--summarise", metavar="DIR", default=None)
    ap.add_argument("--gbps", type=float, default=0.0, help="ntts_k_membw's rate, as the run printed it (for the byte floors of the summary)")
    a = ap.parse_args()
    if a.summarise:
        return summarise(a.summarise, a.batch, a.steps, a.gbps)
    import ctypes as C
    import torch
    from neutts import _hip
    import synthetic as syn
    cfg = syn.BackboneConfig.neutts_air(VOCAB)
    w = {k: v.to(torch.bfloat16).cuda() for k, v in syn.make_weights(cfg, 0).items()}
    B, S, N = a.batch, a.prefill, a.steps
    eng = _hip.BackboneEngine(dict(vocab_size=cfg.vocab_size, hidden_size=cfg.hidden_size, intermediate_size=cfg.intermediate_size,
                                   num_layers=cfg.num_layers, num_heads=cfg.num_heads, num_kv_heads=cfg.num_kv_heads, rms_eps=cfg.rms_eps,
                                   max_context=256, max_batch=B, max_prefill_tokens=CHUNK * S), 0)
    eng.load_state_dict(w, inv_freq=syn.rope_inv_freq(cfg).numpy())
    gbps = C.c_double()
    if eng.lib.ntts_k_membw(1 << 30, 10, C.byref(gbps)) == 0:
        print(f"[full-vocab] ntts_k_membw: {gbps.value:.1f} GB/s", flush=True)
    prompts = [syn.synthetic_prompt(cfg, i, S) for i in range(B)]
    for name, kw, _ in SETTINGS:
        sp = [_hip.Sampling(max_length=S + N + 1, min_new_tokens=N + 1, eos_token_id=cfg.vocab_size - 1, do_sample=True, temperature=1.0,
                            seed=1 + i, **kw) for i in range(B)]
        for c in range(0, B, CHUNK):
            eng.prefill(prompts[c:c + CHUNK], list(range(c, min(c + CHUNK, B))), sp[c:c + CHUNK])
        eng.decode(N)
        eng.sync()
        print(f"[full-vocab] {name}: {N} decode steps, {eng.last_timing()[1] / N:.3f} ms per step", flush=True)
        eng.release_many(list(range(B)))
        eng.sync()
    eng.close()


if __name__ == "__main__":
    main()
