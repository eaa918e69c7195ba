#!/usr/bin/env python
"""What the repetition penalty costs per decode step: a 640-slot engine at NeuTTS-Air geometry (the wide lock-step shape: 256 x 256
lm_head tile, V = 217 488) stepped greedily with (a) no row penalised -- the plain lm_head kernel, a null bitmap pointer -- (b) every row
penalised at 1.3 over its whole prompt and (c) every other row penalised; then (a) once more, with the bitmap now allocated.  Per setting:
the decode step's time (hipEvents around the replayed step graphs) and the lm_head launch by itself (ntts_backbone_time_kernel, which = 5:
the kernel of that setting, replayed at the slot state the steps left).

    python tools/probe_repetition_cost.py [--batch 640] [--prefill 64] [--steps 40] [--repeat 2]
"""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "neutts-air_amd")):
    sys.path.insert(0, p)

SETTINGS = [("no row penalised", lambda i: 1.0), ("every row penalised (1.3)", lambda i: 1.3), ("half the rows penalised (1.3)", lambda i: 1.3 if i % 2 else 1.0),
            ("no row penalised, bitmap allocated", lambda i: 1.0)]
CHUNK = 64          # prompts per prompt pass


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=640)
    ap.add_argument("--prefill", type=int, default=64)
    ap.add_argument("--steps", type=int, default=40)
    ap.add_argument("--repeat", type=int, default=2)
    a = ap.parse_args()
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
    for rep in range(a.repeat):
        for name, pen in SETTINGS:
            sp = [_hip.Sampling(max_length=S + N + 2, min_new_tokens=N + 2, eos_token_id=cfg.vocab_size - 1, do_sample=False,
                                repetition_penalty=pen(i)) for i in range(B)]
            for c in range(0, B, CHUNK):
                eng.prefill(prompts[c:c + CHUNK], list(range(c, min(c + CHUNK, B))), sp[c:c + CHUNK])
            eng.decode(1)               # (captures this setting's step graph: not timed)
            eng.decode(N)
            eng.sync()
            step_ms = eng.last_timing()[1] / N
            head_ms = eng.time_kernel(5, 20)[0]
            print(f"[repetition] run {rep + 1}, {B} rows, {name}: {step_ms:.4f} ms per decode step, lm_head launch {head_ms * 1e3:.1f} us", flush=True)
            eng.release_many(list(range(B)))
            eng.sync()
    eng.close()


if __name__ == "__main__":
    main()
