#!/usr/bin/env python
"""What per-token log-probabilities cost per decode step: an engine at NeuTTS-Air geometry (V = 217 488) with 256 slots (the 256 x 288 lm_head
tile) and with 640 slots (the wide lock-step shape: the 256 x 256 tile) stepped greedily with ntts_backbone_set_logprobs off, on, and off
again.  Per setting: the decode step's time (hipEvents around the replayed step graphs: ntts_backbone_last_timing) and the lm_head launch by
itself (ntts_backbone_time_kernel, which = 5: the kernel of that setting -- with or without the log-sum-exp epilogue -- replayed at the slot
state the steps left).

    python tools/probe_logprobs_cost.py [--batches 256,640] [--prefill 64] [--steps 40] [--repeat 2]
"""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "neutts-air_amd")):
    sys.path.insert(0, p)

SETTINGS = [("log-probabilities off", False), ("log-probabilities on", True), ("log-probabilities off again (record allocated)", False)]
CHUNK = 64          # prompts per prompt pass


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", default="256,640")
    ap.add_argument("--prefill", type=int, default=64)
    ap.add_argument("--steps", type=int, default=40)
    ap.add_argument("--repeat", type=int, default=2)
    a = ap.parse_args()
    import torch
    from neutts import _hip
    import synthetic as syn
    cfg = syn.BackboneConfig.neutts_air(217488)
    w = {k: v.to(torch.bfloat16).cuda() for k, v in syn.make_weights(cfg, 0).items()}
    S, N = a.prefill, a.steps
    for B in [int(x) for x in a.batches.split(",")]:
        eng = _hip.BackboneEngine(dict(vocab_size=cfg.vocab_size, hidden_size=cfg.hidden_size, intermediate_size=cfg.intermediate_size,
                                       num_layers=cfg.num_layers, num_heads=cfg.num_heads, num_kv_heads=cfg.num_kv_heads, rms_eps=cfg.rms_eps,
                                       max_context=256, max_batch=B, max_prefill_tokens=CHUNK * S), 0)
        eng.load_state_dict(w, inv_freq=syn.rope_inv_freq(cfg).numpy())
        prompts = [syn.synthetic_prompt(cfg, i, S) for i in range(B)]
        sp = [_hip.Sampling(max_length=S + N + 2, min_new_tokens=N + 2, eos_token_id=cfg.vocab_size - 1, do_sample=False) for _ in range(B)]
        for rep in range(a.repeat):
            for name, on in SETTINGS:
                eng.set_logprobs(on)
                for c in range(0, B, CHUNK):
                    eng.prefill(prompts[c:c + CHUNK], list(range(c, min(c + CHUNK, B))), sp[c:c + CHUNK])
                eng.decode(1)               # (captures this setting's step graph: not timed)
                eng.decode(N)
                eng.sync()
                step_ms = eng.last_timing()[1] / N
                head_ms = eng.time_kernel(5, 20)[0]
                print(f"[logprobs] run {rep + 1}, {B} rows, {name}: {step_ms:.4f} ms per decode step, lm_head launch {head_ms * 1e3:.1f} us", flush=True)
                eng.release_many(list(range(B)))
                eng.sync()
        eng.close()


if __name__ == "__main__":
    main()
