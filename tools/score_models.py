#!/usr/bin/env python
"""Model-level parity of the fp8 engine against the bf16 engine of the same weights, by teacher-forced scoring (BackboneEngine.score): mean negative
log-likelihood and top-1 agreement on the same sequences -- the measure DESIGN.md section 8.5 lacked ("fp8 MODEL-level parity unpinned").

    python tools/score_models.py [--config nano|air|tiny] [--prompts 32] [--prompt-len 64] [--new 48] [--peak-sigma 0.5]

Synthetic weights at one of synthetic.py's geometries (default: the assumed NeuTTS-Nano shape of bench.py --config nano-fp8).  The bf16 engine
generates a greedy continuation for every synthetic prompt; prompt + continuation is then scored from the first generated token on the bf16
engine, on the fp8 engine with synthetic.default_fp8_input_scales, and on an fp8 engine whose lm_head.input_scale and one layer's q_proj input
scale are 4 x too large (a calibration error of two e4m3 binades).  Printed per engine: mean NLL, its difference to bf16, top-1 agreement with the
given tokens (the bf16 engine's own greedy choice) and with the bf16 engine's teacher-forced argmax."""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "neutts-air_amd")):
    sys.path.insert(0, p)


def build(cfg, w, scales, a, lib):
    import synthetic as syn
    from neutts import _hip
    eng = _hip.BackboneEngine(dict(vocab_size=cfg.vocab_size, hidden_size=cfg.hidden_size, intermediate_size=cfg.intermediate_size,
                                   num_layers=cfg.num_layers, num_heads=cfg.num_heads, num_kv_heads=cfg.num_kv_heads, rms_eps=cfg.rms_eps,
                                   max_context=((a.prompt_len + a.new + 31) // 32) * 32, max_batch=a.prompts,
                                   max_prefill_tokens=a.prompts * (a.prompt_len + a.new), weight_dtype="fp8" if scales else "bf16"), 0, lib)
    eng.load_state_dict({k: v.numpy() for k, v in w.items()}, inv_freq=syn.rope_inv_freq(cfg).numpy(), input_scales=scales)
    return eng


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--config", choices=["nano", "air", "tiny"], default="nano")
    ap.add_argument("--prompts", type=int, default=32)
    ap.add_argument("--prompt-len", type=int, default=64)
    ap.add_argument("--new", type=int, default=48)
    ap.add_argument("--peak-sigma", type=float, default=0.5, help="synthetic.make_weights: heavy-tailed logits, so that the model prefers some tokens")
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--lib", default=os.environ.get("NTTS_SCORE_LIB"), help="library to load (default: build / find libneutts_hip.so)")
    a = ap.parse_args()
    import numpy as np
    import synthetic as syn
    from neutts import _hip
    lib = a.lib
    if not lib:
        import importlib.util
        spec = importlib.util.spec_from_file_location("ntts_build", os.path.join(ROOT, "neutts-air_amd", "build.py"))
        bmod = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(bmod)
        lib = bmod.build(verbose=False)
    cfg = {"nano": syn.BackboneConfig.neutts_nano_like, "air": syn.BackboneConfig.neutts_air,
           "tiny": lambda: syn.BackboneConfig(vocab_size=2048, hidden_size=384, intermediate_size=1024, num_layers=2, num_heads=6, num_kv_heads=2)}[a.config]()
    w = syn.make_weights(cfg, a.seed, peak_sigma=a.peak_sigma)
    prompts = [syn.synthetic_prompt(cfg, i, a.prompt_len) for i in range(a.prompts)]
    eos = cfg.vocab_size - 1
    print(f"# {a.config}: V={cfg.vocab_size} H={cfg.hidden_size} layers={cfg.num_layers}, {a.prompts} prompts x {a.prompt_len} tokens + {a.new} greedy "
          f"tokens of the bf16 engine, peak_sigma={a.peak_sigma}, seed={a.seed}")

    bf16 = build(cfg, w, None, a, lib)
    samp = [_hip.Sampling(max_length=a.prompt_len + a.new, min_new_tokens=a.new, eos_token_id=eos, do_sample=False) for _ in prompts]
    cont = bf16.generate(prompts, samp)
    seqs = [p + c for p, c in zip(prompts, cont)]
    given = np.concatenate([np.asarray(c, dtype=np.int32) for c in cont])
    print(f"# {len(given)} scored tokens, {len(set(given.tolist()))} distinct")

    def measure(eng):
        out = eng.score(seqs, a.prompt_len)
        lp = np.concatenate([t[0] for t in out]).astype(np.float64)
        am = np.concatenate([t[1] for t in out])
        return -lp.mean(), am

    nll16, am16 = measure(bf16)
    bf16.close()
    print(f"{'engine':<52} {'mean NLL':>10} {'NLL - bf16':>11} {'top-1 = given':>14} {'top-1 = bf16 argmax':>20}")
    print(f"{'bf16':<52} {nll16:10.5f} {0.0:11.5f} {np.mean(am16 == given):14.4f} {1.0:20.4f}")
    good = syn.default_fp8_input_scales(cfg)
    mid = cfg.num_layers // 2
    bad = dict(good)
    bad["lm_head.input_scale"] *= 4.0
    bad[f"model.layers.{mid}.self_attn.q_proj.input_scale"] *= 4.0
    for tag, scales in (("fp8, default input scales", good), (f"fp8, lm_head and layer {mid} q_proj input scales x 4", bad)):
        eng = build(cfg, w, scales, a, lib)
        nll, am = measure(eng)
        eng.close()
        print(f"{tag:<52} {nll:10.5f} {nll - nll16:11.5f} {np.mean(am == given):14.4f} {np.mean(am == am16):20.4f}")


if __name__ == "__main__":
    main()
