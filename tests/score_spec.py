"""Teacher-forced scoring of given sequences in numpy, float64 (TEST INFRASTRUCTURE): the contract of include/neutts_hip.h ntts_backbone_score.
For a sequence ids[0 .. len) and every j in [score_from, len): logprob[j] = r_{j-1}[ids[j]] - logsumexp(r_{j-1}) over the whole row of position j-1,
no processor applied -- log_softmax(model(ids).logits)[j-1, ids[j]] of transformers -- together with the first index of each row's maximum and its
log-probability.  tests/test_score_spec.py holds `score` to torch.log_softmax and `oracle_rows` to the live transformers model.
"""
from __future__ import annotations

import numpy as np
import torch
import torch.nn.functional as F

import logprob_spec as spec
from oracle import backbone_ref as br


def score(rows, ids, score_from=1):
    """rows[p] = the logits row of position p (at least positions score_from-1 .. len-2; a mapping or a sequence indexed by position).
    Returns (logprobs, argmax ids, argmax logprobs), len - score_from float64 / int64 / float64 entries."""
    lp, am, alp = [], [], []
    for j in range(score_from, len(ids)):
        r = np.asarray(rows[j - 1], dtype=np.float64)
        lse = spec.logsumexp(r)
        a = int(np.argmax(r))                      # numpy: the first index of the maximum
        lp.append(float(r[int(ids[j])] - lse))
        am.append(a)
        alp.append(float(r[a] - lse))
    return np.asarray(lp, dtype=np.float64), np.asarray(am, dtype=np.int64), np.asarray(alp, dtype=np.float64)


def score_rows(rows, targets):
    """The same on a list of rows that are already the scored positions' (the engine's debug tap, in output order)."""
    lp, am, alp = [], [], []
    for r, t in zip(rows, targets):
        r = np.asarray(r, dtype=np.float64)
        lse = spec.logsumexp(r)
        a = int(np.argmax(r))
        lp.append(float(r[int(t)] - lse)); am.append(a); alp.append(float(r[a] - lse))
    return np.asarray(lp, dtype=np.float64), np.asarray(am, dtype=np.int64), np.asarray(alp, dtype=np.float64)


def oracle_rows(cfg, w, ids) -> np.ndarray:
    """Every position's logits of ONE full-sequence pass of the oracle (oracle.backbone_ref's decoder_layer / rms_norm / linear: model_forward keeps
    the last position only), in the dtype of `w`; returned as float32 [len][V]."""
    dtype = w["model.embed_tokens.weight"].dtype
    t = torch.tensor([list(ids)], dtype=torch.long)
    with torch.no_grad():
        cache = br.KVCache(cfg.num_layers)
        h = F.embedding(t, w["model.embed_tokens.weight"])
        cos, sin = br.rope_cos_sin(cfg, torch.arange(t.shape[1]), dtype)
        for i in range(cfg.num_layers):
            h = br.decoder_layer(cfg, w, i, h, cos, sin, cache)
        h = br.rms_norm(h, w["model.norm.weight"], cfg.rms_eps)
        if "lm_head.weight::q" in w:
            out = br.linear(h[0], w, "lm_head.weight")
        else:
            out = F.linear(h[0], w.get("lm_head.weight", w["model.embed_tokens.weight"]))
    return out.to(torch.float32).numpy()
