"""The repetition penalty's contract in numpy (TEST INFRASTRUCTURE): transformers' RepetitionPenaltyLogitsProcessor
(hf:generation/logits_process.py) -- for every token id that occurs in input_ids[prompt_ignore_length:], score = score * p if
score < 0 else score / p, in fp32 -- followed by the ONE rounding to bf16 the engine applies (include/neutts_hip.h, ntts_sampling:
its top-k select and its argmax partials work on bf16 rows).  The lm_head epilogues (neutts-air_amd/csrc/kernels/gemm.h
rep_penalised) are held to `penalise` bit for bit; tests/test_repetition_spec.py holds `penalise` to the installed transformers.
"""
from __future__ import annotations

import numpy as np


def bf16_round(x):
    """fp32 -> nearest bf16 value (ties to even), as fp32; inf and NaN pass through."""
    x = np.ascontiguousarray(x, dtype=np.float32)
    u = x.view(np.uint32).astype(np.uint64)
    r = (((u + 0x7FFF + ((u >> 16) & 1)) >> 16) << 16).astype(np.uint32).view(np.float32)
    return np.where(np.isfinite(x), r, x).astype(np.float32)


def penalise_fp32(row, seen_ids, p):
    """HF's arithmetic, unrounded: fp32 product / quotient at the seen ids, everything else untouched."""
    out = np.array(row, dtype=np.float32, copy=True)
    ids = np.unique(np.asarray(list(seen_ids), dtype=np.int64))
    if ids.size == 0:
        return out
    v = out[ids]
    p = np.float32(p)
    with np.errstate(invalid="ignore"):
        out[ids] = np.where(v < 0, v * p, v / p).astype(np.float32)
    return out


def penalise(row, seen_ids, p):
    """The engine's processed logits for a bf16-valued `row`: bf16_rne(v * p) below zero, bf16_rne(v / p) from zero up, at the seen ids.
    With p == 1 the row comes back as it is."""
    if np.float32(p) == np.float32(1.0):
        return np.array(row, dtype=np.float32, copy=True)
    out = penalise_fp32(row, seen_ids, p)
    ids = np.unique(np.asarray(list(seen_ids), dtype=np.int64))
    if ids.size:
        out[ids] = bf16_round(out[ids])
    return out


def seen_set(prompt, generated=(), prompt_ignore_length=0):
    """The ids the processor looks at: input_ids[prompt_ignore_length:] with the ignore length clamped to the prompt, plus what was generated."""
    n = min(max(int(prompt_ignore_length), 0), len(prompt))
    return set(int(t) for t in list(prompt)[n:]) | set(int(t) for t in generated)


def first_argmax(row):
    """torch.argmax's choice: the first maximum."""
    return int(np.argmax(np.asarray(row, dtype=np.float32)))
