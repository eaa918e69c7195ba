"""Per-token log-probabilities in numpy, float64 (TEST INFRASTRUCTURE): the contract of include/neutts_hip.h ntts_backbone_set_logprobs.  For a
token `tok` chosen from the processed logits row r (bf16-valued; after the repetition penalty and the MinNewTokens EOS mask):
logprob = r[tok] - logsumexp(r) over the WHOLE row, -inf columns contributing 0 -- temperature, top-k, top-p and min-p do not enter.  That is
transformers' compute_transition_scores(..., normalize_logits=True) for a greedy request; tests/test_logprob_spec.py holds it to torch and to
transformers itself.  A sequence's score is the arithmetic mean of its log-probabilities.
"""
from __future__ import annotations

import numpy as np


def logsumexp(row) -> float:
    """log(sum(exp(row))) in float64 around the row's maximum; -inf entries contribute 0; a row without one finite entry gives -inf."""
    r = np.asarray(row, dtype=np.float64)
    m = r.max()
    if not np.isfinite(m):
        return float(m)
    with np.errstate(under="ignore"):
        return float(m + np.log(np.exp(r - m).sum()))


def logprob(row, tok) -> float:
    """log softmax(row)[tok] in float64."""
    return float(np.float64(np.asarray(row)[int(tok)]) - logsumexp(row))


def sequence_score(logprobs) -> float:
    """Arithmetic mean of a request's log-probabilities."""
    return float(np.mean(np.asarray(logprobs, dtype=np.float64)))


def group_sums(row, width):
    """(max, sum of exp(v - max)) of every group of `width` consecutive columns of `row` (the last group padded with -inf), float64; a group
    whose maximum is -inf has sum 0: what the lm_head epilogues leave in part_val / part_sum."""
    r = np.asarray(row, dtype=np.float64)
    n = (r.size + width - 1) // width
    pad = np.full(n * width, -np.inf)
    pad[: r.size] = r
    g = pad.reshape(n, width)
    mx = g.max(axis=1)
    safe = np.where(np.isfinite(mx), mx, 0.0)
    with np.errstate(under="ignore"):
        s = np.exp(g - safe[:, None]).sum(axis=1)
    return mx, np.where(np.isfinite(mx), s, 0.0)
