"""tests/repetition_spec.py against the installed transformers' RepetitionPenaltyLogitsProcessor: the fp32 formula is HF's exactly, the
engine's value is that rounded once to bf16 (relative deviation below 2^-8), and only the seen ids change.  CPU, no engine."""
import numpy as np
import pytest
import torch

import repetition_spec as spec

V = 3000


def hf_penalise(row, input_ids, p, prompt_ignore_length):
    from transformers import RepetitionPenaltyLogitsProcessor
    kw = {} if prompt_ignore_length is None else dict(prompt_ignore_length=prompt_ignore_length)
    proc = RepetitionPenaltyLogitsProcessor(penalty=float(p), **kw)
    scores = torch.from_numpy(np.asarray(row, dtype=np.float32)).clone()[None]
    return proc(torch.tensor([list(input_ids)], dtype=torch.long), scores)[0].numpy()


def make_inputs(seed):
    rng = np.random.default_rng(seed)
    row = spec.bf16_round(rng.standard_normal(V).astype(np.float32) * np.float32(4.0))
    ids = [0, 31, V - 1, 17, 17, 0] + rng.integers(0, V, size=40).tolist() + [31, V - 1, 512, 512]      # duplicates; ids 0, 31, V - 1
    row[17] = 0.0                # a zero score is divided (stays 0)
    row[512] = -np.inf           # a masked EOS that has been seen stays -inf
    return row, ids


@pytest.mark.parametrize("p", [1.3, 0.8, 2.0])
@pytest.mark.parametrize("ignore", [None, 0, 7, "full"])
def test_penalise_is_hf_rounded_once(p, ignore):
    row, ids = make_inputs(int(p * 10))
    n_ign = len(ids) if ignore == "full" else ignore
    hf = hf_penalise(row, ids, p, n_ign)
    seen = spec.seen_set(ids, (), n_ign or 0)
    assert seen == set(ids[(n_ign or 0):])
    fp = spec.penalise_fp32(row, seen, p)
    assert np.array_equal(fp.view(np.uint32), hf.view(np.uint32))                     # the fp32 formula: HF's, bit for bit
    got = spec.penalise(row, seen, p)
    assert np.array_equal(got.view(np.uint32), spec.bf16_round(hf).view(np.uint32))   # the engine's value: that, rounded once
    fin = np.isfinite(hf) & (hf != 0)
    assert (np.abs(got[fin] - hf[fin]) <= np.abs(hf[fin]) * 2.0 ** -8).all()          # half a bf16 ulp
    changed = set(np.flatnonzero(hf.view(np.uint32) != row.view(np.uint32)).tolist())
    assert changed == {i for i in seen if np.isfinite(row[i]) and row[i] != 0}        # HF touches exactly the seen set
    if seen:
        assert got[512] == -np.inf and got[17] == 0.0 and not np.isnan(got).any()
    assert np.array_equal(got[sorted(set(range(V)) - seen)], row[sorted(set(range(V)) - seen)])


def test_rounding_helper_is_torch_bfloat16():
    x = np.random.default_rng(1).standard_normal(20000).astype(np.float32) * np.float32(37.0)
    x[:4] = [np.inf, -np.inf, 0.0, -0.0]
    want = torch.from_numpy(x).to(torch.bfloat16).to(torch.float32).numpy()
    assert np.array_equal(spec.bf16_round(x).view(np.uint32), want.view(np.uint32))


def test_penalty_one_and_empty_set_change_nothing():
    row, ids = make_inputs(3)
    assert np.array_equal(spec.penalise(row, ids, 1.0), row)
    assert np.array_equal(spec.penalise(row, [], 1.7), row)
    assert spec.seen_set([5, 6, 7], [9], 99) == {9} and spec.seen_set([5, 6, 7], [9], 1) == {6, 7, 9}
    assert spec.first_argmax(np.array([1.0, 3.0, 3.0], dtype=np.float32)) == 1
