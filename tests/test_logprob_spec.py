"""tests/logprob_spec.py against torch.log_softmax and against the installed transformers' own scores: a tiny random Qwen2, greedy generate with
min_new_tokens > 0 and output_scores=True, then compute_transition_scores(normalize_logits=True).  CPU, no engine."""
import numpy as np
import pytest
import torch

import logprob_spec as spec
import repetition_spec as rspec


def make_row(seed, n=3000, scale=4.0):
    rng = np.random.default_rng(seed)
    row = rspec.bf16_round(rng.standard_normal(n).astype(np.float32) * np.float32(scale))
    row[n - 1] = -np.inf             # a masked EOS
    row[7] = -np.inf
    return row


@pytest.mark.parametrize("scale", [0.5, 4.0, 30.0])
def test_logprob_is_torch_log_softmax(scale):
    row = make_row(int(scale * 10), scale=scale)
    want = torch.log_softmax(torch.from_numpy(row).to(torch.float64), dim=-1).numpy()
    for tok in (0, 1, 8, 1500, 2998, int(np.argmax(row))):
        assert abs(spec.logprob(row, tok) - want[tok]) <= 1e-12 * max(1.0, abs(want[tok])), tok
    assert spec.logprob(row, 7) == -np.inf and spec.logprob(row, 2999) == -np.inf
    assert abs(spec.logsumexp(row) - float(torch.logsumexp(torch.from_numpy(row).to(torch.float64), 0))) <= 1e-12 * 64
    assert spec.logprob(row, int(np.argmax(row))) <= 0.0


def test_group_sums_rebuild_the_row():
    row = make_row(3)
    row[96:192] = -np.inf            # a whole group of 96 without a finite entry
    for width in (16, 64, 96):
        mx, s = spec.group_sums(row, width)
        assert mx.size == (row.size + width - 1) // width and (s[~np.isfinite(mx)] == 0).all() and not np.isnan(s).any()
        M = mx.max()
        total = (s * np.exp(np.where(np.isfinite(mx), mx - M, -np.inf))).sum()
        assert abs(M + np.log(total) - spec.logsumexp(row)) <= 1e-12 * 64
    assert spec.group_sums(row, 96)[1][1] == 0.0
    assert spec.logsumexp(np.full(5, -np.inf)) == -np.inf


def test_sequence_score_is_the_mean():
    assert spec.sequence_score([-1.0, -2.0, -6.0]) == -3.0


def test_greedy_logprobs_are_transformers_transition_scores():
    from transformers import Qwen2Config, Qwen2ForCausalLM
    torch.manual_seed(11)
    cfg = Qwen2Config(vocab_size=211, hidden_size=32, intermediate_size=64, num_hidden_layers=2, num_attention_heads=4, num_key_value_heads=2,
                      max_position_embeddings=128, tie_word_embeddings=True)
    model = Qwen2ForCausalLM(cfg).eval()
    with torch.no_grad():
        for p in model.parameters():
            p.mul_(4.0)                                   # logits that are not all but equal
    eos = 5
    ids = torch.tensor([[3, 17, 44, 9, 120, 77, 6]], dtype=torch.long)
    with torch.no_grad():
        out = model.generate(ids, attention_mask=torch.ones_like(ids), max_new_tokens=12, min_new_tokens=6, do_sample=False, eos_token_id=eos,
                             pad_token_id=eos, output_scores=True, return_dict_in_generate=True)
    hf = model.compute_transition_scores(out.sequences, out.scores, normalize_logits=True)[0].numpy()
    new = out.sequences[0, ids.shape[1]:].tolist()
    assert len(new) == len(out.scores) >= 6
    got = []
    for i, tok in enumerate(new):
        row = out.scores[i][0].numpy()                    # the processed row: MinNewTokens has masked EOS in the first six
        if i < 6:
            assert row[eos] == -np.inf
        got.append(spec.logprob(row, tok))
    assert np.abs(np.asarray(got) - hf.astype(np.float64)).max() <= 1e-5, (got, hf)
    assert abs(spec.sequence_score(got) - float(hf.astype(np.float64).mean())) <= 1e-5
    assert all(g <= 0 for g in got)
