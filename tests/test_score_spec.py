"""tests/score_spec.py against torch.log_softmax and against the installed transformers' own full-sequence logits (bit for bit in bf16, as
tests/test_oracle_pin.py holds the last row).  CPU, no engine."""
import numpy as np
import pytest
import torch

from oracle import backbone_ref as br
import logprob_spec as lspec
import score_spec as spec


def test_score_is_torch_log_softmax_gather():
    rng = np.random.default_rng(4)
    L, V = 23, 700
    rows = torch.from_numpy(rng.standard_normal((L, V)).astype(np.float32) * 6.0).to(torch.bfloat16).to(torch.float32).numpy()
    rows[5, 100] = rows[5, 300] = rows[5].max() + 1.0                     # a tied maximum: the first index wins
    ids = rng.integers(0, V, L).tolist()
    ls = torch.log_softmax(torch.from_numpy(rows).to(torch.float64), dim=-1)
    for sf in (1, 9, L - 1):
        lp, am, alp = spec.score(rows, ids, sf)
        want = ls[sf - 1:L - 1].gather(1, torch.tensor(ids[sf:])[:, None])[:, 0].numpy()
        assert lp.shape == am.shape == alp.shape == (L - sf,)
        assert np.abs(lp - want).max() <= 1e-12 * 64
        assert am.tolist() == torch.from_numpy(rows[sf - 1:L - 1]).argmax(dim=-1).tolist()
        assert np.abs(alp - ls[sf - 1:L - 1].max(dim=-1).values.numpy()).max() <= 1e-12 * 64
        assert (lp <= alp).all() and (alp <= 0).all()
        lp2, am2, alp2 = spec.score_rows(rows[sf - 1:L - 1], ids[sf:])
        assert np.array_equal(lp, lp2) and np.array_equal(am, am2) and np.array_equal(alp, alp2)
    assert spec.score(rows, ids, 6)[1][0] == 100
    assert lspec.sequence_score(spec.score(rows, ids)[0]) == float(np.mean(spec.score(rows, ids)[0]))


@pytest.mark.parametrize("arch", ["qwen2", "qwen3"])
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_oracle_rows_are_transformers_logits(dtype, arch):
    pytest.importorskip("transformers")
    from oracle.gen_golden import hf_backbone
    if arch == "qwen3":
        cfg = br.BackboneConfig(vocab_size=512, hidden_size=512, intermediate_size=640, num_layers=2, num_heads=4, num_kv_heads=2, head_dim=128,
                                attention_bias=False, qk_norm=True)
    else:
        cfg = br.BackboneConfig(vocab_size=512, hidden_size=896, intermediate_size=640, num_layers=2)
    w = br.make_weights(cfg, 7)
    m = hf_backbone(cfg, w, dtype)
    ids = br.synthetic_prompt(cfg, 3, 41)
    with torch.no_grad():
        logits = m(torch.tensor([ids])).logits[0]
    rows = spec.oracle_rows(cfg, br.cast_weights(w, dtype), ids)
    assert rows.shape == (len(ids), cfg.vocab_size)
    assert np.array_equal(rows.view(np.uint32), logits.to(torch.float32).numpy().view(np.uint32))
    lp, am, alp = spec.score(rows, ids, 7)
    want = torch.log_softmax(logits.to(torch.float64), dim=-1)[6:-1].gather(1, torch.tensor(ids[7:])[:, None])[:, 0].numpy()
    assert np.abs(lp - want).max() <= 1e-12 * 64
