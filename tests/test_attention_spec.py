"""tests/attention_spec.py held to the oracle (oracle.backbone_ref: bf16 torch, the eager path) on the inputs the attention
parity tests use, and its page-layout helpers held to themselves."""
import numpy as np
import pytest
import torch

import attention_spec as sp
from oracle import backbone_ref as br


def _t(x):
    return torch.from_numpy(np.ascontiguousarray(x, dtype=np.float32)).to(torch.bfloat16)


def test_bf16_rounding_helpers():
    rng = np.random.default_rng(0)
    x = (rng.standard_normal(20000) * np.exp(rng.standard_normal(20000) * 8)).astype(np.float32)
    x = np.concatenate([x, sp.bits_to_f32(np.arange(0x3F80, 0x3F90, dtype=np.uint16)) + np.float32(2.0 ** -8)])     # ties
    want = torch.from_numpy(x).to(torch.bfloat16).float().numpy()
    assert np.array_equal(sp.rb32(x), want)
    assert np.array_equal(sp.rb64(x.astype(np.float64)), want.astype(np.float64))
    assert np.array_equal(sp.bits_to_f32(sp.f32_to_bits(want)), want)
    assert sp.bf16_ulp(1.0) == 2.0 ** -7 and sp.bf16_ulp(1.99) == 2.0 ** -7 and sp.bf16_ulp(0.5) == 2.0 ** -8
    # one rounding, not two: 1 + 2^-8 + 2^-30 lies above the tie, float32 would first round it onto the tie and then to even (1.0)
    assert sp.rb64(1.0 + 2.0 ** -8 + 2.0 ** -30) == 1.0 + 2.0 ** -7


@pytest.mark.parametrize("hd", [64, 128])
def test_rope_equals_oracle_bit_for_bit(hd):
    """real tables (rope_cos_sin in bf16), gaussian bf16 heads, positions up to 2047: apply_rope in bf16 torch is the same chain of
    single fp32 operations, so the spec equals it bit for bit."""
    cfg = br.BackboneConfig(vocab_size=64, hidden_size=hd * 2, intermediate_size=64, num_layers=1, num_heads=2, num_kv_heads=1, head_dim=hd)
    pos = torch.tensor([0, 1, 31, 32, 97, 500, 1023, 1024, 2047])
    cos, sin = br.rope_cos_sin(cfg, pos, torch.bfloat16)            # [1, S, hd]
    rng = np.random.default_rng(hd)
    q = sp.gaussian_bf16(rng, (len(pos), 3, hd)) * 4
    qo, _ = br.apply_rope(_t(q).permute(1, 0, 2)[None], _t(q).permute(1, 0, 2)[None], cos, sin)
    want = qo[0].permute(1, 0, 2).float().numpy()
    c, s = cos[0, :, : hd // 2].float().numpy()[:, None, :], sin[0, :, : hd // 2].float().numpy()[:, None, :]
    assert np.array_equal(sp.f32_to_bits(sp.rope(q, c, s)), sp.f32_to_bits(want))


def test_quarter_turn_tables_keep_the_lattice():
    cos, sin = sp.quarter_turn_tables(2048, 32)
    assert np.array_equal(cos * cos + sin * sin, np.ones_like(cos)) and set(np.unique(cos)) == {-1.0, 0.0, 1.0}
    for t in range(4):                                                # all four turns occur, and neighbours differ
        assert ((cos == [1, 0, -1, 0][t]) & (sin == [0, 1, 0, -1][t])).mean() > 0.2
    rng = np.random.default_rng(1)
    x = sp.lattice(rng, (2048, 64), 4)
    r = sp.rope(x, cos, sin)
    assert np.array_equal(r * 4, np.rint(r * 4)) and np.abs(r).max() <= 4
    assert np.array_equal(np.sort(np.abs(r), -1), np.sort(np.abs(x), -1))


@pytest.mark.parametrize("hd,n_rep,L,qamp", [(64, 7, 97, 4), (64, 2, 300, 1), (128, 4, 130, 4), (128, 1, 64, 1)])
def test_attention_equals_oracle(hd, n_rep, L, qamp):
    """causal attention of L lattice queries / keys against eager_attention in bf16 torch.  The scores are exact on both sides; the oracle's softmax
    and PV accumulate in fp32, so P and the output may differ in a final rounding: within the parity tolerance, and nearly always not at all."""
    rng = np.random.default_rng(hd + L)
    q, k, v = sp.lattice(rng, (n_rep, L, hd), qamp), sp.lattice(rng, (L, hd), 1), sp.gaussian_bf16(rng, (L, hd))
    mask = br.causal_mask(L, L, torch.bfloat16)
    want = br.eager_attention(_t(q)[None], _t(k)[None, None], _t(v)[None, None], mask, sp.scaling(hd), n_rep)[0].float().numpy()   # [L][n_rep][hd]
    out, P, mag, srange, slack = sp.attention(q.reshape(-1, hd), k, v, np.tile(np.arange(1, L + 1), n_rep), hd)
    out = out.reshape(n_rep, L, hd).transpose(1, 0, 2)
    mag, slack = (a.reshape(n_rep, L, hd).transpose(1, 0, 2) for a in (mag, slack))
    assert bool((np.abs(want - out) <= sp.tolerance(out, mag) + slack).all())
    share = float((want != out).mean())
    print(f"spec vs oracle hd {hd} L {L}: {share:.5f} of the outputs differ, score range {srange.max():.1f}")
    assert share < 0.02
    if qamp == 4:
        assert srange.max() >= 8
    # P itself: with v = the unit vectors every output IS one P value (one exact product), so the oracle's P is compared bit for bit
    Lp = min(L, hd)
    eye = np.eye(Lp, hd, dtype=np.float32)
    wantp = br.eager_attention(_t(q[:, :Lp])[None], _t(k[:Lp])[None, None], _t(eye)[None, None], br.causal_mask(Lp, Lp, torch.bfloat16), sp.scaling(hd), n_rep)
    wantp = wantp[0].float().numpy().transpose(1, 0, 2).reshape(-1, hd)[:, :Lp]
    _, P2, _, _, _ = sp.attention(q[:, :Lp].reshape(-1, hd), k[:Lp], eye, np.tile(np.arange(1, Lp + 1), n_rep), hd)
    assert bool((np.abs(wantp - P2) <= sp.bf16_ulp(P2)).all()) and float((wantp != P2).mean()) <= 1e-3


def test_attention_refuses_inexact_inputs():
    rng = np.random.default_rng(3)
    q, k = sp.gaussian_bf16(rng, (4, 64)) * 3, sp.gaussian_bf16(rng, (40, 64))
    with pytest.raises(AssertionError):
        sp.attention(q, k, k, np.full(4, 40), 64)


def test_head_rms_norm_within_one_ulp_of_oracle():
    rng = np.random.default_rng(4)
    x = sp.rb32(sp.gaussian_bf16(rng, (500, 128)) * 3)
    w = sp.rb32(1 + 0.1 * rng.standard_normal(128).astype(np.float32))
    want = br.rms_norm(_t(x), _t(w), 1e-6).float().numpy()
    got = sp.head_rms_norm(x, w, 1e-6)
    assert bool((np.abs(want - got) <= sp.bf16_ulp(got)).all()) and float((want != got).mean()) < 0.002


def test_page_layout_round_trip():
    slots = [sp.v_slot(t) for t in range(32)]
    assert sorted(slots) == list(range(32))
    # the documented grouping: slots 0-7 hold tokens 0-3 and 16-19, slots 8-15 tokens 4-7 and 20-23, ...
    for g in range(4):
        assert [slots.index(8 * g + e) for e in range(8)] == [4 * g + e for e in range(4)] + [16 + 4 * g + e for e in range(4)]
    rng = np.random.default_rng(5)
    nkv, hd = 2, 64
    kpool, vpool = sp.new_pools(9, nkv, hd)
    pages = [7, 2, 5, 0]
    kb = rng.integers(0, 0x7F00, size=(100, nkv, hd)).astype(np.uint16)
    vb = rng.integers(0, 0x7F00, size=(100, nkv, hd)).astype(np.uint16)
    sp.write_tokens(kpool, vpool, pages, 0, kb[:64], vb[:64])
    sp.write_tokens(kpool, vpool, pages, 64, kb[64:], vb[64:])           # a second call that starts on a page boundary (shared prefix)
    k2, v2 = sp.read_tokens(kpool, vpool, pages, 0, 100)
    assert np.array_equal(k2, kb) and np.array_equal(v2, vb)
    # token 37 of the sequence = row 5 of page 2; its v values sit in slot v_slot(5) of every d row
    assert np.array_equal(kpool[2, 1, 5], kb[37, 1]) and np.array_equal(vpool[2, 1, :, sp.v_slot(5)], vb[37, 1])
    used = np.zeros(9, bool)
    used[pages] = True
    assert (kpool[~used] == sp.NAN_BITS).all() and (vpool[~used] == sp.NAN_BITS).all()
    assert (kpool[0, :, 4:] == sp.NAN_BITS).all() and (kpool[0, :, :4] != sp.NAN_BITS).all()      # tokens 96 .. 99 fill rows 0 .. 3 of the last page
    assert np.isnan(sp.bits_to_f32(np.array([sp.NAN_BITS], dtype=np.uint16)))[0]
