"""Engines whose decode rows fit 320-row m-blocks better than 256-row ones (576, 640 slots) run gate/up and the lm_head on the 320 x 192 tile.

Those are whole-K tiles: every output element accumulates the same k-tiles in the same order as on the tiles they replace, so nothing the
engine computes may move.  The 2-layer, 3000-row-vocabulary model of tests/test_gpu_parity_matrix.py, every slot live on ragged contexts
(lengths on both sides of the 32-token page edges among them), 12 steps: with the engine's own choice alone on the chip (the lm_head on the new
tile) and in the shape of a gang of four (gate/up too: ntts_backbone_set_gang), and once with NTTS_GU_TILE /
NTTS_HEAD_TILE / NTTS_WIDE_DOWN forced to the tiles such an engine had before -- ids equal and the dumped fp32 logits rows bit-equal, row for
row, step for step.  Greedy; sampled requests (the lm_head then also leaves the bf16 rows the sampler selects from); and greedy with the
repetition penalty on (the epilogue that penalises seen columns ahead of the argmax partials).
"""
import numpy as np
import pytest
import torch

from oracle import backbone_ref as br
from neutts import _hip
from common import make_engine

pytestmark = pytest.mark.gpu

CFG = br.BackboneConfig(vocab_size=3000, hidden_size=896, intermediate_size=1216, num_layers=2)
EOS = CFG.vocab_size - 1
STEPS = 12
EDGES = [31, 32, 33, 63, 64, 65]


@pytest.fixture(scope="module")
def lib(hip_lib):
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    _hip.load_library(hip_lib)
    return hip_lib


@pytest.fixture(scope="module")
def weights():
    return br.make_weights(CFG, 41)


def old_tiles(B):
    return {"NTTS_GU_TILE": "3" if B % 256 == 128 else "1", "NTTS_HEAD_TILE": "2", "NTTS_WIDE_DOWN": "1"}


def run(lib, w, B, mode, gang=0):
    """ids [B][STEPS] and logits [STEPS][B][V] of one engine of B slots, all live; gang > 0: the engine takes the shape of that many chains side by side."""
    lens = [EDGES[s % 6] if s % 5 == 0 else 20 + (7 * s) % 50 for s in range(B)]
    prompts = [br.synthetic_prompt(CFG, 300 + s, n) for s, n in enumerate(lens)]
    kw = {"greedy": dict(do_sample=False),
          "sample": dict(do_sample=True, top_k=50, temperature=0.9),
          "penalty": dict(do_sample=False, repetition_penalty=1.3)}[mode]
    samp = [_hip.Sampling(max_length=len(p) + STEPS, min_new_tokens=STEPS, eos_token_id=EOS, **(dict(kw, seed=9100 + 37 * s) if mode == "sample" else kw))
            for s, p in enumerate(prompts)]
    eng = make_engine(CFG, w, lib, max_batch=B, max_context=128, max_prefill_tokens=4096, bf16_upload=True)
    try:
        eng.set_debug(True)
        if gang:
            eng.set_gang(gang)
        i = 0
        while i < B:
            j, used = i, 0
            while j < B and (j == i or used + lens[j] <= 4096):
                used += lens[j]
                j += 1
            eng.prefill(prompts[i:j], list(range(i, j)), samp[i:j])
            i = j
        logits = np.empty((STEPS, B, CFG.vocab_size), dtype=np.float32)
        for k in range(STEPS):
            if k:
                eng.decode(1)
            for s in range(B):
                logits[k, s] = eng.read_logits(s)
        ids, _ = eng.read_all()
    finally:
        eng.close()
    assert all(len(t) == STEPS for t in ids)
    return np.asarray(ids, dtype=np.int32), logits


@pytest.mark.parametrize("B,mode", [(576, "greedy"), (640, "greedy"), (640, "sample"), (640, "penalty")])
def test_tile320_engine_bits_equal_the_old_tiles(lib, weights, monkeypatch, B, mode):
    for k in ("NTTS_GU_TILE", "NTTS_HEAD_TILE", "NTTS_WIDE_DOWN"):
        monkeypatch.delenv(k, raising=False)
    news = {"alone": run(lib, weights, B, mode), "gang of 4": run(lib, weights, B, mode, gang=4)}
    for k, v in old_tiles(B).items():
        monkeypatch.setenv(k, v)
    ids_old, lg_old = run(lib, weights, B, mode)
    assert len({tuple(t) for t in ids_old.tolist()}) > B // 2          # the rows do differ from each other
    for tag, (ids_new, lg_new) in news.items():
        same = lg_new.view(np.uint32) == lg_old.view(np.uint32)
        bad = np.argwhere(~same.all(axis=2))
        print(f"tile320 engine B={B} {mode} {tag}: {int((~same).sum())} logits differ in {len(bad)} (step, row) pairs; ids differ in {int((ids_new != ids_old).sum())}")
        assert same.all(), f"{tag}: first differing (step, row): {bad[:4].tolist()}"
        assert np.array_equal(ids_new, ids_old), tag
