"""The 320-row decode tile on the CPU emulator: gate/up and the lm_head on 320 x 192 (12 waves, wave tile 80 x 64, uneven loader split),
forced by knob on a 3-slot engine in the wide decode shape -- the way
tests/test_emu_engine.py forces NTTS_WIDE -- next to the same engine on the wide shape's default tiles.  The tile keeps every K slice
and its summation order, so the ids AND the fp32 logits rows must be the default tiles', bit for bit (ragged contexts, a free slot between
two running ones).  The GPU suite runs the same comparison at 576 and 640 slots (tests/test_gpu_tile320_engine.py)."""
import numpy as np

from oracle import backbone_ref as br
from neutts import _hip
from common import load_fixture, make_engine


def test_tile320_forced_on_a_tiny_wide_engine(emu_lib, monkeypatch):
    monkeypatch.setenv("NTTS_SMALL_BATCH", "0")
    monkeypatch.setenv("NTTS_WIDE", "1")
    z, cfg, w = load_fixture("backbone_small_walk")
    S, N, eos = 40, 5, int(z["eos"])
    prompts = [br.synthetic_prompt(cfg, 0, S), br.synthetic_prompt(cfg, 1, S - 7)]
    samp = [_hip.Sampling(max_length=len(p) + N, min_new_tokens=N, eos_token_id=eos, do_sample=False) for p in prompts]

    def run():
        eng = make_engine(cfg, w, emu_lib, max_batch=3, max_context=96, bf16_upload=True)
        try:
            eng.set_debug(True)
            eng.prefill(prompts, [0, 2], samp)                   # slot 1 stays free
            rows = []
            for k in range(N):
                if k:
                    eng.decode(1)
                rows.append([eng.read_logits(s).copy() for s in (0, 2)])
            return rows, [eng.read(s)[0] for s in (0, 2)]
        finally:
            eng.close()

    rows0, ids0 = run()
    assert all(len(set(i)) == N for i in ids0)
    for knobs in ({"NTTS_GU_TILE": "4"}, {"NTTS_HEAD_TILE": "3"}):
        for k, v in knobs.items():
            monkeypatch.setenv(k, v)
        rows1, ids1 = run()
        for k in knobs:
            monkeypatch.delenv(k)
        assert ids1 == ids0, knobs
        for a, b in zip(rows0, rows1):
            for s in (0, 1):
                assert np.array_equal(a[s].view(np.uint32), b[s].view(np.uint32)), knobs
