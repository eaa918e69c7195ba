"""The whole output chain in ONE decode call -- time stretch, loudness, output format, every subset of the three -- on the CPU SIMT emulator, from
host codes (ntts_codec_decode / ntts_codec_decode_loud) and from device-resident codes (ntts_codec_decode_dev / ntts_codec_decode_dev_loud), against
the stages applied one by one to the plain decode: `stretch`, then `normalize`, then `convert`, float32 between them.  Bit for bit, length for
length: both sides run the same kernels on the same samples, so there is no tolerance to choose.  tests/test_gpu_output_chain.py runs the same
bodies on libneutts_hip.so."""
import itertools

import numpy as np
import pytest

import test_emu_loudness as loud_cases

FRAMES = (104, 85)
SPEEDS = [1.25, 0.8]                                    # 12 480 -> 9 984 and 10 200 -> 12 750 samples: each row still holds a 400 ms gating block
TARGETS = [-16.0, None]
FORMAT = dict(sample_rate=16000, encoding="pcm16")
SUBSETS = [s for k in range(4) for s in itertools.combinations(("speed", "loudness", "format"), k)]


def make_engine(lib, on_gpu):
    return loud_cases.make_engine(lib, on_gpu, max_frames=256, max_rows=1024, hop=loud_cases.DECODE_HOP)


@pytest.fixture(scope="module")
def deng(emu_lib):
    return make_engine(emu_lib, False)


def _codes():
    rng = np.random.default_rng(11)
    return [rng.integers(0, 4 ** 4, size=t).tolist() for t in FRAMES]


def _stages(on):
    """The keyword arguments of `decode` / `decode_device` for a subset of the stages."""
    kw = {}
    if "speed" in on:
        kw["speed"] = SPEEDS
    if "loudness" in on:
        kw["loudness"] = TARGETS
    if "format" in on:
        kw.update(FORMAT)
    return kw


@pytest.fixture(scope="module")
def chain_ref(deng):
    """(the test's codes, per subset the stages one by one on their plain decode): computed once per module, never written to afterwards."""
    eng = deng
    codes = _codes()
    plain = [p.copy() for p in eng.decode(codes)]
    assert [len(p) for p in plain] == [loud_cases.DECODE_HOP * t for t in FRAMES]
    ref = {}
    for on in SUBSETS:
        w = plain
        if "speed" in on:
            w = eng.stretch(w, SPEEDS)
            assert [len(x) for x in w] == [9984, 12750] and all(len(x) != len(p) for x, p in zip(w, plain))
        if "loudness" in on:
            before = w
            w, m = eng.normalize(w, TARGETS, return_measured=True)
            assert np.isfinite(m[0, 0]) and m[0, 2] != 1.0, f"{on}: row 0 is unmeasurable or keeps its level: the chain would prove nothing"
            assert not np.array_equal(w[0], before[0]) and np.array_equal(w[1], before[1]) and m[1, 2] == 1.0
        if "format" in on:
            w = eng.convert(w, **FORMAT)
            assert all(x.dtype == np.int16 for x in w)
        ref[on] = [np.array(x, copy=True) for x in w]
        for x in ref[on]:
            x.setflags(write=False)
    return codes, ref


def _assert_rows(on, got, want):
    assert len(got) == len(want)
    for r, (g, w) in enumerate(zip(got, want)):
        assert g.dtype == w.dtype and len(g) == len(w), f"{on} row {r}: {g.dtype} x {len(g)} vs {w.dtype} x {len(w)}"
        assert np.array_equal(g, w), f"{on} row {r}: {int((g != w).sum())} of {len(w)} samples differ"


@pytest.mark.parametrize("on", SUBSETS, ids=lambda s: "+".join(s) or "plain")
def test_decode_equals_the_stages_one_by_one(deng, chain_ref, on):
    codes, ref = chain_ref
    _assert_rows(on, deng.decode(codes, **_stages(on)), ref[on])


@pytest.mark.parametrize("on", SUBSETS, ids=lambda s: "+".join(s) or "plain")
def test_decode_device_equals_the_stages_one_by_one(deng, chain_ref, on):
    eng = deng
    codes, ref = chain_ref
    stride = max(FRAMES)
    arr = np.zeros((len(codes), stride), dtype=np.int32)
    for r, c in enumerate(codes):
        arr[r, : len(c)] = c
    if eng._on_gpu:
        import torch
        keep = torch.tensor(arr, device="cuda")
        ptr = keep.data_ptr()
        torch.cuda.synchronize()
    else:
        keep, ptr = arr, arr.ctypes.data                # (the emulator's device memory is host memory)
    wav = eng.decode_device(ptr, stride, np.array(FRAMES, dtype=np.int32), **_stages(on))
    eng.sync()
    assert wav.shape == (len(codes), max(len(w) for w in ref[on]))
    _assert_rows(on, [wav[r, : len(w)] for r, w in enumerate(ref[on])], ref[on])
    del keep
