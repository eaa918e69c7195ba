"""The time stretch on a signal that arrives in chunks, in numpy (TEST INFRASTRUCTURE): the contract of include/neutts_hip.h ntts_speed_stream_* /
ntts_streams_set_speed.  The chunks of a stream at a speed, concatenated, are time_stretch_spec.stretch of its concatenated 24 kHz chunks -- positions
and samples -- for every chunking.  Names as time_stretch_spec: HS, DELTA, L, a_k = (k * HS * pm + 500) // 1000.

A stream has one speed pm per signal.  After N input samples:
  not the last chunk: frame k (frame 0 included) is decided and rendered as soon as a_k + DELTA + L <= N.  Then the clamp to pmax = n_in - L cannot
    bind (n_in >= N), the reference window [t_k, t_k + HS) and every candidate window lie inside what has arrived, and (k + 1) * HS <= n_out: the frame
    is the one-shot rule's, whatever arrives later.  The stream has emitted F(N) * HS samples, F(N) = #{k : a_k + DELTA + L <= N}.
  the last chunk: n_in = N is known; frames F .. K - 1 follow time_stretch_spec as it stands (pmax clamp, zeros outside [0, n_in), truncation to
    n_out).  An empty last chunk is a pure flush.
  history: between chunks a stream keeps k, p_{k-1}, N and the inputs from h0 = max(0, min(t_k, a_k - DELTA, N - L)) on, for its next frame k
    (N - L: the lowest pmax a last chunk can still set, when it brings no sample; t_0 = 0).  At most HIST_MAX = 1560 floats.
  pm = 1000: a copy, no lag, no history.
Output lags input by up to DELTA + L = 960 input samples (40 ms) and one frame.
"""
from __future__ import annotations

import numpy as np

from time_stretch_spec import DELTA, HS, L, PM_MAX, PM_MIN, fade, n_frames, out_len
from wav_format_spec import pcm16

LAG = DELTA + L      # 960: input samples behind a_k that decide frame k
HIST_MAX = 1560      # t_k >= a_k - 601 and N <= a_k + 959


def anchor(k: int, pm: int) -> int:
    return (int(k) * HS * int(pm) + 500) // 1000


def frames_ready(N: int, pm: int) -> int:
    """F(N): frames decided after N input samples of a signal that has not ended.  a_k <= N - LAG  <=>  k * HS * pm <= (N - LAG + 1) * 1000 - 501."""
    if N < LAG:
        return 0
    return ((int(N) - LAG + 1) * 1000 - 501) // (HS * int(pm)) + 1


def stream_out_count(N: int, pm: int, last: bool = False) -> int:
    """24 kHz samples a stream at pm has emitted in all after N input samples (ntts_speed_stream_count)."""
    if not PM_MIN <= pm <= PM_MAX:
        raise ValueError(f"speed {pm} per mille outside [{PM_MIN}, {PM_MAX}]")
    if pm == 1000:
        return int(N)
    return out_len(N, pm) if last else frames_ready(N, pm) * HS


def chunk_out_max(max_chunk_samples: int, pm: int) -> int:
    """The most one chunk of up to max_chunk_samples can emit at pm: its last one, which also brings what the LAG held back.
    out_len(N + c) - F(N) * HS < (c + LAG) * 1000 / pm + 2 (F(N) * HS > ((N - LAG + 1) * 1000 - 501) / pm)."""
    if pm == 1000:
        return int(max_chunk_samples)
    return -(-(int(max_chunk_samples) + LAG) * 1000 // int(pm)) + 1


class Stream:
    """One stream's state between chunks: k, p_{k-1}, N and the history from h0 on.  push() reads the history and the chunk, nothing else."""

    def __init__(self, pm: int):
        if not PM_MIN <= pm <= PM_MAX:
            raise ValueError(f"speed {pm} per mille outside [{PM_MIN}, {PM_MAX}]")
        self.pm, self.k, self.p_prev, self.N, self.h0 = int(pm), 0, 0, 0, 0
        self.hist = np.zeros(0, dtype=np.float32)
        self.max_hist = 0

    def push(self, chunk, last: bool = False):
        """-> (out float64: this chunk's samples, positions int32: those decided in this call)."""
        chunk = np.asarray(chunk, dtype=np.float32).reshape(-1)
        pm = self.pm
        if pm == 1000:
            k0, self.N = n_frames(self.N), self.N + len(chunk)
            pos = (np.arange(k0, n_frames(self.N), dtype=np.int64) * HS).astype(np.int32)
            if last:
                self.N = 0
            return chunk.astype(np.float64), pos
        h0, N = self.h0, self.N + len(chunk)
        have = np.concatenate([self.hist, chunk])              # the inputs [h0, N)
        assert h0 + len(have) == N

        def read(lo, n):                                       # x[lo .. lo + n): zero at and behind N (a last chunk only), never below the history
            assert lo >= h0, f"read at {lo} below the history's first sample {h0}"
            assert last or lo + n <= N, f"a chunk that is not the last reads [{lo}, {lo + n}) of {N} samples"
            out = np.zeros(n, dtype=np.float32)
            hi = min(N, lo + n)
            if hi > lo:
                out[: hi - lo] = have[lo - h0: hi - h0]
            return out

        n_out = out_len(N, pm) if last else frames_ready(N, pm) * HS
        k1 = n_frames(n_out)
        pmax = max(0, N - L)                                   # binds in a last chunk only
        f = fade().astype(np.float64)
        out = np.zeros((k1 - self.k) * HS, dtype=np.float64)
        pos = np.zeros(k1 - self.k, dtype=np.int64)
        for k in range(self.k, k1):
            if k == 0:
                t = p = 0
            else:
                t = self.p_prev + HS
                a = anchor(k, pm)
                c_lo, c_hi = min(max(a - DELTA, 0), pmax), min(max(a + DELTA, 0), pmax)
                assert last or c_hi == a + DELTA
                ref = pcm16(read(t, HS)).astype(np.int64)
                win = pcm16(read(c_lo, c_hi - c_lo + HS)).astype(np.int64)
                cand = np.arange(c_lo, c_hi + 1)
                D = np.abs(np.lib.stride_tricks.sliding_window_view(win, HS) - ref[None, :]).sum(axis=1)
                p = int(cand[np.lexsort((cand, np.abs(cand - t), D))[0]])
            xt, xp = read(t, HS).astype(np.float64), read(p, HS).astype(np.float64)
            out[(k - self.k) * HS: (k - self.k + 1) * HS] = xt + f * (xp - xt)
            pos[k - self.k] = p
            self.p_prev = p
        out = out[: n_out - self.k * HS]
        if last:                                               # the stream is empty again and may start a new signal
            self.k, self.p_prev, self.N, self.h0, self.hist = 0, 0, 0, 0, np.zeros(0, dtype=np.float32)
            return out, pos.astype(np.int32)
        self.k, self.N = k1, N
        t_next = self.p_prev + HS if k1 > 0 else 0
        self.h0 = max(0, min(t_next, anchor(k1, pm) - DELTA, N - L))
        self.hist = have[self.h0 - h0:].copy()
        self.max_hist = max(self.max_hist, len(self.hist))
        assert len(self.hist) <= HIST_MAX, f"history of {len(self.hist)} samples"
        return out, pos.astype(np.int32)


def stretch_chunks(chunks, pm: int):
    """chunks: the signal's pieces in order, the last one final (it may be empty) -> (per-chunk outputs float64, per-chunk positions int32,
    the longest history seen)."""
    s = Stream(pm)
    outs, poss = [], []
    for i, c in enumerate(chunks):
        o, p = s.push(c, last=(i == len(chunks) - 1))
        outs.append(o)
        poss.append(p)
    return outs, poss, s.max_hist
