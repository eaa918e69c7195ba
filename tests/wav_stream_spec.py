"""The codec's output stage on a signal that arrives in CHUNKS, in numpy, float64 (TEST INFRASTRUCTURE): the contract of include/neutts_hip.h
ntts_wav_stream_* / ntts_streams_set_format / ntts_streams_pump_end_fmt.  It adds no numerics to tests/wav_format_spec.py (the table, the lengths, the
encodings: all from there): only WHEN a sample comes out is new.  tests/test_wav_stream_spec.py pins `resample_chunks` to `resample` of the concatenation."""
from __future__ import annotations

import numpy as np

from wav_format_spec import NATIVE_RATE, geometry, out_len, table


# The 24 kHz signal of a stream arrives in chunks.  Output sample m = q * new + p reads the inputs x[q * orig - width .. q * orig - width + taps),
# so it can be emitted once N >= q * orig + width + orig inputs have arrived; the last chunk emits the rest with the missing inputs zero, as the
# one-shot stage does.  The numbers are `resample`'s: only WHEN a sample comes out is new.
def stream_out_count(n_in_total: int, rate: int, W: int = 0, last: bool = False) -> int:
    """Output samples a stream has emitted in all after n_in_total input samples (`last`: that was its final chunk)."""
    N = int(n_in_total)
    if rate == NATIVE_RATE:
        return N
    if last:
        return out_len(N, rate)
    orig, new, width, _, _ = geometry(rate, W)
    return ((N - width) // orig) * new if N >= width else 0


def resample_chunks(chunks, rate: int, W: int = 0, coef_dtype=np.float64):
    """chunks: the pieces of ONE signal, in order (the final one is the stream's last chunk) -> one float64 array per chunk: the outputs
    [stream_out_count(N_{k-1}), stream_out_count(N_k)) .  Stated chunk by chunk on a history of at most taps - 1 input samples, never on the
    concatenation."""
    chunks = [np.asarray(c, dtype=np.float64).reshape(-1) for c in chunks]
    if rate == NATIVE_RATE:
        return [c.copy() for c in chunks]
    orig, new, width, taps, _ = geometry(rate, W)
    h = table(rate, W).astype(coef_dtype).astype(np.float64)
    hist = np.zeros(0)                  # the inputs x[N - len(hist) .. N)
    N = M = 0
    out = []
    for k, c in enumerate(chunks):
        last = k == len(chunks) - 1
        have = np.concatenate([hist, c])            # x[lo .. N + len(c))
        lo = N - len(hist)
        N += len(c)
        M1 = stream_out_count(N, rate, W, last)
        y = np.empty(M1 - M, dtype=np.float64)
        for q in range(M // new, -(-M1 // new)):    # (M is a multiple of `new`: only a last chunk ends inside a group of phases)
            i0 = q * orig - width                   # the first input of the outputs q * new .. q * new + new
            seg = np.zeros(taps)
            a, b = max(i0, 0), min(i0 + taps, N)    # (inputs before the signal and, in the last chunk, behind it are zero)
            assert a >= lo or b <= a, "history too short"
            if b > a:
                seg[a - i0: b - i0] = have[a - lo: b - lo]
            n = min(new, M1 - q * new)
            y[q * new - M: q * new - M + n] = (h @ seg)[:n]        # the product `resample` forms for this q
        out.append(y)
        M = M1
        keep = N - max(0, (M // new) * orig - width)       # what the next output still needs: at most taps - 1 samples
        assert last or 0 <= keep <= taps - 1
        hist = have[len(have) - keep:] if keep > 0 else np.zeros(0)
    return out
