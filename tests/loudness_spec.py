"""loudness=: the contract of the codec's loudness normalisation (include/neutts_hip.h ntts_codec_normalize / ntts_codec_decode_loud), in numpy float64.

ITU-R BS.1770-4 integrated loudness at the codec's native 24 kHz on a mono float32 waveform -- K-weighting (two biquads), 400 ms gating blocks at
75 % overlap, the absolute gate at -70 LUFS and the relative gate 10 LU under the mean of what passed it -- then one gain per utterance:

    g = min(10^((target - L) / 20), 10^(max_gain_db / 20), 10^(peak_dbfs / 20) / peak)        (the last term only where peak > 0)

computed in double, rounded once to float32, out[i] = x[i] * g in fp32.  peak is the SAMPLE peak max|x|, not the true (inter-sample) peak.

The biquads are designed for the rate by the bilinear construction whose constants reproduce the standard's 48 kHz table (k_weighting(48000) equals
it to 1e-15).  The measurement is stated so that every 100 ms sub-block is a function of 4800 input samples and nothing else: for sub-block j both
biquads start from zero state at sample max(0, (j - 1) * S) and run to the end of the sub-block; z_j is the mean square of the filter output over the
sub-block's own S samples.  subblock_powers_whole() filters the row from its start instead; the two agree to far below 1e-9 LU (test_loudness_spec).
A trailing partial sub-block is not measured.  A row without a gating block (n < 4 * S), without a block above the absolute gate, or with a non-finite
sample is unmeasurable: L is NaN and its gain is 1 (for a non-finite row the reported peak is +inf)."""
import numpy as np

FS = 24000
S = 2400                                     # samples of a 100 ms sub-block at 24 kHz
ABS_GATE = -70.0
OFFSET = -0.691
TARGET_RANGE, PEAK_RANGE, MAX_GAIN_RANGE = (-70.0, 0.0), (-20.0, 0.0), (0.0, 60.0)
DEFAULT_PEAK_DBFS, DEFAULT_MAX_GAIN_DB = -1.0, 20.0

SHELF_F0, SHELF_G, SHELF_Q, SHELF_VB_EXP = 1681.974450955533, 3.999843853973347, 0.7071752369554196, 0.4996667741545416
HP_F0, HP_Q = 38.13547087602444, 0.5003270373238773
# ITU-R BS.1770-4, tables 1 and 2 (48 kHz): b0 b1 b2 / a1 a2
PUBLISHED_48K = ((1.53512485958697, -2.69169618940638, 1.19839281085285, -1.69065929318241, 0.73248077421585),
                 (1.0, -2.0, 1.0, -1.99004745483398, 0.99007225036621))


def k_weighting(fs=FS):
    """((b0, b1, b2, a1, a2) of the shelf, the same of the high-pass), float64, a0 = 1."""
    K = np.tan(np.pi * SHELF_F0 / fs)
    Vh = 10.0 ** (SHELF_G / 20.0)
    Vb = Vh ** SHELF_VB_EXP
    a0 = 1.0 + K / SHELF_Q + K * K
    shelf = ((Vh + Vb * K / SHELF_Q + K * K) / a0, 2.0 * (K * K - Vh) / a0, (Vh - Vb * K / SHELF_Q + K * K) / a0,
             2.0 * (K * K - 1.0) / a0, (1.0 - K / SHELF_Q + K * K) / a0)
    K = np.tan(np.pi * HP_F0 / fs)
    a0 = 1.0 + K / HP_Q + K * K
    hp = (1.0, -2.0, 1.0, 2.0 * (K * K - 1.0) / a0, (1.0 - K / HP_Q + K * K) / a0)
    return tuple(float(v) for v in shelf), tuple(float(v) for v in hp)


def _biquad_step(c, x, s1, s2):
    """One step of a biquad in transposed direct form II (scalars or vectors): -> (y, s1, s2)."""
    b0, b1, b2, a1, a2 = c
    y = b0 * x + s1
    return y, b1 * x - a1 * y + s2, b2 * x - a2 * y


def subblock_powers_many(rows, fs=FS):
    """z_j of every whole sub-block of every row (the warm-start form), all sub-blocks side by side: -> list of float64 arrays, one per row."""
    sb = fs // 10
    shelf, hp = k_weighting(fs)
    segs, counts = [], []
    for x in rows:
        x = np.asarray(x, dtype=np.float64).reshape(-1)
        J = len(x) // sb
        counts.append(J)
        if J:
            padded = np.concatenate([np.zeros(sb), x[: J * sb]])           # zeros ahead of sub-block 0: zero input leaves the zero state as it is
            segs.append(np.stack([padded[j * sb: (j + 2) * sb] for j in range(J)]))
    if not segs:
        return [np.zeros(0) for _ in rows]
    X = np.concatenate(segs)                                               # [sub-blocks of all rows][2 * sb]
    s1 = np.zeros(len(X)); s2 = np.zeros(len(X)); t1 = np.zeros(len(X)); t2 = np.zeros(len(X)); acc = np.zeros(len(X))
    with np.errstate(all="ignore"):
        for t in range(2 * sb):
            y, s1, s2 = _biquad_step(shelf, X[:, t], s1, s2)
            w, t1, t2 = _biquad_step(hp, y, t1, t2)
            if t >= sb:
                acc += w * w
    z = acc / sb
    out, at = [], 0
    for J in counts:
        out.append(z[at: at + J].copy())
        at += J
    return out


def subblock_powers(x, fs=FS):
    return subblock_powers_many([x], fs)[0]


def subblock_powers_whole(x, fs=FS):
    """The same z_j with both biquads run over the whole row from its start (the textbook form; a plain loop)."""
    sb = fs // 10
    shelf, hp = k_weighting(fs)
    x = np.asarray(x, dtype=np.float64).reshape(-1)
    J = len(x) // sb
    w = np.zeros(J * sb)
    s1 = s2 = t1 = t2 = 0.0
    for i, v in enumerate(x[: J * sb].tolist()):
        y, s1, s2 = _biquad_step(shelf, v, s1, s2)
        w[i], t1, t2 = _biquad_step(hp, y, t1, t2)
    return np.square(w).reshape(J, sb).mean(axis=1) if J else np.zeros(0)


def block_loudness(z):
    """(P_i, l_i) of the gating blocks i in [0, J - 3): four sub-blocks each."""
    z = np.asarray(z, dtype=np.float64)
    if len(z) < 4:
        return np.zeros(0), np.zeros(0)
    P = (z[:-3] + z[1:-2] + z[2:-1] + z[3:]) / 4.0
    with np.errstate(divide="ignore", invalid="ignore"):
        return P, OFFSET + 10.0 * np.log10(P)


def gate(z):
    """-> (L, Gamma, blocks, blocks past the absolute gate, blocks past both); L = NaN where the row is unmeasurable (Gamma too, then)."""
    P, l = block_loudness(z)
    keep1 = l > ABS_GATE
    if not keep1.any():
        return float("nan"), float("nan"), len(P), 0, 0
    gamma = OFFSET + 10.0 * np.log10(P[keep1].mean()) - 10.0
    keep2 = keep1 & (l > gamma)
    return float(OFFSET + 10.0 * np.log10(P[keep2].mean())), float(gamma), len(P), int(keep1.sum()), int(keep2.sum())


def integrated(x, fs=FS, whole=False):
    """Integrated loudness of a row in LUFS (NaN = unmeasurable)."""
    x = np.asarray(x)
    if not np.isfinite(x).all():
        return float("nan")
    return gate(subblock_powers_whole(x, fs) if whole else subblock_powers(x, fs))[0]


def gate_margin(x, fs=FS):
    """The smallest distance of any block's l_i to -70 and to Gamma, in LU (inf for a row without blocks): with a margin far above the engine's
    error the spec alone decides every gate."""
    return gate_margin_z(subblock_powers(x, fs))


def gate_margin_z(z):
    """gate_margin of a row whose sub-block powers are z."""
    P, l = block_loudness(z)
    if not len(l):
        return float("inf")
    gamma = gate(z)[1]
    d = np.abs(l - ABS_GATE)
    if np.isfinite(gamma):
        d = np.minimum(d, np.abs(l - gamma))
    return float(d.min())


def peak(x):
    """max |x| as float32 (0 for an empty row, +inf for a row with a non-finite sample)."""
    x = np.asarray(x, dtype=np.float32).reshape(-1)
    if not len(x):
        return np.float32(0.0)
    if not np.isfinite(x).all():
        return np.float32(np.inf)
    return np.float32(np.abs(x).max())


def gain(L, pk, target, peak_dbfs=DEFAULT_PEAK_DBFS, max_gain_db=DEFAULT_MAX_GAIN_DB):
    """The gain of a row of loudness L (NaN = unmeasurable -> 1) and sample peak pk: double arithmetic on the float32 parameters, one rounding."""
    if not np.isfinite(L):
        return np.float32(1.0)
    target, peak_dbfs, max_gain_db = (float(np.float32(v)) for v in (target, peak_dbfs, max_gain_db))
    g = min(10.0 ** ((target - float(L)) / 20.0), 10.0 ** (max_gain_db / 20.0))
    if float(pk) > 0.0:
        g = min(g, 10.0 ** (peak_dbfs / 20.0) / float(pk))
    return np.float32(g)


def measure(x):
    """(L, peak, z) of a row."""
    x = np.asarray(x, dtype=np.float32).reshape(-1)
    return integrated(x), peak(x), subblock_powers(x)


def normalize(x, target, peak_dbfs=DEFAULT_PEAK_DBFS, max_gain_db=DEFAULT_MAX_GAIN_DB):
    """-> (out float32, L, peak, g float32); target None = the option off: gain 1."""
    x = np.asarray(x, dtype=np.float32).reshape(-1)
    L, pk = integrated(x), peak(x)
    g = np.float32(1.0) if target is None else gain(L, pk, target, peak_dbfs, max_gain_db)
    return (x * g).astype(np.float32), L, pk, g


def sample_bound(want):
    """|engine - spec| per sample: one ulp of g and one product rounding each side."""
    return 4.0 * 2.0 ** -24 * np.abs(np.asarray(want, dtype=np.float64))
