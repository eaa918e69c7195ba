"""The paged-attention contract, written out: plain numpy float64 with the rounding points of the eager path
(hf:models/qwen2/modeling_qwen2.py eager_attention_forward / apply_rotary_pos_emb, hf:models/qwen3 for head_dim 128 and
qk-norm) and nothing of any kernel's structure -- no tiles, no online softmax, no page loop.  It imports no product code;
tests/test_attention_spec.py holds it to oracle.backbone_ref (bf16 torch).

    score  = bf16(q . k) * scaling            head_dim 64: scaling = 2^-3, exact; head_dim 128: scaling = float32(128^-0.5),
                                              fp32 product rounded to bf16 once more (torch's bf16 tensor * python scalar)
    P      = bf16(softmax(score))             softmax in float64 over the visible keys
    out    = bf16(P . v)
    RoPE   = bf16(bf16(x1 c) + bf16(-x2 s)),  bf16(bf16(x2 c) + bf16(x1 s))   for the pair (x1, x2) = (x[i], x[i + HD/2]);
                                              every step ONE correctly rounded fp32 operation (numpy float32 reproduces it)

bf16 values travel as uint16 bit patterns (`bits`) or as the float32 / float64 numbers they stand for.

KV page layout (per layer; a page holds 32 tokens):
    K   [page][kv_head][32][HD]      token t of the page in row t
    V^T [page][kv_head][HD][32]      token t of the page in slot v_slot(t)
"""
import numpy as np

PAGE = 32
NAN_BITS = 0x7FC0          # bf16 quiet NaN: the poison behind every guard


# ------------------------------------------------------------------------------------------------ bf16
def f32_to_bits(x):
    """float32 -> bf16 bit pattern, round to nearest even (finite inputs)."""
    u = np.ascontiguousarray(x, dtype=np.float32).view(np.uint32).astype(np.uint64)
    return (((u + 0x7FFF + ((u >> 16) & 1)) >> 16) & 0xFFFF).astype(np.uint16)


def bits_to_f32(b):
    return (np.ascontiguousarray(b, dtype=np.uint16).astype(np.uint32) << 16).view(np.float32)


def rb32(x):
    """one fp32 value -> the bf16 value next to it, as float32."""
    return bits_to_f32(f32_to_bits(x))


def rb64(x):
    """float64 -> nearest bf16 value (ties to even) in ONE rounding, as float64."""
    x = np.asarray(x, dtype=np.float64)
    _, e = np.frexp(x)                                   # x = m 2^e, 0.5 <= |m| < 1: 8 significant bits -> quantum 2^(e - 8)
    q = np.ldexp(1.0, np.maximum(e - 8, -133))           # (bf16 subnormals share the quantum 2^-133)
    return np.rint(x / q) * q


def bf16_ulp(x):
    """spacing of bf16 at |x| (float64)."""
    x = np.abs(np.asarray(x, dtype=np.float64))
    _, e = np.frexp(np.maximum(x, 2.0 ** -126))
    return np.ldexp(1.0, e - 8)


# ------------------------------------------------------------------------------------------------ RoPE, qk-norm
def rope(x, cos, sin):
    """x [..., HD], cos / sin [..., HD/2] (bf16 values as float32, broadcastable) -> rotated x, bf16 values as float32."""
    x = np.asarray(x, dtype=np.float32)
    c, s = np.asarray(cos, dtype=np.float32), np.asarray(sin, dtype=np.float32)
    h = x.shape[-1] // 2
    x1, x2 = x[..., :h], x[..., h:]
    o1 = rb32(rb32(x1 * c) + rb32(-x2 * s))
    o2 = rb32(rb32(x2 * c) + rb32(x1 * s))
    return np.concatenate([o1, o2], axis=-1)


def head_rms_norm(x, w, eps):
    """Qwen3RMSNorm over the last axis: bf16(w * bf16(x / sqrt(mean(x^2) + eps))), the statistics in float64."""
    x = np.asarray(x, dtype=np.float64)
    inv = 1.0 / np.sqrt((x * x).mean(-1, keepdims=True) + eps)
    return rb64(np.asarray(w, dtype=np.float64) * rb64(x * inv)).astype(np.float32)


def quarter_turn_tables(max_ctx, half, seed=0):
    """Synthetic RoPE tables [max_ctx][half]: (cos, sin) is one of (1, 0), (0, 1), (-1, 0), (0, -1), chosen by a hash of (position, i).
    A rotation by a quarter turn keeps a lattice on the lattice; a wrong position, pairing or sign still moves every score."""
    pos = np.arange(max_ctx, dtype=np.uint64)[:, None]
    i = np.arange(half, dtype=np.uint64)[None, :]
    h = (pos * np.uint64(2654435761) + i * np.uint64(40503) + np.uint64(seed) * np.uint64(97)) & np.uint64(0xFFFFFFFF)
    h ^= h >> np.uint64(15)
    h = (h * np.uint64(0x2C1B3C6D)) & np.uint64(0xFFFFFFFF)
    t = ((h >> np.uint64(13)) & np.uint64(3)).astype(np.int64)
    cos = np.array([1, 0, -1, 0], dtype=np.float32)[t]
    sin = np.array([0, 1, 0, -1], dtype=np.float32)[t]
    return cos, sin


# ------------------------------------------------------------------------------------------------ attention
def scaling(head_dim):
    return 0.125 if head_dim == 64 else float(np.float32(head_dim ** -0.5))


AMBIGUOUS = 2.0 ** -21     # relative distance of a float64 P to a bf16 rounding boundary inside which an fp32 softmax may round it either way


def attention(q, k, v, n_visible, head_dim=None, exact=True):
    """q [nq][HD], k / v [L][HD] (bf16 values), n_visible [nq]: query i sees keys 0 .. n_visible[i] - 1.
    Returns (out bf16 values as float64 [nq][HD], P [nq][L], mag = P . |v|, score range per row, slack [nq][HD]).
    exact: assert that every visible dot product is exact in fp32 (lattice inputs), so no summation order can move a score.
    slack: the contract's softmax is fp32 (torch); where the float64 value of a P lies within AMBIGUOUS of a bf16 rounding boundary -- 8 fp32 ulps: an exp,
    a sum of up to 2048 terms in any grouping and a division, each within an ulp or two -- fp32 may round that P to EITHER neighbour and both are the
    contract.  slack = sum over those keys of ulp_bf16(P_k) |v_k|: what the other rounding would move the output by.  It is zero for nearly every row."""
    q, k, v = (np.asarray(a, dtype=np.float64) for a in (q, k, v))
    hd = head_dim or q.shape[-1]
    nvis = np.asarray(n_visible).reshape(-1, 1)
    vis = np.arange(k.shape[0])[None, :] < nvis
    dot = q @ k.T
    if exact:
        assert np.array_equal(dot.astype(np.float32).astype(np.float64)[vis], dot[vis]), "inputs off the lattice: a dot product is not exact in fp32"
    s = rb32(dot.astype(np.float32))
    if hd == 64:
        s = s.astype(np.float64) * 0.125
    else:
        s = rb32(s * np.float32(scaling(hd))).astype(np.float64)
    s = np.where(vis, s, -np.inf)
    mx = s.max(-1, keepdims=True)
    e = np.exp(s - mx)
    p = e / e.sum(-1, keepdims=True)
    P = rb64(p)
    out = rb64(P @ v)
    mag = P @ np.abs(v)
    srange = mx[:, 0] - np.where(vis, s, np.inf).min(-1)
    u = bf16_ulp(p)
    amb = vis & (np.abs((p / u) % 1.0 - 0.5) * u < p * AMBIGUOUS)
    slack = (amb * u) @ np.abs(v)
    return out, P, mag, srange, slack


def tolerance(ref, mag):
    """|got - ref| <= ulp_bf16(ref) + 2^-12 . sum_k P_k |v_k|: one flip of the final rounding, plus fp32 accumulation of at most 2048 exact
    products in any order (2048 . 2^-24 of the addend magnitude, doubled)."""
    return bf16_ulp(ref) + 2.0 ** -12 * mag


# ------------------------------------------------------------------------------------------------ pages
def v_slot(t):
    """slot of token t (0 .. 31) inside a V^T page row: [0-3, 16-19 | 4-7, 20-23 | 8-11, 24-27 | 12-15, 28-31]."""
    return ((t & 15) >> 2) * 8 + (t >> 4) * 4 + (t & 3)


def new_pools(num_pages, nkv, hd, fill=NAN_BITS):
    """(K pool [page][nkv][32][hd], V^T pool [page][nkv][hd][32]) of bf16 bit patterns, every element `fill`."""
    return (np.full((num_pages, nkv, PAGE, hd), fill, dtype=np.uint16), np.full((num_pages, nkv, hd, PAGE), fill, dtype=np.uint16))


def write_tokens(kpool, vpool, pages, first, k_bits=None, v_bits=None):
    """Place tokens first .. first + n - 1 of a sequence whose block-table row is `pages`: k_bits / v_bits [n][nkv][hd] (either may be None)."""
    n = (k_bits if k_bits is not None else v_bits).shape[0]
    t = first + np.arange(n)
    pg, r = np.asarray(pages)[t // PAGE], t % PAGE
    if k_bits is not None:
        kpool[pg, :, r, :] = k_bits
    if v_bits is not None:
        vpool[pg, :, :, v_slot(r)] = v_bits


def read_tokens(kpool, vpool, pages, first, n):
    """the inverse of write_tokens: (k_bits, v_bits) [n][nkv][hd]."""
    t = first + np.arange(n)
    pg, r = np.asarray(pages)[t // PAGE], t % PAGE
    return kpool[pg, :, r, :], vpool[pg, :, :, v_slot(r)]


# ------------------------------------------------------------------------------------------------ inputs
def lattice(rng, shape, amp):
    """multiples of 1/4 in [-amp, amp] (float32): with |q| <= 4, |k| <= 1 and HD <= 128 every q . k is a multiple of 1/16 below 2^9 -- exact in fp32
    in any summation order, and through the matrix core."""
    return (rng.integers(-4 * amp, 4 * amp + 1, size=shape) / 4.0).astype(np.float32)


def gaussian_bf16(rng, shape):
    return rb32(rng.standard_normal(shape).astype(np.float32))
