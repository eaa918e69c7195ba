// codec.h -- NeuCodec decoder kernels (everything that is not a GEMM).
//
// Replaces NeuCodec.decode_code (ref:neutts/neutts.py:288-291) as restated by transformers' xcodec2
// (hf:models/xcodec2/modeling_xcodec2.py): FSQ de-index + project_out + fc (:806-809, :839), Conv1d k7 / k3
// (as GEMMs over overlapping rows, gemm.h), GroupNorm(32)+SiLU (:650-659), RMSNorm / LayerNorm (:320-325,
// :862), full (non-causal) attention (:268-308), ISTFT head (:762-796).
//
// Row layout ("packed padded rows"): utterance b owns rows [off[b], off[b+1]) = its lens[b] frames between kPadRows pad rows on
// either side; frame t sits at row off[b] + kPadRows + t.  A ragged batch therefore costs its OWN frames, not B x the longest
// utterance (150-350-frame batches: 1.4x fewer GEMM rows); equal lengths give the layout b * (T + 2 kPadRows) of the earlier rounds.
// Pad rows of every bf16 GEMM-input buffer are ZERO, which is exactly Conv1d's zero padding (6 zero rows between two utterances),
// so a k-tap convolution is one GEMM with lda = C and K = k*C over overlapping rows.
// The residual stream is fp32 (the reference codec runs in fp32); only GEMM operands are bf16.
#pragma once
#include <ntts/dev.h>
#include "attn_decode.h"
#include "gemm.h"   // silu_fast

namespace ntts {

constexpr int kPadRows = 3;  // covers the k=7 stem (padding 3) and the k=3 ResNet convs (padding 1)

struct CodecRows {
    const int* lens;   // [B] valid frames of each utterance
    const int* off;    // [B + 1] first row of utterance b (its leading pad rows); off[B] = rows
    int B, Tp;         // Tp = longest utterance + 2 * kPadRows (grid sizing only)
    long rows;         // off[B]
};
NTTS_D long codec_row0(const CodecRows& R, int b) { return (long)R.off[b] + kPadRows; }   // row of frame 0 of utterance b

NTTS_D bool codec_row(const CodecRows& R, long r, int& b, int& t) {   // which (utterance, frame) is row r: binary search in off[]
    int lo = 0, hi = R.B - 1;
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if ((long)R.off[mid] <= r) lo = mid; else hi = mid - 1;
    }
    b = lo;
    t = (int)(r - R.off[lo]) - kPadRows;
    return t >= 0 && t < R.lens[b];
}

// ---- precision = high: SPLIT bf16 GEMM operands -------------------------------------------------------------------------------------
// A bf16 operand row of C values is written as [hi | lo | hi] (3 C columns), hi = bf16(x), lo = bf16(x - hi): x to ~16 mantissa bits.
// Against a weight row [wh | wh | wl] (codec.cpp Finalizer::op) the GEMM's ordinary K-loop forms xh wh + xl wh + xh wl in its fp32
// accumulator: the operand-rounding error of a bf16 GEMM (2^-9 relative per operand -- 7e-3 of the waveform over ~60 GEMMs in series,
// DESIGN.md section 2) drops to ~2^-17 at three times the matrix-core work.  The ISTFT head's DFT operand has always been built this way
// (istft_prep_kernel).  `split` = 0: the plain bf16 row of C columns.
// ---- precision = fp16 (the default, `split` = kOpF16): the plain row of C columns as IEEE HALVES for v_mfma_f32_16x16x32_f16 -- 11 significant
// bits per operand at the bf16 rate and the bf16 bytes: 8.1e-4 relative on the waveform from the GEMM operands (tools/codec_operand_sim.py predicts 8.0e-4; bf16 7.4e-3), 9.5e-4 with the ISTFT as ONE fp16 term per bin (istft_prep_kernel: 37.6 -> 37.0 ms per 256 x 250 frames).
constexpr int kOpBf16 = 0, kOpSplit = 1, kOpF16 = 2;
NTTS_D void put_op(bf16_t* y, long r, int C, int ch, float v, int split) {
    if (split == kOpF16) { y[r * C + ch] = f2h(v); return; }
    const bf16_t hi = f2bf(v);
    if (!split) { y[r * C + ch] = hi; return; }
    bf16_t* row = y + r * 3 * C;
    row[ch] = hi; row[C + ch] = f2bf(v - bf2f(hi)); row[2 * C + ch] = hi;
}
NTTS_D void put_op4(bf16_t* y, long r, int C, int ch, const float (&v)[4], int split) {      // 4 consecutive channels, ch % 4 == 0
    bf16x4 hi, lo;
    if (split == kOpF16) {
#pragma unroll
        for (int e = 0; e < 4; ++e) hi[e] = (short)f2h(v[e]);
        *(bf16x4*)(y + r * C + ch) = hi;
        return;
    }
#pragma unroll
    for (int e = 0; e < 4; ++e) { hi[e] = (short)f2bf(v[e]); lo[e] = (short)f2bf(v[e] - bf2f((bf16_t)hi[e])); }
    if (!split) { *(bf16x4*)(y + r * C + ch) = hi; return; }
    bf16_t* row = y + r * 3 * C;
    *(bf16x4*)(row + ch) = hi; *(bf16x4*)(row + C + ch) = lo; *(bf16x4*)(row + 2 * C + ch) = hi;
}

// ---- FSQ de-index + (project_out o fc) folded into one affine  8 -> H --------------------------------
struct CodecEmbedArgs {
    const int* codes;      // packed, utterance b starts at code_off[b]
    const int* code_off;
    const float* wf;       // [H][nq] folded weight (fp32)
    const float* bf;       // [H]
    bf16_t* out;           // [rows][H]  (split: [rows][3 H], put_op)
    CodecRows R;
    int H, nq;
    int levels[8];
    int split;
};
// kEmbedRows rows per workgroup: a thread keeps the folded weights of its channels (H / 256 channels x nq <= 8 weights) in
// registers across the rows (one row per workgroup was 65 536 launches' worth of tiny workgroups at 256 x 250 frames, each
// re-reading its weights: 0.9 ms per pass)
constexpr int kEmbedRows = 16, kEmbedChMax = 8;   // channels per thread held in registers: H <= 2048
NTTS_KERNEL(256) void codec_embed_kernel(CodecEmbedArgs p) {
    const long r0 = (long)blockIdx.x * kEmbedRows;
    const long rows = p.R.rows;
    float wreg[kEmbedChMax][8], breg[kEmbedChMax];
#pragma unroll
    for (int j = 0; j < kEmbedChMax; ++j) {
        const int c = threadIdx.x + 256 * j;
        breg[j] = c < p.H ? p.bf[c] : 0.f;
#pragma unroll
        for (int i = 0; i < 8; ++i) wreg[j][i] = (c < p.H && i < p.nq) ? p.wf[(long)c * p.nq + i] : 0.f;
    }
    for (int rr = 0; rr < kEmbedRows; ++rr) {
        const long r = r0 + rr;
        if (r >= rows) break;                                   // block-uniform
        int b, t;
        const bool ok = codec_row(p.R, r, b, t);
        float val[8];
#pragma unroll
        for (int i = 0; i < 8; ++i) val[i] = 0.f;
        if (ok) {
            int code = p.codes[p.code_off[b] + t];
#pragma unroll
            for (int i = 0; i < 8; ++i) {
                if (i < p.nq) {
                    const int L = p.levels[i], d = code % L, half = L / 2;   // hf:...modeling_xcodec2.py:680-690
                    code /= L;
                    val[i] = (float)(d - half) / (float)half;
                }
            }
        }
#pragma unroll
        for (int j = 0; j < kEmbedChMax; ++j) {
            const int c = threadIdx.x + 256 * j;
            if (c < p.H) {
                float acc = 0.f;
                if (ok) {
                    acc = breg[j];
#pragma unroll
                    for (int i = 0; i < 8; ++i)
                        if (i < p.nq) acc += wreg[j][i] * val[i];
                }
                put_op(p.out, r, p.H, c, acc, p.split);
            }
        }
    }
}

// ---- GroupNorm(32 groups, eps) + SiLU : fp32 [rows][C] -> bf16 [rows][C], pad rows zeroed ---------------
struct GroupNormArgs {
    const float* x;
    bf16_t* y;
    const float* gamma;
    const float* beta;
    CodecRows R;
    int C;
    float eps;
    int split;             // y is a split operand [rows][3 C] (put_op)
};
// grid (B, 32); block 256 = (256/cg row lanes) x (cg channels)
NTTS_KERNEL(256) void groupnorm_silu_kernel(GroupNormArgs p) {
    NTTS_SHARED float red[2][4];
    const int b = blockIdx.x, grp = blockIdx.y, tid = threadIdx.x;
    const int cg = p.C / 32, nrl = 256 / cg;
    const int ch = grp * cg + tid % cg, rl = tid / cg;
    const int T = p.R.lens[b];
    const long row0 = codec_row0(p.R, b);
    float s = 0.f, ss = 0.f;
    for (int t = rl; t < T; t += nrl) {
        const float v = p.x[(row0 + t) * p.C + ch];
        s += v;
        ss += v * v;
    }
#pragma unroll
    for (int sh = 1; sh < 64; sh <<= 1) { s += shfl_xor(s, sh); ss += shfl_xor(ss, sh); }
    if (lane_id() == 0) { red[0][wave_id()] = s; red[1][wave_id()] = ss; }
    sync();
    s = red[0][0] + red[0][1] + red[0][2] + red[0][3];
    ss = red[1][0] + red[1][1] + red[1][2] + red[1][3];
    const float n = (float)T * (float)cg;
    const float mean = s / n;
    float var = ss / n - mean * mean;
    if (var < 0.f) var = 0.f;
    const float rstd = frsqrt_exact(var + p.eps);
    const float ga = p.gamma[ch], be = p.beta[ch];
    for (int t = rl - kPadRows; t < T + kPadRows; t += nrl) {   // all rows of the utterance, pads included
        float o = 0.f;
        if (t >= 0 && t < T) {
            const float v = (p.x[(row0 + t) * p.C + ch] - mean) * rstd * ga + be;
            o = silu_fast(v);
        }
        put_op(p.y, row0 + t, p.C, ch, o, p.split);
    }
}

// The same for utterances of up to 256 frames with 4-channel (16-byte) accesses and the utterance's slice held in REGISTERS between
// the statistics and the normalisation: every fp32 input is read once, all of a thread's loads are in flight together (the
// kernel above reads each value twice, 4 bytes at a time, one dependent iteration after the other: 205 us per launch at
// 256 x 250 frames against ~70 us of bytes).  Same arithmetic per element; the sums run in another order.
// grid (B, 32); block 256 = (256 / (cg/4) row lanes) x (cg/4 float4 lanes); needs cg % 4 == 0, 256 % (cg/4) == 0, T <= 8 * row lanes
// kGnRegIters = row iterations per thread the instantiation holds in registers: 8 (256 frames at 32 row lanes) or 16 (512 frames)
template <int kGnRegIters>
NTTS_KERNEL(256) void groupnorm_silu_reg_kernel(GroupNormArgs p) {
    NTTS_SHARED float red[2][4];
    const int b = blockIdx.x, grp = blockIdx.y, tid = threadIdx.x;
    const int cg = p.C / 32, vl = cg >> 2, nrl = 256 / vl;
    const int ch = grp * cg + (tid % vl) * 4, rl = tid / vl;
    const int T = p.R.lens[b];
    const long row0 = codec_row0(p.R, b);
    f32x4 v[kGnRegIters];
    float s = 0.f, ss = 0.f;
#pragma unroll
    for (int i = 0; i < kGnRegIters; ++i) {
        const int t = rl + i * nrl;
        v[i] = ld16<f32x4>(p.x + (row0 + (t < T ? t : (T > 0 ? T - 1 : 0))) * p.C + ch);      // clamped address, no branch around the load
    }
#pragma unroll
    for (int i = 0; i < kGnRegIters; ++i) {
        if (rl + i * nrl < T) {
#pragma unroll
            for (int e = 0; e < 4; ++e) { s += v[i][e]; ss += v[i][e] * v[i][e]; }
        }
    }
#pragma unroll
    for (int sh = 1; sh < 64; sh <<= 1) { s += shfl_xor(s, sh); ss += shfl_xor(ss, sh); }
    if (lane_id() == 0) { red[0][wave_id()] = s; red[1][wave_id()] = ss; }
    sync();
    s = red[0][0] + red[0][1] + red[0][2] + red[0][3];
    ss = red[1][0] + red[1][1] + red[1][2] + red[1][3];
    const float n = (float)T * (float)cg;
    const float mean = s / n;
    float var = ss / n - mean * mean;
    if (var < 0.f) var = 0.f;
    const float rstd = frsqrt_exact(var + p.eps);
    const f32x4 ga = ld16<f32x4>(p.gamma + ch), be = ld16<f32x4>(p.beta + ch);
#pragma unroll
    for (int i = 0; i < kGnRegIters; ++i) {
        const int t = rl + i * nrl;
        if (t < T) {
            float o[4];
#pragma unroll
            for (int e = 0; e < 4; ++e) o[e] = silu_fast((v[i][e] - mean) * rstd * ga[e] + be[e]);
            put_op4(p.y, row0 + t, p.C, ch, o, p.split);
        }
    }
    // pad rows of the utterance: zero, as the Conv1d padding wants them
    const float z[4] = {0.f, 0.f, 0.f, 0.f};
    for (int t = rl - kPadRows; t < T + kPadRows; t += nrl)
        if (t < 0 || t >= T) put_op4(p.y, row0 + t, p.C, ch, z, p.split);
}
inline void groupnorm_silu_launch(const GroupNormArgs& p, int Tmax, hipStream_t s) {
    const int cg = p.C / 32, vl = cg / 4;
    if (cg % 4 == 0 && vl >= 1 && 256 % vl == 0 && Tmax <= 8 * (256 / vl)) NTTS_LAUNCH((groupnorm_silu_reg_kernel<8>), dim3(p.R.B, 32), dim3(256), s, p);
    else if (cg % 4 == 0 && vl >= 1 && 256 % vl == 0 && Tmax <= 16 * (256 / vl)) NTTS_LAUNCH((groupnorm_silu_reg_kernel<16>), dim3(p.R.B, 32), dim3(256), s, p);
    else NTTS_LAUNCH((groupnorm_silu_kernel), dim3(p.R.B, 32), dim3(256), s, p);
}

// ---- RMSNorm / LayerNorm over a row: fp32 -> bf16, one wave per row -------------------------------------
struct RowNormArgs {
    const float* x;
    bf16_t* y;
    const float* w;
    const float* bias;  // nullptr -> RMSNorm, else LayerNorm
    long rows;
    int C;
    float eps;
    int split;          // y is a split operand [rows][3 C] (put_op)
};
template <int NV>  // float4 per lane: C <= 256 * NV
NTTS_KERNEL(256) void rownorm_kernel(RowNormArgs p) {
    const int lane = lane_id();
    long row = (long)blockIdx.x * 4 + wave_id();
    const bool rok = row < p.rows;
    if (!rok) row = p.rows - 1;
    const int nvec = p.C >> 2;
    f32x4 v[NV];
    float s = 0.f, ss = 0.f;
#pragma unroll
    for (int i = 0; i < NV; ++i) {
        const int vi = lane + 64 * i;
        v[i] = f32x4{0.f, 0.f, 0.f, 0.f};
        if (vi < nvec) v[i] = ld16<f32x4>(p.x + row * p.C + vi * 4);
#pragma unroll
        for (int e = 0; e < 4; ++e) { s += v[i][e]; ss += v[i][e] * v[i][e]; }
    }
#pragma unroll
    for (int sh = 1; sh < 64; sh <<= 1) { s += shfl_xor(s, sh); ss += shfl_xor(ss, sh); }
    const float n = (float)p.C;
    float mean = 0.f, inv;
    if (p.bias) {
        mean = s / n;
        float var = ss / n - mean * mean;
        if (var < 0.f) var = 0.f;
        inv = frsqrt_exact(var + p.eps);
    } else {
        inv = frsqrt_exact(ss / n + p.eps);
    }
#pragma unroll
    for (int i = 0; i < NV; ++i) {
        const int vi = lane + 64 * i;
        if (vi < nvec && rok) {
            const f32x4 w = ld16<f32x4>(p.w + vi * 4);
            float o[4];
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                float y = (v[i][e] - mean) * inv * w[e];
                if (p.bias) y += p.bias[vi * 4 + e];
                o[e] = y;
            }
            put_op4(p.y, row, p.C, vi * 4, o, p.split);
        }
    }
}
inline void rownorm_launch(const RowNormArgs& p, hipStream_t s) {
    const dim3 grid((unsigned)((p.rows + 3) / 4)), block(256);
    if (p.C <= 256) NTTS_LAUNCH((rownorm_kernel<1>), grid, block, s, p);
    else if (p.C <= 1024) NTTS_LAUNCH((rownorm_kernel<4>), grid, block, s, p);
    else NTTS_LAUNCH((rownorm_kernel<8>), grid, block, s, p);
}

// ---- V -> V^T pages: qkv[rows][3C] (v part) -> vt[b][head][page][64 d][32 frames], frames >= T zeroed ------
struct VTransposeArgs {
    const bf16_t* qkv;
    bf16_t* vt;
    CodecRows R;
    int C, nh, npages;
};
// grid (B * npages, nh)
NTTS_KERNEL(256) void v_transpose_kernel(VTransposeArgs p) {
    NTTS_SHARED bf16_t tile[kPage][64 + 2];
    const int b = blockIdx.x / p.npages, pg = blockIdx.x % p.npages, h = blockIdx.y, tid = threadIdx.x;
    const int T = p.R.lens[b];
    const long row0 = codec_row0(p.R, b) + (long)pg * kPage;
    for (int x = tid; x < kPage * 64; x += 256) {
        const int tk = x >> 6, d = x & 63;
        const int t = pg * kPage + tk;
        tile[tk][d] = (t < T) ? p.qkv[(row0 + tk) * (3L * p.C) + 2 * p.C + h * 64 + d] : (bf16_t)0;
    }
    sync();
    bf16_t* dst = p.vt + (((long)b * p.nh + h) * p.npages + pg) * 64 * kPage;
    for (int x = tid; x < 64 * kPage; x += 256) {
        const int d = x >> 5, tk = x & 31;
        dst[d * kPage + tk] = tile[tk][d];
    }
}

// ---- full (non-causal) multi-head attention within each utterance ----------------------------------------
struct AttnFullArgs {
    const bf16_t* qkv;   // [rows][3C]: q | k | v
    const bf16_t* vt;    // from v_transpose_kernel
    bf16_t* out;         // [rows][C]  (split: [rows][3 C], put_op)
    CodecRows R;
    int C, nh, npages, qtiles;
    int split;
};
// grid (B * qtiles, nh); 4 waves x 16 queries.  Same matrix-core mapping as attn_prefill.h: the workgroup's K page
// (gathered from the qkv rows) and V^T page are staged ONCE in LDS by LDS-DMA (double-buffered) and shared by the 4
// waves, instead of every wave pulling them through its own load path.  Two sweeps (max / denominator, then PV).
//   K image [32 keys][128 B], chunk c of key r at c ^ (r & 7);  V^T image [64 d][64 B], 16-B unit u of row d at
//   u ^ ((d >> 2) & 3)  -- V^T pages come from v_transpose_kernel in plain token order, so a lane's 8 keys are the
//   two 8-byte halves (units g>>1 and 2 + (g>>1)).
template <bool F16>
NTTS_KERNEL(256) void attn_full_kernel(AttnFullArgs p) {
    NTTS_SHARED bf16_t lds[2 * 2 * kPage * 64];
    const int lane = lane_id(), w = wave_id();
    const int g = lane >> 4, l15 = lane & 15;
    const int b = blockIdx.x / p.qtiles, qt = blockIdx.x % p.qtiles, h = blockIdx.y;
    const int T = p.R.lens[b];
    if (qt * 64 >= T) return;                                  // block-uniform
    const int qw0 = qt * 64 + w * 16;
    const bool wave_live = qw0 < T;
    const long row0 = codec_row0(p.R, b);
    const long ld = 3L * p.C;
    int qi = qw0 + l15;
    if (qi > T - 1) qi = T - 1;
    const bf16_t* qr = p.qkv + (row0 + qi) * ld + h * 64 + g * 16;
    bf16x8 qB[2];
    qB[0] = ld16<bf16x8>(qr);
    qB[1] = ld16<bf16x8>(qr + 8);
    const int npg = (T + kPage - 1) / kPage;

    auto stage = [&](int pg, int buf) {
        bf16_t* dst = lds + buf * (2 * kPage * 64);
        if (w < 2) {
#pragma unroll
            for (int i = 0; i < 2; ++i) {
                const int inst = w * 2 + i;                    // 8 keys per instruction
                const int r = inst * 8 + (lane >> 3);
                int kt = pg * kPage + r;
                if (kt > T - 1) kt = T - 1;
                const int c = (lane & 7) ^ (r & 7);
                glds16(p.qkv + (row0 + kt) * ld + p.C + h * 64 + c * 8, dst + inst * 512);
            }
        } else {
            const bf16_t* vp = p.vt + (((long)b * p.nh + h) * p.npages + pg) * 64 * kPage;
#pragma unroll
            for (int i = 0; i < 2; ++i) {
                const int inst = (w - 2) * 2 + i;              // 16 d-rows per instruction
                const int d = inst * 16 + (lane >> 2);
                const int u = (lane & 3) ^ ((d >> 2) & 3);
                glds16(vp + d * kPage + u * 8, dst + kPage * 64 + inst * 512);
            }
        }
    };
    constexpr float kMasked = -1.0e30f;
    auto scores = [&](const bf16_t* kb, int pg, float (&s)[8]) {
#pragma unroll
        for (int u = 0; u < 2; ++u) {
            const int r = u * 16 + l15;
            f32x4 a = {0.f, 0.f, 0.f, 0.f};
            a = mfma16_op<F16>(ld16<bf16x8>(kb + r * 64 + (((2 * g) ^ (r & 7)) << 3)), qB[0], a);
            a = mfma16_op<F16>(ld16<bf16x8>(kb + r * 64 + (((2 * g + 1) ^ (r & 7)) << 3)), qB[1], a);
#pragma unroll
            for (int rr = 0; rr < 4; ++rr) {
                const int key = pg * kPage + u * 16 + g * 4 + rr;
                s[u * 4 + rr] = key < T ? a[rr] * 0.125f : kMasked;
            }
        }
    };
    float m = kMasked, sum = 0.f;
    stage(0, 0);
    for (int pg = 0; pg < npg; ++pg) {
        wait_vmem();
        sync();
        if (pg + 1 < npg) stage(pg + 1, (pg + 1) & 1);
        if (wave_live) {
            float s[8];
            scores(lds + (pg & 1) * (2 * kPage * 64), pg, s);
            const float tm = fmaxf(fmaxf(fmaxf(s[0], s[1]), fmaxf(s[2], s[3])), fmaxf(fmaxf(s[4], s[5]), fmaxf(s[6], s[7])));
            const float mn = fmaxf(m, tm);
            float add = 0.f;
#pragma unroll
            for (int e = 0; e < 8; ++e) add += fexp_neg(s[e] - mn);
            sum = sum * fexp_neg(m - mn) + add;
            m = mn;
        }
    }
#pragma unroll
    for (int sh = 16; sh <= 32; sh <<= 1) {
        const float om = shfl_xor(m, sh), os = shfl_xor(sum, sh);
        const float mn = fmaxf(m, om);
        sum = sum * fexp_neg(m - mn) + os * fexp_neg(om - mn);
        m = mn;
    }
    f32x4 oacc[4];
#pragma unroll
    for (int nt = 0; nt < 4; ++nt) oacc[nt] = f32x4{0.f, 0.f, 0.f, 0.f};
    const float rs = 1.0f / sum;
    sync();
    stage(0, 0);
    for (int pg = 0; pg < npg; ++pg) {
        wait_vmem();
        sync();
        if (pg + 1 < npg) stage(pg + 1, (pg + 1) & 1);
        if (wave_live) {
            const bf16_t* kb = lds + (pg & 1) * (2 * kPage * 64);
            const bf16_t* vb = kb + kPage * 64;
            float s[8];
            scores(kb, pg, s);
            bf16x8 pA;
#pragma unroll
            for (int e = 0; e < 8; ++e) pA[e] = (short)f2op<F16>(fexp_neg(s[e] - m) * rs);
#pragma unroll
            for (int nt = 0; nt < 4; ++nt) {
                const int d = nt * 16 + l15;
                const int sw = (d >> 2) & 3;
                const bf16x4 v0 = ld16<bf16x4>(vb + d * kPage + (((g >> 1) ^ sw) << 3) + (g & 1) * 4);
                const bf16x4 v1 = ld16<bf16x4>(vb + d * kPage + (((2 + (g >> 1)) ^ sw) << 3) + (g & 1) * 4);
                bf16x8 vB;
#pragma unroll
                for (int e = 0; e < 4; ++e) { vB[e] = v0[e]; vB[4 + e] = v1[e]; }
                oacc[nt] = mfma16_op<F16>(pA, vB, oacc[nt]);
            }
        }
    }
    if (wave_live) {
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int q = qw0 + g * 4 + r;
            if (q < T) {
#pragma unroll
                for (int nt = 0; nt < 4; ++nt) put_op(p.out, row0 + q, p.C, h * 64 + l15 + nt * 16, oacc[nt][r], p.split);
            }
        }
    }
}

// ---- the same attention for utterances of up to 256 frames (5 s of audio; the benchmark's 250), with K and V^T RESIDENT ----------
// grid (B, nh): one workgroup per (utterance, head) stages that head's whole K (LDS-DMA, 8 pages) and V^T (transposed on the
// way in: no v_transpose_kernel pass, no V^T round trip through HBM) ONCE -- 64 KB -- and its 8 waves then walk the 16-query
// tiles with no barrier in the loop.  ONE sweep over the keys (online softmax: running maximum m, P = bf16(exp(s - m)) unnormalised,
// accumulator and denominator rescaled by exp(m_old - m_new) per page, one division at the end) instead of two: QK^T is
// computed once and every score costs one exp instead of two.  Allowed here because the codec's reference is fp32 with a
// waveform tolerance -- the backbone's eager contract (P rounded AFTER the global normalisation) is not.
// The rounding of P to bf16 before the PV product is the same 2^-9 relative perturbation as in attn_full_kernel.
// Replaces hf:models/xcodec2/modeling_xcodec2.py:242-331 (Xcodec2Attention, non-causal) like attn_full_kernel.
constexpr int kAttnResPages = 16;  // resident pages at most: 512 frames (NP = 8 / 12 / 16 instantiations: 64 / 96 / 128 KB of LDS)
// 8 waves: the per-page chain K-MFMA -> row maximum (two cross-lane steps) -> exp -> PV-MFMA is serial inside a wave, and the 64 KB of
// LDS allow two workgroups per CU -- with 4 waves each that was 2 waves per SIMD and the kernel ran at the latency of that chain
// (289 us per launch; trimming its arithmetic changed nothing); 8 waves halve the query tiles per wave and double the waves per SIMD.
// NP = pages the instantiation can hold (the launcher picks the smallest that fits the batch's longest utterance): 8 pages = 64 KB, two workgroups
// per CU; 12 / 16 pages (384 / 512 frames: a ragged batch of 150-350-frame utterances used to fall to the paged two-sweep kernel as a whole) one.
template <int NP, bool F16>
NTTS_KERNEL(512) void attn_full_resident_kernel(AttnFullArgs p) {
    NTTS_SHARED bf16_t kres[NP * kPage * 64];    // [page][32 keys][128 B], chunk c of key r at c ^ (r & 7)
    NTTS_SHARED bf16_t vres[NP * 64 * kPage];    // [page][64 d][64 B], 16-B unit u of row d at u ^ ((d >> 2) & 3)
    const int lane = lane_id(), w = wave_id(), tid = threadIdx.x;
    const int g = lane >> 4, l15 = lane & 15;
    const int b = blockIdx.x, h = blockIdx.y;
    const int T = p.R.lens[b];
    if (T < 1) return;                                         // block-uniform
    const long row0 = codec_row0(p.R, b);
    const long ld = 3L * p.C;
    const int npg = (T + kPage - 1) / kPage;                  // <= NP (launcher)
    // ---- K: LDS-DMA, all pages requested at once (frames past T re-read the last one; masked below)
    for (int inst = w; inst < npg * 4; inst += 8) {           // one instruction = 8 keys x 128 B
        const int pg = inst >> 2, r = (inst & 3) * 8 + (lane >> 3);
        int kt = pg * kPage + r;
        if (kt > T - 1) kt = T - 1;
        const int c = (lane & 7) ^ (r & 7);
        glds16(p.qkv + (row0 + kt) * ld + p.C + h * 64 + c * 8, kres + pg * (kPage * 64) + (inst & 3) * 512);
    }
    // ---- V -> V^T: a work item = (frame, 8 d); consecutive lanes = consecutive frames, so the 2-byte LDS stores of a wave
    //      fall on consecutive addresses of one V^T row
    for (int x = tid; x < npg * kPage * 8; x += 512) {
        const int t = x % (npg * kPage), dc = x / (npg * kPage);          // frame, d chunk (8 values)
        bf16x8 v;
#pragma unroll
        for (int e = 0; e < 8; ++e) v[e] = 0;
        if (t < T) v = ld16<bf16x8>(p.qkv + (row0 + t) * ld + 2 * p.C + h * 64 + dc * 8);
        const int pg = t >> 5, tk = t & 31;
#pragma unroll
        for (int e = 0; e < 8; ++e) {
            const int d = dc * 8 + e;
            vres[pg * (64 * kPage) + d * kPage + (((tk >> 3) ^ ((d >> 2) & 3)) << 3) + (tk & 7)] = (bf16_t)v[e];
        }
    }
    wait_vmem();
    sync();

    constexpr float kMasked = -1.0e30f;
    const int ntile = (T + 15) >> 4;
    for (int qt = w; qt < ntile; qt += 8) {                    // wave-uniform: no barrier below
        const int qw0 = qt * 16;
        int qi = qw0 + l15;
        if (qi > T - 1) qi = T - 1;
        const bf16_t* qr = p.qkv + (row0 + qi) * ld + h * 64 + g * 16;
        bf16x8 qB[2];
        qB[0] = ld16<bf16x8>(qr);
        qB[1] = ld16<bf16x8>(qr + 8);
        float m = kMasked, lsum = 0.f;                          // running maximum of query l15 (same in its 4 lanes), lane-partial denominator
        f32x4 oacc[4];
#pragma unroll
        for (int nt = 0; nt < 4; ++nt) oacc[nt] = f32x4{0.f, 0.f, 0.f, 0.f};
        for (int pg = 0; pg < npg; ++pg) {
            const bf16_t* kb = kres + pg * (kPage * 64);
            const bf16_t* vb = vres + pg * (64 * kPage);
            float s[8];
#pragma unroll
            for (int u = 0; u < 2; ++u) {
                const int r = u * 16 + l15;
                f32x4 a = {0.f, 0.f, 0.f, 0.f};
                a = mfma16_op<F16>(ld16<bf16x8>(kb + r * 64 + (((2 * g) ^ (r & 7)) << 3)), qB[0], a);
                a = mfma16_op<F16>(ld16<bf16x8>(kb + r * 64 + (((2 * g + 1) ^ (r & 7)) << 3)), qB[1], a);
                // scores stay in RAW units (q.k, not yet times 1/8): the scale rides in the exponent's constant below.  Only the
                // last page can hold frames past T (wave-uniform test: full pages skip the compare / select)
                if (pg + 1 == npg) {
#pragma unroll
                    for (int rr = 0; rr < 4; ++rr) s[u * 4 + rr] = pg * kPage + u * 16 + g * 4 + rr < T ? a[rr] : kMasked;
                } else {
#pragma unroll
                    for (int rr = 0; rr < 4; ++rr) s[u * 4 + rr] = a[rr];
                }
            }
            float tm = fmaxf(fmaxf(fmaxf(s[0], s[1]), fmaxf(s[2], s[3])), fmaxf(fmaxf(s[4], s[5]), fmaxf(s[6], s[7])));
            tm = fmaxf(tm, shfl_xor(tm, 16));
            tm = fmaxf(tm, shfl_xor(tm, 32));                  // this page's maximum for query l15
            const float mn = fmaxf(m, tm);
            // exp((s - m) / 8) = exp2((s - m) * log2(e) / 8): one subtract, one multiply, one v_exp_f32 per score (~2e-6 relative:
            // the result is rounded to bf16 for the PV product, and the codec's bar is a waveform tolerance against an fp32
            // reference -- the backbone's attention keeps the ~1.5-ulp fexp_neg)
            constexpr float kC = 0.125f * 1.44269504088896340736f;
            const float alpha = fexp2((m - mn) * kC);   // first page: exp2(-huge) = 0 on zeroed accumulators
            m = mn;
            bf16x8 pA;
            float add = 0.f;
#pragma unroll
            for (int e = 0; e < 8; ++e) {
                const float pe = fexp2((s[e] - mn) * kC);
                add += pe;
                pA[e] = (short)f2op<F16>(pe);
            }
            lsum = lsum * alpha + add;
            // accumulator rows are queries g*4 + r: their factors live in the lanes whose l15 is that query
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const float ar = shfl(alpha, g * 4 + r);
#pragma unroll
                for (int nt = 0; nt < 4; ++nt) oacc[nt][r] *= ar;
            }
#pragma unroll
            for (int nt = 0; nt < 4; ++nt) {
                const int d = nt * 16 + l15;
                const int sw = (d >> 2) & 3;
                const bf16x4 v0 = ld16<bf16x4>(vb + d * kPage + (((g >> 1) ^ sw) << 3) + (g & 1) * 4);
                const bf16x4 v1 = ld16<bf16x4>(vb + d * kPage + (((2 + (g >> 1)) ^ sw) << 3) + (g & 1) * 4);
                bf16x8 vB;
#pragma unroll
                for (int e = 0; e < 4; ++e) { vB[e] = v0[e]; vB[4 + e] = v1[e]; }
                oacc[nt] = mfma16_op<F16>(pA, vB, oacc[nt]);
            }
        }
        lsum += shfl_xor(lsum, 16);
        lsum += shfl_xor(lsum, 32);                            // denominator of query l15
        const float rl = 1.0f / lsum;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const float rr = shfl(rl, g * 4 + r);
            const int q = qw0 + g * 4 + r;
            if (q < T) {
#pragma unroll
                for (int nt = 0; nt < 4; ++nt) put_op(p.out, row0 + q, p.C, h * 64 + l15 + nt * 16, oacc[nt][r] * rr, p.split);
            }
        }
    }
}

// ---- ISTFT head: spectrum -> hi/lo-split bf16 DFT operand ------------------------------------------------
// spec fp32 [rows][lds]: log-magnitude bins [0, nb) | phase bins [nb, 2nb), nb = n_fft/2 + 1.
// s3 bf16 [rows][K3]: [re_hi | im_hi | re_lo | im_lo | re_hi | im_hi | 0...]  (pairs with basis [B_hi | B_hi | B_lo])
struct IstftPrepArgs {
    const float* spec;
    long lds;
    bf16_t* s3;
    long K3;
    long rows;
    int nb;
    int f16;               // precision = fp16 (round 6): s3 = [re | im | 0...] as IEEE halves, ONE term per bin (K3 = 2 nb padded) -- against the basis
                           // [B | ...] in halves scaled by kDftScale (codec.cpp); the bf16 engines keep the three-term split below
};
constexpr float kDftScale = 512.0f;   // fp16 DFT basis = window * ck * cos / N * 2^9 (largest entry 0.53; entries below 2^-14 / 2^9 = 1.2e-7 -- 1e-4 of the largest --
                                      // are the only ones in the subnormal range); ola_kernel multiplies by 2^-9 (exact)
NTTS_KERNEL(256) void istft_prep_kernel(IstftPrepArgs p) {
    const long r = blockIdx.x;
    const float* x = p.spec + r * p.lds;
    bf16_t* o = p.s3 + r * p.K3;
    for (int k = threadIdx.x; k < p.nb; k += 256) {
        float mag = fexp(x[k]);
        if (mag > 100.f) mag = 100.f;              // hf:...modeling_xcodec2.py:771
        const float ph = x[p.nb + k];
        const float re = mag * cosf(ph), im = mag * sinf(ph);
        if (p.f16) { o[k] = f2h(re); o[p.nb + k] = f2h(im); continue; }
        const bf16_t rh = f2bf(re), ih = f2bf(im);
        const bf16_t rl = f2bf(re - bf2f(rh)), il = f2bf(im - bf2f(ih));
        o[k] = rh; o[p.nb + k] = ih;
        o[2 * p.nb + k] = rl; o[3 * p.nb + k] = il;
        o[4 * p.nb + k] = rh; o[5 * p.nb + k] = ih;
    }
    for (long k = (p.f16 ? 2L : 6L) * p.nb + threadIdx.x; k < p.K3; k += 256) o[k] = 0;
}

// ---- overlap-add of the windowed frames, trim, divide by the window envelope -------------------------------
struct OlaArgs {
    const float* frames;   // [rows][n_fft]  (window already folded into the DFT basis)
    const float* win2;     // [n_fft] window^2
    float* wav;            // [B][wav_stride]
    long wav_stride;
    CodecRows R;
    int hop, n_fft;
    float scale;           // 1, or 1 / kDftScale when the frames come from the fp16 DFT basis
};
// grid (B, ceil(hop*Tmax / 256))
NTTS_KERNEL(256) void ola_kernel(OlaArgs p) {
    const int b = blockIdx.x;
    const int T = p.R.lens[b];
    const long s = (long)blockIdx.y * 256 + threadIdx.x;
    if (s >= (long)p.hop * T) return;
    const int pad = (p.n_fft - p.hop) / 2;
    const long pos = s + pad;                       // index in the untrimmed overlap-add buffer
    const long row0 = codec_row0(p.R, b);
    int f_hi = (int)(pos / p.hop);
    if (f_hi > T - 1) f_hi = T - 1;
    float acc = 0.f, env = 0.f;
    for (int f = f_hi; f >= 0; --f) {
        const long n = pos - (long)f * p.hop;
        if (n >= p.n_fft) break;
        acc += p.frames[(row0 + f) * p.n_fft + n];
        env += p.win2[n];
    }
    if (env < 1e-11f) env = 1e-11f;                 // hf:...modeling_xcodec2.py:793
    p.wav[(long)b * p.wav_stride + s] = acc * p.scale / env;
}

// ---- output stage behind overlap-add: resample 24 kHz -> 8 .. 48 kHz, encode as float32 / PCM16 / G.711 mu-law -------------------
// The reference has no such stage: its users put torchaudio.functional.resample(wav, 24000, rate) and an int16 cast behind infer()
// (ref:neutts/neutts.py:288-291 hands out 24 kHz float32).  The filter is that function's default construction (sinc_interp_hann, rolloff 0.99,
// lowpass_filter_width W) as a polyphase FIR: output sample m = q * nw + p of an utterance is sum_j coef[j][p] * x[q * orig + j - width], x zero
// outside [0, n_in) of its OWN utterance -- the tail of a shorter row of the input buffer is scratch and is masked by length, never read as signal.
// tests/wav_format_spec.py is the contract (table, lengths, PCM16 rounding, the mu-law segments).
constexpr int kWavF32 = 0, kWavPcm16 = 1, kWavMulaw = 2;
constexpr int kWavBlock = 256;       // output samples per workgroup
constexpr int kWavSpanMax = 1280;    // staged input samples per workgroup: (255 / nw + 1) * orig + taps; 1156 at 8 kHz with W = 64, the largest (checked on the host)
struct WavFormatArgs {
    const float* in;       // [B][in_stride] 24 kHz float32
    long in_stride;
    const int* lens;       // [B]; utterance b holds lens[b] * len_mul input samples (decode: frames x hop; convert: samples x 1)
    int len_mul;
    const float* coef;     // [taps][nw] fp32 (adjacent threads = adjacent phases: coalesced); null at 24 kHz: no filter, conversion only
    void* out;             // [B][out_stride] float / int16_t / uint8_t
    long out_stride;       // elements
    int orig, nw, width, taps;
    int enc;               // kWavF32 / kWavPcm16 / kWavMulaw
};
// clip(rint(x * 2^15), -32768, 32767), ties to even (v_rndne_f32), NaN -> 0
NTTS_D int wav_pcm16(float x) {
    float v = rintf(x * 32768.0f);
    v = fminf(fmaxf(v, -32768.0f), 32767.0f);
    return x != x ? 0 : (int)v;
}
// G.711 mu-law of a 16-bit sample, the 14-bit form (audioop.lin2ulaw(., 2)): bias 0x21, 8 segments of 16 steps
NTTS_D unsigned int wav_mulaw(int s) {
    const int v = s >> 2;
    int mag = v < 0 ? -v : v;
    mag = (mag > 8159 ? 8159 : mag) + 0x21;
    const int seg = 31 - __builtin_clz((unsigned int)mag) - 5;
    const unsigned int code = seg >= 8 ? 0x7Fu : (unsigned int)((seg << 4) | ((mag >> (seg + 1)) & 15));
    return code ^ (v >= 0 ? 0xFFu : 0x7Fu);
}
// THE fp32 output sample m of the workgroup's utterance (all three encodings are applied to this one number): `span` = the staged input
// samples from q0 * orig - width on, zero where the utterance has none
NTTS_D float wav_sample(const WavFormatArgs& p, const float* span, long q0, long m) {
    const long q = m / p.nw;
    const int ph = (int)(m - q * p.nw);
    const float* x = span + (q - q0) * p.orig;
    const float* h = p.coef + ph;
    float acc = 0.f;
    for (int j = 0; j < p.taps; ++j) acc = __builtin_fmaf(h[(long)j * p.nw], x[j], acc);
    return acc;
}
// grid (B, ceil(longest output / kWavBlock))
NTTS_KERNEL(256) void wav_format_kernel(WavFormatArgs p) {
    NTTS_SHARED float span[kWavSpanMax];
    const int b = blockIdx.x;
    const long n_in = (long)p.lens[b] * p.len_mul;
    const long n_out = p.coef ? (n_in * p.nw + p.orig - 1) / p.orig : n_in;
    const long m0 = (long)blockIdx.y * kWavBlock;
    if (m0 >= n_out) return;                                  // (the whole workgroup: nobody is left at the barrier)
    const float* x = p.in + (long)b * p.in_stride;
    const long m = m0 + threadIdx.x;
    float y = 0.f;
    if (p.coef) {
        const long m_last = (m0 + kWavBlock - 1 < n_out ? m0 + kWavBlock : n_out) - 1;
        const long q0 = m0 / p.nw;
        const long i0 = q0 * p.orig - p.width;
        const int n_span = (int)((m_last / p.nw - q0) * p.orig) + p.taps;     // <= kWavSpanMax (host check)
        for (int i = threadIdx.x; i < n_span; i += 256) {
            const long idx = i0 + i;
            span[i] = (idx >= 0 && idx < n_in) ? x[idx] : 0.f;
        }
        sync();
        if (m < n_out) y = wav_sample(p, span, q0, m);
    } else if (m < n_out) {
        y = x[m];
    }
    if (m >= n_out) return;
    const long o = (long)b * p.out_stride + m;
    if (p.enc == kWavF32) ((float*)p.out)[o] = y;
    else if (p.enc == kWavPcm16) ((int16_t*)p.out)[o] = (int16_t)wav_pcm16(y);
    else ((uint8_t*)p.out)[o] = (uint8_t)wav_mulaw(wav_pcm16(y));
}

// ---- the same stage on a signal that arrives in chunks (ntts_wav_stream_*, ntts_streams_pump_end_fmt) ------------------------------------------------
// A stream has received N 24 kHz samples and emitted M output samples so far.  Output m = q * nw + p needs the inputs [q * orig - width,
// q * orig - width + taps): it is emitted as soon as they have all arrived (M = ((N - width) / orig) * nw), the last chunk emits the rest up to
// ceil(N * nw / orig) with the missing inputs zero.  Sample m is wav_sample's dot product over the operands wav_format_kernel stages for it, so the
// concatenated chunks are the one-shot stage's output bit for bit.  What the next outputs still need of the inputs so far -- the last
// N - max(0, (M / nw) * orig - width) of them, at most taps - 1 -- is the stream's history row.  The workgroups of a job read the row while it is
// replaced: two rows per stream, the job reads `parity` and writes the other (as StreamBlendArgs.prev).
struct WavStreamJob {
    long n_before;         // input samples of the stream before this chunk
    long m0, m1;           // output samples before / after it: the job writes m1 - m0 elements
    int u;                 // the stream: its history rows
    int n_new;             // samples of this chunk
    int n_hist;            // samples in the history row: the inputs [n_before - n_hist, n_before)
    int parity;            // which of the two rows holds them
    int last;              // the stream's final chunk: inputs behind it are zero, no history is left
    int phase;             // the launch this job belongs to (two jobs of one stream in a round: the later one in the later launch)
};
struct WavStreamArgs {
    WavFormatArgs f;       // coef (null at 24 kHz: no filter, no history), orig, nw, width, taps, enc; out = [jobs][out_stride] elements
    const WavStreamJob* jobs;
    const float* in;       // [jobs][in_stride]: every job's new samples
    long in_stride;
    float* hist;           // [2][n_streams][hist_stride]
    long hist_stride;
    int n_streams;
};
// input sample `idx` of the job's stream: zero outside [0, N), the chunk from n_before on, the history row below it
NTTS_D float wav_stream_input(const WavStreamJob& j, const float* pv, const float* nx, long idx) {
    if (idx < 0 || idx >= j.n_before + j.n_new) return 0.f;
    if (idx >= j.n_before) return nx[idx - j.n_before];
    const long h = idx - (j.n_before - j.n_hist);
    return h >= 0 ? pv[h] : 0.f;         // (never below the row: the history holds what an output not yet emitted can need)
}
// grid (jobs of the launch, max(1, ceil(longest output / kWavBlock))); jobs job0 .. job0 + gridDim.x - 1, those of `phase`
NTTS_KERNEL(256) void wav_stream_kernel(WavStreamArgs p, int job0, int phase) {
    NTTS_SHARED float span[kWavSpanMax];
    const int jb = job0 + blockIdx.x;
    const WavStreamJob j = p.jobs[jb];
    if (j.phase != phase) return;                             // (block-uniform)
    const float* nx = p.in + (long)jb * p.in_stride;
    const float* pv = p.hist + ((long)j.parity * p.n_streams + j.u) * p.hist_stride;
    float* nv = p.hist + ((long)(j.parity ^ 1) * p.n_streams + j.u) * p.hist_stride;
    const long N = j.n_before + j.n_new;
    const long mb = j.m0 + (long)blockIdx.y * kWavBlock;       // first output sample of this workgroup
    if (mb < j.m1) {                                          // (block-uniform: everybody reaches the barrier or nobody)
        const long m = mb + threadIdx.x;
        float y = 0.f;
        if (p.f.coef) {
            const long m_last = (mb + kWavBlock < j.m1 ? mb + kWavBlock : j.m1) - 1;
            const long q0 = mb / p.f.nw;
            const long i0 = q0 * p.f.orig - p.f.width;
            const int n_span = (int)((m_last / p.f.nw - q0) * p.f.orig) + p.f.taps;   // <= kWavSpanMax (host check, as wav_format_kernel)
            for (int i = threadIdx.x; i < n_span; i += 256) span[i] = wav_stream_input(j, pv, nx, i0 + i);   // a span across history and chunk: by index
            sync();
            if (m < j.m1) y = wav_sample(p.f, span, q0, m);
        } else if (m < j.m1) {
            y = nx[m - j.n_before];                            // 24 kHz: output m is input m
        }
        if (m < j.m1) {
            const long o = (long)jb * p.f.out_stride + (m - j.m0);
            if (p.f.enc == kWavF32) ((float*)p.f.out)[o] = y;
            else if (p.f.enc == kWavPcm16) ((int16_t*)p.f.out)[o] = (int16_t)wav_pcm16(y);
            else ((uint8_t*)p.f.out)[o] = (uint8_t)wav_mulaw(wav_pcm16(y));
        }
    }
    if (!p.f.coef || j.last) return;
    // the history the next chunk finds (in the other row): the inputs from the first one output m1 reads
    const long first = (j.m1 / p.f.nw) * p.f.orig - p.f.width;
    const long h0 = first > 0 ? first : 0;
    long keep = N - h0;                                        // <= taps - 1 (m1 counts every output whose inputs have arrived)
    if (keep > p.hist_stride) keep = p.hist_stride;            // (never past the row, whatever the job says)
    for (int x = blockIdx.y * 256 + threadIdx.x; x < keep; x += gridDim.y * 256) nv[x] = wav_stream_input(j, pv, nx, h0 + x);
}

// ---- time stretch between overlap-add and the output stage: speed without a pitch shift (WSOLA at 24 kHz) ---------------------------------------
// The reference has no such stage (a codec-token model has no duration input; ref:neutts/neutts.py:288-291 hands out what the tokens say).  Speed is
// an integer per mille pm in [500, 2000]; n_out = ceil(n_in * 1000 / pm) and K = ceil(n_out / kStretchHop) output frames are host arithmetic.
// Frame 0 is x[0 .. hop); frame k >= 1 continues at t_k = p_{k-1} + hop unless a position near a_k = (k * hop * pm + 500) / 1000 matches better:
// the candidates c in [clamp(a_k - kStretchDelta), clamp(a_k + kStretchDelta)], clamp to [0, max(0, n_in - kStretchWin)], are scored by
// D(c) = sum_{i < hop} |s[t_k + i] - s[c + i]| on s = wav_pcm16(x) (integers: no order of additions), p_k minimises (D, |c - t_k|, c), and
// out[k * hop + i] = fma(f[i], x[p_k + i] - x[t_k + i], x[t_k + i]) -- the input itself wherever p_k == t_k.  x and s are zero outside [0, n_in) of
// their OWN utterance.  pm = 1000 copies the row.  tests/time_stretch_spec.py is the contract.
constexpr int kStretchWin = 720, kStretchHop = 360, kStretchDelta = 240;
constexpr int kStretchCand = 2 * kStretchDelta + 1;                  // 481 candidates at most: two per thread
constexpr int kStretchSpan = 2 * kStretchDelta + kStretchHop;        // 840 staged samples of the candidate window
constexpr int kStretchImg = 864;                                     // 16-bit elements per LDS image: >= kStretchSpan + 2, and 432 words = 16 mod 32, so the
                                                                     // even and the odd image of adjacent candidates fall into different ds_read_b32 banks
struct WavStretchArgs {
    const float* in;       // [B][in_stride] 24 kHz float32
    long in_stride;
    const int* lens;       // [B]; utterance b holds lens[b] * len_mul input samples (as WavFormatArgs)
    int len_mul;
    const int* pm;         // [B] speed per mille
    const int* n_out;      // [B] ceil(n_in * 1000 / pm)
    int* pos;              // [B][pos_stride]: p_0 .. p_{K-1}
    long pos_stride;
    const float* fade;     // [kStretchHop] fp32
    float* out;            // [B][out_stride] 24 kHz float32
    long out_stride;
};
// the search signal, biased by +32768 into 16 unsigned bits (the differences are the same; v_sad_u16 wants unsigned operands)
NTTS_D unsigned short stretch_s16(const float* x, long n_in, long idx) {
    return (unsigned short)((idx >= 0 && idx < n_in ? wav_pcm16(x[idx]) : 0) + 32768);
}
// sum of |a[i] - b[i]| over kStretchHop 16-bit values, both 4-byte aligned
NTTS_D unsigned int stretch_sad(const unsigned short* a, const unsigned short* b) {
    unsigned int acc = 0;
#if !defined(NTTS_EMU)
    const unsigned int* a2 = (const unsigned int*)a;
    const unsigned int* b2 = (const unsigned int*)b;
#pragma unroll 12
    for (int i = 0; i < kStretchHop / 2; ++i) acc = __builtin_amdgcn_sad_u16(a2[i], b2[i], acc);     // v_sad_u16: both halves of the pair
#else
    for (int i = 0; i < kStretchHop; ++i) acc += (unsigned int)(a[i] > b[i] ? a[i] - b[i] : b[i] - a[i]);
#endif
    return acc;
}
// (D, |c - t|, c) as two words that compare in tuple order: D, then dist << 9 | (c - c_lo)   (c - c_lo < 512, dist < 2^22)
NTTS_D bool stretch_less(unsigned int d0, unsigned int k0, unsigned int d1, unsigned int k1) { return d0 < d1 || (d0 == d1 && k0 < k1); }
// The search of one frame k >= 1 by the whole workgroup: the reference window at t, the candidates around a clamped to [0, pmax], the two images
// in LDS, one v_sad_u16 chain per candidate, the workgroup's argmin of (D, |c - t|, c).  s16(idx) is the search signal at input sample idx.  Every
// thread returns p_k; the barrier before the result also frees ref / img for the next frame.
template <typename S16>
NTTS_D long stretch_search_frame(const S16& s16, long t, long a, long pmax, unsigned short* ref, unsigned short (*img)[kStretchImg],
                                 unsigned int (*red)[4]) {
    long c_lo = a - kStretchDelta, c_hi = a + kStretchDelta;
    c_lo = c_lo < 0 ? 0 : c_lo > pmax ? pmax : c_lo;
    c_hi = c_hi < 0 ? 0 : c_hi > pmax ? pmax : c_hi;
    const int n_cand = (int)(c_hi - c_lo) + 1;          // 1 .. kStretchCand
    for (int i = threadIdx.x; i < kStretchHop; i += 256) ref[i] = s16(t + i);
    for (int i = threadIdx.x; i < n_cand + kStretchHop; i += 256) {      // one sample more than the window: img[1]'s last
        const unsigned short v = s16(c_lo + i);
        if (i < n_cand + kStretchHop - 1) img[0][i] = v;
        if (i > 0) img[1][i - 1] = v;
    }
    sync();
    unsigned int bd = 0xffffffffu, bk = 0xffffffffu;
    for (int j = threadIdx.x; j < n_cand; j += 256) {
        const unsigned int d = stretch_sad(ref, (j & 1) ? &img[1][j - 1] : &img[0][j]);
        const long dist = c_lo + j > t ? c_lo + j - t : t - (c_lo + j);
        const unsigned int key = ((unsigned int)dist << 9) | (unsigned int)j;
        if (stretch_less(d, key, bd, bk)) { bd = d; bk = key; }
    }
    for (int m = 32; m >= 1; m >>= 1) {
        const unsigned int od = (unsigned int)shfl_xor((int)bd, m), ok = (unsigned int)shfl_xor((int)bk, m);
        if (stretch_less(od, ok, bd, bk)) { bd = od; bk = ok; }
    }
    if (lane_id() == 0) { red[0][threadIdx.x >> 6] = bd; red[1][threadIdx.x >> 6] = bk; }
    sync();                                             // (also: everybody is done with ref / img before the next frame overwrites them)
    bd = red[0][0]; bk = red[1][0];
    for (int w = 1; w < 4; ++w)
        if (stretch_less(red[0][w], red[1][w], bd, bk)) { bd = red[0][w]; bk = red[1][w]; }
    return c_lo + (long)(bk & 511u);
}
struct StretchRowS16 {     // the search signal of a whole row in memory
    const float* x;
    long n_in;
    NTTS_D unsigned short operator()(long idx) const { return stretch_s16(x, n_in, idx); }
};
// grid (B): one workgroup walks its utterance's frames in order (p_k needs p_{k-1})
NTTS_KERNEL(256) void wav_stretch_search_kernel(WavStretchArgs p) {
    NTTS_SHARED unsigned short ref[kStretchHop + 8];
    NTTS_SHARED unsigned short img[2][kStretchImg];       // img[0][j] = s[c_lo + j], img[1][j] = s[c_lo + j + 1]: an odd offset reads aligned pairs from img[1]
    NTTS_SHARED unsigned int red[2][4];
    const int b = blockIdx.x;
    const long n_in = (long)p.lens[b] * p.len_mul;
    const int pm = p.pm[b];
    const int K = (p.n_out[b] + kStretchHop - 1) / kStretchHop;
    int* pos = p.pos + (long)b * p.pos_stride;
    if (pm == 1000) {                                      // a copy: position k * hop by definition (block-uniform: no barrier is reached)
        for (int k = threadIdx.x; k < K; k += 256) pos[k] = k * kStretchHop;
        return;
    }
    const StretchRowS16 s16{p.in + (long)b * p.in_stride, n_in};
    const long pmax = n_in > kStretchWin ? n_in - kStretchWin : 0;
    if (threadIdx.x == 0 && K > 0) pos[0] = 0;
    long prev = 0;
    for (int k = 1; k < K; ++k) {
        prev = stretch_search_frame(s16, prev + kStretchHop, ((long)k * kStretchHop * pm + 500) / 1000, pmax, ref, img, red);
        if (threadIdx.x == 0) pos[k] = (int)prev;
    }
}
// grid (B, ceil(longest output / 256)): output sample m of frame k = m / hop
NTTS_KERNEL(256) void wav_stretch_render_kernel(WavStretchArgs p) {
    const int b = blockIdx.x;
    const long n_in = (long)p.lens[b] * p.len_mul;
    const long m = (long)blockIdx.y * 256 + threadIdx.x;
    if (m >= p.n_out[b]) return;
    const float* x = p.in + (long)b * p.in_stride;
    float y;
    if (p.pm[b] == 1000) {
        y = x[m];                                           // n_out == n_in
    } else {
        const int k = (int)(m / kStretchHop), i = (int)(m - (long)k * kStretchHop);
        const int* pos = p.pos + (long)b * p.pos_stride;
        const long pk = pos[k], tk = k ? (long)pos[k - 1] + kStretchHop : 0;
        const float xt = tk + i < n_in ? x[tk + i] : 0.f;
        const float xp = pk + i < n_in ? x[pk + i] : 0.f;
        y = __builtin_fmaf(p.fade[i], xp - xt, xt);
    }
    p.out[(long)b * p.out_stride + m] = y;
}

// ---- the same stretch on a signal that arrives in chunks (ntts_speed_stream_*, ntts_streams_set_speed) ---------------------------------------------
// A stream at pm has received N samples.  Frame k (frame 0 included) is decided and rendered once a_k + kStretchDelta + kStretchWin <= N: the clamp
// to n_in - kStretchWin cannot bind then, the reference window and every candidate window have arrived, and the frame is a whole frame of the final
// output -- position and samples are the one-shot rule's, whatever arrives later.  The last chunk knows n_in = N and runs the remaining frames as
// the one-shot kernels do (clamp, zeros behind N, truncation to n_out).  Between chunks the stream keeps, on the device, its state record
// (p_{k-1}, history length) and the inputs from h0 = max(0, min(t_k, a_k - kStretchDelta, N - kStretchWin)) on -- at most kSpeedHist -- in one of
// two rows: a job reads `parity` and writes the other (as WavStreamArgs.hist).  The host plans a job from counts alone (frames_ready is arithmetic);
// the positions never leave the device unless the caller asks for them.  pm = 1000 copies the chunk.  tests/stream_speed_spec.py is the contract.
constexpr int kSpeedLag = kStretchDelta + kStretchWin;     // 960
constexpr int kSpeedHist = 1560;                           // t_k >= a_k - 601, N <= a_k + 959
struct SpeedStreamJob {
    long n_before;         // input samples of the stream before this chunk
    long m0, m1;           // output samples before / after it: the job writes m1 - m0 floats
    int u;                 // the stream: its history rows and state record
    int pm;                // speed per mille
    int n_new;             // samples of this chunk
    int k0, k1;            // the frames this job decides and renders: [k0, k1)
    int parity;            // which of the two history rows the job reads
    int last;              // the stream's final chunk: inputs behind it are zero, state and history start again
    int phase;             // the launch this job belongs to (as WavStreamJob)
};
struct SpeedStreamState {  // per stream, written by its job, read by its next one (the frames done are host arithmetic: the job's k0)
    int p_prev;            // p_{k-1}
    int n_hist;            // samples in the history row: the inputs [N - n_hist, N)
};
struct SpeedStreamArgs {
    const SpeedStreamJob* jobs;
    const float* in;       // [jobs][in_stride]: every job's new samples
    long in_stride;
    float* hist;           // [2][n_streams][kSpeedHist]
    SpeedStreamState* state;   // [n_streams]
    int n_streams;
    const float* fade;     // [kStretchHop] fp32
    float* out;            // [jobs][out_stride] 24 kHz float32
    long out_stride;
    int* pos;              // [jobs][pos_stride]: p_{k0} .. p_{k1-1}
    long pos_stride;
};
struct SpeedStreamInput {  // input sample idx of the job's stream: the chunk from n_before on, the history row below it, zero outside [0, N)
    const float* pv;
    const float* nx;
    long n_before, N;
    int n_hist;
    NTTS_D float at(long idx) const {
        if (idx < 0 || idx >= N) return 0.f;
        if (idx >= n_before) return nx[idx - n_before];
        const long h = idx - (n_before - n_hist);
        return h >= 0 ? pv[h] : 0.f;      // (never below the row: the history starts at the lowest sample a later frame can read)
    }
    NTTS_D unsigned short operator()(long idx) const { return (unsigned short)(wav_pcm16(at(idx)) + 32768); }
};
// grid (jobs of the launch): one workgroup walks its job's frames in order; jobs job0 .. job0 + gridDim.x - 1, those of `phase`
NTTS_KERNEL(256) void wav_stretch_stream_kernel(SpeedStreamArgs p, int job0, int phase) {
    NTTS_SHARED unsigned short ref[kStretchHop + 8];
    NTTS_SHARED unsigned short img[2][kStretchImg];
    NTTS_SHARED unsigned int red[2][4];
    const int jb = job0 + blockIdx.x;
    const SpeedStreamJob j = p.jobs[jb];
    if (j.phase != phase) return;                             // (block-uniform)
    const float* nx = p.in + (long)jb * p.in_stride;
    float* out = p.out + (long)jb * p.out_stride;
    if (j.pm == 1000) {                                       // a copy: no lag, no history, no state
        for (int i = threadIdx.x; i < j.n_new; i += 256) out[i] = nx[i];
        return;
    }
    const SpeedStreamState st = p.state[j.u];
    sync();                                                   // everybody has the record before thread 0 replaces it (a job may have no frame)
    const int n_hist = st.n_hist < 0 ? 0 : st.n_hist > kSpeedHist ? kSpeedHist : st.n_hist;      // (never past the row, whatever the record says)
    const float* pv = p.hist + ((long)j.parity * p.n_streams + j.u) * kSpeedHist;
    float* nv = p.hist + ((long)(j.parity ^ 1) * p.n_streams + j.u) * kSpeedHist;
    const long N = j.n_before + j.n_new;
    const SpeedStreamInput x{pv, nx, j.n_before, N, n_hist};
    // a chunk that is not the last decides only frames the clamp cannot reach: a_k + kStretchDelta <= N - kStretchWin
    const long pmax = N > kStretchWin ? N - kStretchWin : 0;
    int* pos = p.pos ? p.pos + (long)jb * p.pos_stride : nullptr;
    long prev = st.p_prev;
    for (int k = j.k0; k < j.k1; ++k) {
        long t = 0, pk = 0;
        if (k > 0) {
            t = prev + kStretchHop;
            pk = stretch_search_frame(x, t, ((long)k * kStretchHop * j.pm + 500) / 1000, pmax, ref, img, red);
        }
        for (int i = threadIdx.x; i < kStretchHop; i += 256) {       // the frame's samples, in the same pass
            const long m = (long)k * kStretchHop + i;
            if (m >= j.m0 && m < j.m1 && m - j.m0 < p.out_stride) {
                const float xt = x.at(t + i), xp = x.at(pk + i);
                out[m - j.m0] = __builtin_fmaf(p.fade[i], xp - xt, xt);
            }
        }
        if (threadIdx.x == 0 && pos && k - j.k0 < p.pos_stride) pos[k - j.k0] = (int)pk;
        prev = pk;
    }
    if (j.last) {                                             // the stream is empty again
        if (threadIdx.x == 0) p.state[j.u] = SpeedStreamState{0, 0};
        return;
    }
    // what the next frame k1 (and a last chunk's clamp) can still read of the inputs so far, into the other row
    const long t_next = j.k1 > 0 ? prev + kStretchHop : 0;
    const long a_next = ((long)j.k1 * kStretchHop * j.pm + 500) / 1000 - kStretchDelta;
    long h0 = t_next < a_next ? t_next : a_next;
    h0 = h0 < N - kStretchWin ? h0 : N - kStretchWin;
    h0 = h0 > 0 ? h0 : 0;
    long keep = N - h0;                                       // <= kSpeedHist
    if (keep > kSpeedHist) { h0 = N - kSpeedHist; keep = kSpeedHist; }      // (never past the row)
    for (int i = threadIdx.x; i < keep; i += 256) nv[i] = x.at(h0 + i);
    if (threadIdx.x == 0) p.state[j.u] = SpeedStreamState{(int)prev, (int)keep};
}

// ---- loudness normalisation between the time stretch and the output stage: ITU-R BS.1770-4 integrated loudness, one gain per utterance -------------
// The reference has no such stage (ref:neutts/neutts.py:288-291 hands out the level the reference clip had); its users run a loudness normaliser on
// the 24 kHz float waveform on the host.  Here: K-weighting (two biquads, coefficients built on the host in double), z_j = the mean square of the
// filter output over the 100 ms sub-block j, both biquads started from zero state at sample max(0, (j - 1) * kLoudSub) -- every z_j a function of
// 4800 input samples, so all sub-blocks run side by side; gating blocks of four sub-blocks, the absolute gate at -70 and the relative gate 10 LU
// under the mean of what passed it; g = min(10^((target - L) / 20), 10^(max_gain_db / 20), 10^(peak_dbfs / 20) / peak) in double, rounded once to
// float32; out = x * g in fp32 (g == 1: the row is not touched).  Filters, sums and the gate run in fp64.  tests/loudness_spec.py is the contract.
constexpr int kLoudSub = 2400;                        // samples of a sub-block
constexpr int kLoudLanes = 64;                        // sub-blocks per workgroup: one per lane of its single wave
constexpr int kLoudChunk = 32;                        // samples staged per lane and round; kLoudSub = 75 rounds
constexpr int kLoudRow = kLoudChunk + 1;              // LDS row of a lane, padded: lane l reads bank (l + m) % 32, the staging writes bank (seg + o) % 32
constexpr int kLoudRounds = 2 * kLoudSub / kLoudChunk;
static_assert(kLoudSub % kLoudChunk == 0, "the sub-block's own part starts on a round");
struct WavLoudArgs {
    float* io;             // [B][stride] 24 kHz float32, scaled in place by the apply kernel
    long stride;
    const int* lens;       // [B]; utterance b holds lens[b] * len_mul samples (as WavFormatArgs)
    int len_mul;
    const float* par;      // [B][4]: enable (0 / 1), target_lufs, peak_dbfs, max_gain_db; null: measure only, every gain 1
    double kw[7];          // shelf b0 b1 b2 a1 a2, high-pass a1 a2 (its b is 1 -2 1)
    double* z;             // [B][z_stride] sub-block powers
    long z_stride;
    float* pk;             // [B][pk_stride] max |x| per workgroup of the measure kernel (+inf: a non-finite sample)
    int pk_stride;
    double* res;           // [B][3]: L (NaN = unmeasurable), peak, g
};
// this thread's share of round k: element o = t & 31 of the segments 2 i + (t >> 5) -- 64 consecutive lanes read 2 x 32 consecutive floats
NTTS_D void loud_fetch(float (&r)[kLoudChunk], const float* x, long n, long base, int jn, int k) {
    const int o = threadIdx.x & 31, half = threadIdx.x >> 5;
#pragma unroll
    for (int i = 0; i < kLoudChunk; ++i) {
        const int seg = 2 * i + half;
        const long idx = base + (long)seg * kLoudSub + (long)k * kLoudChunk + o;
        r[i] = (seg < jn && idx >= 0 && idx < n) ? x[idx] : 0.f;          // (ahead of sub-block 0: zeros, which leave the zero state as it is)
    }
}
// grid (B, max(1, ceil(most sub-blocks / kLoudLanes))), one wave: lane l runs sub-block j0 + l through 4800 samples, staged through LDS 32 per lane at
// a time with the next round's loads in flight; the workgroup that holds a row's last sub-block also takes the peak of the unmeasured tail
NTTS_KERNEL(64) void wav_loud_measure_kernel(WavLoudArgs p) {
    NTTS_SHARED float stage[kLoudLanes * kLoudRow];
    const int b = blockIdx.x, t = threadIdx.x;
    const long n = (long)p.lens[b] * p.len_mul;
    const long J = n / kLoudSub;
    const long j0 = (long)blockIdx.y * kLoudLanes;
    const float* x = p.io + (long)b * p.stride;
    float pk = 0.f;
    bool bad = false;
    if (j0 < J) {                                           // (block-uniform)
        const int jn = (int)(J - j0 < kLoudLanes ? J - j0 : kLoudLanes);
        const long base = (j0 - 1) * kLoudSub;
        const double b0 = p.kw[0], b1 = p.kw[1], b2 = p.kw[2], a1 = p.kw[3], a2 = p.kw[4], c1 = p.kw[5], c2 = p.kw[6];
        double s1 = 0.0, s2 = 0.0, t1 = 0.0, t2 = 0.0, acc = 0.0;
        float r[kLoudChunk];
        loud_fetch(r, x, n, base, jn, 0);
        const float* mine = stage + t * kLoudRow;
        for (int k = 0; k < kLoudRounds; ++k) {
            lds_barrier();                                  // everybody has read round k - 1
#pragma unroll
            for (int i = 0; i < kLoudChunk; ++i) stage[(2 * i + (t >> 5)) * kLoudRow + (t & 31)] = r[i];
            lds_barrier();
            if (k + 1 < kLoudRounds) loud_fetch(r, x, n, base, jn, k + 1);
            const bool own = k >= kLoudRounds / 2;          // the sub-block's own samples: summed, and part of the peak
#pragma unroll 8
            for (int m = 0; m < kLoudChunk; ++m) {
                const float xf = mine[m];
                const double v = (double)xf;
                const double y = b0 * v + s1;               // the shelf, transposed direct form II
                s1 = b1 * v - a1 * y + s2;
                s2 = b2 * v - a2 * y;
                const double w = y + t1;                    // the high-pass
                t1 = -2.0 * y - c1 * w + t2;
                t2 = y - c2 * w;
                if (own) {
                    acc += w * w;
                    const float a = __builtin_fabsf(xf);
                    bad |= !(a <= 3.402823466e38f);
                    pk = fmaxf(pk, a);
                }
            }
        }
        if (t < jn) p.z[(long)b * p.z_stride + j0 + t] = acc / (double)kLoudSub;
    }
    const long y_tail = J > 0 ? (J - 1) / kLoudLanes : 0;
    if (blockIdx.y == y_tail)
        for (long i = J * kLoudSub + t; i < n; i += kLoudLanes) {
            const float a = __builtin_fabsf(x[i]);
            bad |= !(a <= 3.402823466e38f);
            pk = fmaxf(pk, a);
        }
    if (bad) pk = INFINITY;
    for (int m = 32; m >= 1; m >>= 1) pk = fmaxf(pk, shfl_xor(pk, m));
    if (t == 0) p.pk[(long)b * p.pk_stride + blockIdx.y] = pk;
}
// the sum of the 64 partial sums and counts, by thread 0, in lane order
NTTS_D void loud_total(const double* red, const int* cnt, double* s, int* c) {
    *s = 0.0; *c = 0;
    for (int i = 0; i < kLoudLanes; ++i) { *s += red[i]; *c += cnt[i]; }
}
// grid (B), one wave: the two gates over the row's blocks, then L, the peak and the gain
NTTS_KERNEL(64) void wav_loud_gate_kernel(WavLoudArgs p) {
    NTTS_SHARED double red[kLoudLanes];
    NTTS_SHARED int cnt[kLoudLanes];
    NTTS_SHARED double gam[1];
    const int b = blockIdx.x, t = threadIdx.x;
    const long n = (long)p.lens[b] * p.len_mul;
    const long J = n / kLoudSub, nb = J >= 4 ? J - 3 : 0;
    const double* z = p.z + (long)b * p.z_stride;
    float pk = 0.f;
    for (int y = t; y < p.pk_stride; y += kLoudLanes) pk = fmaxf(pk, p.pk[(long)b * p.pk_stride + y]);
    for (int m = 32; m >= 1; m >>= 1) pk = fmaxf(pk, shfl_xor(pk, m));
    double s = 0.0;
    int c = 0;
    for (long i = t; i < nb; i += kLoudLanes) {             // the absolute gate
        const double P = (z[i] + z[i + 1] + z[i + 2] + z[i + 3]) * 0.25;
        if (-0.691 + 10.0 * log10(P) > -70.0) { s += P; ++c; }
    }
    red[t] = s; cnt[t] = c;
    sync();
    if (t == 0) {
        loud_total(red, cnt, &s, &c);
        gam[0] = c > 0 ? -0.691 + 10.0 * log10(s / c) - 10.0 : (double)NAN;
    }
    sync();
    const double gamma = gam[0];
    s = 0.0; c = 0;
    for (long i = t; i < nb; i += kLoudLanes) {             // the relative gate (nothing passes a NaN threshold)
        const double P = (z[i] + z[i + 1] + z[i + 2] + z[i + 3]) * 0.25;
        const double l = -0.691 + 10.0 * log10(P);
        if (l > -70.0 && l > gamma) { s += P; ++c; }
    }
    red[t] = s; cnt[t] = c;
    sync();
    if (t != 0) return;
    loud_total(red, cnt, &s, &c);
    const double L = (c > 0 && pk <= 3.402823466e38f) ? -0.691 + 10.0 * log10(s / c) : (double)NAN;
    float g = 1.0f;
    const float* par = p.par ? p.par + 4L * b : nullptr;
    if (par && par[0] != 0.f && L == L) {
        double gd = fmin(pow(10.0, ((double)par[1] - L) / 20.0), pow(10.0, (double)par[3] / 20.0));
        if (pk > 0.f) gd = fmin(gd, pow(10.0, (double)par[2] / 20.0) / (double)pk);
        g = (float)gd;
    }
    p.res[3L * b] = L; p.res[3L * b + 1] = (double)pk; p.res[3L * b + 2] = (double)g;
}
// grid (B, ceil(longest row / 1024)): x *= g in place; a row whose gain is 1 is not touched
NTTS_KERNEL(256) void wav_loud_apply_kernel(WavLoudArgs p) {
    const int b = blockIdx.x;
    const float g = (float)p.res[3L * b + 2];
    if (g == 1.0f) return;
    const long n = (long)p.lens[b] * p.len_mul;
    float* x = p.io + (long)b * p.stride;
    for (int k = 0; k < 4; ++k) {
        const long i = (long)blockIdx.y * 1024 + k * 256 + threadIdx.x;
        if (i < n) x[i] = x[i] * g;
    }
}

}  // namespace ntts
