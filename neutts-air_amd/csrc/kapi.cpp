// kapi.cpp -- kernel-level C entry points (parity tests, micro-benchmarks).  Device pointers in,
// NULL stream, blocking.  See include/neutts_hip.h.
#include <ntts/dev.h>

#include "../../include/neutts_hip.h"
#include "kernels/attn_prefill.h"
#include "kernels/gemm.h"
#include "kernels/gemv.h"
#include "kernels/norm.h"
#include "kernels/sample.h"
#include "kernels/score.h"

#include <string.h>

#include <vector>

using namespace ntts;

extern "C" int ntts_k_gemm_bf16(const void* A, int64_t lda, const void* W, const void* bias, void* C, int64_t ldc,
                                int32_t M, int32_t N, int32_t K, int32_t variant) {
    if (!A || !W || !C || M < 1 || N < 1 || K < 64 || (K % 64) || (lda % 8) || (ldc % 8)) return NTTS_EINVAL;
    GemmArgs a{};
    a.X = (const bf16_t*)A; a.ldx = lda; a.W = (const bf16_t*)W; a.ldw = K; a.bias = (const bf16_t*)bias;
    a.out = C; a.ldo = ldc; a.M = M; a.N = N; a.K = K;
    if (variant == 0) variant = M > 64 ? 1 : 2;
    if (variant == 1) NTTS_GEMM_L(EPI_BF16, a, 1, (hipStream_t)0);
    else if (variant == 2) NTTS_GEMM_S(EPI_BF16, a, 1, (hipStream_t)0);
    else if (variant == 4) NTTS_GEMM_XL(EPI_BF16, a, 1, (hipStream_t)0);
    else if (variant == 5) gemm_launch<4, 4, 4, EPI_BF16, 4, 0, 32>(a, 1, (hipStream_t)0);   // XL tile, 4 ring slots of K = 32
    else if (variant == 6) gemm_launch<2, 2, 4, EPI_BF16, 3, 0, 32>(a, 1, (hipStream_t)0);   // L tile, 3 ring slots of K = 32
    else if (variant == 7) gemm_launch<4, 3, 4, EPI_BF16, 2, 0, 64, false, false, 6>(a, 1, (hipStream_t)0);   // natural-order 256 x 288 tile, 12 waves (prefill QKV)
    else if (variant == 8) gemm_launch<4, 3, 5, EPI_BF16, 2>(a, 1, (hipStream_t)0);   // 320 x 192, 12 waves (80 x 64 per wave): decode gate/up and lm_head of 576- / 640- / 896-row engines
    else if (variant == 9) gemm_launch<4, 2, 5, EPI_BF16, 2>(a, 1, (hipStream_t)0);   // 320 x 128, 8 waves
    else if (variant == 3) {  // split-K slabs reduced by the norm kernel (the decode o_proj / down_proj path)
        if (bias || (N % 16) || ldc != N) return NTTS_EINVAL;
        const int ks = 4, ns = gemm_nsplit(K, ks);
        float* slabs = nullptr;
        if (hipMalloc((void**)&slabs, (size_t)ns * M * N * sizeof(float)) != hipSuccess) return NTTS_ENOMEM;
        a.out = slabs; a.ldo = N;
        NTTS_GEMM_S(EPI_SPLITK, a, ks, (hipStream_t)0);
        NormArgs n{};
        n.slabs = slabs; n.nslab = ns; n.slab_rows = M; n.resid_out = (bf16_t*)C; n.M = M; n.H = N;
        add_rmsnorm_launch(n, (hipStream_t)0);
        if (hipDeviceSynchronize() != hipSuccess) { hipFree(slabs); return NTTS_EHIP; }
        hipFree(slabs);
    } else return NTTS_EINVAL;
    if (hipDeviceSynchronize() != hipSuccess) return NTTS_EHIP;
    return hipGetLastError() == hipSuccess ? NTTS_OK : NTTS_EHIP;
}

// ---- fp8 probes: the conversion the producers use, and one fp8 GEMM (row-major e4m3 operands), for tests against torch
NTTS_KERNEL(256) void fp8_quantize_kernel(const float* in, unsigned char* out, long n, float inv_scale) {
    const long i = ((long)blockIdx.x * 256 + threadIdx.x) * 2;
    if (i + 1 < n) { const unsigned short q = f2fp8x2(in[i] * inv_scale, in[i + 1] * inv_scale); out[i] = (unsigned char)(q & 0xff); out[i + 1] = (unsigned char)(q >> 8); }
    else if (i < n) out[i] = f2fp8c(in[i] * inv_scale);
}
extern "C" int ntts_k_fp8_quantize(const float* in_dev, void* out_dev, int64_t n, float inv_scale) {
    if (!in_dev || !out_dev || n < 1) return NTTS_EINVAL;
    NTTS_LAUNCH((fp8_quantize_kernel), dim3((unsigned)((n + 511) / 512)), dim3(256), (hipStream_t)0, in_dev, (unsigned char*)out_dev, (long)n, inv_scale);
    if (hipDeviceSynchronize() != hipSuccess) return NTTS_EHIP;
    return hipGetLastError() == hipSuccess ? NTTS_OK : NTTS_EHIP;
}
extern "C" int ntts_k_gemm_fp8(const void* A, const void* W, const float* wscale, float xscale, const void* bias, void* C,
                               int32_t M, int32_t N, int32_t K, int32_t variant) {
    if (!A || !W || !wscale || !C || M < 1 || N < 1 || K < 128 || (K % 128) || (N % 8)) return NTTS_EINVAL;
    GemmArgs a{};
    a.X = (const bf16_t*)A; a.ldx = K; a.W = (const bf16_t*)W; a.ldw = K; a.bias = (const bf16_t*)bias;
    a.out = C; a.ldo = N; a.M = M; a.N = N; a.K = K; a.wscale = wscale; a.xscale = xscale;
    if (variant == 2) gemm_launch<4, 1, 1, EPI_BF16, 4, 0, 64, false, true>(a, 1, (hipStream_t)0);          // 64 x 64
    else if (variant == 4) gemm_launch<4, 4, 4, EPI_BF16, 2, 0, 64, false, true>(a, 1, (hipStream_t)0);     // 256 x 256
    else gemm_launch<2, 2, 4, EPI_BF16, 2, 0, 64, false, true>(a, 1, (hipStream_t)0);                       // 128 x 128
    if (hipDeviceSynchronize() != hipSuccess) return NTTS_EHIP;
    return hipGetLastError() == hipSuccess ? NTTS_OK : NTTS_EHIP;
}

extern "C" int ntts_k_rmsnorm_bf16(const void* x, const void* w, void* y, int32_t rows, int32_t cols, float eps) {
    if (!x || !w || !y || rows < 1 || cols < 8 || (cols % 8) || cols > 2048) return NTTS_EINVAL;
    NormArgs n{};
    n.o_bf16 = (const bf16_t*)x; n.norm_w = (const bf16_t*)w; n.normed_out = (bf16_t*)y; n.M = rows; n.H = cols; n.eps = eps;
    add_rmsnorm_launch(n, (hipStream_t)0);
    if (hipDeviceSynchronize() != hipSuccess) return NTTS_EHIP;
    return hipGetLastError() == hipSuccess ? NTTS_OK : NTTS_EHIP;
}

NTTS_KERNEL(256) void membw_copy_kernel(const u32x4* src, u32x4* dst, long n) {
    for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long)gridDim.x * 256) dst[i] = src[i];
}

extern "C" int ntts_k_membw(size_t bytes, int32_t iters, double* gbps) {
    if (!gbps || bytes < 4096 || iters < 1) return NTTS_EINVAL;
    void *a = nullptr, *b = nullptr;
    if (hipMalloc(&a, bytes) != hipSuccess || hipMalloc(&b, bytes) != hipSuccess) { if (a) hipFree(a); return NTTS_ENOMEM; }
    hipMemset(a, 1, bytes);
    hipEvent_t e0, e1;
    hipEventCreate(&e0); hipEventCreate(&e1);
    const long n = bytes / 16;
    NTTS_LAUNCH((membw_copy_kernel), dim3(2048), dim3(256), (hipStream_t)0, (const u32x4*)a, (u32x4*)b, n);
    hipEventRecord(e0, 0);
    for (int i = 0; i < iters; ++i) NTTS_LAUNCH((membw_copy_kernel), dim3(2048), dim3(256), (hipStream_t)0, (const u32x4*)a, (u32x4*)b, n);
    hipEventRecord(e1, 0);
    hipEventSynchronize(e1);
    float ms = 0;
    hipEventElapsedTime(&ms, e0, e1);
    *gbps = ms > 0 ? 2.0 * (double)(n * 16) * iters / (ms * 1e-3) / 1e9 : 0;
    hipEventDestroy(e0); hipEventDestroy(e1);
    hipFree(a); hipFree(b);
    return hipDeviceSynchronize() == hipSuccess ? NTTS_OK : NTTS_EHIP;
}

// Micro-benchmark of one GEMM tile configuration (tools/ubench_gemm.py): `copies` rotating weight buffers keep W
// HBM-cold when copies * N * K * 2 B exceeds the 256 MB Infinity Cache.  config: tile family, abl: ablation bits
// of gemm_kernel.  Returns the average microseconds per launch (back-to-back launches on the NULL stream).
NTTS_KERNEL(64) void empty_kernel(int* p) { if (p && threadIdx.x == 12345) *p = 0; }
// touch `n16` 16-byte words so that they are resident in the memory-side cache (and this XCD's L2) afterwards
NTTS_KERNEL(256) void prefetch_kernel(const u32x4* src, long n16, int* sink) {
    unsigned int acc = 0;
    for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < n16; i += (long)gridDim.x * 256) acc ^= src[i][0];
    if (acc == 0x12345678u && sink) *sink = 1;
}

NTTS_KERNEL(256) void random_fill_kernel(bf16_t* dst, long n, unsigned int seed) {
    for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long)gridDim.x * 256) {
        unsigned int h = (unsigned int)i * 0x9e3779b1u + seed;
        h ^= h >> 15; h *= 0x2c1b3c6du; h ^= h >> 12; h *= 0x297a2d39u; h ^= h >> 15;
        // sign + exponent 120 .. 127 (|v| in [2^-7, 2)) + 7 random mantissa bits: a wide spread of magnitudes, no inf / nan
        dst[i] = (bf16_t)(((h & 1u) << 15) | ((120u + ((h >> 1) & 7u)) << 7) | ((h >> 4) & 0x7fu));
    }
}

template <int WM, int WN, int TM, int NS, int BK = 64>
static void probe_launch(const GemmArgs& a, int ks, int abl) {
    constexpr int EPI = EPI_BF16;
    switch (abl) {
        case 1: gemm_launch<WM, WN, TM, EPI, NS, 1, BK>(a, ks, 0); break;
        case 2: gemm_launch<WM, WN, TM, EPI, NS, 2, BK>(a, ks, 0); break;
        case 3: gemm_launch<WM, WN, TM, EPI, NS, 3, BK>(a, ks, 0); break;
        case 4: gemm_launch<WM, WN, TM, EPI, NS, 4, BK>(a, ks, 0); break;
        case 7: gemm_launch<WM, WN, TM, EPI, NS, 7, BK>(a, ks, 0); break;
        default: gemm_launch<WM, WN, TM, EPI, NS, 0, BK>(a, ks, 0); break;
    }
}

static void probe_dispatch(int config, const GemmArgs& a, int ks, int abl) {
    switch (config) {
        case 0: NTTS_LAUNCH((empty_kernel), dim3(256), dim3(64), (hipStream_t)0, (int*)nullptr); break;
        case 10: probe_launch<4, 1, 1, 2>(a, ks, abl); break;   // 64 x 64, 4 waves
        case 11: probe_launch<4, 1, 1, 3>(a, ks, abl); break;
        case 12: probe_launch<4, 1, 1, 4>(a, ks, abl); break;
        case 13: probe_launch<4, 1, 1, 6>(a, ks, abl); break;
        case 20: probe_launch<2, 1, 1, 4>(a, ks, abl); break;   // 32 x 64, 2 waves
        case 21: probe_launch<2, 1, 2, 4>(a, ks, abl); break;   // 64 x 64, 2 waves
        case 22: probe_launch<1, 1, 4, 4>(a, ks, abl); break;   // 64 x 64, 1 wave
        case 23: probe_launch<2, 2, 2, 3>(a, ks, abl); break;   // 64 x 128, 4 waves
        case 24: probe_launch<4, 2, 1, 3>(a, ks, abl); break;   // 64 x 128, 8 waves
        case 25: probe_launch<8, 1, 1, 3>(a, ks, abl); break;   // 128 x 64, 8 waves
        case 26: probe_launch<4, 1, 2, 3>(a, ks, abl); break;   // 128 x 64, 4 waves
        case 30: probe_launch<2, 2, 4, 2>(a, ks, abl); break;   // 128 x 128, 4 waves (prefill tile)
        case 31: probe_launch<2, 2, 4, 3>(a, ks, abl); break;
        case 40: probe_launch<4, 2, 4, 2>(a, ks, abl); break;   // 256 x 128, 8 waves
        case 41: probe_launch<2, 4, 4, 2>(a, ks, abl); break;   // 128 x 256, 8 waves
        case 42: probe_launch<4, 4, 4, 2>(a, ks, abl); break;   // 256 x 256, 16 waves
        case 43: probe_launch<4, 2, 4, 3>(a, ks, abl); break;   // 256 x 128, 8 waves, 3 stages (144 KB)
        case 44: probe_launch<2, 2, 8, 2>(a, ks, abl); break;   // 256 x 128, 4 waves (128 x 64 per wave)
        case 45: probe_launch<2, 4, 8, 2>(a, ks, abl); break;   // 256 x 256, 8 waves (128 x 64 per wave)
        case 46: probe_launch<4, 4, 4, 4, 32>(a, ks, abl); break;   // 256 x 256, 16 waves, 4 slots of K = 32 (128 KB)
        case 47: probe_launch<4, 4, 4, 3, 32>(a, ks, abl); break;   // ... 3 slots (96 KB)
        case 48: probe_launch<2, 4, 8, 4, 32>(a, ks, abl); break;   // 256 x 256, 8 waves, 4 slots of K = 32
        case 49: probe_launch<2, 2, 4, 4, 32>(a, ks, abl); break;   // 128 x 128, 4 waves, 4 slots of K = 32 (64 KB: 2 blocks / CU)
        case 50: probe_launch<4, 1, 4, 3>(a, ks, abl); break;   // 256 x 64, 4 waves: all decode rows in one block
        case 51: probe_launch<8, 1, 2, 3>(a, ks, abl); break;   // 256 x 64, 8 waves
        case 52: probe_launch<8, 1, 2, 2>(a, ks, abl); break;
        case 53: probe_launch<8, 2, 2, 2>(a, ks, abl); break;   // 256 x 128, 16 waves
        case 54: probe_launch<4, 2, 2, 3>(a, ks, abl); break;   // 128 x 128, 8 waves
        case 55: probe_launch<4, 4, 5, 2>(a, ks, abl); break;   // 320 x 256, 16 waves (80 x 64 per wave): 11 % fewer LDS-DMA bytes per FLOP than 256 x 256; 144 KB
        case 57: probe_launch<2, 4, 10, 2>(a, ks, abl); break;  // 320 x 256, 8 waves (160 x 64 per wave, 2 waves per SIMD: up to 256 registers each)
        case 58: probe_launch<2, 4, 12, 2>(a, ks, abl); break;  // 384 x 256, 8 waves (192 x 64 per wave)
        case 59: probe_launch<4, 3, 5, 2>(a, ks, abl); break;   // 320 x 192, 12 waves (80 x 64 per wave): 128 KB
        case 60: probe_launch<4, 2, 5, 2>(a, ks, abl); break;   // 320 x 128, 8 waves: 112 KB
        case 56: probe_launch<4, 4, 6, 2>(a, ks, abl); break;   // 384 x 256, 16 waves (96 x 64 per wave): 17 % fewer; 160 KB = all of a CU's LDS
        default: break;
    }
}

extern "C" int ntts_k_gemm_probe(int32_t M, int32_t N, int32_t K, int32_t config, int32_t abl, int32_t copies, int32_t iters,
                                 double* us) {
    if (!us || M < 1 || N < 16 || K < 64 || (K % 64) || copies < 1 || iters < 1) return NTTS_EINVAL;
    bf16_t *X = nullptr, *W = nullptr, *C = nullptr;
    const size_t wn = (size_t)N * K;
    if (hipMalloc((void**)&X, (size_t)M * K * 2) != hipSuccess || hipMalloc((void**)&W, wn * 2 * copies) != hipSuccess ||
        hipMalloc((void**)&C, (size_t)M * N * 2) != hipSuccess)
        return NTTS_ENOMEM;
    hipMemset(X, 0x11, (size_t)M * K * 2);
    hipMemset(W, 0x22, wn * 2 * copies);
    if (abl & 32) {   // operands with the statistics of real activations / weights (hashed bf16 values in (-2, 2)) instead of one constant:
                      // the matrix cores' power draw -- and with it the clock the chip sustains -- depends on how many bits toggle
        NTTS_LAUNCH((random_fill_kernel), dim3(2048), dim3(256), (hipStream_t)0, X, (long)M * K, 0x9e3779b9u);
        NTTS_LAUNCH((random_fill_kernel), dim3(2048), dim3(256), (hipStream_t)0, W, (long)(wn * copies), 0x85ebca6bu);
    }
    hipEvent_t e0, e1;
    hipEventCreate(&e0); hipEventCreate(&e1);
    const int ks = config >= 1000 ? config / 1000 : 1;   // config = 1000 * ksplit + tile: the K split in gridDim.y (timing only: every split stores the same bf16 tile)
    config %= 1000;
    const bool pf = (abl & 8) != 0;
    const int tile_major = (abl & 16) ? 1 : 0;     // weights addressed tile-major (same bytes, sequential per workgroup)
    const bool x_ktm = (abl & 64) != 0;            // X addressed k-tile-major ([K / 64][M][64]: a block's X tile is one contiguous run; timing only)
    abl &= 7;   // (bits 8, 16, 32, 64 are handled here)
    auto run = [&](int i) {
        if (pf) NTTS_LAUNCH((prefetch_kernel), dim3(256), dim3(256), (hipStream_t)0, (const u32x4*)(W + (size_t)((i + 1) % copies) * wn), (long)(wn / 8), (int*)nullptr);
        GemmArgs a{};
        a.X = X; a.ldx = K; a.W = W + (size_t)(i % copies) * wn; a.ldw = K; a.out = C; a.ldo = N; a.M = M; a.N = N; a.K = K;
        a.w_tile_major = tile_major;
        if (x_ktm) { a.ldx = 64; a.x_kt_stride = (long)M * 128; }
        probe_dispatch(config, a, ks, abl);
    };
    for (int i = 0; i < copies && i < 8; ++i) run(i);
    hipEventRecord(e0, 0);
    for (int i = 0; i < iters; ++i) run(i);
    hipEventRecord(e1, 0);
    hipEventSynchronize(e1);
    float ms = 0;
    hipEventElapsedTime(&ms, e0, e1);
    *us = (double)ms * 1e3 / iters;
    hipEventDestroy(e0); hipEventDestroy(e1);
    hipFree(X); hipFree(W); hipFree(C);
    return hipDeviceSynchronize() == hipSuccess && hipGetLastError() == hipSuccess ? NTTS_OK : NTTS_EHIP;
}

// MFMA lane-layout probe (diagnostics): three products whose results spell out which (row, col) each
// (lane, reg) of the accumulator holds and whether A and B agree on the k slot.  Expected, under the
// layout documented in ntts/dev.h:  out[0][l][r] = (l>>4)*4 + r,  out[1][l][r] = l & 15,
// out[2][l][r] = ((l & 15) * 2 + 1) % 32 + 1.
NTTS_KERNEL(64) void mfma_probe_kernel(float* out) {
    const int l = lane_id(), g = l >> 4, c = l & 15;
    for (int probe = 0; probe < 3; ++probe) {
        bf16x8 a, b;
        for (int j = 0; j < 8; ++j) {
            float av, bv;
            if (probe == 0) { av = (g == 0 && j == 0) ? (float)c : 0.f; bv = (g == 0 && j == 0) ? 1.f : 0.f; }
            else if (probe == 1) { av = (g == 0 && j == 0) ? 1.f : 0.f; bv = (g == 0 && j == 0) ? (float)c : 0.f; }
            else { av = (float)(g * 8 + j + 1); bv = (g * 8 + j == (c * 2 + 1) % 32) ? 1.f : 0.f; }
            a[j] = (short)f2bf(av);
            b[j] = (short)f2bf(bv);
        }
        f32x4 d = {0.f, 0.f, 0.f, 0.f};
        d = mfma16(a, b, d);
        for (int r = 0; r < 4; ++r) out[(probe * 64 + l) * 4 + r] = d[r];
    }
}

// ---- launch-chain floor: n dependent launches of a kernel that does (almost) nothing, replayed from one hipGraph like the
//      decode step.  What a chain of n kernels costs before any of them moves a byte.
NTTS_KERNEL(256) void chain_probe_kernel(int* sink) {
    if (threadIdx.x == 0 && sink[blockIdx.x & 1023] == 0x7fffffff) sink[0] = 1;   // one 4-byte load per workgroup, never stores
}
// the smallest kernel that does what every decode kernel must: one HBM-cold 16-byte load per thread, then one 16-byte store
NTTS_KERNEL(256) void chain_touch_kernel(const u32x4* src, u32x4* dst) {
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    u32x4 v = src[i];
    v[0] += 1;
    dst[i] = v;
}
extern "C" int ntts_k_launch_chain_probe(int32_t n_kernels, int32_t grid, int32_t block, int32_t iters, double* us_per_chain) {
    if (!us_per_chain || n_kernels < 1 || n_kernels > 4096 || grid < 1 || (block != 256 && block != -256) || iters < 1) return NTTS_EINVAL;
    const bool touch = block < 0;      // block = -256: chain_touch_kernel, every launch of a replay on its own (cold) 16 B x grid x 256 region
    block = 256;
    if (touch) {
        u32x4 *src = nullptr, *dst = nullptr;
        const size_t per = (size_t)grid * 256, total = per * n_kernels;
        hipStream_t st = nullptr; hipGraph_t g = nullptr; hipGraphExec_t ge = nullptr;
        if (hipMalloc((void**)&src, total * 16) != hipSuccess || hipMalloc((void**)&dst, per * 16) != hipSuccess) { hipFree(src); return NTTS_ENOMEM; }
        hipMemset(src, 1, total * 16);
        int rc = NTTS_EHIP;
        if (hipStreamCreateWithFlags(&st, hipStreamNonBlocking) == hipSuccess && hipStreamBeginCapture(st, hipStreamCaptureModeThreadLocal) == hipSuccess) {
            for (int i = 0; i < n_kernels; ++i) NTTS_LAUNCH((chain_touch_kernel), dim3(grid), dim3(256), st, (const u32x4*)(src + per * i), dst);
            if (hipStreamEndCapture(st, &g) == hipSuccess && g && hipGraphInstantiate(&ge, g, nullptr, nullptr, 0) == hipSuccess) {
                hipEvent_t e0, e1;
                hipEventCreate(&e0); hipEventCreate(&e1);
                for (int i = 0; i < 3; ++i) hipGraphLaunch(ge, st);
                hipEventRecord(e0, st);
                for (int i = 0; i < iters; ++i) hipGraphLaunch(ge, st);
                hipEventRecord(e1, st);
                if (hipEventSynchronize(e1) == hipSuccess) { float ms = 0; hipEventElapsedTime(&ms, e0, e1); *us_per_chain = (double)ms * 1e3 / iters; rc = NTTS_OK; }
                hipEventDestroy(e0); hipEventDestroy(e1);
            }
        }
        if (ge) hipGraphExecDestroy(ge);
        if (g) hipGraphDestroy(g);
        if (st) hipStreamDestroy(st);
        hipFree(src); hipFree(dst);
        (void)hipGetLastError();
        return rc;
    }
    int* sink = nullptr;
    hipStream_t st = nullptr;
    hipGraph_t g = nullptr;
    hipGraphExec_t ge = nullptr;
    if (hipMalloc((void**)&sink, 4096) != hipSuccess) return NTTS_ENOMEM;
    hipMemset(sink, 0, 4096);
    int rc = NTTS_EHIP;
    if (hipStreamCreateWithFlags(&st, hipStreamNonBlocking) == hipSuccess &&
        hipStreamBeginCapture(st, hipStreamCaptureModeThreadLocal) == hipSuccess) {
        for (int i = 0; i < n_kernels; ++i) NTTS_LAUNCH((chain_probe_kernel), dim3(grid), dim3(block), st, sink);
        if (hipStreamEndCapture(st, &g) == hipSuccess && g && hipGraphInstantiate(&ge, g, nullptr, nullptr, 0) == hipSuccess) {
            hipEvent_t e0, e1;
            hipEventCreate(&e0); hipEventCreate(&e1);
            for (int i = 0; i < 3; ++i) hipGraphLaunch(ge, st);
            hipEventRecord(e0, st);
            for (int i = 0; i < iters; ++i) hipGraphLaunch(ge, st);
            hipEventRecord(e1, st);
            if (hipEventSynchronize(e1) == hipSuccess) {
                float ms = 0;
                hipEventElapsedTime(&ms, e0, e1);
                *us_per_chain = (double)ms * 1e3 / iters;
                rc = NTTS_OK;
            }
            hipEventDestroy(e0); hipEventDestroy(e1);
        }
    }
    if (ge) hipGraphExecDestroy(ge);
    if (g) hipGraphDestroy(g);
    if (st) hipStreamDestroy(st);
    hipFree(sink);
    (void)hipGetLastError();
    return rc;
}

NTTS_KERNEL(256) void silu_probe_kernel(const bf16_t* in, bf16_t* out, long n, int variant) {
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    if (variant == 2) {   // the packed form of the GEMM epilogues with their guard: pairs (i, i ^ 1), silu_fast below -86.5
        const float a = bf2f(in[i]), b = bf2f(in[(i ^ 1) < n ? (i ^ 1) : i]);
        if (a < -86.5f || b < -86.5f) out[i] = f2bf(silu_fast(a));
        else out[i] = f2bf(silu_fast2(f32x2{a, b})[0]);
        return;
    }
    out[i] = f2bf(variant ? silu_fast(bf2f(in[i])) : silu_f(bf2f(in[i])));
}
extern "C" int ntts_k_silu_probe(const void* in_bf16_dev, void* out_bf16_dev, int64_t n, int32_t variant) {
    if (!in_bf16_dev || !out_bf16_dev || n < 1) return NTTS_EINVAL;
    NTTS_LAUNCH((silu_probe_kernel), dim3((unsigned)((n + 255) / 256)), dim3(256), (hipStream_t)0, (const bf16_t*)in_bf16_dev,
                (bf16_t*)out_bf16_dev, (long)n, (int)variant);
    return hipDeviceSynchronize() == hipSuccess && hipGetLastError() == hipSuccess ? NTTS_OK : NTTS_EHIP;
}

// ---- sampler probe: sample_topk_row (the decode step's token choice) on caller-supplied rows, one workgroup per row like sample_greedy_kernel
struct SampleProbeArgs {
    const bf16_t* logits;    // [rows][ld]
    long ld;
    int vocab;
    const float* part_val;   // [rows][n_part] group maxima (group_max_kernel), or null: full-row path
    int n_part, part_width;
    const int* top_k;        // [rows]
    const float* fparams;    // [3][rows]: temperature, top_p, min_p
    const unsigned int* seed;   // [rows][2]
    unsigned int step;
    int* token;              // [rows]
    int* n_surv;             // [rows]
    int* surv;               // [rows][kSampleCap]
    int rows;
};
// part_val[row][g] = max of columns [g * gw, (g + 1) * gw) of the row (what the lm_head epilogue leaves behind, SampleArgs::part_val)
NTTS_KERNEL(256) void group_max_kernel(SampleProbeArgs p, float* part_val) {
    const bf16_t* row = p.logits + (long)blockIdx.x * p.ld;
    for (int g = threadIdx.x; g < p.n_part; g += 256) {
        float m = -INFINITY;
        for (int c = g * p.part_width; c < (g + 1) * p.part_width && c < p.vocab; ++c) m = fmaxf(m, bf2f(row[c]));
        part_val[(long)blockIdx.x * p.n_part + g] = m;
    }
}
NTTS_KERNEL(256) void sample_probe_kernel(SampleProbeArgs p) {
    const int b = blockIdx.x;
    const int tok = sample_topk_row(p.logits + (long)b * p.ld, p.vocab, p.top_k[b], p.fparams[b], p.fparams[p.rows + b], p.fparams[2 * p.rows + b],
                                    p.seed[2 * b], p.seed[2 * b + 1], p.step, p.part_val ? p.part_val + (long)b * p.n_part : nullptr, p.n_part,
                                    p.part_width, p.surv + (long)b * kSampleCap, p.n_surv + b);
    if (threadIdx.x == 0) p.token[b] = tok;
}
extern "C" int ntts_k_sample_probe(const void* logits_dev, int64_t ld_logits, int32_t rows, int32_t vocab, int32_t group_width, const int32_t* top_k,
                                   const float* temperature, const float* top_p, const float* min_p, const uint64_t* seed, int32_t step,
                                   int32_t* token_out, int32_t* n_out, int32_t* ids_out) {
    if (!logits_dev || !top_k || !temperature || !top_p || !min_p || !seed || !token_out || !n_out || !ids_out) return NTTS_EINVAL;
    if (rows < 1 || vocab < 1 || ld_logits < vocab || (ld_logits % 8) || ((uintptr_t)logits_dev & 15) || step < 0) return NTTS_EINVAL;
    if (group_width < 0 || (group_width % 8)) return NTTS_EINVAL;
    for (int r = 0; r < rows; ++r)
        if (top_k[r] < 1 || !(temperature[r] > 0.f) || !(top_p[r] > 0.f && top_p[r] <= 1.0f) || !(min_p[r] >= 0.f && min_p[r] <= 1.0f)) return NTTS_EINVAL;
    const int n_part = group_width ? (vocab + group_width - 1) / group_width : 0;
    // one device block: [top_k rows][seed 2 rows][token rows][n_surv rows][surv rows * cap] ints | [temperature, top_p, min_p: 3 rows][part_val rows * n_part] floats
    const size_t n_int = (size_t)rows * (5 + kSampleCap), n_flt = (size_t)rows * (3 + n_part);
    std::vector<int> hi(n_int, 0);
    std::vector<float> hf((size_t)rows * 3);
    for (int r = 0; r < rows; ++r) {
        hi[r] = top_k[r];
        hi[rows + 2 * r] = (int)(uint32_t)seed[r];
        hi[rows + 2 * r + 1] = (int)(uint32_t)(seed[r] >> 32);
        hf[r] = temperature[r]; hf[rows + r] = top_p[r]; hf[2 * rows + r] = min_p[r];
    }
    int* di = nullptr;
    float* df = nullptr;
    if (hipMalloc((void**)&di, n_int * sizeof(int)) != hipSuccess) return NTTS_ENOMEM;
    if (hipMalloc((void**)&df, n_flt * sizeof(float)) != hipSuccess) { hipFree(di); return NTTS_ENOMEM; }
    int rc = NTTS_EHIP;
    if (hipMemcpy(di, hi.data(), n_int * sizeof(int), hipMemcpyHostToDevice) == hipSuccess &&
        hipMemcpy(df, hf.data(), hf.size() * sizeof(float), hipMemcpyHostToDevice) == hipSuccess) {
        SampleProbeArgs a{};
        a.logits = (const bf16_t*)logits_dev; a.ld = ld_logits; a.vocab = vocab; a.n_part = n_part; a.part_width = group_width;
        a.top_k = di; a.seed = (const unsigned int*)(di + rows); a.token = di + 3 * rows; a.n_surv = di + 4 * rows; a.surv = di + 5 * rows;
        a.fparams = df; a.step = (unsigned int)step; a.rows = rows;
        if (group_width) {
            NTTS_LAUNCH((group_max_kernel), dim3(rows), dim3(256), (hipStream_t)0, a, df + 3 * (size_t)rows);
            a.part_val = df + 3 * (size_t)rows;
        }
        NTTS_LAUNCH((sample_probe_kernel), dim3(rows), dim3(256), (hipStream_t)0, a);
        if (hipDeviceSynchronize() == hipSuccess && hipGetLastError() == hipSuccess &&
            hipMemcpy(hi.data(), di, n_int * sizeof(int), hipMemcpyDeviceToHost) == hipSuccess) {
            for (int r = 0; r < rows; ++r) {
                token_out[r] = hi[3 * rows + r];
                n_out[r] = hi[4 * rows + r];
                for (int a2 = 0; a2 < kSampleCap; ++a2) ids_out[(size_t)r * kSampleCap + a2] = hi[5 * (size_t)rows + (size_t)r * kSampleCap + a2];
            }
            rc = NTTS_OK;
        }
    }
    hipFree(di); hipFree(df);
    return rc;
}

namespace {
struct ProbeBuf { void* p = nullptr; ~ProbeBuf() { if (p) (void)hipFree(p); } };   // a device allocation of a probe, freed on every return path
}

// ---- whole-vocabulary sampler probe: sample_full_row (top_k = -1) on caller-supplied rows; the survivors come back as a bitmap
struct SampleFullProbeArgs {
    SampleProbeArgs s;                 // logits, ld, vocab, part_val / n_part / part_width, fparams, seed, step, token, n_surv, rows (top_k, surv unused)
    unsigned char* keep;               // [rows][keep_pitch] bytes: bit c & 7 of byte c >> 3
    long keep_pitch;
    unsigned long long* total;         // [rows]
};
NTTS_KERNEL(256) void sample_full_probe_kernel(SampleFullProbeArgs a) {
    const SampleProbeArgs& p = a.s;
    const int b = blockIdx.x;
    const int tok = sample_full_row(p.logits + (long)b * p.ld, p.vocab, p.fparams[b], p.fparams[p.rows + b], p.fparams[2 * p.rows + b], p.seed[2 * b],
                                    p.seed[2 * b + 1], p.step, p.part_val ? p.part_val + (long)b * p.n_part : nullptr, p.n_part,
                                    a.keep + (long)b * a.keep_pitch, p.n_surv + b, a.total + b);
    if (threadIdx.x == 0) p.token[b] = tok;
}
extern "C" int ntts_k_sample_full_probe(const void* logits_dev, int64_t ld_logits, int32_t rows, int32_t vocab, int32_t group_width,
                                        const float* temperature, const float* top_p, const float* min_p, const uint64_t* seed, int32_t step,
                                        int32_t* token_out, int32_t* n_out, uint32_t* keep_bits_out, uint64_t* total_out) {
    if (!logits_dev || !temperature || !top_p || !min_p || !seed || !token_out || !n_out || !keep_bits_out || !total_out) return NTTS_EINVAL;
    if (rows < 1 || vocab < 1 || ld_logits < vocab || (ld_logits % 8) || ((uintptr_t)logits_dev & 15) || step < 0) return NTTS_EINVAL;
    if (group_width < 0 || (group_width % 8)) return NTTS_EINVAL;
    for (int r = 0; r < rows; ++r)
        if (!(temperature[r] > 0.f) || !(top_p[r] > 0.f && top_p[r] <= 1.0f) || !(min_p[r] >= 0.f && min_p[r] <= 1.0f)) return NTTS_EINVAL;
    const int n_part = group_width ? (vocab + group_width - 1) / group_width : 0;
    const size_t kw = ((size_t)vocab + 31) / 32;                    // bitmap words per row
    // device blocks: [seed 2 rows][token rows][n_surv rows] ints | [temperature, top_p, min_p: 3 rows][part_val rows * n_part] floats |
    //                [total rows] 64-bit words, then [rows][kw] bitmap words (zeroed: the kernel writes whole bytes up to column vocab - 1)
    const size_t n_int = (size_t)rows * 4, n_flt = (size_t)rows * (3 + n_part), n_out8 = (size_t)rows * 8 + (size_t)rows * kw * 4;
    std::vector<int> hi(n_int, 0);
    std::vector<float> hf((size_t)rows * 3);
    for (int r = 0; r < rows; ++r) {
        hi[2 * r] = (int)(uint32_t)seed[r];
        hi[2 * r + 1] = (int)(uint32_t)(seed[r] >> 32);
        hf[r] = temperature[r]; hf[rows + r] = top_p[r]; hf[2 * rows + r] = min_p[r];
    }
    ProbeBuf di, df, dk;
    if (hipMalloc(&di.p, n_int * sizeof(int)) != hipSuccess || hipMalloc(&df.p, n_flt * sizeof(float)) != hipSuccess ||
        hipMalloc(&dk.p, n_out8) != hipSuccess)
        return NTTS_ENOMEM;
    if (hipMemcpy(di.p, hi.data(), n_int * sizeof(int), hipMemcpyHostToDevice) != hipSuccess ||
        hipMemcpy(df.p, hf.data(), hf.size() * sizeof(float), hipMemcpyHostToDevice) != hipSuccess || hipMemset(dk.p, 0, n_out8) != hipSuccess)
        return NTTS_EHIP;
    SampleFullProbeArgs a{};
    int* dip = (int*)di.p;
    float* dfp = (float*)df.p;
    a.s.logits = (const bf16_t*)logits_dev; a.s.ld = ld_logits; a.s.vocab = vocab; a.s.n_part = n_part; a.s.part_width = group_width;
    a.s.seed = (const unsigned int*)dip; a.s.token = dip + 2 * rows; a.s.n_surv = dip + 3 * rows;
    a.s.fparams = dfp; a.s.step = (unsigned int)step; a.s.rows = rows;
    a.total = (unsigned long long*)dk.p; a.keep = (unsigned char*)dk.p + (size_t)rows * 8; a.keep_pitch = (long)(kw * 4);
    if (group_width) {
        NTTS_LAUNCH((group_max_kernel), dim3(rows), dim3(256), (hipStream_t)0, a.s, dfp + 3 * (size_t)rows);
        a.s.part_val = dfp + 3 * (size_t)rows;
    }
    NTTS_LAUNCH((sample_full_probe_kernel), dim3(rows), dim3(256), (hipStream_t)0, a);
    if (hipDeviceSynchronize() != hipSuccess || hipGetLastError() != hipSuccess) return NTTS_EHIP;
    if (hipMemcpy(hi.data(), di.p, n_int * sizeof(int), hipMemcpyDeviceToHost) != hipSuccess ||
        hipMemcpy(total_out, dk.p, (size_t)rows * 8, hipMemcpyDeviceToHost) != hipSuccess ||
        hipMemcpy(keep_bits_out, (unsigned char*)dk.p + (size_t)rows * 8, (size_t)rows * kw * 4, hipMemcpyDeviceToHost) != hipSuccess)
        return NTTS_EHIP;
    for (int r = 0; r < rows; ++r) { token_out[r] = hi[2 * rows + r]; n_out[r] = hi[3 * rows + r]; }
    return NTTS_OK;
}

extern "C" int ntts_k_mfma_probe(float* out_dev_768) {
    if (!out_dev_768) return NTTS_EINVAL;
    NTTS_LAUNCH((mfma_probe_kernel), dim3(1), dim3(64), (hipStream_t)0, out_dev_768);
    return hipDeviceSynchronize() == hipSuccess ? NTTS_OK : NTTS_EHIP;
}

// ---- operands of the lm_head probes, packed by the kernels the engine packs its head with: W [N][K] bf16 row-major -> tile-major bf16, or (fp8) e4m3
//      bytes + per-row scales, X then quantised to e4m3 at the static scale xscale.  *X_out = the rows the launch reads.
namespace {
bool probe_alloc(ProbeBuf& b, size_t bytes) { return hipMalloc(&b.p, bytes) == hipSuccess && hipMemset(b.p, 0, bytes) == hipSuccess; }
struct ProbeOperands { ProbeBuf wt, ws, xq, xf; };
int pack_probe_operands(const void* X_dev, const void* W_dev, int M, int N, int K, int fp8, float xscale, ProbeOperands& o, const bf16_t** X_out) {
    const long Np = ((long)N + 63) / 64 * 64;
    const hipStream_t st = (hipStream_t)0;
    if (!probe_alloc(o.wt, (size_t)Np * K * (fp8 ? 1 : 2))) return NTTS_ENOMEM;
    // (plain pointers for the launches: the emulator's launch captures its arguments by value)
    const void* src = W_dev;
    const int* nomap = nullptr;
    if (fp8) {
        if (!probe_alloc(o.ws, (size_t)Np * 4) || !probe_alloc(o.xq, (size_t)M * K) || !probe_alloc(o.xf, (size_t)M * K * 4)) return NTTS_ENOMEM;
        unsigned char* dst = (unsigned char*)o.wt.p;
        float* sc = (float*)o.ws.p;
        NTTS_LAUNCH((pack_weight_fp8_kernel), dim3((unsigned)N), dim3(256), st, src, 0, dst, sc, nomap, 0L, (long)K);
        std::vector<bf16_t> xb((size_t)M * K);
        std::vector<float> xw((size_t)M * K);
        if (hipMemcpy(xb.data(), X_dev, xb.size() * 2, hipMemcpyDeviceToHost) != hipSuccess) return NTTS_EHIP;
        for (size_t i = 0; i < xb.size(); ++i) { const unsigned int u = (unsigned int)xb[i] << 16; memcpy(&xw[i], &u, 4); }
        if (hipMemcpy(o.xf.p, xw.data(), xw.size() * 4, hipMemcpyHostToDevice) != hipSuccess) return NTTS_EHIP;
        const float* xin = (const float*)o.xf.p;
        unsigned char* xout = (unsigned char*)o.xq.p;
        const long nx = (long)M * K;
        NTTS_LAUNCH((fp8_quantize_kernel), dim3((unsigned)((nx + 511) / 512)), dim3(256), st, xin, xout, nx, 1.0f / xscale);
        *X_out = (const bf16_t*)o.xq.p;
    } else {
        bf16_t* dst = (bf16_t*)o.wt.p;
        NTTS_LAUNCH((pack_weight_kernel), dim3((unsigned)N), dim3(256), st, src, 0, dst, nomap, 0L, (long)K, 1);
        *X_out = (const bf16_t*)X_dev;
    }
    return NTTS_OK;
}
}  // namespace

// ---- the lm_head launch of the decode step (gemm.h lm_head_launch / gemv.h lm_head_gemv_launch) on caller-supplied operands: the penalty epilogue of
//      every tile variant against tests/repetition_spec.py.  The head is packed here by the kernels the engine packs it with.
//      part_sum / row_lse non-null (ntts_k_head_logprob_probe): the launch with the log-sum-exp epilogue, then sample.h's own merge of the partials.
static int head_probe(const void* X_dev, const void* W_dev, int32_t M, int32_t N, int32_t K, int32_t variant, int32_t fp8, float xscale,
                      const uint32_t* seen, const float* rep_pen, const int32_t* mask_eos, float* logits_out,
                      uint16_t* logits_bf16_out, float* part_val, int32_t* part_idx, int32_t part_cap, int32_t* n_part,
                      int32_t* part_width, float* part_sum, float* row_lse) {
    if (!X_dev || !W_dev || !logits_out || !logits_bf16_out || !part_val || !part_idx || !n_part || !part_width) return NTTS_EINVAL;
    if (M < 1 || N < 16 || K < 64 || (K % 64) || (fp8 && (K % 128))) return NTTS_EINVAL;
    if (variant != 0 && variant != 1 && variant != 2 && variant != 4 && variant != 8) return NTTS_EINVAL;
    if ((variant == 4 && fp8) || (variant == 8 && (M > kGemvRows || (N % 16) || K > 1024))) return NTTS_EINVAL;
    if (fp8 && !(xscale > 0.f)) return NTTS_EINVAL;
    if (seen) {
        if (!rep_pen) return NTTS_EINVAL;
        for (int m = 0; m < M; ++m)
            if (!(rep_pen[m] > 0.f && rep_pen[m] <= 3.0e38f)) return NTTS_EINVAL;
    }
    const int width = variant == 8 ? 16 : variant == 4 ? 96 : 64;
    const int np = variant == 8 ? N / 16 : variant == 0 ? (N + 63) / 64 : variant == 4 ? ((N + 287) / 288) * 3 : variant == 2 ? ((N + 255) / 256) * 4 : ((N + 127) / 128) * 2;
    if (part_cap < np) return NTTS_EINVAL;
    const long ldl = ((long)N + 7) / 8 * 8, pitch = seen_pitch_for(N), wsrc = ((long)N + 31) / 32;
    typedef ProbeBuf Buf;
    ProbeOperands ops;
    Buf lg, lb, pv, pi, bm, pen, me, psum, rl;
    auto dalloc = [](Buf& b, size_t bytes) { return probe_alloc(b, bytes); };
    if (!dalloc(lg, (size_t)M * N * 4) || !dalloc(lb, (size_t)M * ldl * 2) || !dalloc(pv, (size_t)M * np * 4) ||
        !dalloc(pi, (size_t)M * np * 4) || !dalloc(me, (size_t)M * 4)) return NTTS_ENOMEM;
    if (part_sum && (!dalloc(psum, (size_t)M * np * 4) || !dalloc(rl, (size_t)M * 2 * 4))) return NTTS_ENOMEM;
    const hipStream_t st = (hipStream_t)0;
    const bf16_t* X = nullptr;
    if (const int rc = pack_probe_operands(X_dev, W_dev, M, N, K, fp8, xscale, ops, &X)) return rc;
    if (mask_eos && hipMemcpy(me.p, mask_eos, (size_t)M * 4, hipMemcpyHostToDevice) != hipSuccess) return NTTS_EHIP;
    if (seen) {
        if (!dalloc(bm, (size_t)M * pitch * 4) || !dalloc(pen, (size_t)M * 4)) return NTTS_ENOMEM;
        for (int m = 0; m < M; ++m)
            if (hipMemcpy((unsigned int*)bm.p + (size_t)m * pitch, seen + (size_t)m * wsrc, (size_t)wsrc * 4, hipMemcpyHostToDevice) != hipSuccess) return NTTS_EHIP;
        if (N % 32) {    // bits past column N - 1 in the caller's last word are not columns: dropped
            std::vector<unsigned int> last(M);
            for (int m = 0; m < M; ++m) last[m] = seen[(size_t)m * wsrc + wsrc - 1] & ((1u << (N % 32)) - 1u);
            for (int m = 0; m < M; ++m)
                if (hipMemcpy((unsigned int*)bm.p + (size_t)m * pitch + wsrc - 1, &last[m], 4, hipMemcpyHostToDevice) != hipSuccess) return NTTS_EHIP;
        }
        if (hipMemcpy(pen.p, rep_pen, (size_t)M * 4, hipMemcpyHostToDevice) != hipSuccess) return NTTS_EHIP;
    }
    if (variant == 8) {
        GemvArgs a{};
        a.X = X; a.ldx = K; a.W = (const bf16_t*)ops.wt.p; a.ldw = K; a.w_tile_major = 1; a.slab_rows = M; a.M = M; a.N = N; a.K = K; a.n_valid = N;
        a.wscale = fp8 ? (const float*)ops.ws.p : nullptr; a.xscale = xscale;
        a.part_val = (float*)pv.p; a.part_idx = (int*)pi.p; a.mask_eos = (const int*)me.p;
        a.logits = (float*)lg.p; a.ld_logits = N; a.logits_bf16 = (bf16_t*)lb.p; a.ld_logits_bf16 = ldl;
        if (seen) { a.seen = (const unsigned int*)bm.p; a.seen_pitch = pitch; a.rep_pen = (const float*)pen.p; }
        a.part_sum = (float*)psum.p;
        lm_head_gemv_launch(a, fp8 != 0, st);
    } else {
        GemmArgs a{};
        a.w_tile_major = 1;
        a.X = X; a.ldx = K; a.W = (const bf16_t*)ops.wt.p; a.ldw = K; a.M = M; a.N = N; a.K = K;
        a.wscale = fp8 ? (const float*)ops.ws.p : nullptr; a.xscale = xscale;
        a.part_val = (float*)pv.p; a.part_idx = (int*)pi.p; a.mask_eos = (const int*)me.p;
        a.logits = (float*)lg.p; a.ld_logits = N; a.logits_bf16 = (bf16_t*)lb.p; a.ld_logits_bf16 = ldl;
        if (seen) { a.seen = (const unsigned int*)bm.p; a.seen_pitch = pitch; a.rep_pen = (const float*)pen.p; }
        a.part_sum = (float*)psum.p;
        lm_head_launch(a, variant, fp8 != 0, st);
    }
    if (part_sum) {   // (M, log S) per row, by the code the sampling kernel merges the partials with
        const float* pvp = (const float*)pv.p;
        const float* psp = (const float*)psum.p;
        float* rlp = (float*)rl.p;
        NTTS_LAUNCH((lse_merge_probe_kernel), dim3((unsigned)M), dim3(256), st, pvp, psp, (int)np, rlp);
    }
    if (hipDeviceSynchronize() != hipSuccess || hipGetLastError() != hipSuccess) return NTTS_EHIP;
    if (hipMemcpy(logits_out, lg.p, (size_t)M * N * 4, hipMemcpyDeviceToHost) != hipSuccess) return NTTS_EHIP;
    if (hipMemcpy2D(logits_bf16_out, (size_t)N * 2, lb.p, (size_t)ldl * 2, (size_t)N * 2, (size_t)M, hipMemcpyDeviceToHost) != hipSuccess) return NTTS_EHIP;
    if (hipMemcpy(part_val, pv.p, (size_t)M * np * 4, hipMemcpyDeviceToHost) != hipSuccess) return NTTS_EHIP;
    if (hipMemcpy(part_idx, pi.p, (size_t)M * np * 4, hipMemcpyDeviceToHost) != hipSuccess) return NTTS_EHIP;
    if (part_sum) {
        if (hipMemcpy(part_sum, psum.p, (size_t)M * np * 4, hipMemcpyDeviceToHost) != hipSuccess) return NTTS_EHIP;
        if (hipMemcpy(row_lse, rl.p, (size_t)M * 2 * 4, hipMemcpyDeviceToHost) != hipSuccess) return NTTS_EHIP;
    }
    *n_part = np;
    *part_width = width;
    return NTTS_OK;
}

extern "C" int ntts_k_head_penalty_probe(const void* X_dev, const void* W_dev, int32_t M, int32_t N, int32_t K, int32_t variant, int32_t fp8, float xscale,
                                         const uint32_t* seen, const float* rep_pen, const int32_t* mask_eos, float* logits_out,
                                         uint16_t* logits_bf16_out, float* part_val, int32_t* part_idx, int32_t part_cap, int32_t* n_part,
                                         int32_t* part_width) {
    return head_probe(X_dev, W_dev, M, N, K, variant, fp8, xscale, seen, rep_pen, mask_eos, logits_out, logits_bf16_out, part_val, part_idx, part_cap,
                      n_part, part_width, nullptr, nullptr);
}

extern "C" int ntts_k_head_logprob_probe(const void* X_dev, const void* W_dev, int32_t M, int32_t N, int32_t K, int32_t variant, int32_t fp8, float xscale,
                                         const uint32_t* seen, const float* rep_pen, const int32_t* mask_eos, float* logits_out,
                                         uint16_t* logits_bf16_out, float* part_val, int32_t* part_idx, float* part_sum, int32_t part_cap,
                                         int32_t* n_part, int32_t* part_width, float* row_lse) {
    if (!part_sum || !row_lse) return NTTS_EINVAL;
    return head_probe(X_dev, W_dev, M, N, K, variant, fp8, xscale, seen, rep_pen, mask_eos, logits_out, logits_bf16_out, part_val, part_idx, part_cap,
                      n_part, part_width, part_sum, row_lse);
}

// ---- the scoring launch (backbone.cpp ntts_backbone_score: lm_head_launch with a target column per row, then score.h's merge) on caller-supplied
//      operands, packed as head_probe packs them.  target_val and the merged outputs start as NaN / -1: a capture or a row that is missed shows.
extern "C" int ntts_k_head_score_probe(const void* X_dev, const void* W_dev, int32_t M, int32_t N, int32_t K, int32_t variant, int32_t fp8, float xscale,
                                       const int32_t* target, float* logits_out, float* part_val, int32_t* part_idx, float* part_sum, int32_t part_cap,
                                       int32_t* n_part, int32_t* part_width, float* target_val, float* logprob, int32_t* argmax, float* argmax_logprob) {
    if (!X_dev || !W_dev || !target || !logits_out || !part_val || !part_idx || !part_sum || !n_part || !part_width || !target_val || !logprob ||
        !argmax || !argmax_logprob) return NTTS_EINVAL;
    if (M < 1 || N < 16 || K < 64 || (K % 64) || (fp8 && (K % 128))) return NTTS_EINVAL;
    if ((variant != 0 && variant != 1 && variant != 2 && variant != 4) || (variant == 4 && fp8)) return NTTS_EINVAL;
    if (fp8 && !(xscale > 0.f)) return NTTS_EINVAL;
    for (int m = 0; m < M; ++m)
        if (target[m] < 0 || target[m] >= N) return NTTS_EINVAL;
    const int width = variant == 4 ? 96 : 64;
    const int np = variant == 0 ? (N + 63) / 64 : variant == 4 ? ((N + 287) / 288) * 3 : variant == 2 ? ((N + 255) / 256) * 4 : ((N + 127) / 128) * 2;
    if (part_cap < np) return NTTS_EINVAL;
    ProbeOperands ops;
    ProbeBuf lg, pv, pi, psum, tg, outs;
    if (!probe_alloc(lg, (size_t)M * N * 4) || !probe_alloc(pv, (size_t)M * np * 4) || !probe_alloc(pi, (size_t)M * np * 4) ||
        !probe_alloc(psum, (size_t)M * np * 4) || !probe_alloc(tg, (size_t)M * 4) || !probe_alloc(outs, (size_t)M * 4 * 4)) return NTTS_ENOMEM;
    const hipStream_t st = (hipStream_t)0;
    const bf16_t* X = nullptr;
    if (const int rc = pack_probe_operands(X_dev, W_dev, M, N, K, fp8, xscale, ops, &X)) return rc;
    // outs: [target_val | logprob | argmax | argmax_logprob], M entries each; NaN bits (argmax: -1) ahead of the launch
    std::vector<uint32_t> init((size_t)M * 4, 0x7fc00000u);
    for (int m = 0; m < M; ++m) init[(size_t)2 * M + m] = 0xffffffffu;
    if (hipMemcpy(tg.p, target, (size_t)M * 4, hipMemcpyHostToDevice) != hipSuccess) return NTTS_EHIP;
    if (hipMemcpy(outs.p, init.data(), init.size() * 4, hipMemcpyHostToDevice) != hipSuccess) return NTTS_EHIP;
    float* o = (float*)outs.p;
    GemmArgs a{};
    a.w_tile_major = 1;
    a.X = X; a.ldx = K; a.W = (const bf16_t*)ops.wt.p; a.ldw = K; a.M = M; a.N = N; a.K = K;
    a.wscale = fp8 ? (const float*)ops.ws.p : nullptr; a.xscale = xscale;
    a.part_val = (float*)pv.p; a.part_idx = (int*)pi.p; a.part_sum = (float*)psum.p;
    a.logits = (float*)lg.p; a.ld_logits = N;
    a.target = (const int*)tg.p; a.target_val = o;
    lm_head_launch(a, variant, fp8 != 0, st);
    ScoreMergeArgs sm{(const float*)pv.p, (const int*)pi.p, (const float*)psum.p, np, o, o + M, (int*)(o + 2 * (size_t)M), o + 3 * (size_t)M};
    NTTS_LAUNCH((score_merge_kernel), dim3((unsigned)M), dim3(256), st, sm);
    if (hipDeviceSynchronize() != hipSuccess || hipGetLastError() != hipSuccess) return NTTS_EHIP;
    if (hipMemcpy(logits_out, lg.p, (size_t)M * N * 4, hipMemcpyDeviceToHost) != hipSuccess) return NTTS_EHIP;
    if (hipMemcpy(part_val, pv.p, (size_t)M * np * 4, hipMemcpyDeviceToHost) != hipSuccess) return NTTS_EHIP;
    if (hipMemcpy(part_idx, pi.p, (size_t)M * np * 4, hipMemcpyDeviceToHost) != hipSuccess) return NTTS_EHIP;
    if (hipMemcpy(part_sum, psum.p, (size_t)M * np * 4, hipMemcpyDeviceToHost) != hipSuccess) return NTTS_EHIP;
    if (hipMemcpy(target_val, o, (size_t)M * 4, hipMemcpyDeviceToHost) != hipSuccess) return NTTS_EHIP;
    if (hipMemcpy(logprob, o + M, (size_t)M * 4, hipMemcpyDeviceToHost) != hipSuccess) return NTTS_EHIP;
    if (hipMemcpy(argmax, o + 2 * (size_t)M, (size_t)M * 4, hipMemcpyDeviceToHost) != hipSuccess) return NTTS_EHIP;
    if (hipMemcpy(argmax_logprob, o + 3 * (size_t)M, (size_t)M * 4, hipMemcpyDeviceToHost) != hipSuccess) return NTTS_EHIP;
    *n_part = np;
    *part_width = width;
    return NTTS_OK;
}

// ---- attention probes: the decode launch of one form and one layer's prompt-pass attention (writer + the three tiers over the engine's own work
//      lists) on caller-supplied pools and block tables, against tests/attention_spec.py.  Argument checks and one call each: the instantiations, grids,
//      work lists, the meta block's packing and the launch sequence are attn_decode.h's / attn_prefill.h's own (attn_decode_launch_form,
//      prefill_work_lists, prefill_pack, prefill_attn_layer), the ones the engine calls.
extern "C" int ntts_k_attn_decode_form(int32_t batch, int32_t nkv, int32_t max_ctx, int32_t nt_pages, int32_t head_dim) {
    if (batch < 1 || nkv < 1 || max_ctx < 1 || (head_dim != 64 && head_dim != 128)) return NTTS_EINVAL;
    return attn_decode_form(batch, nkv, max_ctx, nt_pages, head_dim);
}

namespace {
struct DevBuf { void* p = nullptr; ~DevBuf() { if (p) (void)hipFree(p); } };
// every block-table entry names a page of the pool (the kernels may request any entry of a row, used or not)
bool block_table_ok(const int32_t* bt_dev, long entries, int num_pages) {
    std::vector<int> bt((size_t)entries);
    if (hipMemcpy(bt.data(), bt_dev, (size_t)entries * sizeof(int), hipMemcpyDeviceToHost) != hipSuccess) return false;
    for (long i = 0; i < entries; ++i)
        if (bt[i] < 0 || bt[i] >= num_pages) return false;
    return true;
}
}  // namespace

extern "C" int ntts_k_attn_decode_probe(const void* qkv_dev, int64_t ld_qkv, void* out_dev, float out_fp8_inv, void* kpool_dev, void* vpool_dev,
                                        int32_t num_pages, const int32_t* block_table_dev, int32_t max_pages, const int32_t* pos_dev,
                                        const int32_t* state_dev, int32_t batch, int32_t nh, int32_t nkv, int32_t head_dim, int32_t max_ctx,
                                        int32_t form, int32_t nsplit, int32_t xcd_rows, float* slabs_out_dev) {
    if (!qkv_dev || !out_dev || !kpool_dev || !vpool_dev || !block_table_dev || !pos_dev || !state_dev) return NTTS_EINVAL;
    if (batch < 1 || nh < 1 || nkv < 1 || (nh % nkv) || nh / nkv > kGroupMax || num_pages < 1 || max_pages < 1) return NTTS_EINVAL;
    if (form < 0 || form >= kAttnFormCount) return NTTS_EINVAL;
    const bool hd128 = form == kAttnFormHD128_1024 || form == kAttnFormHD128_2048;
    const bool lmax1024 = form == kAttnFormNT1024 || form == kAttnFormW4_1024 || form == kAttnFormHD128_1024;
    if (head_dim != (hd128 ? 128 : 64)) return NTTS_EINVAL;
    if (max_ctx < 1 || max_ctx > (lmax1024 ? 1024 : kAttnLMax) || (long)max_pages * kPage < max_ctx) return NTTS_EINVAL;
    if (ld_qkv < (long)(nh + 2 * nkv) * head_dim || (ld_qkv % 8) || ((uintptr_t)qkv_dev & 15)) return NTTS_EINVAL;
    if (xcd_rows && (form == kAttnFormSplit || hd128 || (xcd_rows != 1 && xcd_rows != 2 && xcd_rows != 4 && xcd_rows != 8) || batch != 512 / xcd_rows)) return NTTS_EINVAL;
    if (form == kAttnFormSplit ? (nsplit < 2 || nsplit > 64 || out_fp8_inv > 0.f) : (nsplit != 0 || slabs_out_dev)) return NTTS_EINVAL;
    {   // positions inside the context, pages inside the pool
        std::vector<int> pos(batch);
        if (hipMemcpy(pos.data(), pos_dev, (size_t)batch * sizeof(int), hipMemcpyDeviceToHost) != hipSuccess) return NTTS_EHIP;
        for (int b = 0; b < batch; ++b)
            if (pos[b] < 0 || pos[b] >= max_ctx) return NTTS_EINVAL;
        if (!block_table_ok(block_table_dev, (long)batch * max_pages, num_pages)) return NTTS_EINVAL;
    }
    AttnDecodeArgs a{};
    a.qkv = (const bf16_t*)qkv_dev; a.ld_qkv = ld_qkv; a.out = (bf16_t*)out_dev; a.ld_out = (long)nh * head_dim; a.out_fp8_inv = out_fp8_inv;
    a.kpool = (bf16_t*)kpool_dev; a.vpool = (bf16_t*)vpool_dev; a.block_table = block_table_dev; a.max_pages = max_pages;
    a.pos = pos_dev; a.state = state_dev; a.nh = nh; a.nkv = nkv;
    a.xcd_rows = xcd_rows;
    a.nt_pages = form == kAttnFormNT1024 || form == kAttnFormNT2048;
    const hipStream_t st = (hipStream_t)0;
    if (form != kAttnFormSplit) {
        attn_decode_launch_form(a, batch, st, form);
        return hipDeviceSynchronize() == hipSuccess && hipGetLastError() == hipSuccess ? NTTS_OK : NTTS_EHIP;
    }
    // context-split with the combine pass (the tile path's form); the scratch is the probe's own, NaN-filled: a slab or a statistic that a kernel
    // should have written and did not reaches the output
    AttnSplitArgs q{};
    q.a = a; q.a.slab_rows = batch; q.ld_scores = max_ctx + 16; q.nsplit = nsplit;
    const size_t n_sc = (size_t)batch * nkv * kGroupMax * q.ld_scores * sizeof(bf16_t), n_st = (size_t)batch * nkv * nsplit * kGroupMax * 2 * sizeof(float),
                 n_os = (size_t)nsplit * batch * a.ld_out * sizeof(float);
    DevBuf sc, stt, os;
    if (hipMalloc(&sc.p, n_sc) != hipSuccess || hipMalloc(&stt.p, n_st) != hipSuccess || hipMalloc(&os.p, n_os) != hipSuccess) return NTTS_ENOMEM;
    if (hipMemset(sc.p, 0xFF, n_sc) != hipSuccess || hipMemset(stt.p, 0xFF, n_st) != hipSuccess || hipMemset(os.p, 0xFF, n_os) != hipSuccess) return NTTS_EHIP;
    q.scores = (bf16_t*)sc.p; q.stats = (float*)stt.p; q.oslabs = (float*)os.p;
    attn_split_launch(q, batch, st, true);
    if (hipDeviceSynchronize() != hipSuccess || hipGetLastError() != hipSuccess) return NTTS_EHIP;
    if (slabs_out_dev && hipMemcpy(slabs_out_dev, os.p, n_os, hipMemcpyDeviceToDevice) != hipSuccess) return NTTS_EHIP;
    return NTTS_OK;
}

extern "C" int ntts_k_attn_prefill_probe(void* qkv_dev, int64_t ld_qkv, void* out_dev, float out_fp8_inv, void* kpool_dev, void* vpool_dev,
                                         int32_t num_pages, const int32_t* block_table_dev, int32_t bt_rows, int32_t max_pages, int32_t n,
                                         const int32_t* lens, const int32_t* pos0, const int32_t* slots, int32_t nh, int32_t nkv, int32_t head_dim,
                                         const void* rope_cos_dev, const void* rope_sin_dev, int32_t max_ctx, const void* q_norm_dev,
                                         const void* k_norm_dev, float eps, int32_t res_cap, int32_t deep_cap, int32_t only_last) {
    if (!qkv_dev || !out_dev || !kpool_dev || !vpool_dev || !block_table_dev || !lens || !pos0 || !slots || !rope_cos_dev || !rope_sin_dev) return NTTS_EINVAL;
    if (n < 1 || nh < 1 || nkv < 1 || (nh % nkv) || nh / nkv > kGroupMax || num_pages < 1 || bt_rows < 1 || max_pages < 1) return NTTS_EINVAL;
    if ((head_dim != 64 && head_dim != 128) || max_ctx < 1 || (long)max_pages * kPage < max_ctx) return NTTS_EINVAL;
    if (ld_qkv < (long)(nh + 2 * nkv) * head_dim || (ld_qkv % 8) || ((uintptr_t)qkv_dev & 15)) return NTTS_EINVAL;
    if (((uintptr_t)rope_cos_dev & 15) || ((uintptr_t)rope_sin_dev & 15)) return NTTS_EINVAL;
    long T = 0;
    for (int i = 0; i < n; ++i) {
        if (pos0[i] < 0 || (pos0[i] % kPage) || lens[i] <= pos0[i] || lens[i] > max_ctx || slots[i] < 0 || slots[i] >= bt_rows) return NTTS_EINVAL;
        T += lens[i] - pos0[i];
    }
    if (T > 0x7fffffffL / (long)ld_qkv) return NTTS_EINVAL;
    if (!block_table_ok(block_table_dev, (long)bt_rows * max_pages, num_pages)) return NTTS_EINVAL;
    const bool generic = head_dim == 128 || q_norm_dev || k_norm_dev;   // (ntts_backbone_create: head_dim 128 and / or qk-norm)
    int cap = 0, dcap = 0;
    prefill_clamp_caps(res_cap, deep_cap, &cap, &dcap);
    if (generic) cap = dcap = 0;                                        // every query on the (head_dim-templated) two-sweep kernel
    std::vector<int> m;                                                 // the probe's own block: the packer's part alone (no ids in front)
    const PrefillPacked packed = prefill_pack(prefill_work_lists(n, lens, pos0, cap, dcap), n, lens, pos0, slots, m);
    DevBuf mb;
    if (hipMalloc(&mb.p, m.size() * sizeof(int)) != hipSuccess) return NTTS_ENOMEM;
    if (hipMemcpy(mb.p, m.data(), m.size() * sizeof(int), hipMemcpyHostToDevice) != hipSuccess) return NTTS_EHIP;
    prefill_attn_layer((bf16_t*)qkv_dev, ld_qkv, (bf16_t*)out_dev, (long)nh * head_dim, out_fp8_inv, (bf16_t*)kpool_dev, (bf16_t*)vpool_dev,
                       block_table_dev, max_pages, packed.bind((const int*)mb.p), nh, nkv, head_dim, (const bf16_t*)rope_cos_dev,
                       (const bf16_t*)rope_sin_dev, (const bf16_t*)q_norm_dev, (const bf16_t*)k_norm_dev, eps, generic, (int)T, cap, dcap,
                       only_last != 0, (hipStream_t)0);
    return hipDeviceSynchronize() == hipSuccess && hipGetLastError() == hipSuccess ? NTTS_OK : NTTS_EHIP;
}
