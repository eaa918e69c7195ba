// sample.h -- token choice + per-slot generation bookkeeping, on device (so a decode step is replayable
// as a hipGraph: nothing about a step depends on host-side state).
//
// Replaces the tail of GenerationMixin._sample (hf:generation/utils.py:2894-2941):
//   fp32 logits -> MinNewTokensLength (applied in the lm_head epilogue via mask_eos) ->
//     do_sample=0: argmax (first max wins, torch.argmax)
//     do_sample=1: [TemperatureLogitsWarper: scores / T] -> TopKLogitsWarper (scores < k-th largest -> -inf, ties at the
//                  k-th value kept; hf:generation/logits_process.py:542-595) -> [TopPLogitsWarper, top_p < 1] ->
//                  [MinPLogitsWarper, min_p > 0] -> softmax -> multinomial(1)
//                  (the reference's own call: do_sample=True, temperature=1.0, top_k=50, ref:neutts/neutts.py:338-347; top_p /
//                  min_p are generate()'s own keyword arguments, off -- 1.0 / 0.0 -- in that call)
//                  top_k = -1 (transformers' top_k=0 / None, serving stacks' -1): no TopKLogitsWarper -- temperature, top_p and min_p act on the
//                  whole vocabulary and the draw is over the model's own distribution (sample_full_row below: integer masses of 2^-32 of the
//                  likeliest token's, so a token less likely than that is never drawn)
//   -> append -> EosTokenCriteria / MaxLengthCriteria.
// RepetitionPenaltyLogitsProcessor (repetition_penalty != 1; first in hf:generation/utils.py _get_logits_processor, ahead of MinNewTokensLength and the
// warpers) also lives in the lm_head epilogue (gemm.h EPI_ARGMAX_PEN): it reads a per-slot bitmap of the lm_head columns the request has seen.  This file
// keeps that bitmap: the prompt pass clears a slot's row and marks its prompt's ids, the sampling kernel marks every token it appends (so step t + 1's
// lm_head sees the token of step t), ntts_backbone_activate moves the row with the rest of the slot.
// Sampling reads the row of bf16 logits the lm_head epilogue leaves behind (HF's logits ARE bf16 values cast to fp32, so a
// 16-bit radix select finds the exact k-th largest), draws its uniform from Philox4x32-10 keyed by the request's seed with
// the step index as counter: reproducible for a given seed whatever slot / batch the request runs in (callers give each
// request its own seed); torch's own generator stream is not reproduced.
#pragma once
#include <ntts/dev.h>

namespace ntts {

enum SlotState { SLOT_FREE = 0, SLOT_RUNNING = 1, SLOT_FINISHED = 2, SLOT_PREFILLED = 3 };

struct SlotArrays {      // device arrays, one entry per decode slot
    int* state;
    int* pos;            // tokens in the KV cache == position of cur_tok
    int* n_new;          // generated so far
    int* cur_tok;        // token fed to the next step
    int* prompt_len;
    int* min_new;
    int* max_len;
    int* eos;
    int* mask_eos;       // eos+1 while EOS is masked for the NEXT sampled token (n_new < min_new), else 0
    int* top_k;          // 0 = greedy (do_sample=0); k >= 1 = sample among the k largest logits; -1 = sample over the whole vocabulary
    float* temperature;  // > 0
    float* top_p;        // (0, 1]; 1 = no nucleus cut
    float* min_p;        // [0, 1]; 0 = no min-p cut
    float* rep_pen;      // repetition penalty, finite and > 0; exactly 1 = off (every row holds 1 until a penalised request fills it)
    unsigned int* seed;  // [slots][2] Philox key
    int* out_tokens;     // [slots][out_stride]
    int out_stride;
};

struct SampleArgs {
    const float* part_val;   // [rows][n_part] per-row partial maxima from the lm_head epilogue
    const int* part_idx;
    int n_part;
    int part_width;          // columns per partial (consecutive: partial i covers columns [i * part_width, (i + 1) * part_width)); 0 = unknown
    const bf16_t* logits;    // [rows][ld_logits] processed bf16 logits (EOS mask applied); null if no slot samples
    long ld_logits;
    int vocab;
    SlotArrays sl;
    int phase;               // SLOT_RUNNING: decode step; SLOT_PREFILLED: first token after prefill
    // compacted head (ntts_backbone_set_logits_range): column c of the lm_head is token id_base + c for c < n_range and the EOS id for
    // c == n_range; n_range = 0: column = token id
    int n_range, id_base, id_tail;
    unsigned int* seen;      // [slots][seen_pitch] seen-column bitmap (gemm.h GemmArgs::seen); null while no penalised request is live
    long seen_pitch;
    // per-token log-probabilities (ntts_backbone_set_logprobs): with both pointers non-null a live row also records log softmax(row)[token] over the
    // WHOLE processed row (all `vocab` columns, -inf ones contributing 0) -- temperature and the warpers do not enter
    const float* part_sum;   // [rows][n_part] sum of exp(v - part_val) per partial (gemm.h EPI_ARGMAX_LSE); null = off
    float* out_logprobs;     // [slots][sl.out_stride], entry for entry beside sl.out_tokens
};

// one bit of a seen bitmap, from any number of workgroups at once (duplicates are the norm).  Spelled with the compiler's builtin so that the same
// line is a global_atomic_or on the device and a host atomic on the CPU emulator
NTTS_D void seen_mark(unsigned int* row, int col) { __atomic_fetch_or(row + (col >> 5), 1u << (col & 31), __ATOMIC_RELAXED); }

constexpr int kSampleCap = 512;   // candidates kept (k plus ties at the k-th value, capped)

// Philox4x32-10 (Salmon et al. 2011), one block: 128-bit counter, 64-bit key -> 4 x 32 random bits
NTTS_D void philox4x32(unsigned int (&c)[4], unsigned int k0, unsigned int k1) {
#pragma unroll
    for (int r = 0; r < 10; ++r) {
        const unsigned long long p0 = 0xD2511F53ull * c[0], p1 = 0xCD9E8D57ull * c[2];
        const unsigned int n0 = (unsigned int)(p1 >> 32) ^ c[1] ^ k0, n1 = (unsigned int)p1;
        const unsigned int n2 = (unsigned int)(p0 >> 32) ^ c[3] ^ k1, n3 = (unsigned int)p0;
        c[0] = n0; c[1] = n1; c[2] = n2; c[3] = n3;
        k0 += 0x9E3779B9u; k1 += 0xBB67AE85u;
    }
}
// order-preserving 16-bit key of a bf16 value (larger value <-> larger key; -inf smallest of the non-NaN keys)
NTTS_D unsigned int bf16_key(bf16_t v) { return (v & 0x8000u) ? (~(unsigned int)v & 0xFFFFu) : ((unsigned int)v | 0x8000u); }

// top-k + multinomial for one row; all 256 threads of the block take part.  Returns the token in every thread.
// The lm_head epilogue leaves one maximum per group of `gw` consecutive columns (pv[0 .. n_part-1]; SampleArgs::part_val).  The k-th
// largest of those maxima, T, is a lower bound of the k-th largest logit (k groups hold an element >= T), and a group whose maximum is
// below T holds no element >= T: only the groups with maximum >= T -- k of them plus ties, ~50 x 96 columns of the 217 488 -- are
// scanned for the exact threshold and the survivors.  Same result as three sweeps over the whole row (the fallback when a row has more
// than kGroupCap such groups, e.g. constant logits, or when there are fewer groups than k), 1/45 of the bytes and LDS atomics.
//
// top_p < 1 / min_p > 0 (TopPLogitsWarper, MinPLogitsWarper behind TopK: hf:generation/logits_process.py) filter the candidate list
// between the softmax numerators and the draw, in LDS and registers only:
//   top_p: candidates ranked by value descending, ties by token id ascending; c_0 = 0, c_{j+1} = c_j + e_(j) summed in that order by one
//          thread (like `total`: the cut depends on the order of those additions), every c_j kept; rank j survives iff j == 0 or c_j < top_p * c_n
//          ("keep while the mass strictly before the token is < top_p", min_tokens_to_keep = 1);
//   min_p: survives iff e_a >= min_p (prob >= min_p * max prob: the normaliser cancels and the maximum has e = 1).
// The survivors stay in token-id order with their e_a; the draw is the same code either way.  With top_p >= 1 and min_p <= 0 the stage is
// one block-uniform branch not taken.  surv_out / n_out (ntts_k_sample_probe; null in the decode step): the final survivors.
constexpr int kGroupCap = 1024;
NTTS_D int sample_topk_row(const bf16_t* row, int V, int k, float temperature, float top_p, float min_p, unsigned int s0, unsigned int s1,
                           unsigned int step, const float* pv, int n_part, int gw, int* surv_out = nullptr, int* n_out = nullptr) {
    NTTS_SHARED unsigned int hist[256];
    NTTS_SHARED unsigned int sel[6];          // [0] high byte, [1] elements above that bin, [2] threshold key, [3] list length, [4] group threshold key, [5] groups kept
    NTTS_SHARED int cidx[kSampleCap];
    NTTS_SHARED unsigned short cval[kSampleCap];
    NTTS_SHARED int sidx[kSampleCap];
    NTTS_SHARED unsigned short sval[kSampleCap];
    NTTS_SHARED int glist[kGroupCap];
    NTTS_SHARED unsigned int wsum[4];
    NTTS_SHARED float ev[kSampleCap];
    NTTS_SHARED float wmax[4];
    NTTS_SHARED unsigned int fcnt[8];         // nucleus / min-p stage: survivors per wave, candidates [0, 256) and [256, 512)
    NTTS_SHARED int result;
    const int tid = threadIdx.x;
    if (k > V) k = V;
    if (k > kSampleCap) k = kSampleCap;
    // Walking the 256 bins from the top, the bin at which the running count (starting from `base`) first reaches k, and the count above
    // it -> sel[0], sel[1].  All threads call it; thread t owns bin t: suffix sums by wave shuffles instead of one thread's 256 dependent
    // LDS reads (the two serial walks of a select were ~8 us of a 62 us kernel).  Bin 0 takes the row if no higher bin reaches k.
    auto find_bin = [&](unsigned int base) {
        const int lane = lane_id(), w = wave_id();
        const unsigned int h = hist[tid];
        int incl = (int)h;                                 // bins tid .. end of this wave's 64
#pragma unroll
        for (int d = 1; d < 64; d <<= 1) {
            const int o = shfl(incl, (lane + d) & 63);
            if (lane + d < 64) incl += o;
        }
        if (lane == 0) wsum[w] = (unsigned int)incl;
        sync();
        unsigned int excl = base + (unsigned int)incl - h;  // count strictly above bin tid
        for (int ww = w + 1; ww < 4; ++ww) excl += wsum[ww];
        if (tid == 0 ? excl < (unsigned int)k : (excl < (unsigned int)k && excl + h >= (unsigned int)k)) { sel[0] = (unsigned int)tid; sel[1] = excl; }
        sync();
    };
    // the k-th largest of `count` keys (two histogram passes over 16-bit keys): key_at(i) = key of element i or 0x10000 to skip it;
    // lo_bound: only keys >= lo_bound are counted.  Leaves the key in sel[out]
    auto kth_key = [&](auto&& for_each_key, int out) {
        hist[tid] = 0;
        sync();
        for_each_key([&](unsigned int key) { atomic_add_lds(&hist[key >> 8], 1u); });
        sync();
        find_bin(0u);
        const unsigned int hb = sel[0], above = sel[1];
        hist[tid] = 0;
        sync();
        for_each_key([&](unsigned int key) { if ((key >> 8) == hb) atomic_add_lds(&hist[key & 255u], 1u); });
        sync();
        find_bin(above);
        if (tid == 0) sel[out] = (hb << 8) | sel[0];
        sync();
    };
    if (tid < 6) sel[tid] = 0;
    sync();
    // ---- which column groups can hold one of the k largest logits
    bool grouped = pv != nullptr && gw >= 8 && (gw & 7) == 0 && n_part >= k;
    if (grouped) {
        kth_key([&](auto&& f) { for (int i = tid; i < n_part; i += 256) f(bf16_key(f2bf(pv[i]))); }, 4);
        const unsigned int gthr = sel[4];
        for (int i = tid; i < n_part; i += 256)
            if (bf16_key(f2bf(pv[i])) >= gthr) {
                const unsigned int at = atomic_add_lds(&sel[5], 1u);
                if (at < (unsigned int)kGroupCap) glist[at] = i;
            }
        sync();
        if (sel[5] > (unsigned int)kGroupCap) grouped = false;      // (block-uniform)
    }
    const int ng = grouped ? (int)sel[5] : 0;
    const unsigned int floor_key = grouped ? sel[4] : 0u;            // elements below the group threshold cannot be among the k largest
    const int vpg = gw >> 3;                                         // 16-byte vectors per group
    const int nvec = V >> 3;                                         // full row: 16-byte vectors; the scalar tail is handled by the first threads
    // every element (index, value) that can matter: the listed groups, or the whole row
    auto for_each_elem = [&](auto&& f) {
        if (grouped) {
            for (int i = tid; i < ng * vpg; i += 256) {
                const int c0 = glist[i / vpg] * gw + (i % vpg) * 8;
                if (c0 + 8 <= V) {
                    const bf16x8 v = ld16<bf16x8>(row + c0);
#pragma unroll
                    for (int e = 0; e < 8; ++e) f(c0 + e, (bf16_t)v[e]);
                } else {
                    for (int e = 0; e < 8 && c0 + e < V; ++e) f(c0 + e, row[c0 + e]);
                }
            }
        } else {
            for (int i = tid; i < nvec; i += 256) {
                const bf16x8 v = ld16<bf16x8>(row + (long)i * 8);
#pragma unroll
                for (int e = 0; e < 8; ++e) f(i * 8 + e, (bf16_t)v[e]);
            }
            for (int i = nvec * 8 + tid; i < V; i += 256) f(i, row[i]);
        }
    };
    // ---- the exact k-th largest logit (16-bit radix select: HF's logits ARE bf16 values)
    kth_key([&](auto&& f) { for_each_elem([&](int, bf16_t v) { const unsigned int key = bf16_key(v); if (key >= floor_key) f(key); }); }, 2);
    const unsigned int thr = sel[2];
    // ---- gather every logit >= the k-th largest (ties kept, like scores < kth -> -inf)
    for_each_elem([&](int idx, bf16_t v) {
        if (bf16_key(v) >= thr) {
            const unsigned int at = atomic_add_lds(&sel[3], 1u);
            if (at < (unsigned int)kSampleCap) { cidx[at] = idx; cval[at] = v; }
        }
    });
    sync();
    int n = (int)sel[3];
    if (n > kSampleCap) {                                            // (block-uniform; constant rows, a threshold of -inf, k near the cap with ties)
        // More candidates than the list holds: which of them the appends above kept depends on the order the atomics arrived in.  Keep
        // the kSampleCap LOWEST token ids instead (oracle/sampling_ref.py: token-id order, capped): the id of the last one is found by a
        // radix select over the bytes of ~id (larger = lower id) with the histogram walk used above, then the list is gathered again
        k = kSampleCap;                                              // (find_bin's target)
        int top = 3;
        while (top > 0 && ((unsigned int)(V - 1) >> (8 * top)) == 0u) --top;     // bytes of ~id above this one are 0xff for every id < V
        unsigned int pre = ~0u, base = 0u;
        for (int b = top; b >= 0; --b) {
            const unsigned int hm = b == 3 ? 0u : (~0u << (8 * (b + 1)));        // the bytes already decided
            hist[tid] = 0;
            sync();
            for_each_elem([&](int idx, bf16_t v) {
                const unsigned int u = ~(unsigned int)idx;
                if (bf16_key(v) >= thr && (u & hm) == (pre & hm)) atomic_add_lds(&hist[(u >> (8 * b)) & 255u], 1u);
            });
            sync();
            find_bin(base);
            pre = (pre & hm) | (sel[0] << (8 * b)) | (b ? (~0u >> (32 - 8 * b)) : 0u);
            base = sel[1];
        }
        const int id_last = (int)~pre;                               // the largest id that is kept
        if (tid == 0) sel[3] = 0;                                    // (every thread read the count long ago: barriers in between)
        sync();
        for_each_elem([&](int idx, bf16_t v) {
            if (bf16_key(v) >= thr && idx <= id_last) {
                const unsigned int at = atomic_add_lds(&sel[3], 1u);
                if (at < (unsigned int)kSampleCap) { cidx[at] = idx; cval[at] = v; }
            }
        });
        sync();
        n = (int)sel[3];
        if (n > kSampleCap) n = kSampleCap;
    }
    // ---- order the candidates by token id (the append order above is not deterministic): rank sort
    for (int a = tid; a < n; a += 256) {
        const int ia = cidx[a];
        int rank = 0;
        for (int b = 0; b < n; ++b) rank += cidx[b] < ia;
        sidx[rank] = ia;
        sval[rank] = cval[a];
    }
    sync();
    // ---- softmax over the survivors + inverse-CDF draw: maximum and exponentials in parallel, the two running sums by one thread in
    //      token order (the draw depends on the order of those additions: kept)
    float mx = -INFINITY;
    for (int a = tid; a < n; a += 256) mx = fmaxf(mx, bf2f(sval[a]));
#pragma unroll
    for (int sh = 1; sh < 64; sh <<= 1) mx = fmaxf(mx, shfl_xor(mx, sh));
    if (lane_id() == 0) wmax[wave_id()] = mx;
    sync();
    const float m = fmaxf(fmaxf(wmax[0], wmax[1]), fmaxf(wmax[2], wmax[3]));
    const float it = 1.0f / temperature;
    for (int a = tid; a < n; a += 256) ev[a] = fexp((bf2f(sval[a]) - m) * it);
    sync();
    const bool nucleus = top_p < 1.0f;
    if (nucleus || min_p > 0.0f) {                                   // (block-uniform)
        // ---- TopP / MinP: every thread owns candidates tid and tid + 256 (n <= 512)
        int rk[2] = {0, 0};
        bool pass[2] = {true, true};                                 // the nucleus test of this thread's candidates
        if (nucleus) {
            float* re = reinterpret_cast<float*>(glist);             // e in rank order (the group list is dead by now: 1024 ints)
#pragma unroll
            for (int q = 0; q < 2; ++q) {
                const int a = tid + q * 256;
                if (a < n) {
                    const float va = bf2f(sval[a]);
                    int r = 0;
                    for (int b = 0; b < n; ++b) { const float vb = bf2f(sval[b]); r += (vb > va) || (vb == va && b < a); }
                    rk[q] = r;
                    re[r] = ev[a];
                }
            }
            sync();
            if (tid == 0) {                                          // one walk, no data-dependent exit: re[j] <- c_j, the mass before rank j
                float c = 0.f;
                for (int j = 0; j < n; ++j) { const float e = re[j]; re[j] = c; c += e; }
                wmax[0] = top_p * c;
            }
            sync();
            const float lim = wmax[0];                               // (c_j never decreases: the ranks that pass are a prefix)
#pragma unroll
            for (int q = 0; q < 2; ++q) pass[q] = rk[q] == 0 || re[rk[q]] < lim;
        }
        bool kp[2];
        int id[2];
        float ee[2];
#pragma unroll
        for (int q = 0; q < 2; ++q) {
            const int a = tid + q * 256;
            id[q] = a < n ? sidx[a] : 0;
            ee[q] = a < n ? ev[a] : 0.f;
            kp[q] = a < n && pass[q] && ee[q] >= min_p;
        }
        // order-preserving compaction (export_codes_kernel's scheme), in place: everything is in registers before the barrier
        const unsigned long long m0 = ballot(kp[0]), m1 = ballot(kp[1]);
        const int lane = lane_id(), w = wave_id();
        if (lane == 0) { fcnt[w] = (unsigned int)popc64(m0); fcnt[4 + w] = (unsigned int)popc64(m1); }
        sync();
        const int n0 = (int)(fcnt[0] + fcnt[1] + fcnt[2] + fcnt[3]), n1 = (int)(fcnt[4] + fcnt[5] + fcnt[6] + fcnt[7]);
        if (n0 + n1 > 0) {                                           // (a row of NaNs keeps its list; block-uniform)
            int off0 = 0, off1 = n0;
            for (int ww = 0; ww < w; ++ww) { off0 += (int)fcnt[ww]; off1 += (int)fcnt[4 + ww]; }
            const unsigned long long below = (1ull << lane) - 1ull;
            if (kp[0]) { const int at = off0 + popc64(m0 & below); sidx[at] = id[0]; ev[at] = ee[0]; }
            if (kp[1]) { const int at = off1 + popc64(m1 & below); sidx[at] = id[1]; ev[at] = ee[1]; }
            n = n0 + n1;
        }
        sync();
    }
    if (surv_out) {                                                  // (probe only; folded away in the decode step)
        for (int a = tid; a < n; a += 256) surv_out[a] = sidx[a];
        if (tid == 0) *n_out = n;
    }
    if (tid == 0) {
        float total = 0.f;
        for (int a = 0; a < n; ++a) total += ev[a];
        unsigned int c[4] = {step, 0u, 0u, 0u};
        philox4x32(c, s0, s1);
        const float u = (float)(c[0] >> 8) * (1.0f / 16777216.0f);   // [0, 1)
        const float target = u * total;
        float acc = 0.f;
        int pick = sidx[n - 1];
        for (int a = 0; a < n; ++a) {
            acc += ev[a];
            if (acc > target) { pick = sidx[a]; break; }
        }
        result = pick;
    }
    sync();
    return result;
}

// ---- whole-vocabulary sampling (top_k = NTTS_TOP_K_OFF = -1): temperature -> top_p -> min_p -> draw over ALL V columns, no top-k cut and no
// candidate list.  The contract is tests/sampling_full_spec.py; what makes it a function of the row and the parameters alone is that the masses
// are INTEGERS: e_a = fp32 exp((x_a - max) * (1 / T)) as in sample_topk_row, q_a = floor(e_a * 2^32) (exact, <= 2^32, a maximum has 2^32), and
// every sum is an exact 64-bit sum of q -- no order of additions to keep, so 256 threads sum in whatever order they like, with no float atomics
// and no single-thread walk over the row.  A token whose probability is below 2^-32 of the likeliest token's has q = 0 and is never drawn.
//   top_p < 1: ranked by value descending, ties by token id ascending, rank j survives iff j == 0 or (mass strictly before it) < lim =
//              floor(top_p * Q) (top_p taken as its exact fp32 value M * 2^-s: lim = (M * Q) >> s).  Tokens of equal logit have equal q, so the
//              nucleus is "every key above a threshold key K, plus the r lowest ids at K": K by a 16-ary search over the 16-bit bf16_key (four
//              passes over the row; each LANE has 16 bins of its own in LDS, shared by the four waves with 64-bit LDS atomics -- logits crowd
//              into three or four exponent bins, bins shared inside a wave would serialise), r = ceil((lim - mass above K) / q_K), and, only when r cuts inside the tie group, the id of the r-th tie;
//   min_p > 0: survives iff e_a >= min_p; both stages are evaluated on the whole row and ANDed (tests/sampling_spec.survivors);
//   draw:      survivors in token-id order, S their mass, target = (u24 * S) >> 24 with the sampler's uniform u24 = philox(seed, step)[0] >> 8;
//              the token is the first survivor whose running mass exceeds target.
// "The first column, in id order, whose running weight exceeds a target" (the draw, and the r-th tie) is one routine: one pass adds every 8-column
// unit's weight to its slot of 2048 * g columns in LDS, a block scan over the <= kFullSlots slots finds the slot, its tiles are read again and a
// scan over the 256 threads finds the unit.  State in LDS and registers only.  pv / n_part: the lm_head's per-group maxima (the row's maximum is
// theirs), or null: one more pass.  keep_out / n_out / total_out (ntts_k_sample_full_probe; null in the decode step): the survivor bitmap (byte
// c >> 3, bit c & 7), their number, S.
// Kept OUT of line: inlined, its code inside sample_greedy_kernel cost the default top-k path 1.0 us of its 26.8 us per decode step (256 rows, Air
// geometry); as a call that path runs at the speed it had without it (profiles/full_vocab_sampling_bench.txt).
constexpr int kFullSlots = 1024;
NTTS_D unsigned long long shfl_u64(unsigned long long v, int src) {
    const unsigned int lo = (unsigned int)shfl((int)(unsigned int)v, src), hi = (unsigned int)shfl((int)(unsigned int)(v >> 32), src);
    return ((unsigned long long)hi << 32) | lo;
}
NTTS_D unsigned long long mul_shr24(unsigned long long a, unsigned long long x) {      // floor(a * x / 2^24) for a < 2^24, without the 88-bit product
    return a * (x >> 24) + ((a * (x & 0xFFFFFFull)) >> 24);
}
// exclusive prefix of v over the block's 256 threads, in thread order, and the block's total; sc: 4 words of LDS (free again after the call's
// first barrier).  All threads call it
NTTS_D unsigned long long block_exscan_u64(unsigned long long v, unsigned long long* sc, unsigned long long& total) {
    const int lane = lane_id(), w = wave_id();
    unsigned long long inc = v;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const unsigned long long o = shfl_u64(inc, (lane - d) & 63);
        if (lane >= d) inc += o;
    }
    sync();
    if (lane == 63) sc[w] = inc;
    sync();
    unsigned long long ex = inc - v;
    total = 0;
    for (int ww = 0; ww < 4; ++ww) { if (ww < w) ex += sc[ww]; total += sc[ww]; }
    return ex;
}
__attribute__((noinline)) NTTS_D int sample_full_row(const bf16_t* row, int V, float temperature, float top_p, float min_p, unsigned int s0, unsigned int s1, unsigned int step,
                           const float* pv, int n_part, unsigned char* keep_out = nullptr, int* n_out = nullptr, unsigned long long* total_out = nullptr) {
    typedef unsigned long long u64;
    NTTS_SHARED u64 work[kFullSlots];         // search: bin d of lane l at [d * 64 + l]; locate: one sum per slot
    NTTS_SHARED u64 red[16][16];
    NTTS_SHARED u64 msum[16];
    u64* const tsum = work;
    NTTS_SHARED u64 sc[4];
    NTTS_SHARED u64 hit[2];                   // [0] the slot / the column found, [1] the weight before the slot
    NTTS_SHARED unsigned int wk[4];
    NTTS_SHARED unsigned int nkeep;
    const int tid = threadIdx.x;
    const int nvec = V >> 3, nunit = (V + 7) >> 3;                   // 8-column units: 16-byte loads, the last one scalar if V % 8
    const int ntile = (nunit + 255) >> 8;                            // 256 units = 2048 columns
    const int g = (ntile + kFullSlots - 1) / kFullSlots;             // tiles per slot (1 up to 2 M columns)
    const int nslot = (ntile + g - 1) / g;
    // unit u of this thread: its first column, its values, how many are columns of the row
    auto load_unit = [&](int u, bf16x8& v) -> int {
        if (u < nvec) { v = ld16<bf16x8>(row + (long)u * 8); return 8; }
        const int cnt = V - u * 8;
#pragma unroll
        for (int e = 0; e < 8; ++e) v[e] = e < cnt ? (short)row[(long)u * 8 + e] : (short)0;
        return cnt;
    };
    auto for_each_elem = [&](auto&& f) {                             // f(unit, column, value)
        for (int u = tid; u < nunit; u += 256) {
            bf16x8 v;
            const int cnt = load_unit(u, v);
#pragma unroll
            for (int e = 0; e < 8; ++e) if (e < cnt) f(u, u * 8 + e, (bf16_t)v[e]);
        }
    };
    constexpr unsigned int kInfKey = 0xFF80u;                        // bf16_key(+inf): the keys above it are NaNs
    // ---- the row's maximum
    unsigned int mk = 0;
    if (pv) {
        for (int i = tid; i < n_part; i += 256) { const unsigned int key = bf16_key(f2bf(pv[i])); if (key <= kInfKey && key > mk) mk = key; }
    } else {
        for_each_elem([&](int, int, bf16_t v) { const unsigned int key = bf16_key(v); if (key <= kInfKey && key > mk) mk = key; });
    }
#pragma unroll
    for (int sh = 1; sh < 64; sh <<= 1) { const unsigned int o = (unsigned int)shfl_xor((int)mk, sh); mk = o > mk ? o : mk; }
    if (lane_id() == 0) wk[wave_id()] = mk;
    if (tid == 0) { hit[0] = 0; hit[1] = 0; nkeep = 0; }
    sync();
    mk = wk[0];
    for (int w = 1; w < 4; ++w) mk = wk[w] > mk ? wk[w] : mk;
    auto unkey = [](unsigned int key) { return (bf16_t)((key & 0x8000u) ? (key & 0x7FFFu) : (~key & 0xFFFFu)); };
    const float m = bf2f(unkey(mk));
    const float it = 1.0f / temperature;
    auto e_of = [&](bf16_t v) { return fexp((bf2f(v) - m) * it); };
    auto q_of_e = [](float e) -> u64 { return e >= 1.0f ? (1ull << 32) : (e > 0.f ? (u64)(unsigned int)(e * 4294967296.0f) : 0ull); };   // (a NaN: 0)
    // ---- the first column, in id order, at which the running sum of wf(column, value) exceeds the target: (u24 * total) >> 24 if `draw`, else `fixed`
    //      (< total).  *total_p = the total
    auto locate = [&](auto&& wf, bool draw, u64 fixed, u64* total_p) -> int {
        for (int i = tid; i < nslot; i += 256) tsum[i] = 0;
        sync();
        for (int u = tid; u < nunit; u += 256) {
            bf16x8 v;
            const int cnt = load_unit(u, v);
            u64 part = 0;
#pragma unroll
            for (int e = 0; e < 8; ++e) if (e < cnt) part += wf(u * 8 + e, (bf16_t)v[e]);
            if (part) __atomic_fetch_add(&tsum[(u >> 8) / g], part, __ATOMIC_RELAXED);
        }
        sync();
        const int spt = (nslot + 255) >> 8;                          // slots per thread, consecutive (<= 4)
        u64 mine = 0;
        for (int j = 0; j < spt; ++j) { const int i = tid * spt + j; if (i < nslot) mine += tsum[i]; }
        u64 total;
        u64 ex = block_exscan_u64(mine, sc, total);
        const u64 target = draw ? mul_shr24((u64)fixed, total) : fixed;
        if (mine && ex <= target && target - ex < mine) {            // (one thread, as target < total)
            for (int j = 0; j < spt; ++j) {
                const int i = tid * spt + j;
                const u64 t = i < nslot ? tsum[i] : 0;
                if (target - ex < t) { hit[0] = (u64)i; hit[1] = ex; break; }
                ex += t;
            }
        }
        sync();
        const int slot = (int)hit[0];
        u64 rem = target - hit[1];
        sync();
        const int t_end = (slot + 1) * g < ntile ? (slot + 1) * g : ntile;
        for (int tile = slot * g; tile < t_end; ++tile) {            // (block-uniform)
            const int u = tile * 256 + tid;
            bf16x8 v;
            const int cnt = u < nunit ? load_unit(u, v) : 0;
            u64 part = 0;
#pragma unroll
            for (int e = 0; e < 8; ++e) if (e < cnt) part += wf(u * 8 + e, (bf16_t)v[e]);
            u64 ttot;
            u64 exu = block_exscan_u64(part, sc, ttot);
            if (rem < ttot) {
                if (part && exu <= rem && rem - exu < part) {
                    int col = -1;
#pragma unroll
                    for (int e = 0; e < 8; ++e) {
                        const u64 t = e < cnt ? wf(u * 8 + e, (bf16_t)v[e]) : 0;
                        if (col < 0 && rem - exu < t) col = u * 8 + e;
                        if (col < 0) exu += t;
                    }
                    hit[0] = (u64)(col < 0 ? u * 8 : col);
                }
                break;
            }
            rem -= ttot;
        }
        sync();
        int col = (int)hit[0];
        if (total_p) *total_p = total;
        sync();
        return col < V ? col : V - 1;
    };
    // ---- top_p: the threshold key, and the last id kept at it
    const bool nucleus = top_p < 1.0f;
    unsigned int thr = 0;
    int id_last = 0x7fffffff;
    if (nucleus) {                                                   // (block-uniform, like every branch below)
        const unsigned int pb = __builtin_bit_cast(unsigned int, top_p);
        const int pe = (int)(pb >> 23);                              // (top_p in (0, 1): no sign, exponent <= 126)
        const u64 pm = pe ? ((pb & 0x7FFFFFu) | 0x800000u) : (pb & 0x7FFFFFu);
        const int ps = (pe ? 150 - pe : 149) - 24;                   // top_p = pm * 2^-(ps + 24), ps >= 0
        u64 above = 0, lim = 0, mass_k = 0;
        unsigned int prefix = 0;
        bool search = true;
        for (int L = 0; L < 4 && search; ++L) {
            const int sh = 12 - 4 * L;
#pragma unroll
            for (int d = 0; d < 4; ++d) work[d * 256 + tid] = 0;
            sync();
            for_each_elem([&](int, int, bf16_t v) {
                const unsigned int key = bf16_key(v);
                if ((key >> (sh + 4)) == prefix) {
                    const u64 q = q_of_e(e_of(v));
                    if (q) __atomic_fetch_add(&work[((key >> sh) & 15u) * 64 + (tid & 63)], q, __ATOMIC_RELAXED);
                }
            });
            sync();
            {
                const int d = tid & 15, grp = tid >> 4;
                u64 s = 0;
#pragma unroll
                for (int j = 0; j < 4; ++j) s += work[d * 64 + grp * 4 + j];
                red[d][grp] = s;
            }
            sync();
            if (tid < 16) {
                u64 s = 0;
#pragma unroll
                for (int j = 0; j < 16; ++j) s += red[tid][j];
                msum[tid] = s;
            }
            sync();
            if (L == 0) {
                u64 Q = 0;
                for (int d = 0; d < 16; ++d) Q += msum[d];
                lim = ps < 64 ? (mul_shr24(pm, Q) >> ps) : 0ull;
                if (lim == 0) search = false;                        // only rank 0 survives: the lowest id at the maximum
            }
            if (search) {
                // walking down from bin 15: the bin that holds the smallest key K with (mass above K) < lim -- the first whose own mass takes the
                // running mass to lim or past it (`above` < lim holds on entry at every level)
                int d = 15;
                for (; d > 0; --d) {
                    if (above + msum[d] >= lim) break;
                    above += msum[d];
                }
                mass_k = msum[d];
                prefix = (prefix << 4) | (unsigned int)d;
            }
        }
        u64 r = 1, n_k = 2;                                          // (lim == 0: one id at the maximum; the number of ties is not known)
        thr = mk;
        if (search) {
            thr = prefix;
            const u64 qk = q_of_e(e_of(unkey(thr)));                 // (> 0: a key of mass 0 has all of Q above it, and lim < Q)
            n_k = qk ? mass_k / qk : 0;
            r = qk ? (lim - above + qk - 1) / qk : 0;
        }
        if (r < n_k) {                                               // the cut falls inside the ties at thr: the r lowest ids stay
            const unsigned int tk = thr;
            id_last = locate([&](int, bf16_t v) -> u64 { return bf16_key(v) == tk ? 1ull : 0ull; }, false, r - 1, nullptr);
        }
    }
    const bool use_min = min_p > 0.0f;
    auto weight = [&](int col, bf16_t v) -> u64 {                    // q of a survivor, 0 of anything else
        const unsigned int key = bf16_key(v);
        if (nucleus && !(key > thr || (key == thr && col <= id_last))) return 0ull;
        const float e = e_of(v);
        if (use_min && !(e >= min_p)) return 0ull;
        return q_of_e(e);
    };
    if (keep_out) {                                                  // (probe only; folded away in the decode step)
        for (int u = tid; u < nunit; u += 256) {
            bf16x8 v;
            const int cnt = load_unit(u, v);
            unsigned int bits = 0;
#pragma unroll
            for (int e = 0; e < 8; ++e) {
                const unsigned int key = bf16_key((bf16_t)v[e]);
                const bool kp = e < cnt && (!nucleus || key > thr || (key == thr && u * 8 + e <= id_last)) && (!use_min || e_of((bf16_t)v[e]) >= min_p);
                bits |= (kp ? 1u : 0u) << e;
            }
            keep_out[u] = (unsigned char)bits;
            if (bits) atomic_add_lds(&nkeep, (unsigned int)popc64((u64)bits));
        }
    }
    unsigned int c[4] = {step, 0u, 0u, 0u};
    philox4x32(c, s0, s1);
    u64 S = 0;
    const int tok = locate(weight, true, (u64)(c[0] >> 8), &S);
    if (keep_out && tid == 0) { *n_out = (int)nkeep; *total_out = S; }
    return tok;
}

// The row's n_part (max, sum of exp(v - max)) pairs -> sum of exp(v - M) over the whole row, M = the row's maximum (block-uniform, from the argmax
// reduction).  The walk is the argmax's: kU requests in flight, branch-free (an index past the end re-reads the last pair and counts it 0 times).
// A partial whose maximum is -inf holds sum 0 and exp(-inf - M) = 0; a row without one finite logit (M = -inf) returns 0 without forming an exponent.
// Every thread returns the total.  ss: 4 floats of LDS.  The order of the additions depends on n_part alone: a request's values do not depend on its slot
NTTS_D float lse_merge_row(const float* pv, const float* ps, int n_part, float M, float* ss) {
    const int tid = threadIdx.x;
    constexpr int kU = 8;
    float S = 0.f;
    if (M > -INFINITY) {
        for (int i0 = tid; i0 < n_part; i0 += 256 * kU) {
            float v[kU], q[kU];
#pragma unroll
            for (int u = 0; u < kU; ++u) {
                const int i = i0 + u * 256 < n_part ? i0 + u * 256 : n_part - 1;
                v[u] = pv[i];
                q[u] = ps[i];
            }
#pragma unroll
            for (int u = 0; u < kU; ++u) S += (i0 + u * 256 < n_part ? q[u] : 0.f) * fexp(v[u] - M);
        }
    }
#pragma unroll
    for (int sh = 1; sh < 64; sh <<= 1) S += shfl_xor(S, sh);
    if (lane_id() == 0) ss[wave_id()] = S;
    sync();
    return (ss[0] + ss[1]) + (ss[2] + ss[3]);
}
// (kapi.cpp ntts_k_head_logprob_probe: the merge on the partials of a probe launch; out[2 b] = M, out[2 b + 1] = log S)
NTTS_KERNEL(256) void lse_merge_probe_kernel(const float* part_val, const float* part_sum, int n_part, float* out) {
    NTTS_SHARED float sv[4];
    NTTS_SHARED float ss[4];
    const int b = blockIdx.x, tid = threadIdx.x;
    const float* pv = part_val + (long)b * n_part;
    float best = -INFINITY;
    for (int i = tid; i < n_part; i += 256) best = pv[i] > best ? pv[i] : best;
#pragma unroll
    for (int sh = 1; sh < 64; sh <<= 1) { const float ov = shfl_xor(best, sh); best = ov > best ? ov : best; }
    if (lane_id() == 0) sv[wave_id()] = best;
    sync();
    float M = sv[0];
    for (int w = 1; w < 4; ++w) M = sv[w] > M ? sv[w] : M;
    const float S = lse_merge_row(pv, part_sum + (long)b * n_part, n_part, M, ss);
    if (tid == 0) { out[2 * b] = M; out[2 * b + 1] = logf(S); }
}

NTTS_KERNEL(256) void sample_greedy_kernel(SampleArgs p) {
    NTTS_SHARED float sv[4];
    NTTS_SHARED int si[4];
    NTTS_SHARED float ss[4];
    const int b = blockIdx.x, tid = threadIdx.x;
    float best = -INFINITY;
    int bidx = 0x7fffffff;
    // The lm_head leaves n_part (max, first index) pairs per row (2 268 - 3 400 at NeuTTS-Air's vocabulary): 9 - 14 per thread.  A
    // plain loop is a chain of that many dependent round trips (the compare carries `best`): 9.1 us per decode step.  Here
    // the requests of kU iterations are in flight together, branch-free (an index past the end re-reads the last pair, which
    // changes nothing: max value / lowest index is idempotent).
    constexpr int kU = 8;
    const float* pv = p.part_val + (long)b * p.n_part;
    const int* pi = p.part_idx + (long)b * p.n_part;
    for (int i0 = tid; i0 < p.n_part; i0 += 256 * kU) {
        float v[kU];
        int ix[kU];
#pragma unroll
        for (int u = 0; u < kU; ++u) {
            const int i = i0 + u * 256 < p.n_part ? i0 + u * 256 : p.n_part - 1;
            v[u] = pv[i];
            ix[u] = pi[i];
        }
#pragma unroll
        for (int u = 0; u < kU; ++u)
            if (v[u] > best || (v[u] == best && ix[u] < bidx)) { best = v[u]; bidx = ix[u]; }
    }
#pragma unroll
    for (int sh = 1; sh < 64; sh <<= 1) {
        const float ov = shfl_xor(best, sh);
        const int oi = shfl_xor(bidx, sh);
        if (ov > best || (ov == best && oi < bidx)) { best = ov; bidx = oi; }
    }
    if (lane_id() == 0) { sv[wave_id()] = best; si[wave_id()] = bidx; }
    sync();
    const bool live = p.sl.state[b] == p.phase;                     // block-uniform
    const int k = (live && p.logits) ? p.sl.top_k[b] : 0;
    int sampled = -1;
    if (k > 0) {
        const int step = (p.phase == SLOT_PREFILLED) ? 0 : p.sl.n_new[b];
        sampled = sample_topk_row(p.logits + (long)b * p.ld_logits, p.vocab, k, p.sl.temperature[b], p.sl.top_p[b], p.sl.min_p[b],
                                  p.sl.seed[2 * b], p.sl.seed[2 * b + 1], (unsigned int)step, pv, p.n_part, p.part_width);
    } else if (k != 0) {                                            // top_k = -1: the whole vocabulary
        const int step = (p.phase == SLOT_PREFILLED) ? 0 : p.sl.n_new[b];
        sampled = sample_full_row(p.logits + (long)b * p.ld_logits, p.vocab, p.sl.temperature[b], p.sl.top_p[b], p.sl.min_p[b],
                                  p.sl.seed[2 * b], p.sl.seed[2 * b + 1], (unsigned int)step, pv, p.n_part);
    }
    const bool lse = live && p.part_sum && p.out_logprobs;      // block-uniform
    float M = -INFINITY, S = 0.f;
    if (lse) {
        for (int w = 0; w < 4; ++w) M = sv[w] > M ? sv[w] : M;
        S = lse_merge_row(pv, p.part_sum + (long)b * p.n_part, p.n_part, M, ss);
    }
    if (tid == 0) {
        for (int w = 1; w < 4; ++w)
            if (sv[w] > best || (sv[w] == best && si[w] < bidx)) { best = sv[w]; bidx = si[w]; }
        SlotArrays& s = p.sl;
        if (live) {
            int tok = k != 0 ? sampled : bidx;
            if (lse) {   // log softmax of the whole processed row at the chosen COLUMN: a greedy row's logit is M itself, a drawn one's is in the bf16 row
                const float vt = (k != 0 && (unsigned int)tok < (unsigned int)p.vocab) ? bf2f(p.logits[(long)b * p.ld_logits + tok]) : M;
                const int n0 = (p.phase == SLOT_PREFILLED) ? 0 : s.n_new[b];
                p.out_logprobs[(long)b * s.out_stride + n0] = (vt - M) - logf(S);
            }
            // (a COLUMN: before the compacted head's id mapping; a row without one finite logit yields no index -- nothing to mark)
            if (p.seen && s.rep_pen[b] != 1.0f && (unsigned int)tok < (unsigned int)p.vocab) seen_mark(p.seen + (long)b * p.seen_pitch, tok);
            if (p.n_range > 0) tok = tok < p.n_range ? tok + p.id_base : p.id_tail;
            const int n = (p.phase == SLOT_PREFILLED) ? 0 : s.n_new[b];
            s.out_tokens[(long)b * s.out_stride + n] = tok;
            s.n_new[b] = n + 1;
            if (p.phase == SLOT_RUNNING) s.pos[b] = s.pos[b] + 1;
            s.cur_tok[b] = tok;
            s.mask_eos[b] = (n + 1 < s.min_new[b]) ? s.eos[b] + 1 : 0;
            const bool fin = (tok == s.eos[b]) || (s.prompt_len[b] + n + 1 >= s.max_len[b]);
            s.state[b] = fin ? SLOT_FINISHED : SLOT_RUNNING;
        }
    }
}

// ---- small host->device state plumbing kernels -------------------------------------------------
struct PrefillInit {
    const int* slot;       // [n]
    const int* seq_len;
    const int* min_new;
    const int* max_len;
    const int* eos;
    const int* top_k;      // 0 = greedy
    const int* temp_bits;  // float bits
    const int* top_p_bits; // float bits
    const int* min_p_bits; // float bits
    const int* pen_bits;   // float bits: the repetition penalty, 1 = off
    const int* seed;       // [n][2]
    const int* bt_rows;    // [n][max_pages]
    int* block_table;      // [slots][max_pages]
    int max_pages;
    int n;
    SlotArrays sl;
    unsigned int* seen;    // seen bitmap (null: none allocated yet): the rows of the slots being filled are cleared here
    long seen_pitch;
};
NTTS_KERNEL(64) void prefill_init_kernel(PrefillInit p) {
    const int i = blockIdx.x;
    const int s = p.slot[i];
    for (int k = threadIdx.x; k < p.max_pages; k += 64) p.block_table[(long)s * p.max_pages + k] = p.bt_rows[(long)i * p.max_pages + k];
    if (p.seen) {
        u32x4* row = (u32x4*)(p.seen + (long)s * p.seen_pitch);      // (the pitch is a multiple of 4 words)
        for (long k = threadIdx.x; k < p.seen_pitch / 4; k += 64) row[k] = u32x4{0u, 0u, 0u, 0u};
    }
    if (threadIdx.x == 0) {
        p.sl.state[s] = SLOT_PREFILLED;
        p.sl.pos[s] = p.seq_len[i];
        p.sl.n_new[s] = 0;
        p.sl.prompt_len[s] = p.seq_len[i];
        p.sl.min_new[s] = p.min_new[i];
        p.sl.max_len[s] = p.max_len[i];
        p.sl.eos[s] = p.eos[i];
        p.sl.top_k[s] = p.top_k[i];
        p.sl.temperature[s] = __builtin_bit_cast(float, p.temp_bits[i]);
        p.sl.top_p[s] = __builtin_bit_cast(float, p.top_p_bits[i]);
        p.sl.min_p[s] = __builtin_bit_cast(float, p.min_p_bits[i]);
        p.sl.rep_pen[s] = __builtin_bit_cast(float, p.pen_bits[i]);
        p.sl.seed[2 * s] = (unsigned int)p.seed[2 * i];
        p.sl.seed[2 * s + 1] = (unsigned int)p.seed[2 * i + 1];
        p.sl.mask_eos[s] = p.min_new[i] > 0 ? p.eos[i] + 1 : 0;
        p.sl.cur_tok[s] = 0;
    }
}
// The prompt's share of a penalised request's bitmap (launched behind prefill_init_kernel, which cleared the rows): cols = the lm_head columns of the
// ids at positions >= prompt_ignore_length of the FULL prompts of the call's penalised requests, back to back; request i owns cols[off[i] .. off[i + 1])
// (empty for an unpenalised one).  The host has already mapped ids to columns and dropped those a restricted head does not have.
struct SeenMarkArgs {
    const int* slot;       // [n]
    const int* off;        // [n + 1]
    const int* cols;
    unsigned int* seen;
    long seen_pitch;
};
NTTS_KERNEL(256) void seen_mark_prompt_kernel(SeenMarkArgs p) {
    const int i = blockIdx.x;
    unsigned int* row = p.seen + (long)p.slot[i] * p.seen_pitch;
    for (int t = p.off[i] + (int)threadIdx.x; t < p.off[i + 1]; t += 256) seen_mark(row, p.cols[t]);
}
NTTS_KERNEL(64) void zero_slots_kernel(const int* slots, int n, int* state) {   // ntts_backbone_release_many: state[slots[i]] = FREE
    const int i = blockIdx.x * 64 + threadIdx.x;
    if (i < n) state[slots[i]] = 0;
}
NTTS_KERNEL(64) void bt_update_kernel(const int* trip, int n, int* block_table, int max_pages) {
    const int i = blockIdx.x * 64 + threadIdx.x;
    if (i < n) block_table[(long)trip[3 * i] * max_pages + trip[3 * i + 1]] = trip[3 * i + 2];
}

// dst[dst_row(r)][:] = bf16(src[r][:])  -- weight packing (fp32 -> bf16 RNE like `.to(bfloat16)`)
NTTS_KERNEL(256) void pack_rows_kernel(const void* src, int src_is_f32, bf16_t* dst, const int* dst_rows, long cols) {
    const long r = blockIdx.x;
    const long dr = dst_rows ? dst_rows[r] : r;
    for (long c = threadIdx.x; c < cols; c += 256)
        dst[dr * cols + c] = src_is_f32 ? f2bf(((const float*)src)[r * cols + c]) : ((const bf16_t*)src)[r * cols + c];
}

// GEMM weight packing: logical row r of the source lands in row dr = row0 + (dst_rows ? dst_rows[r] : r) of the packed matrix
// [*, cols]; tile_major = 1 stores it "tile-major" (gemm.h GemmArgs::w_tile_major): groups of 64 rows, inside a group the
// 64 x 64 blocks of consecutive K tiles follow each other, so a workgroup's weight stream is one sequential run of addresses
NTTS_KERNEL(256) void pack_weight_kernel(const void* src, int src_is_f32, bf16_t* dst, const int* dst_rows, long row0, long cols,
                                         int tile_major) {
    const long r = blockIdx.x;
    const long dr = row0 + (dst_rows ? dst_rows[r] : r);
    for (long c = threadIdx.x; c < cols; c += 256) {
        const bf16_t v = src_is_f32 ? f2bf(((const float*)src)[r * cols + c]) : ((const bf16_t*)src)[r * cols + c];
        const long at = tile_major ? (dr >> 6) * 64 * cols + (c >> 6) * 4096 + (dr & 63) * 64 + (c & 63) : dr * cols + c;
        dst[at] = v;
    }
}

// Compacted lm_head (ntts_backbone_set_logits_range): row r of dst = row rows[r] of src, both tile-major in 64-row x 128-byte blocks
// (esz = 2: 64 bf16 per block row, esz = 1: 128 e4m3); one workgroup per destination row, 16 bytes per thread and k-tile; the fp8 head's
// per-row scales travel along
NTTS_KERNEL(64) void gather_head_rows_kernel(const unsigned char* src, unsigned char* dst, const int* rows, long K_bytes, const float* sc_src, float* sc_dst) {
    const long r = blockIdx.x, sr = rows[r];
    const long ktiles = K_bytes / 128;
    for (long i = threadIdx.x; i < ktiles * 8; i += 64) {
        const long kt = i >> 3, c = i & 7;
        *(u32x4*)(dst + (r >> 6) * 64 * K_bytes + kt * 8192 + (r & 63) * 128 + c * 16) =
            *(const u32x4*)(src + (sr >> 6) * 64 * K_bytes + kt * 8192 + (sr & 63) * 128 + c * 16);
    }
    if (sc_src && threadIdx.x == 0) sc_dst[r] = sc_src[sr];
}
// running max |x| over bf16 rows (fp8 calibration, ntts_backbone_calibrate): 8 values per thread and iteration; the bit pattern of a
// non-negative float orders like the value, so the combine is an integer atomic max
NTTS_KERNEL(256) void amax_bf16_kernel(const bf16_t* x, long nvec, float* out) {
    float m = 0.f;
    for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < nvec; i += (long)gridDim.x * 256) {
        const bf16x8 v = ld16<bf16x8>(x + i * 8);
#pragma unroll
        for (int e = 0; e < 8; ++e) {
            const float a = __builtin_fabsf(bf2f((bf16_t)v[e]));
            m = a > m ? a : m;             // (NaN never wins)
        }
    }
#pragma unroll
    for (int sh = 1; sh < 64; sh <<= 1) { const float o = shfl_xor(m, sh); m = o > m ? o : m; }
    if (lane_id() == 0) atomic_max_global_u32((unsigned int*)out, __builtin_bit_cast(unsigned int, m));
}

// ---- parking (ntts_backbone_activate): the per-slot state of parked request src[i] becomes decode slot dst[i]'s; one workgroup per pair
struct ActivateArgs {
    const int* pairs;        // [n][2] = (parking row, decode slot)
    SlotArrays sl;
    int* block_table;        // [slots][max_pages]
    int max_pages;
    unsigned int* seen;      // seen bitmap (null: none allocated): the row moves with the request
    long seen_pitch;
    float* out_logprobs;     // [slots][sl.out_stride] log-probability record (null: ntts_backbone_set_logprobs is off)
};
NTTS_KERNEL(64) void activate_slots_kernel(ActivateArgs p) {
    const int src = p.pairs[2 * blockIdx.x], dst = p.pairs[2 * blockIdx.x + 1];
    const int lane = threadIdx.x;
    const int nn = p.sl.n_new[src];
    for (int k = lane; k < nn; k += 64) p.sl.out_tokens[(long)dst * p.sl.out_stride + k] = p.sl.out_tokens[(long)src * p.sl.out_stride + k];
    if (p.out_logprobs)      // (the first token's log-probability moves with it)
        for (int k = lane; k < nn; k += 64) p.out_logprobs[(long)dst * p.sl.out_stride + k] = p.out_logprobs[(long)src * p.sl.out_stride + k];
    for (int k = lane; k < p.max_pages; k += 64) p.block_table[(long)dst * p.max_pages + k] = p.block_table[(long)src * p.max_pages + k];
    if (p.seen)              // (an unpenalised request's row is all zeros: it replaces whatever the decode slot's last occupant left)
        for (long k = lane; k < p.seen_pitch; k += 64) p.seen[(long)dst * p.seen_pitch + k] = p.seen[(long)src * p.seen_pitch + k];
    if (lane == 0) {
        p.sl.pos[dst] = p.sl.pos[src]; p.sl.n_new[dst] = nn; p.sl.cur_tok[dst] = p.sl.cur_tok[src]; p.sl.prompt_len[dst] = p.sl.prompt_len[src];
        p.sl.min_new[dst] = p.sl.min_new[src]; p.sl.max_len[dst] = p.sl.max_len[src]; p.sl.eos[dst] = p.sl.eos[src]; p.sl.mask_eos[dst] = p.sl.mask_eos[src];
        p.sl.top_k[dst] = p.sl.top_k[src]; p.sl.temperature[dst] = p.sl.temperature[src];
        p.sl.top_p[dst] = p.sl.top_p[src]; p.sl.min_p[dst] = p.sl.min_p[src]; p.sl.rep_pen[dst] = p.sl.rep_pen[src];
        p.sl.seed[2 * dst] = p.sl.seed[2 * src]; p.sl.seed[2 * dst + 1] = p.sl.seed[2 * src + 1];
        p.sl.state[dst] = p.sl.state[src];
        p.sl.state[src] = SLOT_FREE;
    }
}

// ids -> codec codes on the device (ref:neutts/neutts.py:349 tokenizer.decode + :276 regex, as one pass): of slot s's new ids
// keep those in [speech_base, speech_base + n_codes), as id - speech_base, in order; `modulo` (synthetic benchmark only: random
// weights do not stay in the speech range) maps every id to id mod n_codes instead.  One workgroup per utterance.
struct ExportCodesArgs {
    const int* slots;       // [n] decode slots
    SlotArrays sl;
    int speech_base, n_codes, modulo;
    int* codes;             // [n][stride]
    int stride;
    int* lens;              // [n] number of codes written
};
NTTS_KERNEL(256) void export_codes_kernel(ExportCodesArgs p) {
    NTTS_SHARED int wcount[4];
    NTTS_SHARED int base_s;
    const int u = blockIdx.x, s = p.slots[u], tid = threadIdx.x, lane = lane_id(), w = wave_id();
    const int n = p.sl.n_new[s];
    const int* ids = p.sl.out_tokens + (long)s * p.sl.out_stride;
    if (tid == 0) base_s = 0;
    sync();
    for (int t0 = 0; t0 < n; t0 += 256) {      // order-preserving compaction, 256 ids per round
        const int t = t0 + tid;
        int code = -1;
        if (t < n) {
            const int id = ids[t];
            if (p.modulo) code = id % p.n_codes;
            else if (id >= p.speech_base && id < p.speech_base + p.n_codes) code = id - p.speech_base;
        }
        const unsigned long long m = ballot(code >= 0);
        const int before = popc64(m & ((1ull << lane) - 1ull));
        if (lane == 0) wcount[w] = popc64(m);
        sync();
        int off = base_s;
        for (int k = 0; k < w; ++k) off += wcount[k];
        if (code >= 0 && off + before < p.stride) p.codes[(long)u * p.stride + off + before] = code;
        sync();
        if (tid == 0) base_s += wcount[0] + wcount[1] + wcount[2] + wcount[3];
        sync();
    }
    if (tid == 0) p.lens[u] = base_s < p.stride ? base_s : p.stride;
}

// The same hand-off for STREAMS (ref:neutts/neutts.py:390-404: every generated "<|speech_N|>" token is appended to the stream's token
// cache as it arrives): of slot s's ids generated since the previous call (seen[u]), the speech codes are appended to the stream's
// device-side code cache behind its clen[u] entries; seen / clen are advanced and the slot's state is reported.  One workgroup per stream.
struct AppendCodesArgs {
    const int* slots;       // [n] decode slots
    SlotArrays sl;
    int speech_base, n_codes, modulo;
    int* cache;             // [n][stride] reference codes + generated codes so far
    int stride;
    int* clen;              // [n] codes in cache[u]
    int* seen;              // [n] generated ids already looked at
    int* fin;               // [n] out: 1 once the slot has finished (EOS / max_length) -- with everything it generated appended
};
NTTS_KERNEL(256) void append_codes_kernel(AppendCodesArgs p) {
    NTTS_SHARED int wcount[4];
    NTTS_SHARED int base_s;
    const int u = blockIdx.x, s = p.slots[u], tid = threadIdx.x, lane = lane_id(), w = wave_id();
    const int st = p.sl.state[s];
    const int n = (st == SLOT_RUNNING || st == SLOT_FINISHED) ? p.sl.n_new[s] : 0;
    const int from = p.seen[u];
    const int* ids = p.sl.out_tokens + (long)s * p.sl.out_stride;
    if (tid == 0) base_s = p.clen[u];
    sync();
    for (int t0 = from; t0 < n; t0 += 256) {      // order-preserving compaction, 256 ids per round (export_codes_kernel)
        const int t = t0 + tid;
        int code = -1;
        if (t < n) {
            const int id = ids[t];
            if (p.modulo) code = id % p.n_codes;
            else if (id >= p.speech_base && id < p.speech_base + p.n_codes) code = id - p.speech_base;
        }
        const unsigned long long m = ballot(code >= 0);
        const int before = popc64(m & ((1ull << lane) - 1ull));
        if (lane == 0) wcount[w] = popc64(m);
        sync();
        int off = base_s;
        for (int k = 0; k < w; ++k) off += wcount[k];
        if (code >= 0 && off + before < p.stride) p.cache[(long)u * p.stride + off + before] = code;
        sync();
        if (tid == 0) base_s += wcount[0] + wcount[1] + wcount[2] + wcount[3];
        sync();
    }
    if (tid == 0) {
        p.clen[u] = base_s < p.stride ? base_s : p.stride;
        p.seen[u] = n > from ? n : from;
        p.fin[u] = st == SLOT_FINISHED ? 1 : 0;
    }
}

// fp8 model: one source row -> e4m3 bytes + its scale.  The row is first rounded to bf16 (what the bf16 checkpoint holds), then
// scale = max|w| / 448 (1 for an all-zero row), w_q = e4m3(w / scale) -- per output channel, as static-fp8 checkpoints store
// them.  Layout of the byte matrix: tile-major in 64-row x 128-byte blocks (gemm.h F8).
NTTS_KERNEL(256) void pack_weight_fp8_kernel(const void* src, int src_is_f32, unsigned char* dst, float* scales, const int* dst_rows,
                                             long row0, long cols) {
    NTTS_SHARED float red[4];
    const long r = blockIdx.x;
    const long dr = row0 + (dst_rows ? dst_rows[r] : r);
    auto val = [&](long c) { return src_is_f32 ? rbf(((const float*)src)[r * cols + c]) : bf2f(((const bf16_t*)src)[r * cols + c]); };
    float am = 0.f;
    for (long c = threadIdx.x; c < cols; c += 256) am = fmaxf(am, fabsf(val(c)));
#pragma unroll
    for (int sh = 1; sh < 64; sh <<= 1) am = fmaxf(am, shfl_xor(am, sh));
    if (lane_id() == 0) red[wave_id()] = am;
    sync();
    am = fmaxf(fmaxf(red[0], red[1]), fmaxf(red[2], red[3]));
    const float scale = am > 0.f ? am / kFp8Max : 1.0f;
    if (threadIdx.x == 0) scales[dr] = scale;
    for (long c = threadIdx.x; c < cols; c += 256)
        dst[(dr >> 6) * 64 * cols + (c >> 7) * 8192 + (dr & 63) * 128 + (c & 127)] = f2fp8c(val(c) / scale);
}

// pre-quantised fp8 checkpoints: the matrix arrives as e4m3 bytes [rows][cols] and is stored as it is (same layout as above);
// its per-output-channel scales arrive separately (one fp32 per row, or one for the whole matrix: `broadcast`)
NTTS_KERNEL(256) void pack_weight_fp8_raw_kernel(const unsigned char* src, unsigned char* dst, const int* dst_rows, long row0, long cols) {
    const long r = blockIdx.x;
    const long dr = row0 + (dst_rows ? dst_rows[r] : r);
    for (long c = threadIdx.x; c < cols; c += 256)
        dst[(dr >> 6) * 64 * cols + (c >> 7) * 8192 + (dr & 63) * 128 + (c & 127)] = src[r * cols + c];
}
NTTS_KERNEL(256) void scatter_scales_kernel(const float* src, int broadcast, float* dst, const int* dst_rows, long row0, long n) {
    const long r = (long)blockIdx.x * 256 + threadIdx.x;
    if (r < n) dst[row0 + (dst_rows ? dst_rows[r] : r)] = src[broadcast ? 0 : r];
}

// number of elements of `src` ([rows][cols], fp32 or bf16) whose bf16 value differs from ref[rows][cols]: the tied-head check
NTTS_KERNEL(256) void rows_mismatch_kernel(const void* src, int src_is_f32, const bf16_t* ref, long cols, unsigned int* count) {
    const long r = blockIdx.x;
    unsigned int bad = 0;
    for (long c = threadIdx.x; c < cols; c += 256) {
        const bf16_t v = src_is_f32 ? f2bf(((const float*)src)[r * cols + c]) : ((const bf16_t*)src)[r * cols + c];
        bad += v != ref[r * cols + c];
    }
    if (bad) atomic_add_global(count, bad);
}

}  // namespace ntts
