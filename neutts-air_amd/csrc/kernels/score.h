// score.h -- teacher-forced scoring of GIVEN tokens (ntts_backbone_score): the merge behind the lm_head's EPI_ARGMAX_LSE_TGT epilogue (gemm.h).
//
// The lm_head leaves, per scored row, n_part (max, first index, sum of exp(v - max)) partials and ONE value, the processed logit of the row's
// target column; the [rows][V] logits are never materialised.  One workgroup per row merges the partials with sample_greedy_kernel's own
// arithmetic (sample.h: the branch-free walk, first index wins, lse_merge_row for the sum) and writes
//     logprob        = target_val - (M + log S)   as (target_val - M) - log S, the form the decoder's record uses
//     argmax         = the first index of the row maximum M (what greedy decoding would emit there)
//     argmax_logprob = -log S                      ((M - M) - log S)
// A partial whose maximum is -inf carries sum 0 and contributes 0 * exp(-inf - M) = 0; a row without one finite logit (M = -inf) forms no
// exponent at all (lse_merge_row) and reports -inf / index 0x7fffffff / -inf -- no real head produces one.
#pragma once
#include "sample.h"

namespace ntts {

struct ScoreMergeArgs {
    const float* part_val;     // [rows][n_part]
    const int* part_idx;
    const float* part_sum;
    int n_part;
    const float* target_val;   // [rows]
    float* logprob;            // [rows] outputs
    int* argmax;
    float* argmax_logprob;
};

NTTS_KERNEL(256) void score_merge_kernel(ScoreMergeArgs p) {
    NTTS_SHARED float sv[4];
    NTTS_SHARED int si[4];
    NTTS_SHARED float ss[4];
    const int b = blockIdx.x, tid = threadIdx.x;
    float best = -INFINITY;
    int bidx = 0x7fffffff;
    constexpr int kU = 8;      // (sample_greedy_kernel: kU requests in flight; an index past the end re-reads the last pair, which changes nothing)
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
    float M = sv[0];
    int mi = si[0];
    for (int w = 1; w < 4; ++w)
        if (sv[w] > M || (sv[w] == M && si[w] < mi)) { M = sv[w]; mi = si[w]; }
    const float S = lse_merge_row(pv, p.part_sum + (long)b * p.n_part, p.n_part, M, ss);
    if (tid == 0) {
        const bool any = M > -INFINITY;                     // (-inf - -inf is never formed)
        const float ls = any ? logf(S) : 0.f;
        p.logprob[b] = any ? (p.target_val[b] - M) - ls : -INFINITY;
        p.argmax[b] = mi;
        p.argmax_logprob[b] = any ? -ls : -INFINITY;
    }
}

// block_table[slots[i]][:] = rows[i][:] -- the only device slot state a score call writes: the prompt-pass attention finds the pages of the
// sequences through it.  The slots are free (their state words stay FREE: no decode step looks at them) and are free again when the call returns.
NTTS_KERNEL(64) void score_block_table_kernel(const int* slots, const int* rows, int* block_table, int max_pages) {
    const int i = blockIdx.x;
    const long s = slots[i];
    for (int k = threadIdx.x; k < max_pages; k += 64) block_table[s * max_pages + k] = rows[(long)i * max_pages + k];
}

}  // namespace ntts
