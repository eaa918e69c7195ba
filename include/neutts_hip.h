/* neutts_hip.h -- C ABI of libneutts_hip.so (MI355X / gfx950).
 *
 * The drop-in boundary for the NeuTTS synthesis hot path.  The reference has no FFI of its own:
 * its seam is two third-party Python calls, and each entry point below names the one it replaces.
 *
 *   backbone:  self.backbone.generate(prompt[1,S], max_length, eos_token_id, do_sample, temperature,
 *              top_k, use_cache, min_new_tokens) -> ids            ref:neutts/neutts.py:338-347
 *              (transformers Qwen2ForCausalLM + GenerationMixin._sample, un-vendored dependency)
 *   codec:     self.codec.decode_code(codes[1,1,T]) -> wav[1,1,480*T]   ref:neutts/neutts.py:288-291
 *              (neucodec NeuCodec.decode_code, un-vendored dependency)
 *
 * Conventions
 *   - plain C types, raw pointers and sizes; no torch / C++ types cross the boundary.
 *   - every function returns 0 on success, a negative NTTS_E* code on failure, and never throws;
 *     ntts_last_error() returns the message of the most recent failure on that engine
 *     (pass NULL for failures of ntts_*_create itself).
 *   - the CALLER owns every buffer it passes in; the library owns only what it allocates itself
 *     (weight arena, KV page pool, workspaces), all in the HBM of the device given at create time.
 *   - an engine is bound to ONE device, is not re-entrant and not thread-safe: serialise calls per
 *     engine (the Python host holds the GIL across each call).  One process per GPU; there is no
 *     cross-GPU collective inside any entry point (utterances are independent).
 *   - work is enqueued on the engine's HIP stream -- its own, or one the caller lends with ntts_backbone_set_stream /
 *     ntts_codec_set_stream (ABI 6); functions named *_sync or documented as "blocking" wait for it, the others return
 *     once the work is enqueued.
 *   - there is NO CPU fallback: without a gfx950 device ntts_*_create fails with NTTS_ENODEV.
 */
#ifndef NEUTTS_HIP_H
#define NEUTTS_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define NTTS_ABI_VERSION 11

enum {
    NTTS_OK = 0,
    NTTS_EINVAL = -1,   /* bad argument / unknown tensor name / shape mismatch */
    NTTS_ENODEV = -2,   /* no usable gfx950 device */
    NTTS_ENOMEM = -3,   /* HBM allocation or KV page pool exhausted */
    NTTS_ESTATE = -4,   /* call out of order (weights not finalised, slot busy, ...) */
    NTTS_EHIP = -5      /* a HIP runtime call failed; see ntts_last_error */
};

enum { NTTS_DT_F32 = 0, NTTS_DT_BF16 = 1, NTTS_DT_I32 = 2, NTTS_DT_FP8_E4M3 = 3 /* ABI 6: pre-quantised matrices of an fp8 checkpoint (bytes) */ };

/* ------------------------------------------------------------------------------------------ */
/* Backbone engine: Qwen2-style decoder, paged KV cache, continuous batching over `max_batch`   */
/* decode slots.  Replaces transformers' Qwen2ForCausalLM.forward + GenerationMixin._sample     */
/* (hf:models/qwen2/modeling_qwen2.py:342-477, hf:generation/utils.py:2783-2973) behind         */
/* ref:neutts/neutts.py:338-347.                                                                */
/* ------------------------------------------------------------------------------------------ */
typedef struct ntts_backbone ntts_backbone;

typedef struct ntts_backbone_config {
    int32_t vocab_size;         /* V (lm_head tied to the embedding) */
    int32_t hidden_size;        /* 896 */
    int32_t intermediate_size;  /* 4864 */
    int32_t num_layers;         /* 24 */
    int32_t num_heads;          /* 14 */
    int32_t num_kv_heads;       /* 2  (num_heads / num_kv_heads must be <= 16) */
    int32_t head_dim;           /* 64 (NeuTTS-Air: the fused / tiered attention kernels) or 128 (ABI 9: the general attention path -- plain QKV GEMM +
                                 * a norm / RoPE / KV-append pass, head_dim-templated two-sweep prompt attention and decode attention; bf16 only;
                                 * the small-batch GEMV step, context-split attention and the resident / deep prompt tiers are off) */
    float rms_eps;              /* 1e-6 */
    int32_t max_context;        /* ref:neutts/neutts.py:85  (2048) */
    int32_t max_batch;          /* number of slots; the decode step runs over the first max_batch - park_slots of them */
    int32_t num_pages;          /* KV pool size in pages of NTTS_PAGE_TOKENS tokens; 0 = max_batch * max_context / page */
    int32_t max_prefill_tokens; /* workspace rows for one packed prefill call; 0 = 16384 */
    /* ABI 2: architecture / precision switches of the decoder family the reference's AutoModelForCausalLM dispatch covers
     * (ref:neutts/neutts.py:164: NeuTTS-Air = Qwen2; NeuTTS-Nano ships under the same class surface). */
    int32_t tie_word_embeddings; /* 1: lm_head = embedding (Qwen2.5-0.5B / NeuTTS-Air); 0: a separate "lm_head.weight" must be loaded */
    int32_t attention_bias;      /* 1: q/k/v_proj carry a bias (Qwen2); 0: none (Llama-style) */
    int32_t qk_norm;             /* ABI 9: 1 = Qwen3-style per-head RMSNorm of q and k (over head_dim, weights "self_attn.q_norm.weight" / "k_norm.weight",
                                  * before RoPE: hf:models/qwen3/modeling_qwen3.py Qwen3Attention.forward); takes the general attention path like head_dim 128 */
    int32_t weight_dtype;        /* NTTS_W_BF16 | NTTS_W_FP8_E4M3: fp8 weights with per-output-channel scales, fp8 GEMM inputs with
                                    static per-tensor scales ("*.input_scale" tensors), bf16 residual stream / KV / attention */
    int32_t park_slots;          /* ABI 9.  The LAST park_slots slots are PARKING rows: a prompt pass fills them like any slot (KV pages, first token) but no
                                  * decode step touches them; ntts_backbone_activate moves a parked request into a free decode slot.  A continuous-batching
                                  * scheduler admits prompts in efficient waves into the parking rows while every decode row stays busy (the reference has no
                                  * scheduler: ref:neutts/neutts.py:335 runs one utterance at a time).  0 = none (a zeroed field: ABI 8 behaviour) */
} ntts_backbone_config;
enum { NTTS_W_BF16 = 0, NTTS_W_FP8_E4M3 = 1 };

#define NTTS_PAGE_TOKENS 32

int ntts_abi_version(void);
const char* ntts_last_error(const ntts_backbone* e);

int ntts_backbone_create(const ntts_backbone_config* cfg, int device, ntts_backbone** out);
void ntts_backbone_destroy(ntts_backbone* e);

/* Weight upload.  `name` is the HF state-dict key of Qwen2ForCausalLM ("model.embed_tokens.weight",
 * "model.layers.{i}.self_attn.q_proj.weight|bias", ..., "model.norm.weight"; "lm_head.weight": with tie_word_embeddings
 * it must hold the embedding's values -- anything else is NTTS_EINVAL, never silently dropped -- without, it is the
 * separate head matrix) plus "rope.inv_freq" (fp32 [head_dim/2], the buffer hf:models/qwen2/modeling_qwen2.py:86 computes).
 * NTTS_W_FP8_E4M3: the matrices are quantised on upload (per output channel: scale = max|w| / 448, w_q = e4m3(w / scale)) and
 * the static activation scales of the four GEMM inputs of a layer and of the head are loaded as fp32 scalars named
 * "model.layers.{i}.self_attn.q_proj.input_scale" (= k_proj / v_proj), "...self_attn.o_proj.input_scale",
 * "...mlp.gate_proj.input_scale" (= up_proj), "...mlp.down_proj.input_scale", "lm_head.input_scale" (the naming of
 * static-fp8 checkpoints).  ABI 6, PRE-QUANTISED fp8 checkpoints: a matrix may arrive as NTTS_DT_FP8_E4M3 bytes ([N][K] row-major e4m3fn) together with
 * its "<module>.weight_scale" tensor (fp32: one value per output channel, [N] or [N, 1], or ONE value for the whole matrix) -- in either order; it is
 * then stored as it is, not re-quantised (finalize insists on the scale; a scale for a matrix that was quantised on upload is NTTS_EINVAL).  The
 * embedding stays bf16 / fp32 (it is gathered, not multiplied); with tie_word_embeddings the head's fp8 copy is derived from it.
 * `data` may be a host or a device pointer
 * (is_device); dtype NTTS_DT_F32 or NTTS_DT_BF16 (fp32 is rounded to bf16 RNE, like `.to(bfloat16)`).
 * The tensor is copied into the engine's packed arena (fused QKV rows, gate/up interleaved in 16-row
 * groups) -- the caller's buffer can be freed on return.  Blocking. */
int ntts_backbone_load_tensor(ntts_backbone* e, const char* name, const void* data, int dtype,
                              const int64_t* shape, int ndim, int is_device);
/* All tensors present?  Builds the RoPE table and freezes the arena. */
int ntts_backbone_finalize(ntts_backbone* e);
/* The packed arena (device pointer + bytes): what rank 0 broadcasts over RCCL/xGMI to the other
 * ranks at start-up instead of every rank reading the checkpoint.  Valid after
 * finalize on the sender; a receiver calls ntts_backbone_adopt_arena() after the broadcast landed. */
int ntts_backbone_arena(ntts_backbone* e, void** dev_ptr, size_t* bytes);
int ntts_backbone_adopt_arena(ntts_backbone* e);
/* The byte range of the arena that is derived from another part of it (the tied lm_head's own tile-major / fp8 copy of the
 * embedding; *bytes = 0 if there is none): a broadcast may skip it, ntts_backbone_adopt_arena rebuilds it on the receiver. */
int ntts_backbone_arena_derived(ntts_backbone* e, size_t* off, size_t* bytes);
/* Device-to-device copy between the arena and a caller buffer of exactly the arena size (the staging
 * tensor torch.distributed broadcasts): to_arena = 0 arena -> buf, 1 buf -> arena.  Blocking. */
int ntts_backbone_arena_copy(ntts_backbone* e, void* buf, size_t bytes, int to_arena);
/* (ABI 7) A second engine on the SAME weights: `e` (created with the donor's configuration on the donor's device, nothing loaded
 * yet) drops its own arena and reads the finalised donor's; KV pool, slots, workspaces, stream and step graph stay its own.  For
 * several decode chains side by side on one GPU (ref:neutts/neutts.py:338-347 run for more than one batch at a time: each engine
 * replays its own step graph on its own stream, the launching thread alternates between them).  Weight loads into either
 * engine are refused from then on (NTTS_ESTATE); at most 16 engines per arena. */
int ntts_backbone_share_arena(ntts_backbone* e, ntts_backbone* donor);

/* How many decode chains run side by side on this GPU, this engine's included (an engine gang: several engines on one arena, each
 * on a lane stream, their step graphs replayed alternately).  The decode step's shape follows it: alone, an engine tiles its
 * GEMMs to fill the chip by itself (64-row m-blocks, split-K aimed at 224 workgroups, row-block XCD placement); in a gang the
 * other chains fill the chip and what counts is how many bytes each CU pulls, so o_proj / down_proj take the 256-row tile (a weight
 * tile passes through a CU's load path once per chain) and the XCD placement is off.  Same arithmetic, same
 * summation order per output element: ids and logits do not depend on it, bit for bit.
 * ABI 9: the engine COUNTS the chains itself -- at every ntts_backbone_decode call, the engines of its arena (ntts_backbone_share_arena)
 * whose latest decode call lies within the last 50 ms, itself included -- and keeps one captured step graph per shape, so a caller
 * that never heard of this function gets the right shape, and an engine that leaves its gang for a while (one utterance on engine 0)
 * runs the single-chain shape meanwhile.  This call PINS the count instead (chains > 0: tests, sweeps, profiling one engine in the
 * gang's shape); chains = 0 returns to counting.  ABI 8 had only the pinned form (and dropped the captured graph on every call).
 * Replaces nothing in the reference (ref:neutts/neutts.py runs one utterance at a time); the arena is reference-counted (atomically since
 * ABI 9): donor and readers may be destroyed in any order, from any thread. */
int ntts_backbone_set_gang(ntts_backbone* e, int32_t chains);

/* ABI 8, OPT-IN.  Restrict the lm_head to the token ids [lo, hi) plus eos_id: the decode step streams a compacted copy of those
 * rows (NeuTTS-Air: 65 537 x 896 bf16 = 118 MB instead of 390 MB) and every other id is treated as logit -inf.  The reference
 * only ever CONSUMES ids of that shape -- ref:neutts/neutts.py:276 keeps `<|speech_N|>` tokens, ref:neutts/neutts.py:336-341 stops
 * at `<|SPEECH_GENERATION_END|>` -- but hf:generation/utils.py:2894-2925 takes the argmax / top-k over the WHOLE vocabulary: the
 * GREEDY ids are the reference's whenever its argmax lies in the range, and differ otherwise; a SAMPLED draw (do_sample, top_k)
 * matches the reference's only when the WHOLE full-vocabulary top-k set lies in range + EOS (one candidate outside changes the
 * candidate set and the softmax normaliser) and eos_id > hi (the compacted columns are in column order = token-id order only
 * then; true for NeuTTS-Air).  Never the parity configuration.
 * lo < 0 restores the full head.  While a range is set, requests must use eos_token_id == eos_id; no slot may be in use when this
 * is called.  Per engine (twins of a gang each build their own 118 MB copy). */
int ntts_backbone_set_logits_range(ntts_backbone* e, int32_t lo, int32_t hi, int32_t eos_id);

/* ABI 8.  fp8 activation-scale calibration.  The reference's quantised builds are ready-made files (ref:README.md:59-64: Q4 / Q8 GGUF);
 * the fp8 model here takes static per-tensor `input_scale`s as a static-fp8 checkpoint ships them.  For a user who holds the bf16
 * checkpoint: calibration mode on a BF16 engine (enable = 1 resets the record, 0 ends the mode) makes every prompt pass record
 * max |x| of every GEMM's input rows; ntts_backbone_read_amax hands the n = 4 * num_layers + 1 values out, [layer][q_proj (QKV), o_proj,
 * gate_proj (gate/up), down_proj] and the lm_head's last.  input_scale = amax / 448 (tools/calibrate_fp8.py writes them). */
int ntts_backbone_calibrate(ntts_backbone* e, int32_t enable);
int ntts_backbone_read_amax(ntts_backbone* e, float* out, int32_t n);

/* ABI 9.  Move `n` parked requests into free decode slots: park_slots[i] (a parking row holding a prefilled request: its KV pages, position, first token and
 * sampling state) -> slots[i] (a FREE decode slot, < max_batch - park_slots).  Stream-ordered behind the prompt pass that filled the parking row and ahead of
 * the next decode step, which then treats the request like any other; the parking row is free again.  Ids cannot depend on it: a request's arithmetic does
 * not depend on the slot it runs in (tests/test_gpu_backbone.py slot-invariance tests). */
int ntts_backbone_activate(ntts_backbone* e, int32_t n, const int32_t* park_slots, const int32_t* slots);

/* Sampling contract of one request = the keyword arguments of the reference's generate() call
 * (ref:neutts/neutts.py:338-347).
 * ABI 10: top_p / min_p, appended (generate()'s own keyword arguments of those names, which the reference's call leaves at their
 * defaults).  The warpers run in the order of hf:generation/utils.py _get_logits_processor: temperature -> top_k -> top_p -> min_p ->
 * multinomial.  With top_p = 1 and min_p = 0 a request draws exactly the ids it drew under ABI 9.
 * ABI 11: repetition_penalty / prompt_ignore_length, appended (generate()'s keyword argument `repetition_penalty`, which the reference's call leaves at
 * 1.0, and RepetitionPenaltyLogitsProcessor's `prompt_ignore_length`: hf:generation/logits_process.py).  The processor runs FIRST in
 * hf:generation/utils.py _get_logits_processor -- before MinNewTokensLength and the warpers -- and so applies to greedy and sampled requests alike: for
 * every token id that occurs in the request's prompt (from position prompt_ignore_length on) or in what it has generated so far,
 * score = score * p if score < 0 else score / p.  It lives in the lm_head epilogue, on a per-slot bitmap of seen tokens that follows the request
 * through parking rows and slot recycling.
 * NUMERICS: the penalised value is bf16_rne(fp32(v) * p) or bf16_rne(fp32(v) / p), v = the bf16 logit the lm_head produces.  HF keeps the fp32 product;
 * the engine rounds it ONCE, because its exact 16-bit top-k select and its argmax partials both work on bf16 rows and must agree with each other.  The
 * deviation from HF is at most half a bf16 ulp of the penalised logit (relative 2^-8) and touches penalised tokens only: the one place where the
 * processed logits (ntts_backbone_read_logits) are not HF's value for value.  -inf (a masked EOS) stays -inf for any valid p; no NaN arises.
 * With repetition_penalty = 1 (or 0, a zeroed field) a request computes exactly what it computed under ABI 10, and an engine that has no penalised
 * request in flight runs exactly the kernels it ran under ABI 10.
 * top_k = NTTS_TOP_K_OFF (-1; transformers spells it top_k=0 / None, serving stacks -1): no top-k cut.  Temperature, top_p and min_p act on the WHOLE
 * vocabulary and the draw is over the model's own distribution -- the one `logprobs` and ntts_backbone_score describe.  Same struct, same ABI version:
 * the value was NTTS_EINVAL before.  The contract (tests/sampling_full_spec.py): e_a = fp32 exp((x_a - max) * (1 / T)), the mass of token a is the
 * INTEGER q_a = floor(e_a * 2^32), every sum is an exact integer sum; top_p: ranked by value descending, ties by token id ascending, a token survives
 * while the mass strictly before it is < floor(top_p * sum q) (the first always survives); min_p: e_a >= min_p; both evaluated on the whole row and
 * ANDed; draw: the first survivor, in token-id order, whose running mass exceeds (u24 * S) >> 24, S the survivors' mass, u24 the top 24 bits of
 * Philox(seed, step)[0].  The ids depend on the row and the parameters only -- not on slot, batch or the order of any additions.  A token whose
 * probability is below 2^-32 of the likeliest token's has mass 0 and is never drawn. */
#define NTTS_TOP_K_OFF (-1)
typedef struct ntts_sampling {
    int32_t max_length;      /* total length cap (prompt + new), <= max_context        [2048] */
    int32_t min_new_tokens;  /* EOS logit = -inf while fewer new tokens than this      [50]   */
    int32_t eos_token_id;    /* <|SPEECH_GENERATION_END|>                                      */
    int32_t do_sample;       /* 0 = greedy argmax (first max wins); 1 = temperature, top-k, multinomial [1] */
    int32_t top_k;           /* [50]  >= 1; logits below the k-th largest are dropped, ties at the k-th kept (<= 512 kept: a larger k is capped there --
                              * NTTS_TOP_K_OFF (-1) samples over the whole vocabulary instead).  0 and anything below -1: NTTS_EINVAL.  Ignored when do_sample = 0 */
    float temperature;       /* [1.0] > 0 */
    uint64_t seed;           /* Philox4x32-10 key for do_sample=1; the draw of step t depends on (seed, t) only: give each request its own seed */
    float top_p;             /* [1.0] (0, 1].  < 1: nucleus cut over the top-k survivors, ranked by probability descending (ties: lowest token id first) --
                              * a token survives while the probability mass strictly before it is < top_p; the most probable one always survives
                              * (TopPLogitsWarper with min_tokens_to_keep = 1, hf:generation/logits_process.py).  Ignored when do_sample = 0 */
    float min_p;             /* [0.0] [0, 1].  > 0: a token survives iff its probability is >= min_p x the largest probability
                              * (MinPLogitsWarper, hf:generation/logits_process.py).  Ignored when do_sample = 0.
                              * Either field NaN or out of range: NTTS_EINVAL from the prefill call, naming the prompt; no slot is touched */
    float repetition_penalty;      /* [1.0] finite and > 0; 1 = off, and so is 0 (a zeroed field, as with ntts_backbone_config.park_slots).  NaN, negative or
                                    * inf: NTTS_EINVAL from the prefill call, naming the prompt; no slot is touched */
    int32_t prompt_ignore_length;  /* [0] >= 0: the first so many prompt ids do not count as seen (0 = HF's default, the whole prompt counts; a value above
                                    * the prompt length means the whole prompt is ignored: generated tokens only).  Ignored when the penalty is off */
} ntts_sampling;

/* Prefill `n` prompts (packed back to back in `ids`, prompt i has lens[i] tokens) into the decode
 * slots slots[i] (each must be free), run the model over them (causal attention, KV written to
 * freshly allocated pages) and choose each sequence's first new token.  `ids`, `lens`, `slots`,
 * `samp` are HOST pointers (samp: one entry per prompt).  sum(lens) <= max_prefill_tokens.
 * Non-blocking on the engine stream except for the small H2D copies. */
int ntts_backbone_prefill(ntts_backbone* e, int32_t n, const int32_t* ids, const int32_t* lens,
                          const int32_t* slots, const ntts_sampling* samp);

/* Prefix sharing.  The reference rebuilds, for every utterance of a speaker, a prompt that begins
 * with the same tokens -- chat header + phonemised reference text (ref:neutts/neutts.py:307,315-325) -- and runs the
 * whole prompt through the model again (ref:neutts/neutts.py:338-347 via generate()).  Here prompt i may name a donor:
 * a RUNNING slot, or a prompt given earlier in this same call (by its slot), whose prompt starts with the same
 * shared_len[i] tokens (checked; NTTS_EINVAL on a mismatch).  The KV pages holding the first
 * floor(min(shared_len, donor length, lens[i]-1) / NTTS_PAGE_TOKENS) * NTTS_PAGE_TOKENS tokens are then shared
 * (reference-counted, never written again) and only the remaining tokens of prompt i are computed.  `ids` / `lens`
 * still describe the FULL prompts; only the computed tokens count against max_prefill_tokens.  donor_slot[i] < 0 = no
 * sharing for prompt i.  Results are identical to ntts_backbone_prefill: every K/V row and every query sees the same
 * operands in the same order (tests/test_emu_prefix.py, tests/test_gpu_backbone.py). */
int ntts_backbone_prefill_shared(ntts_backbone* e, int32_t n, const int32_t* ids, const int32_t* lens,
                                 const int32_t* slots, const ntts_sampling* samp, const int32_t* donor_slot,
                                 const int32_t* shared_len);
/* KV pool occupancy and prompt-token accounting since create: free / total pages, prompt tokens pushed through the
 * layers and prompt tokens served from shared pages.  Any out pointer may be NULL.  Host state only (no sync). */
int ntts_backbone_kv_stats(ntts_backbone* e, int32_t* free_pages, int32_t* total_pages, int64_t* prompt_tokens_computed,
                           int64_t* prompt_tokens_shared);

/* Run `n_steps` decode steps over all `max_batch` rows (one hipGraph replay per step).  Rows whose
 * slot is free or finished are carried along masked: they attend to nothing and emit nothing.
 * KV pages for up to n_steps more tokens per running slot are reserved first (NTTS_ENOMEM if the
 * pool is exhausted; nothing is enqueued then). */
int ntts_backbone_decode(ntts_backbone* e, int32_t n_steps);

/* Blocking.  Copy out what slot `slot` has generated so far (prompt stripped, like
 * ref:neutts/neutts.py:348-351): up to `cap` ids into out_ids, the count into *n_out, and
 * *finished = 1 once EOS was emitted or max_length reached.  The EOS id itself is included, as in
 * generate()'s return value. */
int ntts_backbone_read(ntts_backbone* e, int32_t slot, int32_t* out_ids, int32_t cap, int32_t* n_out,
                       int32_t* finished);
/* Blocking.  ntts_backbone_read for every slot at once (three device-to-host copies in total): row s of
 * out_ids (row stride `cap` ints) gets slot s's new ids, n_out[s] / finished[s] as above; free slots report 0. */
int ntts_backbone_read_all(ntts_backbone* e, int32_t* out_ids, int32_t cap, int32_t* n_out, int32_t* finished);
/* Blocking.  One int32 per slot: 0 free, 1 running, 2 finished; new-token counts in n_new (may be NULL). */
int ntts_backbone_poll(ntts_backbone* e, int32_t* state, int32_t* n_new);
/* ABI 5.  The same poll WITHOUT stopping the stream, for a scheduler that keeps one burst of decode steps queued ahead of its own
 * bookkeeping (the stopping criteria of hf:generation/utils.py:2783-2973 are evaluated on the device every step; the host only
 * has to notice finished rows some steps later).  _begin enqueues a copy of every slot's state / new-token count into page-locked
 * memory behind the work issued so far and returns; _end waits for THAT copy only -- not for anything enqueued after _begin -- and
 * hands the values out (n_new may be NULL).  One snapshot may be open at a time (NTTS_ESTATE otherwise). */
int ntts_backbone_poll_begin(ntts_backbone* e);
int ntts_backbone_poll_end(ntts_backbone* e, int32_t* state, int32_t* n_new);
/* ABI 5.  ntts_backbone_read for a slot that the last completed snapshot (poll_begin / poll_end) showed FINISHED and that has not
 * been released since: its ids are final, so the copy runs on a side stream past the decode steps still queued on the engine's
 * stream (ntts_backbone_read would wait for all of them).  NTTS_ESTATE if the slot was not finished in that snapshot. */
int ntts_backbone_read_finished(ntts_backbone* e, int32_t slot, int32_t* out_ids, int32_t cap, int32_t* n_out);
/* The id -> code hand-off of ref:neutts/neutts.py:349 (tokenizer.decode) + :276 (regex over "<|speech_N|>") without leaving the
 * device: for each of the `n` decode slots `slots[i]` (HOST array), the new ids that are speech tokens -- speech_base <= id <
 * speech_base + n_codes -- are written in order as id - speech_base to codes_dev[i * stride ...] (DEVICE int32, at most `stride`
 * per slot) and their count to lens_dev[i] (DEVICE).  modulo != 0 (synthetic benchmark only): every id becomes
 * id mod n_codes.  Enqueued on the engine's stream (ntts_backbone_stream) behind the decode steps issued so far. */
int ntts_backbone_export_codes(ntts_backbone* e, int32_t n, const int32_t* slots, int32_t speech_base, int32_t n_codes,
                               int32_t modulo, int32_t* codes_dev, int32_t stride, int32_t* lens_dev);
/* ABI 6.  The same hand-off for STREAMS (ref:neutts/neutts.py:390-404 appends every generated "<|speech_N|>" token to the stream's token
 * cache as it arrives): for stream i (decode slot slots[i], HOST array) the ids generated since the previous call -- counted by seen_dev[i] --
 * are filtered / mapped like ntts_backbone_export_codes does and APPENDED to cache_dev[i * stride + clen_dev[i] ...]; clen_dev[i] and
 * seen_dev[i] advance, fin_dev[i] = 1 once the slot has finished (EOS / max_length), else 0.  All four are DEVICE int32 arrays owned by the
 * caller (ntts_streams_* below is the in-tree user).  Enqueued on the engine's stream behind the decode steps issued so far. */
int ntts_backbone_append_codes(ntts_backbone* e, int32_t n, const int32_t* slots, int32_t speech_base, int32_t n_codes, int32_t modulo,
                               int32_t* cache_dev, int32_t stride, int32_t* clen_dev, int32_t* seen_dev, int32_t* fin_dev);
/* The engine's HIP stream (a hipStream_t), for a consumer that must order its own work behind the engine's. */
int ntts_backbone_stream(ntts_backbone* e, void** stream);
/* ABI 6.  SURVEY.md 8b ("all work enqueued on a caller-provided hipStream_t"): the engine creates a stream of its own; a caller that wants
 * the engine's launches, copies and graph replays ordered inside ITS stream (e.g. torch's current stream) lends it here; NULL returns to the
 * engine's own stream.  Blocking (drains the stream in use); NTTS_ESTATE while a snapshot (poll_begin) is open. */
int ntts_backbone_set_stream(ntts_backbone* e, void* stream);
/* Serving-side scheduling knob (no reference counterpart: ref:neutts/neutts.py runs one utterance at a time): run this engine's
 * prompt passes (ntts_backbone_prefill*) on a side stream restricted to the compute units whose bits are set in `mask` (n_words
 * 32-bit words, bit i of word w = CU 32 w + i; hipExtStreamCreateWithCUMask), ordered behind and before the engine's own stream.
 * A prefill is compute-bound and its 1024-thread workgroups occupy whole CUs; confined to a subset it leaves the rest of the GPU
 * to another engine's decode steps, which are latency-bound (bench.py pipelines consecutive batches this way).  n_words = 0
 * restores the default (prompt pass on the engine's stream, all CUs).  Blocking (drains the engine's streams). */
int ntts_backbone_set_prefill_cu_mask(ntts_backbone* e, const uint32_t* mask, int32_t n_words);
/* (ABI 7) The same side-stream arrangement on a stream the CALLER owns (no CU mask): every later prompt pass is enqueued there,
 * ordered behind the work already on the engine's stream and before what follows on it by events -- nothing blocks per pass.
 * For several engines side by side: all matrix-core-bound passes in one hardware queue, each engine's decode chain in its own
 * (the HIP runtime multiplexes streams onto four hardware queues; a prompt pass in the queue of another engine's decode chain
 * stalls that chain).  NULL restores the default.  Replaces a CU-masked side stream and vice versa.  Blocking (drains the engine's
 * streams) at the switch itself. */
int ntts_backbone_set_prefill_stream(ntts_backbone* e, void* stream);
/* Return the slot's KV pages to the pool and mark it free. */
int ntts_backbone_release(ntts_backbone* e, int32_t slot);
/* ntts_backbone_release for `n` distinct slots with ONE stream operation (a server frees a whole batch at once); nothing is released if a
 * slot is invalid or repeated. */
int ntts_backbone_release_many(ntts_backbone* e, int32_t n, const int32_t* slots);
int ntts_backbone_sync(ntts_backbone* e);

/* Test / profiling taps (blocking).  Last-step fp32 logits are only materialised when
 * `keep_logits` was enabled; row = slot. */
int ntts_backbone_set_debug(ntts_backbone* e, int32_t keep_logits);
int ntts_backbone_read_logits(ntts_backbone* e, int32_t slot, float* out, int32_t n);
/* ABI 11.  Blocking debug read of slot `slot`'s row of the seen bitmap the repetition penalty works on: bit c (word c >> 5, bit c & 31) = lm_head
 * COLUMN c has occurred -- the token id itself, or with ntts_backbone_set_logits_range the position in [lo, hi) followed by the EOS column (ids outside
 * are not recorded).  n_words 32-bit words are written (zeros past the row's end).  Rows of requests whose penalty is 1 are cleared by the prompt pass
 * and then left alone.  NTTS_ESTATE while no bitmap exists: it is allocated with the first request whose penalty is not 1. */
int ntts_backbone_read_seen(ntts_backbone* e, int32_t slot, uint32_t* words_out, int32_t n_words);
/* Per-token log-probabilities.  NEW SYMBOLS ONLY: NTTS_ABI_VERSION stays 11 and ntts_sampling keeps its layout -- a caller that never names these
 * functions sees the library it saw before.
 * DEFINITION.  For a request's i-th new token t_i, chosen from the processed logits row r_i -- the bf16-valued row the lm_head produces, after the
 * repetition penalty and the MinNewTokens EOS mask: exactly what ntts_backbone_read_logits taps and what HF hands its warpers --
 *     logprob_i = r_i[t_i] - logsumexp(r_i)      over the whole lm_head row: all V columns, -inf columns contributing 0.
 * Temperature, top_k, top_p and min_p do NOT enter.  For a greedy request this is transformers' compute_transition_scores(sequences, scores,
 * normalize_logits=True); for a sampled one it is the model's own probability of the drawn token (the convention of serving stacks' `logprobs`), not
 * the renormalised mass among the warpers' survivors.  With ntts_backbone_set_logits_range the row is the COMPACTED row (the range's columns + EOS): the
 * tokens outside the range are not part of the sum.  The first token (chosen behind the prompt pass) and the EOS token both get a value: a request
 * always has exactly n_new log-probabilities.  A sequence's score is their arithmetic mean.
 * The log-sum-exp is reduced inside the lm_head epilogue (the [B][V] logits are never materialised) and carried to the sampling kernel beside the
 * argmax partials; fp32 throughout, within 1e-4 absolute of the float64 value on the tapped row.
 * ntts_backbone_set_logprobs: the engine-level switch (per engine: every twin of a gang has its own).  NTTS_ESTATE while any slot or parking row is in
 * use, like ntts_backbone_set_logits_range.  The first enable allocates the record ([slots][max_context] fp32) and the third partial array; switching
 * drops the captured step graphs.  While on, every request records.  While off (the default) nothing is allocated and the step launches exactly the
 * kernels it launched before. */
int ntts_backbone_set_logprobs(ntts_backbone* e, int32_t enable);
/* Blocking read of slot `slot`'s log-probabilities, ordered like ntts_backbone_read: *n_out = n_new, min(cap, n_new) values are written, entry i
 * belongs to the i-th id ntts_backbone_read returns.  NTTS_ESTATE while the switch is off. */
int ntts_backbone_read_logprobs(ntts_backbone* e, int32_t slot, float* out, int32_t cap, int32_t* n_out);
/* The same for a slot the last completed snapshot showed FINISHED, on the side copy stream, under the rule of ntts_backbone_read_finished. */
int ntts_backbone_read_finished_logprobs(ntts_backbone* e, int32_t slot, float* out, int32_t cap, int32_t* n_out);
/* Teacher-forced scoring of GIVEN sequences.  NEW SYMBOLS ONLY: NTTS_ABI_VERSION stays 11.
 * DEFINITION.  Sequence i has tokens ids_i[0 .. len_i).  For every j in [score_from_i, len_i), with 1 <= score_from_i < len_i,
 *     logprob_i[j] = r_{j-1}[ids_i[j]] - logsumexp(r_{j-1})
 * where r_{j-1} is the bf16-valued lm_head row of position j-1 as the prompt pass computes it, over all V columns.  No processor enters: no
 * repetition penalty, no MinNewTokens EOS mask, no temperature, no warper -- this is log_softmax(model(ids).logits)[j-1, ids[j]] of transformers, and
 * what ntts_backbone_read_logprobs records for a request that ran with repetition_penalty = 1 and min_new_tokens = 0, up to the arithmetic difference
 * between the prompt pass and the decode step.  Per scored position the call also returns argmax[j], the first index of the row maximum (what greedy
 * decoding would have emitted there), and argmax_logprob[j] = max - logsumexp.  fp32 throughout, within 1e-4 absolute of the float64 value on the
 * tapped row.
 * ntts_backbone_score: blocking.  ids = the n sequences back to back, lens[i] tokens each; slots[i] = a FREE slot per sequence -- they and their KV
 * pages are free again on return, on success and on error alike (ntts_backbone_kv_stats shows the same free-page count before and after).  The prompt
 * pass runs as for ntts_backbone_prefill, without pruning the last layer and without a first token; the final norm and the lm_head run over the scored
 * source positions only (score_from_i - 1 .. len_i - 2), in chunks of chunk_rows rows -- 0 = the engine's default, 2048: a chunk streams the head once,
 * which is ~10 % of its time there, and the partial arrays cost 12 bytes x (V / 96) per chunk row (56 MB at V = 217 488; V / 64 on an fp8 engine); a value above 8192 or above
 * max_prefill_tokens is taken as the smaller of the two (larger chunks only cost scratch: measured no faster); negative: NTTS_EINVAL.  The [rows][V] logits are
 * never materialised: the lm_head epilogue keeps (max, first index, sum of exp) partials and the one logit of the given next token.  The scratch is
 * sized for ONE chunk, allocated by the first call and freed at destroy.  The head tile is the engine's 256-row one (256 x 288 bf16, 256 x 256 fp8)
 * whatever the call holds: a sequence's results are bit-identical for every chunking and whichever sequences share its call.  Outputs are packed sequence after sequence, len_i - score_from_i entries each; *n_out = their total.  cap
 * smaller than that: NTTS_EINVAL with the needed count in *n_out, nothing run.
 * Works on bf16 and fp8 engines of every shape (small-batch ones included) and on the general attention path.  No running or parked request is
 * touched (nothing of the decode step's workspaces or slot state is written) and no captured step graph is disturbed.
 * Refusals (nothing is touched): NTTS_ESTATE while ntts_backbone_set_logits_range or calibration mode is on; NTTS_EINVAL, naming the sequence, for a
 * busy or repeated slot, score_from outside [1, len), len > max_context, an id outside [0, V), sum(lens) above max_prefill_tokens; NTTS_ENOMEM when
 * the KV pages do not fit.
 * Debug tap: with ntts_backbone_set_debug(e, 1) the call also keeps the fp32 rows of the scored positions (NTTS_EINVAL if rows x V x 4 exceeds
 * 64 MB); ntts_backbone_read_score_logits reads row `row` (in output order) of the most recent call, n <= V values. */
int ntts_backbone_score(ntts_backbone* e, int32_t n, const int32_t* ids, const int32_t* lens, const int32_t* slots,
                        const int32_t* score_from, int32_t chunk_rows,
                        float* out_logprobs, int32_t* out_argmax, float* out_argmax_logprobs, int64_t cap, int64_t* n_out);
int ntts_backbone_read_score_logits(ntts_backbone* e, int64_t row, float* out, int32_t n);
/* Teacher forcing for the margin-aware parity tests: replace the token slot `slot` emitted last
 * (and will feed to the next step) by `token`. */
int ntts_backbone_debug_force(ntts_backbone* e, int32_t slot, int32_t token);
/* Timing: elapsed GPU milliseconds (hipEvents on the engine stream) of the most recent
 * ntts_backbone_decode call (all its steps) and of the most recent prefill. */
int ntts_backbone_last_timing(ntts_backbone* e, float* prefill_ms, float* decode_ms);
/* Replay ONE kernel of the decode step `iters` times at the current slot state and report its average
 * duration (hipEvents on the engine stream), its algorithmic HBM bytes per launch and how many times a
 * decode step launches it.  which: 0 paged attention (+RoPE/KV append), 1 QKV GEMM, 2 o_proj GEMM,
 * 3 gate/up GEMM (+SiLU*mul), 4 down_proj GEMM, 5 lm_head GEMM (+argmax partials), 6 add+RMSNorm.
 * Replay k runs on layer (k mod num_layers): consecutive replays touch different weights / KV pools, as
 * consecutive launches inside a decode step do, so the operands come from HBM and not from the Infinity Cache. */
int ntts_backbone_time_kernel(ntts_backbone* e, int32_t which, int32_t iters, float* avg_ms, double* alg_bytes,
                              int32_t* launches_per_step);
/* Diagnostics: launch the decode attention kernel of `layer` once at the current slot state and return the phase
 * timestamps it records: out[((slot * num_kv_heads + kv_head) * 4 + wave) * 8 + phase], 100 MHz ticks; phases: 0 kernel
 * entry, 1 slot state known, 2 RoPE / KV-append prologue done, 3 first K page through the matrix core, 4 scores done,
 * 5 softmax statistics merged, 6 PV done, 7 exit.  cap = entries available in `out` (>= max_batch * kv_heads * 32). */
int ntts_backbone_attn_timeline(ntts_backbone* e, int32_t layer, uint64_t* out, int64_t cap);
/* Diagnostics (tools/gemv_timeline.py): phase timestamps (100 MHz ticks) of ONE small-batch GEMV launch at the current slot state --
 * which = 1 QKV (+ RoPE + K append; slot 5 = K slices met in LDS, slot 6 = stores done), 2 o_proj, 3 gate/up, 4 down_proj of `layer`.  out[workgroup][16]: slots 0..5 of a workgroup's first feature wave (entry,
 * weights requested, weights landed, X panel complete, matrix-core chain done, stores done), slots 8..10 of its first helper wave (entry,
 * panel written, past the barrier).  cap >= 4096 * 16; *n_wg = workgroups that reported.  On a large-batch engine the same call times the tile kernels
 * (gemm.h / qkv_rope.h): slots 0..5 of wave 0 = entry, first ring slots requested, first tile landed, k-loop done, epilogue issued (qkv: K slices
 * met in LDS), stores drained.
 * which = 1 rewrites the residual ping-pong buffer out of sequence: do not continue generating from this slot state. */
int ntts_backbone_gemv_timeline(ntts_backbone* e, int32_t which, int32_t layer, uint64_t* out, int64_t cap, int32_t* n_wg);
/* Algorithmic HBM bytes of one decode step at the current slot lengths (SURVEY.md 8d formula:
 * layer weights + lm_head + sum_b len_b * kv_bytes_per_token + new-token KV writes). */
int ntts_backbone_step_bytes(ntts_backbone* e, double* bytes);

/* ------------------------------------------------------------------------------------------ */
/* Codec engine: NeuCodec decoder, codes -> 24 kHz waveform.  Replaces NeuCodec.decode_code behind  */
/* ref:neutts/neutts.py:288-291 (FSQ de-index -> Linear -> Conv/ResNet -> 12 x transformer ->       */
/* ResNet -> LayerNorm -> ISTFT head; hf:models/xcodec2/modeling_xcodec2.py:746-862).                */
/* ------------------------------------------------------------------------------------------ */
typedef struct ntts_codec ntts_codec;

typedef struct ntts_codec_config {
    int32_t hidden_size;        /* 1024 */
    int32_t intermediate_size;  /* 4096 */
    int32_t num_layers;         /* 12 */
    int32_t num_heads;          /* 16 */
    int32_t head_dim;           /* 64 */
    int32_t quantization_dim;   /* 2048 */
    int32_t n_levels;           /* 8 */
    int32_t levels[8];          /* FSQ levels, 4 each: 65 536 codes */
    int32_t hop_length;         /* 480 (ref:neutts/neutts.py:86); n_fft = 4 * hop */
    float rms_eps;              /* 1e-6 */
    int32_t max_frames;         /* longest utterance, in codec frames */
    int32_t max_rows;           /* workspace rows: sum over a decode call of (max frames of the call + 6) */
    int32_t precision;          /* ABI 9 (the field is ABI 8's; the numbering changed so that a zeroed struct gets the setting that holds the parity bar).
                                 * 0 = fp16 GEMM operands (DEFAULT): activations and weights as IEEE halves on v_mfma_f32_16x16x32_f16, fp32 accumulate --
                                 *     waveform within ~1e-3 RELATIVE rms (measured 9.5e-4) of the fp32 reference decoder (ref:neutts/neutts.py:288-291 runs it in fp32), i.e.
                                 *     inside BASELINE's 1e-3 absolute at any amplitude a [-1, 1] waveform can have; same matrix-core rate and bytes as
                                 *     bf16.  Operands must fit fp16's range: weights are checked at finalize (NTTS_EINVAL beyond 65504), activations
                                 *     saturate at +-65504 (post-norm activations are O(1-10));
                                 * 1 = "high": every GEMM operand as a split bf16 pair (hi + lo, K-concatenated [xh | xl | xh] x [wh | wh | wl]): ~16
                                 *     significant bits per operand at 3x the matrix-core work, bf16's range;
                                 * 2 = bf16 operands (rounds 1-5's default): 7e-3 RELATIVE rms, i.e. inside 1e-3 absolute only up to signal rms ~0.14;
                                 *     for weights outside fp16's range */
} ntts_codec_config;

const char* ntts_codec_last_error(const ntts_codec* c);
int ntts_codec_create(const ntts_codec_config* cfg, int device, ntts_codec** out);
void ntts_codec_destroy(ntts_codec* c);
/* `name` = parameter name of transformers' Xcodec2Model: "quantizer.project_out.{weight,bias}",
 * "decoder.fc.*", "decoder.embed.*", "decoder.{prior_net,post_net}.{0,1}.{norm1,conv1,norm2,conv2}.*",
 * "decoder.layers.{i}.{input_layernorm,post_attention_layernorm}.weight",
 * "decoder.layers.{i}.self_attn.{q,k,v,o}_proj.weight", "decoder.layers.{i}.mlp.{fc1,fc2}.weight",
 * "decoder.norm.*", "decoder.head.linear.*".  Host or device pointer, fp32 or bf16.  Blocking. */
int ntts_codec_load_tensor(ntts_codec* c, const char* name, const void* data, int dtype, const int64_t* shape,
                           int ndim, int is_device);
int ntts_codec_finalize(ntts_codec* c);
/* Decode `n` utterances: codes packed back to back (HOST int32, utterance i has lens[i] frames) ->
 * wav_out (HOST float32) row i = hop_length * lens[i] samples at offset i * wav_stride (wav_stride >= hop_length *
 * max(lens); the tail of a shorter row up to that length is scratch).  One strided D2H copy.  Blocking. */
int ntts_codec_decode(ntts_codec* c, int32_t n, const int32_t* codes, const int32_t* lens, float* wav_out,
                      int64_t wav_stride);
/* The same pass over codes that are already ON THE DEVICE (ntts_backbone_export_codes): utterance i's codes at
 * codes_dev + i * codes_stride, lens[i] of them (`lens` is a HOST array: the launch geometry depends on it).  Asynchronous:
 * the pass is ordered behind `producer_stream` (a hipStream_t, e.g. the backbone's; may be NULL), the waveforms are copied to
 * wav_out -- a DEVICE buffer (wav_on_device != 0) or page-locked host memory -- on the codec's own stream, and the call
 * returns once everything is enqueued; ntts_codec_sync() waits for it.  SURVEY.md 8b: device pointers + caller stream. */
int ntts_codec_decode_dev(ntts_codec* c, int32_t n, const int32_t* codes_dev, int32_t codes_stride, const int32_t* lens,
                          float* wav_out, int64_t wav_stride, int32_t wav_on_device, void* producer_stream);
/* Waits for the engine's stream; on a stream lent with ntts_codec_set_stream: for the most recent asynchronous pass and its hand-over
 * only (an event behind them), not for what the caller enqueued on that stream afterwards. */
int ntts_codec_sync(ntts_codec* c);
/* ABI 6.  Test taps (blocking), like ntts_encoder_read_stage: with keep_stages != 0 every decode call keeps the fp32 residual stream after
 * the stages of hf:models/xcodec2/modeling_xcodec2.py:838-862 -- 0 embed (fc + k = 7 conv :839-841), 1 prior_net (:845), 2 the transformer
 * layers (:855-856), 3 post_net (:859); read_stage copies utterance `utt`'s rows of the most recent call: HOST float32 [rows = frames][cols = hidden]. */
int ntts_codec_set_debug(ntts_codec* c, int32_t keep_stages);
int ntts_codec_read_stage(ntts_codec* c, int32_t stage, int32_t utt, float* out, int64_t cap, int32_t* rows, int32_t* cols);
/* ABI 6.  The codec engine's HIP stream (a hipStream_t) and its workspace limits (config fields max_frames / max_rows as created), for a
 * consumer that puts its own kernels before / behind a decode pass (ntts_streams_*). */
int ntts_codec_stream(ntts_codec* c, void** stream);
/* The codec passes on a stream of the caller's (as ntts_backbone_set_stream); NULL returns to the engine's own.  Blocking. */
int ntts_codec_set_stream(ntts_codec* c, void* stream);
int ntts_codec_limits(ntts_codec* c, int32_t* max_frames, int64_t* max_rows);
/* The same knob for the codec engine: re-create its stream restricted to the CUs of `mask` (n_words = 0: unrestricted).  Blocking. */
int ntts_codec_set_cu_mask(ntts_codec* c, const uint32_t* mask, int32_t n_words);
/* Page-locked host memory for wav_out: a pinned destination lets the D2H copy run at PCIe speed (pageable memory is
 * staged by the runtime at a fraction of it).  Plain malloc/free semantics; not tied to an engine. */
int ntts_host_alloc(size_t bytes, void** out);
int ntts_host_free(void* p);
/* (ABI 7) A non-blocking HIP stream on `device` (hipStreamCreateWithFlags) to lend to ntts_backbone_set_stream /
 * ntts_backbone_set_prefill_stream / ntts_codec_set_stream, for hosts that have no HIP runtime binding of their own (the Python
 * host creates the lanes of an engine gang with it); destroy drains it first.  No reference counterpart (one utterance, one stream). */
int ntts_stream_create(int32_t device, void** stream);
int ntts_stream_destroy(int32_t device, void* stream);
/* GPU milliseconds (hipEvents) of the most recent decode call, H2D/D2H excluded (with an output format: the output stage included; after
 * ntts_codec_convert: that stage alone, its last round). */
int ntts_codec_last_timing(ntts_codec* c, float* ms);

/* Output stage of the codec, on the device behind overlap-add.  NEW SYMBOLS ONLY: NTTS_ABI_VERSION stays 11; ntts_codec_decode and
 * ntts_codec_decode_dev are unchanged.
 *
 * The reference has no such stage: NeuCodec.decode_code hands out 24 kHz float32 (ref:neutts/neutts.py:288-291) and every consumer of another
 * format puts torchaudio.functional.resample(wav, 24000, rate) and an int16 cast behind infer() on the host.  Here the waveform is already
 * resident, and the D2H copy shrinks with the format (2x for PCM16 at 24 kHz, 12x for mu-law at 8 kHz).
 *
 * Resampling: the polyphase FIR torchaudio.functional.resample builds by default (sinc_interp_hann, rolloff 0.99, lowpass_filter_width W).
 * g = gcd(24000, rate), orig = 24000 / g, new = rate / g, base = min(orig, new) * 0.99, width = ceil(W * orig / base), taps = 2 width + orig;
 * phase p in [0, new), tap j in [0, taps): t = clamp((-p / new + (j - width) / orig) * base, -W, W),
 * h[p][j] = sinc(pi t) * cos(pi t / (2 W))^2 * base / orig; output sample m = q * new + p is sum_j h[p][j] * x[q * orig + j - width] with x zero
 * outside its own utterance; n_out = ceil(n_in * new / orig); rate 24000 copies.  The table is built in double on the host and rounded once to
 * fp32, the sum runs in fp32.  W = 6 is torchaudio's default and rolls off early (a tone at 0.8 of the output Nyquist frequency comes out ~6 % low):
 * telephony callers will want 16 or more.  tests/wav_format_spec.py states all of this in numpy and is the authority.
 * PCM16: clip(rint(x * 32768), -32768, 32767), ties to even, NaN -> 0.  mu-law: G.711 of that PCM16 sample, the 14-bit form
 * (audioop.lin2ulaw(pcm16, 2)).  The three encodings are applied to ONE fp32 sample. */
enum { NTTS_WAV_F32 = 0, NTTS_WAV_PCM16 = 1, NTTS_WAV_MULAW = 2 };
typedef struct ntts_wav_format {
    int32_t sample_rate;   /* 8000, 16000, 22050, 24000, 32000, 44100 or 48000; 0 = 24000 */
    int32_t encoding;      /* NTTS_WAV_*: float32 / int16_t / uint8_t elements */
    int32_t filter_width;  /* W in [1, 64]; 0 = 6 */
} ntts_wav_format;         /* zeroed (or a NULL pointer) = 24000 / F32 / 6: the native output, nothing more is launched */
/* Samples of an utterance of n_in 24 kHz samples in `fmt`.  Pure host arithmetic; message through ntts_codec_last_error(NULL). */
int ntts_wav_out_len(const ntts_wav_format* fmt, int64_t n_in, int64_t* n_out);
/* ntts_codec_decode / ntts_codec_decode_dev with the output stage: `out` holds elements of the format's type, row i at offset i * out_stride
 * ELEMENTS (out_stride >= the longest utterance's samples in that format), out_lens[i] (HOST) = its samples.  The same pass, then one kernel;
 * with the native format the very same calls as the plain entry points, bit for bit.
 * ntts_codec_convert: the stage alone on waveforms of the caller's -- HOST float32 [n][in_stride] at 24 kHz, utterance i of n_samples[i]
 * samples (what follows them in its row is never read as signal) -- H2D, kernel, D2H on the engine's stream; blocking.  For a host library
 * that works on the 24 kHz float waveform between the codec and the output (a watermarker).
 * Refused with NTTS_EINVAL and a message, nothing run: an unknown rate or encoding, filter_width outside [0, 64], out_stride below the largest
 * out_lens; for convert also n_samples[i] < 0, n_samples[i] > in_stride, or more samples than the engine's max_frames * hop_length. */
int ntts_codec_decode_fmt(ntts_codec* c, int32_t n, const int32_t* codes, const int32_t* lens, const ntts_wav_format* fmt,
                          void* out, int64_t out_stride, int32_t* out_lens);
int ntts_codec_decode_dev_fmt(ntts_codec* c, int32_t n, const int32_t* codes_dev, int32_t codes_stride, const int32_t* lens,
                              void* out, int64_t out_stride, int32_t out_on_device, void* producer_stream,
                              const ntts_wav_format* fmt, int32_t* out_lens);
int ntts_codec_convert(ntts_codec* c, int32_t n, const float* wav, int64_t in_stride, const int32_t* n_samples,
                       const ntts_wav_format* fmt, void* out, int64_t out_stride, int32_t* out_lens);

/* Speed: a pitch-preserving time stretch on the device, between overlap-add and the output stage.  NEW SYMBOLS ONLY: NTTS_ABI_VERSION stays 11.
 *
 * The reference has no such knob (a codec-token language model has no duration input); its users resample, which moves the pitch, or run a
 * time-stretch library on the 24 kHz float waveform on the host.  Here it is WSOLA (waveform-similarity overlap-add) at the native 24 kHz, stated so
 * that the choice of every segment is a function of the row and the speed alone -- integer arithmetic, no order of additions:
 * L = 720 (30 ms), Hs = 360, D = 240 (+-10 ms).  Speed is an integer per mille pm in [500, 2000]; n_out = ceil(n_in * 1000 / pm), K = ceil(n_out / Hs)
 * output frames.  pm = 1000 copies the row bit for bit (positions k * Hs), and a call whose rows are all 1000 launches nothing of this stage.
 * The search signal is s = PCM16(x) (the rounding of the output stage); x and s read as zero outside [0, n_in) of their own utterance;
 * pmax = max(0, n_in - L).  Frame 0: p_0 = 0, out[0 .. Hs) = x[0 .. Hs).  Frame k >= 1: t_k = p_{k-1} + Hs (the natural continuation),
 * a_k = (k * Hs * pm + 500) / 1000, candidates c from clamp(a_k - D) to clamp(a_k + D) with clamp to [0, pmax],
 * D(c) = sum_{i < Hs} |s[t_k + i] - s[c + i]|, p_k = the c that minimises the tuple (D, |c - t_k|, c), and
 * out[k * Hs + i] = fmaf(f[i], x[p_k + i] - x[t_k + i], x[t_k + i]) in fp32 with f[i] = 0.5 - 0.5 cos(pi (i + 0.5) / Hs) built in double and rounded once:
 * the input bit for bit wherever p_k == t_k.  Up to the last 30 ms of an utterance may be compressed or dropped; rows shorter than L come out as the
 * rule says and mean nothing.  tests/time_stretch_spec.py states all of this in numpy and is the authority.
 *
 * ntts_wav_stretch_len: n_out of n_in samples at a speed; pure host arithmetic (message through ntts_codec_last_error(NULL)).
 * ntts_codec_stretch: the stage alone (and the output stage behind it) on HOST float32 waveforms, the twin of ntts_codec_convert -- for a host library
 * between the codec and the output (a watermarker) and for the tests.  speed_permille[n]; out_lens[i] = the samples of row i in `fmt`;
 * positions (may be NULL): row i receives p_0 .. p_{K_i - 1} at offset i * pos_stride.  Blocking.
 * ntts_codec_decode_speed / ntts_codec_decode_dev_speed: ntts_codec_decode_fmt / ntts_codec_decode_dev_fmt with speed_permille[n]; NULL means all
 * 1000, and that (like an array of 1000s) makes the very same calls as those entry points, bit for bit.
 * Refused with NTTS_EINVAL and a message, nothing run, the engine stays usable: a speed outside [500, 2000], out_stride below the largest out_lens,
 * pos_stride below the largest K, and what ntts_codec_convert / ntts_codec_decode_fmt refuse.
 * ntts_codec_last_stretch_timing: GPU milliseconds of the search and the render kernel of the most recent stretch (NTTS_ESTATE before the first). */
int ntts_wav_stretch_len(int32_t speed_permille, int64_t n_in, int64_t* n_out);
int ntts_codec_stretch(ntts_codec* c, int32_t n, const float* wav, int64_t in_stride, const int32_t* n_samples, const int32_t* speed_permille,
                       const ntts_wav_format* fmt, void* out, int64_t out_stride, int32_t* out_lens, int32_t* positions, int64_t pos_stride);
int ntts_codec_decode_speed(ntts_codec* c, int32_t n, const int32_t* codes, const int32_t* lens, const int32_t* speed_permille,
                            const ntts_wav_format* fmt, void* out, int64_t out_stride, int32_t* out_lens);
int ntts_codec_decode_dev_speed(ntts_codec* c, int32_t n, const int32_t* codes_dev, int32_t codes_stride, const int32_t* lens,
                                const int32_t* speed_permille, void* out, int64_t out_stride, int32_t out_on_device, void* producer_stream,
                                const ntts_wav_format* fmt, int32_t* out_lens);
int ntts_codec_last_stretch_timing(ntts_codec* c, float* search_ms, float* render_ms);

/* Loudness: ITU-R BS.1770-4 loudness normalisation on the device, between the time stretch and the output stage.  NEW SYMBOLS ONLY: NTTS_ABI_VERSION
 * stays 11.
 *
 * The reference has no such knob: a cloned voice comes out as loud as its reference clip was, and its users run a loudness normaliser on the 24 kHz
 * float waveform on the host.  Here the row is measured and scaled where it lies, at the native 24 kHz, behind the time stretch (if any) and ahead of
 * resampling and encoding.  K-weighting: two biquads designed for 24 kHz by the bilinear construction that gives the standard's 48 kHz table at
 * 48 kHz (coefficients built on the host in double).  Sub-blocks of S = 2400 samples (100 ms), J = n / S of them; a trailing partial one is not
 * measured.  For sub-block j both biquads start from zero state at sample max(0, (j - 1) * S); z_j = the mean square of the filter output over the
 * sub-block's own samples (against filtering the whole row this moves L by about 2e-12 LU).  Gating block i = sub-blocks i .. i + 3, i in [0, J - 3):
 * P_i = mean(z_i .. z_{i+3}), l_i = -0.691 + 10 log10 P_i; the absolute gate keeps l_i > -70, Gamma = -0.691 + 10 log10(mean P_i of those) - 10, the
 * relative gate keeps those with l_i > Gamma as well, L = -0.691 + 10 log10(mean P_i of those).  Filters, sums and gates run in fp64.
 * A row without a block (n < 9600), without a block past the absolute gate, or with a non-finite sample is UNMEASURABLE: L = NaN, gain 1.
 * peak = max |x| over the row: the SAMPLE peak, not the true (inter-sample) peak (+inf for a row with a non-finite sample).
 * g = min(10^((target_lufs - L) / 20), 10^(max_gain_db / 20), 10^(peak_dbfs / 20) / peak) (the last term only where peak > 0), in double, rounded
 * once to float32; out[i] = x[i] * g in fp32.  A row whose g is exactly 1, and every row with enable == 0, is the input bit for bit.  Resampling behind
 * the gain can overshoot the ceiling slightly.  tests/loudness_spec.py states all of this in numpy and is the authority.
 *
 * ntts_wav_loudness, one per row: enable (0 = the row is left alone, the other fields are not looked at); target_lufs in [-70, 0]; peak_dbfs in
 * [-20, 0] (-1 is the usual ceiling); max_gain_db in [0, 60] (20 keeps a near-silent utterance from being lifted into its noise).
 * measured (may be NULL): [n][3] doubles, row i = (L_i, peak_i, g_i).
 * ntts_codec_normalize: the stage alone (and the output stage behind it) on HOST float32 waveforms, the twin of ntts_codec_stretch / ntts_codec_convert
 * -- for a host library between the codec and the output, and for the tests; out_lens[i] = the samples of row i in `fmt`.  Blocking.
 * ntts_codec_measure_loudness: the measurement alone, nothing scaled (g = 1 in `measured`).  Blocking.
 * ntts_codec_decode_loud / ntts_codec_decode_dev_loud: ntts_codec_decode_speed / ntts_codec_decode_dev_speed with loudness[n]; NULL, or every enable
 * 0, makes the very same calls as those entry points, bit for bit.
 * Refused with NTTS_EINVAL and a message that names the row and the value, nothing run, the engine stays usable: a parameter of an enabled row
 * outside its range or NaN, and what ntts_codec_stretch / ntts_codec_decode_speed refuse.  Batches larger than the workspace are split as the
 * stretch splits them.
 * ntts_codec_last_loudness_timing: GPU milliseconds of the measure and the apply kernel of the most recent loudness stage (NTTS_ESTATE before the
 * first). */
typedef struct ntts_wav_loudness {
    int32_t enable;
    float target_lufs;
    float peak_dbfs;
    float max_gain_db;
} ntts_wav_loudness;
int ntts_codec_normalize(ntts_codec* c, int32_t n, const float* wav, int64_t in_stride, const int32_t* n_samples, const ntts_wav_loudness* loudness,
                         const ntts_wav_format* fmt, void* out, int64_t out_stride, int32_t* out_lens, double* measured);
int ntts_codec_measure_loudness(ntts_codec* c, int32_t n, const float* wav, int64_t in_stride, const int32_t* n_samples, double* measured);
int ntts_codec_decode_loud(ntts_codec* c, int32_t n, const int32_t* codes, const int32_t* lens, const int32_t* speed_permille,
                           const ntts_wav_loudness* loudness, const ntts_wav_format* fmt, void* out, int64_t out_stride, int32_t* out_lens);
int ntts_codec_decode_dev_loud(ntts_codec* c, int32_t n, const int32_t* codes_dev, int32_t codes_stride, const int32_t* lens,
                               const int32_t* speed_permille, const ntts_wav_loudness* loudness, void* out, int64_t out_stride,
                               int32_t out_on_device, void* producer_stream, const ntts_wav_format* fmt, int32_t* out_lens);
int ntts_codec_last_loudness_timing(ntts_codec* c, float* measure_ms, float* apply_ms);

/* The output stage on a signal that arrives in CHUNKS (a stream).  NEW SYMBOLS ONLY: NTTS_ABI_VERSION stays 11.
 *
 * After N input samples in all a stream has emitted M(N) output samples: M = N at 24 kHz; otherwise M = ((N - width) / orig) * new once
 * N >= width (0 before) -- every output sample whose `taps` inputs x[q * orig - width, q * orig + width + orig) have all arrived -- and
 * M = ceil(N * new / orig) with the stream's LAST chunk, the missing inputs zero as in the one-shot stage.  Chunk k delivers the outputs
 * [M(N_{k-1}), M(N_k)).  Sample m is the dot product of the one-shot stage: the same table, the same operands, the same order.  THE CONCATENATED
 * CHUNKS OF A STREAM ARE BIT-IDENTICAL TO ntts_codec_convert OF THE CONCATENATED SIGNAL, in all three encodings, for every chunking.
 * Between chunks a stream keeps the inputs its next outputs still need: at most taps - 1 samples (390 floats at 8 kHz with W = 64).  The output
 * lags the input by at most width + orig input samples (231: under 10 ms); only a stream's first chunk is shorter for it, and a chunk may be
 * empty.  tests/wav_stream_spec.py (stream_out_count, resample_chunks; the numbers are tests/wav_format_spec.py's) is the authority.
 *
 * ntts_wav_stream: that stage alone for `n_streams` independent streams on a codec engine -- the streaming twin of ntts_codec_convert, for a
 * host library between the codec and the output (a watermarker).  A chunk holds at most max_chunk_samples samples.
 * ntts_wav_stream_push: n entries; entry i appends n_samples[i] samples (HOST float32, row i of wav [n][in_stride]; what follows them in the
 * row is never read as signal) to stream stream[i] and receives out_lens[i] elements of the format in row i of out [n][out_stride ELEMENTS].
 * n_samples[i] = 0 is legal; with last[i] it is the pure flush.  After last[i] the stream is empty and may start a new signal.  H2D, one
 * kernel, D2H on the codec engine's stream; blocking.
 * Refused with NTTS_EINVAL and a message (ntts_wav_stream_last_error), nothing run and no stream moved: a bad format (as ntts_codec_convert),
 * a stream index out of range or named twice in one call, n_samples[i] negative, above in_stride or above max_chunk_samples, out_stride below
 * the largest out_lens.
 * ntts_wav_stream_count: M(n_in_total) of a format; pure host arithmetic (message through ntts_wav_stream_last_error(NULL)). */
typedef struct ntts_wav_stream ntts_wav_stream;
int ntts_wav_stream_create(ntts_codec* c, const ntts_wav_format* fmt, int32_t n_streams, int32_t max_chunk_samples, ntts_wav_stream** out);
void ntts_wav_stream_destroy(ntts_wav_stream* ws);
const char* ntts_wav_stream_last_error(const ntts_wav_stream* ws);
int ntts_wav_stream_push(ntts_wav_stream* ws, int32_t n, const int32_t* stream, const float* wav, int64_t in_stride, const int32_t* n_samples,
                         const int32_t* last, void* out, int64_t out_stride, int32_t* out_lens);
int ntts_wav_stream_count(const ntts_wav_format* fmt, int64_t n_in_total, int32_t last, int64_t* n_out_total);

/* The time stretch on a signal that arrives in CHUNKS (a stream).  NEW SYMBOLS ONLY: NTTS_ABI_VERSION stays 11.
 * A stream has one speed pm in [500, 2000] per signal, named with every chunk.  The chunks of a stream at a speed, concatenated, are
 * ntts_codec_stretch of its concatenated 24 kHz chunks -- positions and samples, bit for bit -- for every chunking (tests/stream_speed_spec.py is
 * the contract; names as above: frames of 360, search +-240, window 720, a_k = (k * 360 * pm + 500) / 1000).
 *   Not the last chunk: after N input samples frame k (frame 0 included) is decided and rendered as soon as a_k + 960 <= N.  Then the clamp to
 *     n_in - 720 cannot bind, the reference window and every candidate window have arrived, and the frame is a whole frame of the final output: its
 *     position and samples are the one-shot rule's, whatever arrives later.  The stream has emitted F(N) * 360 samples, F(N) = #{k: a_k + 960 <= N}.
 *   The last chunk: n_in = N is known; the remaining frames follow the one-shot rule as it stands (clamp, zeros behind N, truncation to
 *     ceil(N * 1000 / pm)).  It may be empty: a pure flush.  The stream is empty afterwards and may start a new signal at another speed.
 *   Between chunks a stream keeps, ON THE DEVICE, p_{k-1} and the inputs from max(0, min(t_k, a_k - 240, N - 720)) on for its
 *     next frame k -- at most 1 560 floats, two rows per stream (one read, one written).
 *   pm = 1000: a copy, no lag, no history, bit for bit.
 * Output lags input by up to 960 input samples (40 ms) and one frame: a stream's first audio at a speed other than 1 comes that much later, only
 * its last chunk is longer for it, and a chunk may be empty.
 * ntts_speed_stream: that stage alone for `n_streams` independent streams of HOST chunks, the output format `fmt` (NULL / zeroed = 24 kHz
 * float32) behind it with its own history -- the streaming twin of ntts_codec_stretch.
 * ntts_speed_stream_push: as ntts_wav_stream_push, entry i at speed_permille[i]; out_lens[i] ELEMENTS of the format go to row i of `out`
 * (out_stride elements apart).  pos (may be NULL): the positions decided in this call, row i (pos_stride apart), n_pos[i] of them (at 1000: k * 360
 * of the frames that begin in the chunk).  Refused with NTTS_EINVAL and a message (ntts_speed_stream_last_error), nothing run and no stream moved: a
 * speed outside [500, 2000]; a speed other than the one the stream's current signal began with; and what ntts_wav_stream_push refuses.  Blocking.
 * ntts_speed_stream_count: 24 kHz samples a stream at that speed has emitted in all after n_in_total inputs; pure host arithmetic. */
typedef struct ntts_speed_stream ntts_speed_stream;
int ntts_speed_stream_create(ntts_codec* c, const ntts_wav_format* fmt, int32_t n_streams, int32_t max_chunk_samples, ntts_speed_stream** out);
void ntts_speed_stream_destroy(ntts_speed_stream* ss);
const char* ntts_speed_stream_last_error(const ntts_speed_stream* ss);
int ntts_speed_stream_push(ntts_speed_stream* ss, int32_t n, const int32_t* stream, const int32_t* speed_permille, const float* wav, int64_t in_stride,
                           const int32_t* n_samples, const int32_t* last, void* out, int64_t out_stride, int32_t* out_lens,
                           int32_t* pos, int64_t pos_stride, int32_t* n_pos);
int ntts_speed_stream_count(int32_t speed_permille, int64_t n_in_total, int32_t last, int64_t* n_out_total);

/* ------------------------------------------------------------------------------------------ */
/* Device-side streaming (ABI 6): the per-chunk post-process of infer_stream for `n` concurrent    */
/* utterances -- token cache, window assembly, the 27-frame slice and the triangular cross-fade    */
/* with the previous chunk (ref:neutts/neutts.py:46-70, :385-388, :401-465) -- without the codes   */
/* or the decoded windows visiting the host: per burst only a few integers per stream travel up    */
/* and each stream's NEW samples come back.  Watermarking (ref :422-425, host library) is not      */
/* part of it: a caller with a watermarker keeps the host path.                                    */
/* ------------------------------------------------------------------------------------------ */
typedef struct ntts_streams ntts_streams;
typedef struct ntts_stream_params {
    int32_t chunk;          /* streaming_frames_per_chunk  25   ref:neutts/neutts.py:88 */
    int32_t lookforward;    /* streaming_lookforward        5   ref :89 */
    int32_t lookback;       /* streaming_lookback          50   ref :90 */
    int32_t overlap;        /* streaming_overlap_frames     1   ref :87 */
    int32_t hop_length;     /* 480                              ref :86 */
    int32_t speech_base;    /* token id of "<|speech_0|>" */
    int32_t n_codes;        /* 65 536 */
    int32_t modulo;         /* != 0: every id becomes id mod n_codes (synthetic benchmark only, as ntts_backbone_export_codes) */
} ntts_stream_params;
const char* ntts_streams_last_error(const ntts_streams* s);
/* Stream i runs in decode slot slots[i] of `e` (already prefilled); its token cache starts with its ref_lens[i] reference codes (packed
 * back to back in ref_codes, HOST) -- ref :385-387 -- and can take max_new_tokens generated ones.  Windows are decoded by `c`. */
int ntts_streams_create(ntts_backbone* e, ntts_codec* c, const ntts_stream_params* prm, int32_t device, int32_t n, const int32_t* slots,
                        const int32_t* ref_codes, const int32_t* ref_lens, int32_t max_new_tokens, ntts_streams** out);
void ntts_streams_destroy(ntts_streams* s);
/* After a burst of decode steps has been ENQUEUED on the backbone: append the new codes to the caches and snapshot every stream's cache
 * length / finished flag behind that burst (asynchronous; the caller may enqueue the NEXT burst right away -- it runs beside pump_end). */
int ntts_streams_pump_begin(ntts_streams* s);
/* Optional: wait for that snapshot alone and report how many streams were still generating in it -- what a caller needs to know before
 * it enqueues the next burst (which then runs beside pump_end's codec passes). */
int ntts_streams_pump_wait(ntts_streams* s, int32_t* n_running);
/* Wait for that snapshot, decode every window it completes (one regular window per stream and round; a finished stream's final window
 * once no regular one is left), cross-fade, and hand out the new samples: chunk k belongs to stream chunk_stream[k], has
 * chunk_samples[k] samples at (*chunks) + k * (*row_stride) (page-locked memory owned by the set, valid until the next pump_end) and is
 * the stream's last one if chunk_last[k].  cap >= 2 n entries in the three HOST arrays.  *n_running = streams still generating;
 * *more = 1: further windows are already complete -- call pump_end again (without pump_begin) to get them.  Blocking. */
int ntts_streams_pump_end(ntts_streams* s, int32_t cap, int32_t* n_chunks, int32_t* chunk_stream, int32_t* chunk_samples, int32_t* chunk_last,
                          const float** chunks, int64_t* row_stride, int32_t* n_running, int32_t* more);
/* Streams that have emitted their last chunk.  (After a failed pump the set's bookkeeping is ahead of what was emitted: destroy it.) */
int ntts_streams_done(ntts_streams* s, int32_t* n_done);
/* Chunks in another output format (ntts_wav_format; NEW SYMBOLS ONLY).  ntts_streams_set_format: legal until the first pump_begin
 * (NTTS_ESTATE after); a bad format is NTTS_EINVAL.  A non-native format puts the chunked output stage (above: one history row per stream)
 * behind the cross-fade on the codec's stream; the page-locked buffer and the D2H copy are sized in the format's element type.
 * ntts_streams_pump_end_fmt is pump_end for such a set: chunk k holds chunk_samples[k] ELEMENTS of the format (possibly none: the output lags
 * the input by up to width + orig samples) at (char*)(*chunks) + k * (*row_stride) * element size.  The chunks of a stream, concatenated, are
 * ntts_codec_convert of its concatenated 24 kHz chunks, bit for bit.  With the native format (zeroed, NULL, or never set) it runs the launches
 * and copies of ntts_streams_pump_end and returns the same bits.  Plain ntts_streams_pump_end on a set with a non-native format is
 * NTTS_ESTATE: its float** would lie. */
int ntts_streams_set_format(ntts_streams* s, const ntts_wav_format* fmt);
int ntts_streams_pump_end_fmt(ntts_streams* s, int32_t cap, int32_t* n_chunks, int32_t* chunk_stream, int32_t* chunk_samples, int32_t* chunk_last,
                              const void** chunks, int64_t* row_stride, int32_t* n_running, int32_t* more);
/* Chunks at a speed (the chunked time stretch above; NEW SYMBOLS ONLY).  ntts_streams_set_speed: speed_permille[i] of stream i, each in
 * [500, 2000] (NTTS_EINVAL otherwise); NULL = all 1000.  Legal until the first pump_begin (NTTS_ESTATE after), in either order with set_format.
 * With a speed other than 1000 in the set the stage runs behind the cross-fade, ahead of the output format's stage if there is one; buffers and
 * the D2H copy are sized for the stretched rows.  A stream's chunks then lag by up to 40 ms and a frame, may be empty, and a stream that ends
 * on a window's edge gets a flush chunk of its own.  Both pump_end variants serve a set with speeds in the native format.  A set all at 1000
 * makes the launches and copies it made before and returns the same bits. */
int ntts_streams_set_speed(ntts_streams* s, const int32_t* speed_permille);

/* ------------------------------------------------------------------------------------------ */
/* NeuCodec ENCODER engine: reference enrolment.  Replaces                                       */
/*     codec.encode_code(audio_or_path=wav16k[1,1,L]) -> int codes [1,1,T]                       */
/* (ref:neutts/neutts.py:266-271; neucodec is un-vendored, the architecture is restated from      */
/* hf:models/xcodec2/modeling_xcodec2.py:974-1049 = zero-pad to a hop multiple -> [kaldi fbank -> */
/* w2v-BERT 2.0 conformer layers 1..16 -> semantic adapter] || [acoustic conv encoder] -> concat  */
/* -> Linear -> FSQ).  One-off per speaker, off the synthesis hot path; fp32 throughout.          */
/* ------------------------------------------------------------------------------------------ */
typedef struct ntts_encoder ntts_encoder;

typedef struct ntts_encoder_config {
    int32_t sem_hidden;         /* 1024  w2v-BERT hidden size */
    int32_t sem_layers;         /* 16    conformer layers run (neucodec reads hidden_states[16]) */
    int32_t sem_heads;          /* 16 */
    int32_t sem_ffn;            /* 4096 */
    int32_t sem_conv_kernel;    /* 31    causal depthwise kernel */
    int32_t sem_left;           /* 64    relative_key distance clamp */
    int32_t sem_right;          /* 8 */
    float sem_ln_eps;           /* 1e-5 */
    int32_t ac_hidden;          /* 48    acoustic encoder base width */
    int32_t n_ratios;           /* 5 */
    int32_t ratios[8];          /* 2,2,4,4,5: 16 kHz -> 50 Hz (hop 320) */
    int32_t codec_hidden;       /* 1024  acoustic encoder output channels */
    int32_t n_levels;           /* 8 */
    int32_t levels[8];          /* FSQ levels, 4 each */
    int32_t max_samples;        /* longest clip (16 kHz samples) one encode call accepts */
} ntts_encoder_config;

const char* ntts_encoder_last_error(const ntts_encoder* e);
int ntts_encoder_create(const ntts_encoder_config* cfg, int device, ntts_encoder** out);
void ntts_encoder_destroy(ntts_encoder* e);
/* `name` = parameter name of transformers' Xcodec2Model: "semantic_encoder.feature_projection.*",
 * "semantic_encoder.encoder.layers.{i}.*", "semantic_adapter.conv{1..4}.*", "acoustic_encoder.*", "fc_encoder.*",
 * "quantizer.project_in.*".  Host or device pointer, fp32 or bf16 (widened to fp32).  Blocking. */
int ntts_encoder_load_tensor(ntts_encoder* e, const char* name, const void* data, int dtype, const int64_t* shape,
                             int ndim, int is_device);
/* Lists every missing tensor in the error text; repacks Conv1d weights for the implicit GEMM. */
int ntts_encoder_finalize(ntts_encoder* e);
/* wav: HOST float32 mono at 16 kHz, n_samples of them -> codes_out (HOST int32, capacity `cap`), *n_codes =
 * n_samples / hop + 1 (the reference appends one zero, then pads to a hop multiple).  Blocking. */
int ntts_encoder_encode(ntts_encoder* e, const float* wav, int64_t n_samples, int32_t* codes_out, int32_t cap, int32_t* n_codes);
/* Stage outputs of the most recent encode call, for the per-stage parity tests: 0 = fbank features [T,160], 1 = semantic
 * adapter || acoustic encoder [T, sem_hidden + codec_hidden], 2 = fc_encoder output [T, same], 3 = twice-bounded FSQ
 * latents [T, n_levels].  HOST float32 out of capacity `cap` floats. */
int ntts_encoder_read_stage(ntts_encoder* e, int32_t stage, float* out, int64_t cap, int32_t* rows, int32_t* cols);
/* GPU milliseconds (hipEvents) of the most recent encode call, H2D/D2H excluded. */
int ntts_encoder_last_timing(ntts_encoder* e, float* ms);

/* ------------------------------------------------------------------------------------------ */
/* Kernel-level entry points (used by the parity tests and micro-benchmarks; all pointers are   */
/* DEVICE pointers, bf16 unless noted, row-major; run on the NULL stream and block).           */
/* ------------------------------------------------------------------------------------------ */
/* C[M,N] = A[M,K] (lda) * W[N,K]^T (+ bias[N]); fp32 accumulate on MFMA, one RNE rounding to bf16.
 * variant: 0 = auto, 1 = 128x128 tile, 2 = 64x64 tile, 3 = 64x64 split-K slabs + reduce, 4 = 256x256 tile,
 * 5 / 6 = 256x256 / 128x128 on ring slots of K = 32, 7 = 256x288 natural-order tile, 8 = 320x192 tile (12 waves), 9 = 320x128 tile (8 waves). */
int ntts_k_gemm_bf16(const void* A, int64_t lda, const void* W, const void* bias, void* C, int64_t ldc,
                     int32_t M, int32_t N, int32_t K, int32_t variant);
/* fp8 probes (tests): out[i] = e4m3(clamp(in[i] * inv_scale, +-448)), round-to-nearest-even -- the conversion every fp8
 * producer on the path uses; and C[M,N] = bf16(fma(A[M,K] . W[N,K]^T, xscale * wscale[n], bias[n])) with e4m3 BYTE operands
 * (row-major, K % 128 == 0) on v_mfma_f32_16x16x32_fp8_fp8.  variant: 2 = 64x64 tile, 4 = 256x256, else 128x128. */
int ntts_k_fp8_quantize(const float* in_dev, void* out_dev, int64_t n, float inv_scale);
int ntts_k_gemm_fp8(const void* A, const void* W, const float* wscale, float xscale, const void* bias, void* C,
                    int32_t M, int32_t N, int32_t K, int32_t variant);
/* y = rmsnorm(x) * w with Qwen2RMSNorm's rounding (hf:models/qwen2/modeling_qwen2.py:247-252). */
int ntts_k_rmsnorm_bf16(const void* x, const void* w, void* y, int32_t rows, int32_t cols, float eps);
/* Micro-benchmark of one GEMM tile configuration on synthetic operands (tools/ubench_gemm.py); see csrc/kapi.cpp. */
int ntts_k_gemm_probe(int32_t M, int32_t N, int32_t K, int32_t config, int32_t abl, int32_t copies, int32_t iters,
                      double* us);
/* Achieved HBM copy bandwidth probe: copies `bytes` device->device `iters` times, returns GB/s. */
int ntts_k_membw(size_t bytes, int32_t iters, double* gbps);
/* Diagnostics: writes 3 x 64 x 4 floats describing the MFMA 16x16x32 lane layout (see csrc/kapi.cpp). */
int ntts_k_mfma_probe(float* out_dev_768);
/* Launch-chain floor (diagnostics): captures `n_kernels` dependent launches of a kernel that only reads 4 bytes per workgroup
 * (`grid` workgroups of 256 threads; block = 256) into one hipGraph, replays it `iters` times and returns the microseconds per
 * replay -- what a decode step of that many launches costs before any kernel moves a byte.  block = -256: every thread of every
 * launch also loads 16 HBM-cold bytes and stores 16 (the least a kernel of the step does: one dependent round trip + a store). */
int ntts_k_launch_chain_probe(int32_t n_kernels, int32_t grid, int32_t block, int32_t iters, double* us_per_chain);
/* SiLU as the GEMM epilogues compute it (hf:activations.py SiLUActivation), elementwise on DEVICE bf16 values: out[i] =
 * bf16(silu(in[i])).  variant 0 = x / (1 + expf(-x)), 1 = the epilogues' fast form (gemm.h silu_fast); the parity tests run
 * every bf16 bit pattern through both and compare with torch. */
int ntts_k_silu_probe(const void* in_bf16_dev, void* out_bf16_dev, int64_t n, int32_t variant);

/* ABI 10.  The engine's own token choice (the device function the decode step's sampling kernel calls: top-k radix select, nucleus / min-p cut,
 * Philox draw) on caller-supplied rows: logits_dev = DEVICE bf16 [rows][ld_logits] processed logits (ld_logits % 8 == 0, 16-byte aligned; -inf where
 * a token is masked), `vocab` columns of each row count.  group_width > 0 (a multiple of 8): the grouped path -- the probe first computes the
 * maximum of every group of that many consecutive columns, as the lm_head epilogue leaves them, and the sampler scans only the groups that can
 * hold one of the k largest (it falls back to the full row by itself when there are fewer groups than k or more than 1024 candidates groups);
 * group_width = 0: the full-row path.  Per row r (HOST arrays of `rows` entries): top_k[r] >= 1, temperature[r] > 0, top_p[r], min_p[r], seed[r] as
 * in ntts_sampling (same validation: NTTS_EINVAL); `step` is the Philox counter (the index of the new token).  Out (HOST): token_out[r] the drawn
 * token, n_out[r] the number of final survivors (<= 512), ids_out[r * 512 ...] their ids in token-id order. */
int ntts_k_sample_probe(const void* logits_dev, int64_t ld_logits, int32_t rows, int32_t vocab, int32_t group_width, const int32_t* top_k,
                        const float* temperature, const float* top_p, const float* min_p, const uint64_t* seed, int32_t step,
                        int32_t* token_out, int32_t* n_out, int32_t* ids_out);

/* The whole-vocabulary token choice (ntts_sampling.top_k = NTTS_TOP_K_OFF; the device function the decode step's sampling kernel calls for such a
 * slot) on caller-supplied rows.  logits_dev, ld_logits, rows, vocab, temperature / top_p / min_p / seed (HOST, per row), step and the validation are
 * ntts_k_sample_probe's (which keeps refusing top_k < 1: its id list holds 512).  group_width means what it means there -- > 0: the row's maximum is
 * taken from the maxima of groups of that many columns, as in the decode step; 0: from one more pass over the row -- and the results do not depend
 * on it.  Out (HOST): token_out[r] the drawn token, n_out[r] the number of survivors, keep_bits_out[r * ((vocab + 31) / 32) ...] their bitmap (bit
 * c & 31 of word c >> 5), total_out[r] their total integer mass S. */
int ntts_k_sample_full_probe(const void* logits_dev, int64_t ld_logits, int32_t rows, int32_t vocab, int32_t group_width, const float* temperature,
                             const float* top_p, const float* min_p, const uint64_t* seed, int32_t step, int32_t* token_out, int32_t* n_out,
                             uint32_t* keep_bits_out, uint64_t* total_out);

/* ABI 11.  The engine's lm_head launch (the GEMM tile + argmax / penalty epilogue the decode step runs) on caller-supplied data.  X_dev: DEVICE bf16
 * [M][K]; W_dev: DEVICE bf16 [N][K] row-major -- the probe packs it the way the engine packs the head (tile-major; fp8 != 0: quantised per output
 * channel to e4m3, X to e4m3 at the static scale xscale, K % 128 == 0).  variant: 0 = 64 x 64 tile, 1 = 128 x 128, 2 = 256 x 256, 4 = 256 x 288 natural-order
 * tile (bf16 only), 8 = the small-batch GEMV form (M <= 16, N % 16 == 0).  HOST inputs: seen = [M][(N + 31) / 32] words of seen-column bits, or NULL
 * for the plain lm_head (rep_pen is then not read); rep_pen = [M] penalties (finite, > 0; 1 = row untouched); mask_eos = [M] column + 1 whose logit is
 * -inf for that row, 0 = none (may be NULL).  HOST outputs: logits_out fp32 [M][N] (the debug dump), logits_bf16_out [M][N] bit patterns (the row the
 * sampler reads), part_val / part_idx [M][*n_part] the (max, first index) partials, partial i covering columns [i * *part_width, (i + 1) * *part_width);
 * part_cap = entries per row available in the two arrays (NTTS_EINVAL if too few). */
int ntts_k_head_penalty_probe(const void* X_dev, const void* W_dev, int32_t M, int32_t N, int32_t K, int32_t variant, int32_t fp8, float xscale,
                              const uint32_t* seen, const float* rep_pen, const int32_t* mask_eos, float* logits_out, uint16_t* logits_bf16_out,
                              float* part_val, int32_t* part_idx, int32_t part_cap, int32_t* n_part, int32_t* part_width);
/* ntts_k_head_penalty_probe with the log-sum-exp epilogue (the kernels the decode step launches while ntts_backbone_set_logprobs is on): same inputs,
 * same outputs, plus part_sum [M][*n_part] = the sum over partial i's columns n < N of exp(v - part_val[i]) (0 where part_val is -inf), and
 * row_lse [M][2] = (M, log S) per row as the sampling kernel's own merge of the partials computes them: M = the row maximum, S = sum of
 * exp(v - M) over the row, so that logsumexp(row) = M + log S. */
int ntts_k_head_logprob_probe(const void* X_dev, const void* W_dev, int32_t M, int32_t N, int32_t K, int32_t variant, int32_t fp8, float xscale,
                              const uint32_t* seen, const float* rep_pen, const int32_t* mask_eos, float* logits_out, uint16_t* logits_bf16_out,
                              float* part_val, int32_t* part_idx, float* part_sum, int32_t part_cap, int32_t* n_part, int32_t* part_width,
                              float* row_lse);

/* The scoring launch (ntts_backbone_score: the lm_head tile with the EPI_ARGMAX_LSE_TGT epilogue, then score.h's merge) on caller-supplied data: X_dev,
 * W_dev, variant (0, 1, 2, 4: the tiles; no GEMV form), fp8 and xscale as for ntts_k_head_penalty_probe; target = HOST [M] columns in [0, N) (checked).
 * HOST outputs: logits_out, part_val, part_idx, part_sum as for ntts_k_head_logprob_probe, target_val [M] = the processed logit of the target column,
 * and the merged logprob / argmax / argmax_logprob [M].  target_val and the three merged arrays are filled with NaN (argmax: -1) before the launch,
 * so that a missed capture shows. */
int ntts_k_head_score_probe(const void* X_dev, const void* W_dev, int32_t M, int32_t N, int32_t K, int32_t variant, int32_t fp8, float xscale,
                            const int32_t* target, float* logits_out, float* part_val, int32_t* part_idx, float* part_sum, int32_t part_cap,
                            int32_t* n_part, int32_t* part_width, float* target_val, float* logprob, int32_t* argmax, float* argmax_logprob);

/* Paged-attention probes (parity tests against tests/attention_spec.py; no ABI bump).  The KV page layout they read and write, per layer:
 *   K   [page][kv_head][32 tokens][head_dim]          token t of a page in row t
 *   V^T [page][kv_head][head_dim][32 token slots]     token t of a page in slot ((t & 15) >> 2) * 8 + (t >> 4) * 4 + (t & 3)
 * block_table_dev = DEVICE int32 [rows][max_pages] page numbers; EVERY entry must name a page of the pool (0 <= entry < num_pages: checked),
 * because the kernels may request any entry of a row ahead of knowing the context length.
 *
 * ntts_k_attn_decode_form: the decode-attention instantiation ("form") the engine's launchers pick for a decode batch -- 0 = 8 waves, 4 workgroups
 * per (sequence, kv-head); 1 = 8 waves, 2 workgroups; 2 = 8 waves; 3 / 4 = 4 waves with non-temporal page loads, 1024 / 2048 score rows; 5 / 6 = 4
 * waves, 1024 / 2048 score rows; 7 / 8 = head_dim 128, 1024 / 2048 score rows (form 9 = the context-split path, which the engine switches on by
 * itself and this function never returns).  Pure host arithmetic. */
int ntts_k_attn_decode_form(int32_t batch, int32_t nkv, int32_t max_ctx, int32_t nt_pages, int32_t head_dim);
/* One decode-attention launch of `form` through the engine's own launcher.  qkv_dev = DEVICE bf16 [batch][ld_qkv] rows q heads (ALREADY rotated) | k
 * heads (ignored: the K entry of this step is already in its page) | v heads (raw; the kernel places them in the V^T page of position pos[b]).
 * out_dev = [batch][nh * head_dim] bf16, or e4m3 bytes = bf16 result * out_fp8_inv when out_fp8_inv > 0.  pos_dev / state_dev = DEVICE int32 [batch]
 * (tokens already cached, 0 <= pos < max_ctx: checked; 1 = running, other rows are left untouched).  max_ctx <= 1024 for forms 3, 5, 7, <= 2048 else,
 * and max_pages * 32 >= max_ctx.  form 9: nsplit = chunks per (sequence, kv-head), 2 .. 64 (head_dim 64, bf16 out); the probe allocates the score /
 * statistics / slab scratch itself, fills it with 0xFF bytes (NaN) and runs scores, PV and combine; slabs_out_dev (may be NULL) receives the fp32
 * chunk slabs [nsplit][batch][nh * 64].  Other forms: nsplit = 0, slabs_out_dev = NULL.  xcd_rows = 0, or xps in {1, 2, 4, 8} with batch = 512 / xps
 * (workgroup x takes row xcd_row(x, xps)). */
int ntts_k_attn_decode_probe(const void* qkv_dev, int64_t ld_qkv, void* out_dev, float out_fp8_inv, void* kpool_dev, void* vpool_dev,
                             int32_t num_pages, const int32_t* block_table_dev, int32_t max_pages, const int32_t* pos_dev,
                             const int32_t* state_dev, int32_t batch, int32_t nh, int32_t nkv, int32_t head_dim, int32_t max_ctx,
                             int32_t form, int32_t nsplit, int32_t xcd_rows, float* slabs_out_dev);
/* What one layer of ntts_backbone_prefill does between the QKV GEMM and o_proj: the RoPE / KV-page writer, then causal attention over the pages by the
 * two-sweep, resident and deep kernels over the engine's own work lists.  qkv_dev = DEVICE bf16 [T][ld_qkv] packed RAW q | k | v rows of n prompts
 * (prompt i: rows of positions pos0[i] .. lens[i] - 1; HOST arrays lens = total context after the pass, pos0 = tokens already in the pages, a
 * multiple of 32, slots = block-table row, 0 <= slot < bt_rows).  rope_cos_dev / rope_sin_dev = DEVICE bf16 [max_ctx][head_dim / 2].  head_dim 128, or
 * q_norm_dev / k_norm_dev (DEVICE bf16 [head_dim], may be NULL) given: the generic writer (per-head RMSNorm with eps, RoPE; q rows rotated IN PLACE)
 * and the two-sweep kernel alone; else the head_dim-64 writer (k, v only) and attention kernels that rotate q as they load it.  res_cap / deep_cap:
 * queries below res_cap take the resident kernel, below deep_cap the deep one, clamped as ntts_backbone_create clamps NTTS_PF_RES_CAP / NTTS_PF_DEEP_CAP
 * (whole pages, at most 512 / 1024, deep >= res).  only_last != 0: the last layer's work lists (only the block that holds each prompt's last position
 * is computed; other rows of out_dev are left untouched).  out_dev as in the decode probe, [T][nh * head_dim]. */
int ntts_k_attn_prefill_probe(void* qkv_dev, int64_t ld_qkv, void* out_dev, float out_fp8_inv, void* kpool_dev, void* vpool_dev,
                              int32_t num_pages, const int32_t* block_table_dev, int32_t bt_rows, int32_t max_pages, int32_t n,
                              const int32_t* lens, const int32_t* pos0, const int32_t* slots, int32_t nh, int32_t nkv, int32_t head_dim,
                              const void* rope_cos_dev, const void* rope_sin_dev, int32_t max_ctx, const void* q_norm_dev,
                              const void* k_norm_dev, float eps, int32_t res_cap, int32_t deep_cap, int32_t only_last);

#ifdef __cplusplus
}
#endif
#endif /* NEUTTS_HIP_H */
