/*
 * ance_amd -- C ABI of the MI355X-native ANN hard-negative refresh path.
 *
 * The reference (microsoft/ANCE) has no FFI: its hot path calls two Python packages.  These
 * entry points are what a binding for that path replaces, one for one:
 *
 *   ance_encode_*      <- model.module.query_emb / body_emb
 *                         (drivers/run_ann_data_gen.py:171-180; model/models.py:149-157,165-199,
 *                          235-259) i.e. transformers' RobertaModel / BertModel forward + head
 *   ance_ip_topk       <- faiss.IndexFlatIP(dim).add(x); .search(q, k)
 *                         (drivers/run_ann_data_gen.py:269-276,303; run_ann_data_gen_dpr.py:238-252)
 *   ance_topk_merge    <- the shard-search-then-merge of utils/eval_mrr.py:173-183
 *                         (all_gather of (D, I), concat, argsort) under the canonical order
 *
 * Conventions: plain pointers and sizes, no exceptions, no torch types.  Every pointer named
 * d_* is DEVICE memory owned by the caller; nothing is allocated or freed behind the caller's
 * back except the small host-side handle of ance_encoder_create and the pinned staging buffers of ance_lamb_step (kept for the
 * process's lifetime).  All work is enqueued on the
 * caller's hipStream_t (passed as void* so this header needs no HIP include) and is asynchronous;
 * the functions never synchronise the device.  Return value: 0 on success, negative ANCE_E_* on
 * error (nothing enqueued in that case).
 *
 * Canonical result order of every top-k list: score descending, then row id ascending.
 * Scores are exact fp32: an fmaf chain over k = 0..d-1 ascending starting from +0.0f.
 */
#ifndef ANCE_AMD_H
#define ANCE_AMD_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define ANCE_OK 0
#define ANCE_E_INVALID (-1)   /* bad argument (null pointer, k/d/L out of the supported range) */
#define ANCE_E_WORKSPACE (-2) /* workspace too small */
#define ANCE_E_LAUNCH (-3)    /* HIP reported a launch error */
#define ANCE_E_NOMEM (-4)

#define ANCE_ABI_VERSION 7  /* still 7: ance_nll_backward, ance_inbatch_nll_*, ance_lamb_step_clipped, ance_lamb_step_amp, ance_adamw_step, ance_gather_batch, ance_attention_*, ance_layer_tail_*, ance_bias_gelu_*, ance_embed_*, ance_layer_tail16_*, ance_bias_gelu16_*, ance_*_dstream, ance_dropout_stream_advance, ance_*_plan_*, ance_*_step_planned, ance_linear_warmup_step, ance_attention_row0_*, ance_pack_tokens, ance_embed_rows_*, ance_first_rows_*, ance_record_lengths, ance_gather_batch_packed, ance_pack_tokens_by_id, ance_*_step_scaled, ance_loss_scale_update only ADD symbols, which
                               callers built against the earlier 7 never look up; nothing that existed changed;
                               7: + ance_debug_attention (AnceAttnDebugArgs); + ance_lamb_step (additive);
                               6: + ance_debug_gemm_hw (AnceGemmDebugArgs);
                               5: AnceEncoderDesc.precision (the arithmetic is an argument, not an environment variable), ance_encoder_range_faults,
                               ance_ip_topk_scan; 4: blocked pair rows in the split mode (ance_pair_layout; ance_debug_gemm_split + d_wscale_inv);
                               3: + ance_nll_forward, ance_search_bad_image_calls, ance_debug_gemm_split; split encoder mode */
int ance_abi_version(void);
/* last HIP error string seen by this library on the calling thread ("" if none) */
const char *ance_last_error(void);

/*
 * Measurement hook (bench.py's roofline): when enabled, every kernel launch of this library is
 * bracketed by HIP events on the launch stream.  ance_profile_read synchronises those events and
 * returns, per category, the summed kernel time (ms), the summed algorithmic work (FLOP) and the
 * launch count, then keeps accumulating.  Categories, in order:
 *   0 plan/pack  1 embed+LN  2 gemm Q|K  3 gemm V^T  4 attention  5 gemm attn-out  6 LayerNorm
 *   7 gemm FFN1+GELU  8 gemm FFN2  9 head  10 ip_topk scan  11 top-k finalize/merge
 *   12 exact re-scoring of the two-precision search
 * Returns the number of categories.  Not thread safe; off by default (no events are created).
 */
#define ANCE_PROFILE_CATEGORIES 13
void ance_profile_enable(int on);
int ance_profile_read(double *ms, double *work, long long *count, int n);

/* ------------------------------------------------------------------ exact IP top-k search -- */

#define ANCE_TOPK_MAX_K 1792

/* Bytes of scratch ance_ip_topk needs for (n rows, nq queries, dimension d, k).  0 if unsupported. */
size_t ance_ip_topk_workspace_bytes(int64_t n, int64_t nq, int d, int k);

/*
 * Exact inner-product top-k of nq queries against one shard of n rows.
 *   d_x   float32 [n, d] row-major, 16-byte aligned, d % 4 == 0
 *   d_q   float32 [nq, d]
 *   row_base  global id of the shard's first row (ids returned are row_base + local row)
 *   d_out_d   float32 [nq, k] scores, canonical order; -FLT_MAX where fewer than k rows exist
 *   d_out_i   int64   [nq, k] global row ids; -1 where fewer than k rows exist
 * Requires n < 2^32, 1 <= k <= ANCE_TOPK_MAX_K.
 *
 * Two kernels produce the same bits: an fp32-MFMA scan (any shape), and -- when d % 128 == 0,
 * 128 <= d <= 2048, k <= 1024 and n >= 4096 -- a two-precision path: fp16 MFMA scores filter the
 * corpus under a rigorous error slack, every survivor is re-scored with the exact fp32 fmaf chain.
 * A query whose candidates cannot be bounded that way (row or query norms above 65504 or NaN, i.e.
 * possible fp16 overflow; thousands of rows inside one error band) is detected on the device and
 * redone by the scan, alone; heavy classes of bit-identical rows (all-pad MaxP chunks) are scored
 * once and expanded in id order.  Environment (tuning / A-B only; read ONCE, the first time the library needs a
 * knob -- ance_reload_env() re-reads all of them):
 *   ANCE_SEARCH=exact            force the scan
 *   ANCE_FAST_SPLITS=<2^j>       corpus splits per query tile (default 2)
 *   ANCE_FAST_WINDOW_TILES=<n>   corpus window all workgroups finish together, in 256-row tiles
 *                                (default 256 = 100 MB of fp16 rows at d = 768; 0 = no windows)
 *   ANCE_FAST_WINDOW_WAIT_US     bound of the wait at a window boundary (default 200, 0 = none)
 *   ANCE_FAST_SHARE=0            do not exchange thresholds between the splits of a query
 *   ANCE_FAST_DEDUP=0            do not collapse duplicate classes when an image is built
 *   ANCE_FAST_CENTER=0           do not centre the fp16 image on the shard's mean row (the filter's error
 *                                slack then scales with |x| instead of |x - mean|)
 */
int ance_ip_topk(const float *d_x, int64_t n, int64_t row_base, const float *d_q, int64_t nq, int d, int k,
                 float *d_out_d, int64_t *d_out_i, void *d_workspace, size_t workspace_bytes, void *stream);

/*
 * The same search by the fp32-MFMA scan ALONE (csrc/ip_topk.hip: ip_topk_scan_kernel), whatever the shape and the environment:
 * the independent audit path of the two-precision kernel -- both must return the same bits (bench.py checks the headline-size
 * search against it on a sample of its queries; tests/test_gpu_search.py pins the scan to oracle/ip_topk_ref.c).  ~7 x slower.
 */
size_t ance_ip_topk_scan_workspace_bytes(int64_t n, int64_t nq, int d, int k);
int ance_ip_topk_scan(const float *d_x, int64_t n, int64_t row_base, const float *d_q, int64_t nq, int d, int k,
                      float *d_out_d, int64_t *d_out_i, void *d_workspace, size_t workspace_bytes, void *stream);

/*
 * Search image of a shard: what faiss.IndexFlatIP.add builds once and every .search reuses
 * (drivers/run_ann_data_gen.py:269-276 adds once, :276 and :303 search twice).  ance_ip_topk rebuilds
 * it inside its workspace on every call; a caller that searches the same rows repeatedly builds it once:
 *   bytes = ance_ip_index_bytes(n, d)        0: the shape has no image (the scan is used), pass NULL
 *   ance_ip_index_build(d_x, n, d, d_index, bytes, stream)
 *   ance_ip_topk_indexed(d_x, n, row_base, d_index, ...)   with ance_ip_topk_indexed_workspace_bytes
 * The image is stamped with the (n, d, d_x) it was built from when the build completes; a search whose arguments do not
 * match the stamp -- another shard's image, a buffer never built -- ignores the image on the device (no host
 * synchronisation) and answers every query with the exact scan: slower, never wrong rows.
 * The image is valid for exactly the (d_x, n, d) it was built from; d_x must stay alive and unchanged
 * (the exact re-scoring reads the fp32 rows).  Contents: the shard's mean row, fp16(row - mean) for every
 * row kept (n d 2 bytes), row map, duplicate classes.  Results are those of ance_ip_topk, bit for bit.
 */
size_t ance_ip_index_bytes(int64_t n, int d);
int ance_ip_index_build(const float *d_x, int64_t n, int d, void *d_index, size_t index_bytes, void *stream);
size_t ance_ip_topk_indexed_workspace_bytes(int64_t n, int64_t nq, int d, int k);
int ance_ip_topk_indexed(const float *d_x, int64_t n, int64_t row_base, const void *d_index, const float *d_q,
                         int64_t nq, int d, int k, float *d_out_d, int64_t *d_out_i, void *d_workspace,
                         size_t workspace_bytes, void *stream);

/* Bytes of scratch ance_topk_merge needs. */
size_t ance_topk_merge_workspace_bytes(int n_parts, int64_t nq, int k);

/*
 * Merge n_parts canonical lists (e.g. one per corpus shard / GPU) into one.
 *   d_parts_d float32 [n_parts, nq, k], d_parts_i int64 [n_parts, nq, k] (ids < 2^32, -1 = empty)
 */
int ance_topk_merge(const float *d_parts_d, const int64_t *d_parts_i, int n_parts, int64_t nq, int k,
                    float *d_out_d, int64_t *d_out_i, void *d_workspace, size_t workspace_bytes, void *stream);

/*
 * Restricted-candidate scoring (the rerank of evaluation/"Calculate Metrics.ipynb" cell 11 and
 * utils/eval_mrr.py:94-105, where a per-query faiss sub-index is built from the BM25 candidates):
 * d_scores[j] = <d_q[qi], d_x[d_rows[j]]> for d_offsets[qi] <= j < d_offsets[qi+1], with the same
 * fp32 fmaf chain (k ascending from +0) as ance_ip_topk, so scores are bitwise those of the full scan.
 * d_rows: int64 row ids in [0, n) (an id outside the range scores -inf); d_offsets: int64 [nq + 1]
 * ascending, d_offsets[0] = 0.  Enqueues on `stream` and returns.
 */
int ance_ip_score_rows(const float *d_x, int64_t n, const float *d_q, int64_t nq, int d, const int64_t *d_rows,
                       const int64_t *d_offsets, float *d_scores, void *stream);

/* ------------------------------------------------------------------------ dual encoder ------ */

#define ANCE_ARCH_ROBERTA 0 /* positions = cumsum(id != pad) * (id != pad) + pad, type 0     */
#define ANCE_ARCH_BERT 1    /* positions = 0..len-1, token type 0                              */
#define ANCE_ARCH_SEED 2    /* SEED-Encoder (model/models.py:201-221): RoBERTa's tower, but every key whose id is the pad id is
                               masked, inside the record's length too -- those tokens are dropped before the tower (exact: positions
                               skip them); token-type row 0 must be zero (there is no segment embedding); n_chunks must be 1.  A
                               record that is empty (ANCE_E_INVALID) or starts with the pad id (range-guard counter [1]) has no
                               defined output */

typedef struct AnceEncoderDesc {
    int32_t arch;         /* ANCE_ARCH_*                                                     */
    int32_t n_layers;     /* 12 (base) / 24 (large)                                          */
    int32_t hidden;       /* 768, or 1024 (RoBERTa-large: ANCE_ARCH_ROBERTA with has_head = 1 only); hidden = 64 n_heads */
    int32_t n_heads;      /* 12 at hidden 768, 16 at hidden 1024 (head dimension 64)         */
    int32_t intermediate; /* 3072 / 4096; a multiple of 128 (of 256 at hidden 1024)          */
    int32_t vocab_size;
    int32_t max_position; /* rows of the position table (514 RoBERTa / 512 BERT)             */
    int32_t pad_token_id; /* 1 RoBERTa / 0 BERT                                              */
    float ln_eps;         /* 1e-5 RoBERTa / 1e-12 BERT (encoder LayerNorms)                  */
    int32_t has_head;     /* 1: LayerNorm_768(W h_cls + b), eps 1e-5 (models.py:145-153); 0: raw h_cls */
    int32_t max_seq_len;  /* longest single sequence (chunk) this handle will see, <= 512    */
    int32_t max_tokens;   /* token capacity of one micro-batch (workspace sizing)            */
    int32_t precision;    /* ANCE_PRECISION_*: the arithmetic of the handle (and of the two size queries)  */
} AnceEncoderDesc;

#define ANCE_PRECISION_DEFAULT 0 /* what the environment says (ANCE_ENCODER_* below); nothing set: split */
#define ANCE_PRECISION_SPLIT 1   /* fp16 pair operands, three MFMAs per k-step: fp32-grade (2e-5), the default */
#define ANCE_PRECISION_FP16 2    /* fp16 operands: the fast mode (5e-3) */
#define ANCE_PRECISION_FP32 3    /* fp32 operands on the fp32-input matrix cores: the audit path */

typedef struct AnceEncoder AnceEncoder;

/*
 * Order of the fp32 device weight pointers handed to ance_encoder_create (HF state-dict names,
 * prefix = "roberta." / "question_model." / "ctx_model."):
 *   [0] embeddings.word_embeddings.weight        [vocab, H]
 *   [1] embeddings.position_embeddings.weight    [max_position, H]
 *   [2] embeddings.token_type_embeddings.weight  [>=1, H]   (row 0 used)
 *   [3] embeddings.LayerNorm.weight  [4] embeddings.LayerNorm.bias
 *   then per layer i (16 pointers, base 5 + 16 i):
 *     +0 attention.self.query.weight  +1 .bias     +2 attention.self.key.weight   +3 .bias
 *     +4 attention.self.value.weight  +5 .bias     +6 attention.output.dense.weight +7 .bias
 *     +8 attention.output.LayerNorm.weight +9 .bias
 *     +10 intermediate.dense.weight   +11 .bias    +12 output.dense.weight +13 .bias
 *     +14 output.LayerNorm.weight     +15 .bias
 *   then, if has_head: embeddingHead.weight, embeddingHead.bias, norm.weight, norm.bias
 */
#define ANCE_ENCODER_N_WEIGHTS(n_layers, has_head) (5 + 16 * (n_layers) + ((has_head) ? 4 : 0))

/* Bytes of the packed weight arena (fp16 GEMM operands + fp32 vectors) and of the activation
 * workspace for desc->max_tokens.  Both are caller-allocated device buffers, 256-byte aligned.
 *
 * Shapes.  Both return 0 (and ance_encoder_create ANCE_E_INVALID) unless hidden == 64 n_heads and hidden is 768 or 1024; hidden 1024
 * also needs arch == ANCE_ARCH_ROBERTA and has_head == 1 (DPR's BiEncoder is BERT-base, SEED's config is base width, and a head-less
 * large tower would change the output width).  The output rows are [n * n_chunks, 768] at either width.  Large tower (24 layers,
 * 1024 / 16 / 4096, vocab 50265, 514 positions), max_tokens 131,072: arena 2.03 GB split / 0.82 GB fp16 / 2.03 GB fp32, workspace
 * 15.8 GB / 7.2 GB / 17.9 GB.
 *
 * Arithmetic.  DEFAULT (nothing in the environment): the SPLIT mode -- an fp32-GRADE result from the fp16 matrix cores: every GEMM
 * operand an fp16 pair v = hi + lo, three MFMAs per k-step (hi hi + lo hi + hi lo) from four operand tiles staged once, fp32
 * accumulation, fp32 softmax, erf-GELU to fp32 grade, fp32 head; max |delta| 2e-5 (stated; 7e-6 measured at 12 layers) against the
 * reference's fp32 arithmetic (model/models.py:149-157 runs in fp32).  Preconditions of the split mode, both CHECKED on the device
 * (ance_encoder_range_faults): pre-LayerNorm values, Q | K | V and GELU outputs must stay below 65,504 (the hi half of a pair is an fp16)
 * -- the reference's fp32 has no such limit, --encoder_precision fp32 / ANCE_PRECISION_FP32 is the way out; and no NaN in the output
 * rows.  Activation magnitudes: the lo half of an element below 2^-3 is an fp16 subnormal, i.e. good to 2^-25 ABSOLUTE -- fp32-grade for
 * the O(1) values of the post-residual streams; the embedding sum (0.05 in trained BERT / RoBERTa checkpoints, followed by a LayerNorm
 * with rstd ~ 20) is therefore stored times 16 and its LayerNorm epsilon times 256 (exact: powers of two).  Weights may have any scale
 * (stored times a per-matrix power of two).
 * The arithmetic of a handle is AnceEncoderDesc.precision.  ANCE_PRECISION_DEFAULT (0) defers to the environment, read when the handle
 * is created (the two size queries resolve the mode the same way) -- a drivers' --encoder_precision flag overrides it:
 *   ANCE_ENCODER_FP16=1      the fp16 FAST mode (ANCE_ENCODER_SPLIT=0 is another spelling): fp16 MFMA operands, fp32 accumulation, fp32
 *                            softmax / statistics / head; LayerNorm folded into the GEMMs and the residual stream kept as fp16 (hi, lo)
 *                            pairs (22 mantissa bits) -- max |delta| 3e-3 on unit-variance embeddings (stated tolerance of the tests:
 *                            5e-3), 2.2 x the default's throughput.  A folded GEMM takes fp16(v) of the PRE-LayerNorm row v as its token
 *                            operand, so its rounding error scales with |v|, not |v - mean|: a GEMM tile with a token whose |mean| rstd
 *                            exceeds 2 runs a second K loop over the lo halves OF THOSE TOKENS (masked per row: a row's bits never
 *                            depend on its tile mates); below that threshold the error is at most sqrt(1 + 2^2) x the random-init figure
 *   ANCE_ENCODER_SPLIT=1     names the default explicitly; wins over ANCE_ENCODER_FP16
 *   ANCE_ENCODER_PRECISE=1   fp32 mode: fp32 operands on the fp32-input matrix cores, exact erf GELU, fp32 softmax -- the
 *                            reference's arithmetic (model/models.py:149-157); max |delta| 1e-5, 4.4 x slower than the default (the audit
 *                            path); wins over the other two switches
 *   ANCE_ENCODER_STREAMS=n   internal streams / activation sets (1 or 2, default 2)
 *   ANCE_CLS_TAIL=0          the full last layer instead of the CLS-only tail (bit-identical: the tail's reference; per handle)
 *   ANCE_GEMM_STREAM=0       the launch-per-tile split GEMM for QKV and FFN1 instead of the persistent streaming one
 *                            (bit-identical: the streaming kernel's reference; read once per process, ance_reload_env re-reads)
 *   ANCE_ATTN_TWO_PASS=0     the online softmax for every sequence in the split attention instead of the two-pass form for
 *                            sequences of <= 128 tokens (same bits up to 32 tokens, rounding only above; A/B; read once per process,
 *                            ance_reload_env re-reads) */
size_t ance_encoder_weight_bytes(const AnceEncoderDesc *desc);
size_t ance_encoder_workspace_bytes(const AnceEncoderDesc *desc);

/* Packs the fp32 weights into d_weight_arena (enqueued on stream; the fp32 sources may be freed
 * once the stream has passed this point) and returns a handle bound to the two buffers. */
int ance_encoder_create(const AnceEncoderDesc *desc, const void *const *d_weights_fp32, int n_weights,
                        void *d_weight_arena, size_t weight_bytes, void *d_workspace, size_t workspace_bytes,
                        void *stream, AnceEncoder **out);
void ance_encoder_destroy(AnceEncoder *enc);
/* The arithmetic the handle runs: ANCE_PRECISION_SPLIT / FP16 / FP32 (never DEFAULT). */
int ance_encoder_precision(const AnceEncoder *enc);

/*
 * Range guard.  The handle keeps two sticky device counters, updated by the kernels of every ance_encode_* call:
 *   [0] threads of the split mode's pair-forming stages (embedding sum, Q | K | V, GELU output, residual stream) that saw a
 *       value above 65,504 in magnitude or a non-finite one -- the split mode's precondition is violated, the embeddings of
 *       that call are NOT fp32-grade (the fp16 hi half overflowed);
 *   [1] output rows (any mode) whose statistics are NaN or infinite; under ANCE_ARCH_SEED also the records that start with the
 *       pad id (the reference's output for them is a pad row or NaN).
 * Enqueues on `stream` a copy of both to h_out (HOST pointer, uint32[2]; pinned memory keeps the copy asynchronous) and, if
 * reset != 0, zeroes them behind it.  Never synchronises: h_out is valid once `stream` has passed this point.
 */
int ance_encoder_range_faults(AnceEncoder *enc, uint32_t *h_out, int reset, void *stream);

/*
 * Encode n records.  Each record is L int32 token ids split into n_chunks chunks of L / n_chunks
 * tokens (n_chunks = 1: FirstP / queries; 4 with L = 2048: MaxP).  Pad tokens cost nothing: a
 * chunk contributes only its first len_c = clamp(len - c * L/n_chunks, 0, L/n_chunks) tokens
 * (an all-pad chunk is encoded as the single pad token it is equivalent to).
 *   d_out float32 [n * n_chunks, 768], row = record * n_chunks + chunk.
 *
 * ance_encode_records: d_records = raw rows of the reference's tokenised cache
 *   (utils/util.py:279-283): 4-byte BIG-endian length then L little-endian int32, record_bytes =
 *   4 + 4 L, so the cache file can be copied to HBM verbatim.
 * ance_encode_ids: d_ids int32 [n, L] (row stride ld_ids int32 elements), d_lens int32 [n].
 *
 * h_lens (HOST pointer, int32 [n], may be NULL): the same lengths the device will read, used by
 *   the host-side micro-batch planner.  With h_lens the call never synchronises; with NULL the
 *   library reads the lengths back once per 262,144 records (a stream synchronisation).
 *   Precondition: h_lens[i] equals the record's header / d_lens[i].
 */
int ance_encode_records(AnceEncoder *enc, const void *d_records, const int32_t *h_lens, int64_t n, int L,
                        int n_chunks, float *d_out, void *stream);
int ance_encode_ids(AnceEncoder *enc, const int32_t *d_ids, int64_t ld_ids, const int32_t *d_lens,
                    const int32_t *h_lens, int64_t n, int L, int n_chunks, float *d_out, void *stream);

/*
 * Test hook: C = A . B^T (+ epilogue) with the encoder's fp16 GEMM kernel (ping-pong main loop) on caller data.
 *   epi 0: out f16 = acc + bias[n]; 1: out f16 = gelu(acc + bias[n]); 2: out f32 = acc + bias[n] + res32
 *   d_a_f16 [M,K], d_b_f16 [N,K] fp16 row-major; M, N multiples of 256, K a multiple of 64, >= 128.
 *   ablate must be 0 (kept for the ABI; any other value returns ANCE_E_INVALID, in every build of the library).
 */
int ance_debug_gemm(int ablate, int epi, const void *d_a_f16, const void *d_b_f16, int M, int N, int K,
                    const float *d_bias, void *d_out, const float *d_res32, void *stream);

/* Diagnostic: the number of ance_ip_topk_indexed launch chunks on the current device whose search image did not carry the stamp
 * of the matrix searched (moved / copied rows, a view at another address, a buffer that was never built).  Such calls are
 * answered by the exact scan -- same results, several times slower -- and nothing else reports it.  Synchronises the device. */
int ance_search_bad_image_calls(unsigned long long *out);

/* Forward of the training objective on embeddings the encoder produced -- the consumer side of the refresh's file contract
 * (forward only): replaces the tail of NLL.forward (model/models.py:71-81) and NLL_MultiChunk.forward
 * (:97-134) after the three query_emb / body_emb calls.
 *   d_q [n, d], d_a / d_b [n * chunks, d] fp32 (row = triplet * chunks + chunk); chunks = 1 for FirstP;
 *   d_mask_a / d_mask_b [n, chunks] fp32 = the attention mask's first entry of every chunk (MaxP: an all-pad chunk is biased by
 *   -9999 before the max over chunks, :109-113); may be NULL when chunks == 1;
 *   d_logits [n, 2] = (logit_a, logit_b); d_loss_rows [n] = -log_softmax(logits)[:, 0]; d_loss_mean [1] = their mean (fixed
 *   summation order: the same input gives the same bits).  d a multiple of 4. */
int ance_nll_forward(const float *d_q, const float *d_a, const float *d_b, const float *d_mask_a, const float *d_mask_b, int64_t n,
                     int d, int chunks, float *d_logits, float *d_loss_rows, float *d_loss_mean, void *stream);

/* Gradient of ance_nll_forward's mean loss with respect to q, a, b (csrc/nll.hip), same arguments and layouts.  With
 * p = sigmoid(logit_b - logit_a) and s = *d_grad_output / n:  d logit_a = -p s, d logit_b = +p s;
 *   d_gq [n, d] = d logit_a a[ca] + d logit_b b[cb];  d_ga [n * chunks, d]: row ca = d logit_a q;  d_gb: row cb = d logit_b q,
 * ca, cb = the chunk that won the max (the lowest index among equal biased scores, the forward's comparison; the logits are
 * recomputed, bit for bit the forward's).  Every other chunk row of d_ga, d_gb is written as zeros: no pre-zeroing.
 * d_grad_output: DEVICE fp32 scalar (the upstream gradient of the mean loss), so the call never waits for the host.
 * One launch; the same inputs give the same bits.  Refuses (ANCE_E_INVALID, before the launch) what ance_nll_forward refuses. */
int ance_nll_backward(const float *d_q, const float *d_a, const float *d_b, const float *d_mask_a, const float *d_mask_b, int64_t n,
                      int d, int chunks, const float *d_grad_output, float *d_gq, float *d_ga, float *d_gb, void *stream);

/* The DPR trainer's in-batch-negatives objective (csrc/inbatch_nll.hip; drivers/run_ann_dpr.py:356-365 and its evaluate_dev):
 *   scores = q ctx^T [nq, nc] (fp32 FMA over 16-deep k tiles, the tiles summed in fp64, fixed order);  *d_loss_mean = mean_i -log_softmax(scores[i])[positive_idx[i]];
 *   d_counts[0] = #{i : argmax_j scores[i][j] == positive_idx[i]} (the lowest j among equal scores);
 *   d_counts[1] = #{i : positive_idx[i] outside [0, nc)}: such an index is never used as an address, the row's loss and the mean
 *   are NaN, the row never counts as correct, and the backward makes that row's part of the gradients NaN.
 * d_q [nq, d], d_ctx [nc, d] fp32; d_positive_idx int64 [nq] on the device; d_counts int64 [2].
 * The scores, the rows' log-sum-exp (as its two terms, the row's max and log sum exp(s - max): exp((s - max) - log sum) keeps its
 * precision at scores in the hundreds, where exp(s - lse) would be ulp(|s|) off, relatively) and gS live in d_workspace (16-byte aligned, ance_inbatch_nll_workspace_bytes; 0: shape not
 * supported); the backward reads what the forward of the SAME arguments left there and may be repeated.
 * Backward: gS = (softmax(scores) - onehot) *d_grad_output / nq (d_grad_output a DEVICE fp32 scalar); d_gq [nq, d] = gS ctx;
 * d_gctx [nc, d] = gS^T q.  Three launches each way, no atomics: the same inputs give the same bits.
 * Supported: 1 <= nq <= 1024, nq <= nc <= 2048, 128 <= d <= 1024, d % 4 == 0.  Refuses (ANCE_E_INVALID, before any launch) anything
 * else, a null pointer and a null, unaligned or too small workspace. */
size_t ance_inbatch_nll_workspace_bytes(int64_t nq, int64_t nc, int d);
int ance_inbatch_nll_forward(const float *d_q, const float *d_ctx, const int64_t *d_positive_idx, int64_t nq, int64_t nc, int d,
                             float *d_loss_mean, int64_t *d_counts, void *d_workspace, size_t workspace_bytes, void *stream);
int ance_inbatch_nll_backward(const float *d_q, const float *d_ctx, const int64_t *d_positive_idx, int64_t nq, int64_t nc, int d,
                              const float *d_grad_output, float *d_gq, float *d_gctx, void *d_workspace, size_t workspace_bytes,
                              void *stream);

/* The trainers' self-attention core with its gradient (csrc/attention_train.hip): what transformers' eager BertSelfAttention.forward
 * computes between its three Linear outputs and context_layer, for right-padded sequences and heads of width 64.  Per sequence s
 * (len_s valid rows) and head h:
 *   S = Q_h K_h^T * 0.125 over keys j < len_s;  P = softmax_j(S) in fp32 with a full-precision exp;
 *   P' = keep o P / (1 - p) when training != 0 and dropout_p > 0, else P;  ctx_h = P' V_h
 *   backward, given dctx:  dV = P'^T dctx;  dP = keep o (dctx V^T) / (1 - p);  dS = P o (dP - rowsum(dP o P));
 *   dQ = 0.125 dS K;  dK = 0.125 dS^T Q.
 * Pad keys (j >= len_s) are skipped: in fp32 that is the reference's additive -10000 mask, whose terms underflow to exactly 0 in the
 * exp.  Pad query rows are not computed, and whatever dctx holds there is ignored.  seq_rows > 0 (the padded form): sequence s owns
 * rows d_seq_first[s] .. + seq_rows - 1 (clamped to n_rows), and the rows behind its length are WRITTEN AS ZEROS in ctx, dq, dk and
 * dv by the call -- no pre-zeroing; seq_rows = 0 (the packed form): nothing outside the valid rows is written.  A sequence of
 * length <= 0 is skipped (in the padded form all its rows are zeroed; the reference's all-pad chunk attends uniformly instead; its
 * embedding never reaches the loss: INTEGRATION.md 3i).
 * Layout: q, k, v, ctx (and dctx, dq, dk, dv) are fp32 row matrices of at least n_rows rows, each with its own 16-byte aligned base
 * and its own row stride in elements (a multiple of 4, at least 64 n_heads); head h is columns 64 h .. 64 h + 63.  So three separate
 * [B, L, H] tensors, views of a fused [B, L, 3H] and the packed [T, 3H] form all pass as they are.  Sequence s is rows
 * d_seq_first[s] .. d_seq_first[s] + d_seq_len[s] - 1 (two DEVICE int32 arrays of n_seq entries).  The grid is sized from n_seq and
 * max_seq_len; the kernels clamp a length to max_seq_len and to n_rows - first and skip a first row outside [0, n_rows): no row
 * >= n_rows is touched whatever the descriptors say, nothing is read back, nothing synchronises -- both calls can be captured.
 * Dropout: Philox4x32-10 with key (seed lo32, seed hi32) and counter (i * 128 + (j >> 2), s * n_heads + h, offset lo32, offset
 * hi32) for query i and key j inside sequence s; output word j & 3 decides key j: keep iff word >= floor(dropout_p * 2^32); kept
 * values are scaled by 1.0f / (1.0f - dropout_p).  The backward regenerates the mask from the same (seed, offset).
 * The device dropout stream (every *_dstream entry point of this header: the attention cores, the layer tails, the embeddings):
 * d_stream points to a 16-byte aligned DEVICE object {uint64 seed, uint64 base}.  Given one, every kernel of the call draws under
 * seed = d_stream[0] and offset = d_stream[1] + args->offset (a 64-bit add with carry into the high word); args->seed is ignored and
 * args->offset is the call's index within the training step.  Key, counter layout, keep threshold and scaling are untouched: a call
 * with d_stream = {s, b} and args->offset = r produces exactly the bits of the plain call with (seed, offset) = (s, b + r).  The
 * pair is one uniform 16-byte read at kernel entry, so the values a captured graph bakes in are only the pointer and r: replays
 * draw under whatever the object holds when they run.  ance_dropout_stream_advance adds n to the base (one thread, an ordinary
 * 64-bit load, add and store); enqueue it once per step BEHIND the step's backward -- the backward regenerates the forward's masks
 * from the same object, so the base must not move between them.  A null d_stream is the plain call; one that is not 16-byte
 * aligned is refused (ANCE_E_INVALID, before any launch).
 * d_workspace (16-byte aligned, ance_attention_workspace_bytes) is the saved state, linear in the rows: the forward leaves the
 * log-sum-exp there as fp32 [n_heads][n_rows] (entry h * n_rows + row; only valid rows are written), the backward reads it, recomputes P
 * from q, k and it, and adds its own [n_heads][n_rows] of dctx . ctx behind it.  Nothing of size L^2 is ever stored.  The backward
 * takes the SAME AnceAttnTrainArgs as the forward, with ctx as the forward left it.  One launch forward, three backward, no
 * atomics, one owning workgroup per output tile: the same inputs give the same bits.
 * Supported: n_heads 12 or 16, 1 <= max_seq_len <= 512, 1 <= n_seq <= 65535, n_rows >= 1.  Refuses (ANCE_E_INVALID, before any
 * launch) anything else, a null pointer, an unaligned base, a stride that is not a multiple of 4 or below 64 n_heads, seq_rows
 * outside 0 .. max_seq_len, dropout_p outside [0, 1), and a null, unaligned or too small workspace. */
typedef struct AnceAttnTrainArgs {
    const float *q, *k, *v;
    float *ctx;
    int32_t ld_q, ld_k, ld_v, ld_ctx;
    const int32_t *d_seq_first, *d_seq_len;
    int32_t n_seq, max_seq_len, n_rows, n_heads;
    int32_t seq_rows; /* 0: packed form; 1 .. max_seq_len: rows per sequence of the padded form, pad rows zeroed */
    int32_t reserved; /* 0 */
    float dropout_p;
    int32_t training;
    uint64_t seed, offset;
    void *d_workspace;
    size_t workspace_bytes;
} AnceAttnTrainArgs;
typedef struct AnceAttnGradArgs {
    const float *dctx;
    float *dq, *dk, *dv;
    int32_t ld_dctx, ld_dq, ld_dk, ld_dv;
} AnceAttnGradArgs;
size_t ance_attention_workspace_bytes(int64_t n_rows, int n_heads); /* 0: n_heads not 12 or 16, or n_rows outside 1 .. 2^31 - 1 */
int ance_attention_forward(const AnceAttnTrainArgs *args, void *stream);
int ance_attention_backward(const AnceAttnTrainArgs *args, const AnceAttnGradArgs *grads, void *stream);
int ance_attention_forward_dstream(const AnceAttnTrainArgs *args, const uint64_t *d_stream, void *stream);
int ance_attention_backward_dstream(const AnceAttnTrainArgs *args, const AnceAttnGradArgs *grads, const uint64_t *d_stream, void *stream);
int ance_dropout_stream_advance(uint64_t *d_stream, uint64_t n, void *stream); /* base += n; n = 0 launches nothing */

/* The same core with 16-bit I/O (csrc/attention_train_half.hip): the recipe's --fp16, i.e. torch.autocast plus a GradScaler.  q, k,
 * v, ctx (and dctx, dq, dk, dv) are fp16 (dtype ANCE_DTYPE_F16) or bf16 (ANCE_DTYPE_BF16) row matrices, all of the one type; strides
 * are in elements, multiples of 8, at least 64 n_heads; bases 16-byte aligned.  Everything else -- the two forms, the pad-row zeros,
 * the device lengths and their clamps, the dropout stream (the same (seed, offset, s, h, i, j) keeps the same element as in the fp32
 * core), the workspace (fp32 log-sum-exp [n_heads][n_rows], then [n_heads][n_rows] of dctx . ctx; ance_attention16_workspace_bytes
 * equals the fp32 query), no atomics, one owner per output tile, capturable -- is as stated above.  The arithmetic, T = the I/O type,
 * "rounded" = to nearest even with overflow to +-inf (never a truncating or saturating conversion: under a GradScaler an overflowing
 * dS must reach found_inf as a non-finite gradient):
 *   S = Q K^T with T operands, fp32 accumulation (v_mfma_f32_32x32x16_f16 / _bf16); the 0.125 scale, max, exp and sum are fp32;
 *   the exp is the hardware exp2 of (x * log2 e), one expression for the forward and the backward;
 *   forward: online softmax over ascending 32-key blocks; P' (the unnormalised exp after keep) is rounded to T before P' V; ctx
 *   accumulates in fp32 over all key blocks and is rounded once at the store, after the fp32 factor (1.0f / (1.0f - p)) / sum;
 *   backward: P = exp(S * 0.125f - lse) recomputed from the same score expression; D = dctx . ctx in fp32 from the stored ctx;
 *   dP = dctx V^T accumulates in fp32; dS = P o (dP - D) in fp32, rounded to T for dQ = 0.125 dS K and dK = 0.125 dS^T Q;
 *   P' = keep o P * (1.0f / (1.0f - p)) rounded to T for dV; dq, dk, dv accumulate in fp32 registers in a fixed block order and are
 *   rounded once at the store (dq, dk after the fp32 factor 0.125f).
 * One launch forward, three backward.  Refuses what the fp32 calls refuse, a dtype that is neither, and a stride that is not a
 * multiple of 8. */
#define ANCE_DTYPE_F16 1
#define ANCE_DTYPE_BF16 2
typedef struct AnceAttn16Args {
    const void *q, *k, *v;
    void *ctx;
    int32_t ld_q, ld_k, ld_v, ld_ctx;
    const int32_t *d_seq_first, *d_seq_len;
    int32_t n_seq, max_seq_len, n_rows, n_heads;
    int32_t seq_rows; /* 0: packed form; 1 .. max_seq_len: rows per sequence of the padded form, pad rows zeroed */
    int32_t dtype;    /* ANCE_DTYPE_F16 or ANCE_DTYPE_BF16 */
    float dropout_p;
    int32_t training;
    uint64_t seed, offset;
    void *d_workspace;
    size_t workspace_bytes;
} AnceAttn16Args;
typedef struct AnceAttn16GradArgs {
    const void *dctx;
    void *dq, *dk, *dv;
    int32_t ld_dctx, ld_dq, ld_dk, ld_dv;
} AnceAttn16GradArgs;
size_t ance_attention16_workspace_bytes(int64_t n_rows, int n_heads); /* 0: n_heads not 12 or 16, or n_rows outside 1 .. 2^31 - 1 */
int ance_attention16_forward(const AnceAttn16Args *args, void *stream);
int ance_attention16_backward(const AnceAttn16Args *args, const AnceAttn16GradArgs *grads, void *stream);
int ance_attention16_forward_dstream(const AnceAttn16Args *args, const uint64_t *d_stream, void *stream); /* the device dropout stream: above */
int ance_attention16_backward_dstream(const AnceAttn16Args *args, const AnceAttn16GradArgs *grads, const uint64_t *d_stream, void *stream);

/* The same core for the FIRST query row of every sequence (csrc/attention_row0.hip): what the last layer of a tower needs when only
 * h[:, 0] is read.  The calls take AnceAttn16Args / AnceAttn16GradArgs with these meanings: dtype is ANCE_DTYPE_F32, _F16 or _BF16,
 * the type of every row in memory; q, ctx, dctx and dq are [n_seq, 64 n_heads] matrices, row s belonging to sequence s (q its first
 * row's query, ctx its first row's context); k, v, dk, dv are the [n_rows, 64 n_heads] matrices of the full core, sequence s being
 * rows d_seq_first[s] .. + d_seq_len[s] - 1 with the full core's clamps.  Strides are in elements, multiples of a 16-byte piece (4
 * fp32, 8 16-bit elements), at least 64 n_heads; bases 16-byte aligned.  Per sequence s and head h, q0 = q[s]:
 *   t_j = 0.125f * (q0 . K_j) for j < len;  m = max_j t_j;  l = sum_j expf(t_j - m);  P_j = expf(t_j - m) / l;
 *   P'_j = keep_j ? P_j * (1.0f / (1.0f - p)) : 0 under dropout, else P_j;  ctx[s] = sum_j P'_j V_j;
 *   backward: dP_j = keep_j ? (dctx[s] . V_j) * (1.0f / (1.0f - p)) : 0;  D = sum_j dP_j P_j;  dS_j = P_j (dP_j - D);
 *   dq[s] = 0.125f sum_j dS_j K_j;  dK_j = 0.125f dS_j q0;  dV_j = P'_j dctx[s].
 * All arithmetic is fp32 whatever the dtype; every output element is rounded once at its store (to nearest even, overflow to +-inf);
 * P is never rounded.  seq_rows > 0: rows len .. seq_rows - 1 of the sequence in dk and dv are WRITTEN AS ZEROS by the backward (every
 * valid row of dk and dv is written too: no pre-zeroing); seq_rows = 0: only the valid rows are written.  A sequence of length <= 0
 * gets a zero ctx[s] and a zero dq[s].  A sequence whose first row lies outside [0, n_rows) is treated as one of length 0 that owns
 * no rows: ctx[s] and dq[s] are written as zeros and nothing of dk or dv is touched, in both forms (a negative length with a first
 * row inside is an empty sequence: seq_rows > 0 zeroes the rows it owns, clamped to n_rows).  Dropout is the full core's query row
 * i = 0 of sequence s, bit for bit: counter (j >> 2, s * n_heads + h, offset lo32, offset hi32), word j & 3; the _dstream forms as
 * above.  d_workspace (ance_attention_row0_workspace_bytes) is the saved state: fp32 (m, l) per (sequence, head), entry 2 (s n_heads + h).  One launch
 * forward, one backward, one workgroup per (sequence, head), no atomics, every sum in a fixed order: the same inputs give the same
 * bits.  The grid is sized from n_seq and n_heads; nothing is read back -- both calls can be captured.  Refuses what the 16-bit core
 * refuses (with the stride rule above), before any launch. */
#define ANCE_DTYPE_F32 0
size_t ance_attention_row0_workspace_bytes(int64_t n_seq, int n_heads); /* 0: n_heads not 12 or 16, or n_seq outside 1 .. 65535 */
int ance_attention_row0_forward(const AnceAttn16Args *args, void *stream);
int ance_attention_row0_backward(const AnceAttn16Args *args, const AnceAttn16GradArgs *grads, void *stream);
int ance_attention_row0_forward_dstream(const AnceAttn16Args *args, const uint64_t *d_stream, void *stream);
int ance_attention_row0_backward_dstream(const AnceAttn16Args *args, const AnceAttn16GradArgs *grads, const uint64_t *d_stream, void *stream);

/* The row-wise seams of a BertLayer with their gradients (csrc/layer_tail.hip), fp32 throughout: what transformers' eager
 * BertSelfOutput.forward / BertOutput.forward compute after their dense matmul (the layer tail), and BertIntermediate.forward after
 * its own (bias + GELU).
 * Layer tail, per row r of n_rows, H = 768 or 1024:
 *   u = x[r] + bias (bias NULL: zeros);  d = keep o u * (1.0f / (1.0f - dropout_p)) when training != 0 and dropout_p > 0, else u;
 *   z = d + res[r];  mean = sum z / H;  var = sum (z - mean)^2 / H (two passes over the row in registers, biased);
 *   rstd = 1.0f / sqrtf(var + eps);  xhat = (z - mean) rstd;  y[r] = xhat o gamma + beta
 *   backward, given dy:  g = dy o gamma;  dz = rstd (g - mean_H(g) - xhat mean_H(g o xhat));  dres = dz;
 *   dx = keep o dz / (1 - dropout_p);  dgamma = sum_r dy o xhat;  dbeta = sum_r dy;  dbias = sum_r dx.
 *   xhat is recomputed from x, bias, res, the regenerated mask and the saved (mean, rstd) -- never from y: gamma may hold zeros.
 * Bias + GELU, per row, N = 3072 or 4096:
 *   u = x[r] + bias;  y[r] = 0.5 u (1 + erff(u / sqrt 2));  dx = dy (0.5 (1 + erff(u / sqrt 2)) + u expf(-u^2 / 2) / sqrt(2 pi));
 *   dbias = sum_r dx.  u is recomputed from x; nothing else is saved.
 * Layout: x, res, y (and dy, dx, dres) are fp32 row matrices of n_rows rows, each with its own 16-byte aligned base and its own row
 * stride in elements (a multiple of 4, at least the width); bias, gamma, beta and the three column sums are 16-byte aligned vectors
 * of the width.  No element outside the n_rows x width window of an output is written.  No output may overlap an input or another
 * output.  1 <= n_rows <= 2^31 - 1; the grid is sized from n_rows, nothing is read back, nothing synchronises: every call can be
 * captured.
 * Dropout: Philox4x32-10 with key (seed lo32, seed hi32) and counter (row lo32, col >> 2, offset lo32, offset hi32); output word
 * col & 3 decides column col (one call per four columns): keep iff word >= floor(dropout_p * 2^32); kept values are scaled by
 * 1.0f / (1.0f - dropout_p).  The backward regenerates the mask from the same (seed, offset).
 * Column sums: a workgroup owns ANCE_LAYER_TAIL_ROWS_PER_WORKGROUP consecutive rows (ance_layer_tail_rows_per_workgroup returns
 * the same number), sums their terms per column in a fixed order and writes ONE partial row; a second launch sums the
 * n_part = ceil(n_rows / ANCE_LAYER_TAIL_ROWS_PER_WORKGROUP) partial rows per column as a fixed binary tree.  No atomics: the same
 * inputs give the same bits.
 * d_workspace (16-byte aligned):
 *   layer tail  ance_layer_tail_workspace_bytes(n_rows, H) = S + n_part * 3 * H * 4, S = 2 * roundup(4 * n_rows, 256): mean [n_rows]
 *               at byte 0 and rstd [n_rows] at byte S / 2, fp32, written by the forward and read by the backward -- the only saved
 *               state; behind them the backward's partial rows [n_part][3][H] (dgamma, dbeta, dbias).  The forward touches and
 *               requires only the first S bytes; the backward requires all of it and takes the SAME AnceLayerTailArgs (of which
 *               it reads neither y nor beta: they are not checked there).
 *   bias + GELU ance_bias_gelu_workspace_bytes(n_rows, N) = n_part * N * 4: the backward's partial rows [n_part][N].  The forward
 *               neither reads nor checks d_workspace; the backward neither reads nor checks y.
 * One launch forward, two backward.  dx, dres, dgamma, dbeta, dbias may each be NULL when not wanted (the bias + GELU's dx and
 * dbias likewise); with bias NULL no dbias is produced.
 * Refuses (ANCE_E_INVALID, before any launch) a width outside {768, 1024} / {3072, 4096}, n_rows < 1, a null pointer other than
 * those named above, an unaligned base, a stride that is not a multiple of 4 or below the width, dropout_p outside [0, 1),
 * eps <= 0, and a null, unaligned or too small workspace.  The workspace queries return 0 for what is not supported. */
#define ANCE_LAYER_TAIL_ROWS_PER_WORKGROUP 16
typedef struct AnceLayerTailArgs {
    const float *x, *res;
    const float *bias;            /* [H] or NULL                                                  */
    const float *gamma, *beta;    /* [H]                                                          */
    float *y;
    int32_t ld_x, ld_res, ld_y;
    int32_t H, n_rows;
    float eps;
    float dropout_p;
    int32_t training;
    uint64_t seed, offset;
    void *d_workspace;
    size_t workspace_bytes;
} AnceLayerTailArgs;
typedef struct AnceLayerTailGradArgs {
    const float *dy;
    float *dx, *dres;             /* [n_rows, ld], each nullable                                  */
    float *dgamma, *dbeta, *dbias; /* [H], each nullable                                          */
    int32_t ld_dy, ld_dx, ld_dres;
    int32_t reserved;             /* 0 */
} AnceLayerTailGradArgs;
typedef struct AnceBiasGeluArgs {
    const float *x, *bias;
    float *y;
    int32_t ld_x, ld_y, N, n_rows;
    void *d_workspace;
    size_t workspace_bytes;
} AnceBiasGeluArgs;
typedef struct AnceBiasGeluGradArgs {
    const float *dy;
    float *dx, *dbias;            /* each nullable                                                */
    int32_t ld_dy, ld_dx;
} AnceBiasGeluGradArgs;
int ance_layer_tail_rows_per_workgroup(void);
size_t ance_layer_tail_workspace_bytes(int64_t n_rows, int H);
size_t ance_bias_gelu_workspace_bytes(int64_t n_rows, int N);
int ance_layer_tail_forward(const AnceLayerTailArgs *args, void *stream);
int ance_layer_tail_backward(const AnceLayerTailArgs *args, const AnceLayerTailGradArgs *grads, void *stream);
int ance_layer_tail_forward_dstream(const AnceLayerTailArgs *args, const uint64_t *d_stream, void *stream); /* the device dropout stream: ance_attention_* */
int ance_layer_tail_backward_dstream(const AnceLayerTailArgs *args, const AnceLayerTailGradArgs *grads, const uint64_t *d_stream, void *stream);
int ance_bias_gelu_forward(const AnceBiasGeluArgs *args, void *stream);
int ance_bias_gelu_backward(const AnceBiasGeluArgs *args, const AnceBiasGeluGradArgs *grads, void *stream);

/* The same seams with 16-bit matmul-side I/O and an fp32 residual stream (csrc/layer_tail_half.hip): the recipe's --fp16, i.e.
 * torch.autocast plus a GradScaler.  T = fp16 (dtype ANCE_DTYPE_F16) or bf16 (ANCE_DTYPE_BF16); "rounded" = once, to nearest even,
 * overflow to +-inf (never clamped: under a GradScaler an overflowing dx must reach found_inf as a non-finite gradient).
 * Layer tail: x [n_rows, H] is T (the dense output without its bias); res, y, bias, gamma, beta stay fp32.  u = float(x[r]) + bias;
 *   everything behind the load is the fp32 tail's arithmetic in fp32 -- the same dropout stream (the same (seed, offset, row, col)
 *   keeps the same element in both precisions), z = d + res, the two-pass LayerNorm, mean / rstd in the workspace.  y is fp32; y16
 *   (nullable) is the same registers rounded to T, for the Linears that read y: y16 == (T)y bit for bit.
 *   backward: dy (fp32) and dy16 (T) are each nullable, at least one is given; g = dy + float(dy16) in fp32 registers (the sum
 *   autograd would otherwise make of the residual's and the Linears' gradients).  dx is T, rounded; dres, dgamma, dbeta, dbias are
 *   fp32 and every output is nullable.  xhat is recomputed from x, bias, res, the regenerated mask and the saved statistics.
 *   On an x that holds T values, y, dres, dgamma, dbeta, dbias are the fp32 tail's on float(x), and dx is that dx rounded.
 * Bias + GELU: x, y, dy, dx [n_rows, N] are T, bias and dbias fp32.  u = float(x[r]) + bias; the erf form and its derivative in fp32
 *   as above; y and dx rounded; dbias = sum_r of the unrounded dx.  Nothing but x is saved.
 * Layout: a T matrix has a 16-byte aligned base and a row stride in elements that is a multiple of 8 and at least the width; the
 * fp32 matrices and vectors are as above.  Lane l of the row's wave holds columns 4 (64 i + l) .. + 3 as in the fp32 kernels: one
 * 8-byte access of a T row next to one 16-byte access of an fp32 row, one Philox call per four columns.
 * Workspaces, partial rows, the column-sum tree (so a parameter gradient over the same fp32 terms has the fp32 kernels' summation
 * order), launch counts (one forward, two backward), no atomics, nothing synchronises, capturable: as above;
 * ance_layer_tail16_workspace_bytes / ance_bias_gelu16_workspace_bytes equal the fp32 queries.
 * Refuses what the fp32 calls refuse, a dtype that is neither, a T stride that is not a multiple of 8, and dy == dy16 == NULL. */
typedef struct AnceLayerTail16Args {
    const void *x;                /* T [n_rows, ld_x]                                             */
    const float *res;
    const float *bias;            /* [H] or NULL                                                  */
    const float *gamma, *beta;    /* [H]                                                          */
    float *y;
    void *y16;                    /* T [n_rows, ld_y16] or NULL                                   */
    int32_t ld_x, ld_res, ld_y, ld_y16;
    int32_t H, n_rows;
    int32_t dtype;                /* ANCE_DTYPE_F16 or ANCE_DTYPE_BF16                            */
    float eps;
    float dropout_p;
    int32_t training;
    uint64_t seed, offset;
    void *d_workspace;
    size_t workspace_bytes;
} AnceLayerTail16Args;
typedef struct AnceLayerTail16GradArgs {
    const float *dy;              /* fp32 or NULL                                                 */
    const void *dy16;             /* T or NULL; not both NULL                                     */
    void *dx;                     /* T, nullable                                                  */
    float *dres;                  /* nullable                                                     */
    float *dgamma, *dbeta, *dbias; /* [H], each nullable                                          */
    int32_t ld_dy, ld_dy16, ld_dx, ld_dres;
} AnceLayerTail16GradArgs;
typedef struct AnceBiasGelu16Args {
    const void *x;                /* T                                                            */
    const float *bias;
    void *y;                      /* T                                                            */
    int32_t ld_x, ld_y, N, n_rows;
    int32_t dtype;                /* ANCE_DTYPE_F16 or ANCE_DTYPE_BF16                            */
    int32_t reserved;             /* 0 */
    void *d_workspace;
    size_t workspace_bytes;
} AnceBiasGelu16Args;
typedef struct AnceBiasGelu16GradArgs {
    const void *dy;               /* T                                                            */
    void *dx;                     /* T, nullable                                                  */
    float *dbias;                 /* nullable                                                     */
    int32_t ld_dy, ld_dx;
} AnceBiasGelu16GradArgs;
size_t ance_layer_tail16_workspace_bytes(int64_t n_rows, int H);
size_t ance_bias_gelu16_workspace_bytes(int64_t n_rows, int N);
int ance_layer_tail16_forward(const AnceLayerTail16Args *args, void *stream);
int ance_layer_tail16_backward(const AnceLayerTail16Args *args, const AnceLayerTail16GradArgs *grads, void *stream);
int ance_layer_tail16_forward_dstream(const AnceLayerTail16Args *args, const uint64_t *d_stream, void *stream); /* the device dropout stream: ance_attention_* */
int ance_layer_tail16_backward_dstream(const AnceLayerTail16Args *args, const AnceLayerTail16GradArgs *grads, const uint64_t *d_stream, void *stream);
int ance_bias_gelu16_forward(const AnceBiasGelu16Args *args, void *stream);
int ance_bias_gelu16_backward(const AnceBiasGelu16Args *args, const AnceBiasGelu16GradArgs *grads, void *stream);

/* The input end of a trainable tower with its gradients (csrc/embed_train.hip), fp32 throughout: what transformers' eager
 * BertEmbeddings / RobertaEmbeddings compute, ids -> word + token_type + position -> LayerNorm -> dropout.  T = n_seq * L token rows,
 * row r = s * L + l; H = 768 or 1024; 1 <= L <= 512; ids and type_ids are int32 [n_seq, L]; y and dy are contiguous [T, H].
 * Arithmetic, per row:
 *   id = clamp(ids[r], 0, vocab - 1);  tt = type_ids ? clamp(type_ids[r], 0, n_types - 1) : 0;
 *   p  = l                                                                     (ANCE_EMBED_POSITION_ABSOLUTE: BERT, DPR)
 *   p  = padding_idx + (id != padding_idx ? #{t <= l : id(s, t) != padding_idx} : 0)   (ANCE_EMBED_POSITION_ROBERTA:
 *        create_position_ids_from_input_ids, pads anywhere in the row; counted inside the forward kernel, no extra launch)
 *   p  = clamp(p, 0, max_pos - 1)
 *   The clamps are the first thing done with an id, a type id or a position, before an address is formed from it, in the forward
 *   and in every backward kernel: an out-of-range id is READ AS the nearest valid one (forward bits and gradient row), and nothing
 *   is reported -- nothing synchronises.  `id != padding_idx` compares the clamped id.
 *   v = (word[id] + type[tt]) + pos[p] (this association);  mean = sum v / H;  var = sum (v - mean)^2 / H (two passes over the row
 *   in registers, biased);  rstd = 1.0f / sqrtf(var + eps);  xhat = (v - mean) rstd;  u = xhat o gamma + beta;
 *   y[r] = keep o u * (1.0f / (1.0f - dropout_p)) when training != 0 and dropout_p > 0, else u.
 *   backward, given dy:  d = keep o dy / (1 - dropout_p);  g = d o gamma;  dv = rstd (g - mean_H(g) - xhat mean_H(g o xhat));
 *   dgamma = sum_r d o xhat;  dbeta = sum_r d;  dword[k] = sum of dv over the rows with id k, dpos[k] and dtype[k] likewise.
 * Dropout: the layer tail's Philox contract above -- key (seed lo32, seed hi32), counter (row lo32, col >> 2, offset lo32, offset
 * hi32), output word col & 3 decides column col, keep iff word >= floor(dropout_p * 2^32).  seed and offset are host values.
 * Saved state: mean [T] and rstd [T] in the first S = 2 * roundup(4 * T, 256) bytes of d_workspace (mean at byte 0, rstd at byte
 * S / 2, as the layer tail lays them out), and in roberta mode positions [T] int32.  ids and type_ids are read again by the backward.
 * No mask and no [T, H] activation is kept: the backward recomputes v from the tables and regenerates the mask.
 * Table gradients (dense: dword [vocab, H], dpos [max_pos, H], dtype [n_types, H]; the CALLER zero-fills them, the kernels store only
 * the rows that occur, with plain vector stores; no atomics anywhere):
 *   grouping  the caller passes, per table, the keys in the order of a STABLE ascending sort of the T raw int32 keys (word_keys:
 *             ids; type_keys: type_ids; pos_keys: the saved positions) and the int64 permutation (sorted position j -> row).  The
 *             kernels clamp the sorted keys (which keeps them sorted) and every row index.  Absolute positions are grouped
 *             analytically (key p: rows s * L + p, s ascending) and take no arrays; a type table with n_types == 1 or with
 *             type_ids NULL takes none either: dtype[0] is the column sum of dv over all rows, by the layer tail's partial rows
 *             and tree.
 *   order     the sorted positions are cut into aligned chunks of ANCE_EMBED_SEGMENT_CHUNK (ance_embed_segment_chunk returns the
 *             same number).  A piece is a maximal run of one key inside a chunk; one wave adds a piece's rows in ascending sorted
 *             position, starting from the first row (no zero is added).  A key whose run crosses chunk boundaries gets its pieces'
 *             partial rows added in ascending chunk order by one wave in a second launch.  The order is a function of the sorted
 *             keys alone: the same inputs give the same bits, whatever the grid.  Longest serial chain for a key with n rows:
 *             about ANCE_EMBED_SEGMENT_CHUNK + n / ANCE_EMBED_SEGMENT_CHUNK row additions.
 *   padding   rows whose (clamped) id equals padding_idx add nothing to dword -- its row padding_idx keeps the caller's zeros --
 *             and in roberta mode rows at position padding_idx add nothing to dpos: nn.Embedding(padding_idx=...)'s gradient.
 *             padding_idx = -1: none (absolute mode only; the type table and the absolute position table never have one).
 * d_workspace (16-byte aligned), ance_embed_workspace_bytes(T, H) = S + T * H * 4 + n_part * 3 * H * 4 + 3 * n_chunk * 2 * H * 4,
 * n_part = ceil(T / ANCE_LAYER_TAIL_ROWS_PER_WORKGROUP), n_chunk = ceil(T / ANCE_EMBED_SEGMENT_CHUNK): the statistics; dv [T, H];
 * the partial rows [n_part][3][H] (dgamma, dbeta, sum dv); per table (word, position, type) the chunks' partial rows
 * [n_chunk][2][H].  The forward touches and requires only the first S bytes; the backward takes the SAME AnceEmbedArgs (of which it
 * reads neither y nor beta) and all of the workspace.
 * Launches: ONE forward.  Backward FOUR: the row kernel, the column-sum tree, the pieces, the joins (all wanted tables ride in the
 * same two launches); TWO when none of dword, dpos, dtype needs the segmented sum.  The sort that produces the keys is the caller's.
 * Nothing is read back, nothing synchronises: every call can be captured.
 * Refuses (ANCE_E_INVALID, before any launch): a null pointer other than type_ids, positions in absolute mode, the gradient
 * outputs and the keys / permutations of tables not wanted; H outside {768, 1024}; L outside 1 .. 512; n_seq < 1; n_types outside
 * {1, 2}; a position_mode other than the two; absolute mode with L > max_pos; roberta mode with L + padding_idx + 1 > max_pos or
 * padding_idx outside 0 .. vocab - 1; dropout_p outside [0, 1); eps <= 0; an unaligned base; a null, unaligned or too small
 * workspace.  ance_embed_workspace_bytes returns 0 for H outside {768, 1024} or T outside 1 .. 2^31 - 1. */
#define ANCE_EMBED_SEGMENT_CHUNK 64
#define ANCE_EMBED_POSITION_ABSOLUTE 0
#define ANCE_EMBED_POSITION_ROBERTA 1
typedef struct AnceEmbedArgs {
    const int32_t *ids;           /* [n_seq, L]                                                   */
    const int32_t *type_ids;      /* [n_seq, L] or NULL: type 0                                   */
    const float *word, *pos, *type; /* [vocab, H], [max_pos, H], [n_types, H]                     */
    const float *gamma, *beta;    /* [H]                                                          */
    float *y;                     /* [n_seq * L, H]                                               */
    int32_t *positions;           /* [n_seq * L], roberta mode: written forward, read backward    */
    int32_t n_seq, L, H;
    int32_t vocab, max_pos, n_types;
    int32_t position_mode;        /* ANCE_EMBED_POSITION_*                                        */
    int32_t padding_idx;          /* -1: none                                                     */
    float eps;
    float dropout_p;
    int32_t training;
    int32_t reserved;             /* 0 */
    uint64_t seed, offset;
    void *d_workspace;
    size_t workspace_bytes;
} AnceEmbedArgs;
typedef struct AnceEmbedGradArgs {
    const float *dy;              /* [n_seq * L, H]                                               */
    float *dword, *dpos, *dtype;  /* dense tables, zero-filled by the caller, each nullable       */
    float *dgamma, *dbeta;        /* [H], each nullable                                           */
    const int32_t *word_keys;     /* [T] sorted ids; with dword                                   */
    const int64_t *word_perm;     /* [T] sorted position -> row                                   */
    const int32_t *pos_keys;      /* sorted saved positions; with dpos in roberta mode            */
    const int64_t *pos_perm;
    const int32_t *type_keys;     /* sorted type_ids; with dtype when n_types == 2 and type_ids   */
    const int64_t *type_perm;
} AnceEmbedGradArgs;
int ance_embed_segment_chunk(void);
size_t ance_embed_workspace_bytes(int64_t n_rows, int H);
int ance_embed_forward(const AnceEmbedArgs *args, void *stream);
int ance_embed_backward(const AnceEmbedArgs *args, const AnceEmbedGradArgs *grads, void *stream);
int ance_embed_forward_dstream(const AnceEmbedArgs *args, const uint64_t *d_stream, void *stream); /* the device dropout stream: ance_attention_* */
int ance_embed_backward_dstream(const AnceEmbedArgs *args, const AnceEmbedGradArgs *grads, const uint64_t *d_stream, void *stream);

/* Packed token rows of a fixed capacity (csrc/pack_rows.hip; the rows forms of the embeddings: csrc/embed_train.hip).  A right-padded
 * batch ids [n_seq, L] with device lengths becomes R = `rows` token rows that hold the sequences back to back; R is the CALLER's
 * capacity, a host value that fixes every shape and grid, while the number of rows in use lives on the device only.  Nothing is
 * read back, nothing synchronises, there are no atomics, and the same inputs give the same bits: every call here can be captured.
 *
 * ance_pack_tokens -- the plan and the packed keys, TWO launches whatever the inputs (the plan: one workgroup; the fill):
 *   len_s  = clamp(d_seq_len[s], 0, L);  off_s = len_0 + .. + len_{s-1};  sequence s is KEPT iff off_s + len_s <= R.  off_s + len_s
 *            never decreases with s, so the dropped sequences are a suffix; T = the rows of the kept ones.
 *   d_seq_off [n_seq + 1]  off_s for a kept sequence; T for every dropped one and for the last entry -- the differences are the
 *            kept lengths and 0 for a dropped sequence, which is what ance_attention_* take as the packed form
 *   d_seq_kept [n_seq]     len_s, or -1 for a dropped sequence
 *   d_dropped              int64 on the device: the call ADDS the number of dropped sequences (one thread, a plain load and store)
 *   packed row off_s + l, l < len_s, of a kept sequence: packed_ids = ids[s, l] as it is; packed_type_ids = type_ids[s, l] (only when
 *            type_ids is given); packed_positions = ance_embed_forward's p of (s, l), its clamps included: l, or padding_idx + (id !=
 *            padding_idx ? #{t <= l : id(s, t) != padding_idx} : 0) over the ids clamped into the vocabulary, then clamp(p, 0, max_pos - 1)
 *   slack rows T .. R - 1: id padding_idx (0 when it is -1), type 0, position padding_idx in roberta mode and 0 otherwise
 *   No row >= R of a packed array is written whatever d_seq_len holds, and every offset read back from memory is clamped first.
 *   Refuses (ANCE_E_INVALID, before any launch): a null pointer other than type_ids / packed_type_ids (type_ids given needs
 *   packed_type_ids); an integer array not 4-byte aligned, d_dropped not 8-byte aligned; n_seq outside 1 .. 65535; L outside
 *   1 .. 512; rows < 1; vocab or max_pos < 1; a position_mode other than the two; padding_idx outside -1 .. vocab - 1 (roberta:
 *   0 .. vocab - 1).
 *
 * ance_pack_tokens_by_id -- the same outputs (without type ids) for a batch whose pad tokens may sit ANYWHERE in a row, the SEED-Encoder's
 *   rule: every id equal to padding_idx is left out, inside a record too, and the positions count the ids that stay.  THREE launches
 *   whatever the inputs -- count (a wave per sequence, one ballot per 64 columns), the plan above over the counted lengths, fill (a wave
 *   per kept sequence walks all L columns) -- no atomics, nothing read back, capturable.
 *   d_seq_len [n_seq]      WRITTEN by the call: #{l < L : ids[s, l] != padding_idx} (the raw ids are compared), or -1 when
 *            ids[s, 0] == padding_idx (a LEADING pad; an all-pad row included): the first row of such a sequence would not be its
 *            first token, so it is DROPPED whatever the capacity: it scans as 0 rows, d_seq_kept = -1, d_dropped grows by one, and
 *            d_seq_off keeps its own running offset (while that is <= R), so d_seq_off stays non-decreasing and the neighbours'
 *            differences stay their lengths; ance_first_rows_gather hands out NaN for it.  Capacity overflow is ance_pack_tokens':
 *            a suffix of the batch gets d_seq_kept = -1 and d_seq_off = T.
 *   packed row off_s + r of a kept sequence, r = the rank of column l among the sequence's non-pad columns: packed_ids = ids[s, l] as
 *            it is; packed_positions = clamp(padding_idx + 1 + r, 0, max_pos - 1).  Slack rows T .. R - 1: id and position padding_idx.
 *   For sequences that begin with a non-pad id (whose ids inside the vocabulary do not clamp onto padding_idx) every output equals,
 *   bit for bit, ance_pack_tokens' in roberta mode on the batch with each row's non-pad ids moved to the front and d_seq_len their
 *   counts.  No row >= R is written, and every offset read back from memory is clamped into [0, R] first.
 *   Refuses (ANCE_E_INVALID, before any launch): a null pointer; an integer array not 4-byte aligned, d_dropped not 8-byte aligned;
 *   n_seq outside 1 .. 65535; L outside 1 .. 512; rows < 1; vocab or max_pos < 1; padding_idx outside 0 .. vocab - 1.
 *
 * ance_embed_rows_forward / _backward (+ _dstream) -- ance_embed_* over T = n_seq rows with L = 1 whose positions are GIVEN:
 *   AnceEmbedArgs.positions [n_seq] is read in both directions (clamped into the table) and never written; position_mode only
 *   says whether the position table has a padding row (roberta: positions equal to padding_idx add nothing to dpos; absolute:
 *   none).  dpos ALWAYS goes through the sorted keys (pos_keys / pos_perm are required with dpos in both modes: a row is no longer
 *   s * L + p).  Everything else is ance_embed_*'s, by the same kernels: the arithmetic, the dropout counter (the row is the PACKED
 *   row index), the saved state, the workspace (ance_embed_workspace_bytes(n_seq, H)), the launch counts, the padding rule of
 *   dword, the order of every sum.  Refuses what ance_embed_* refuse, L != 1 and null positions; max_pos is not tied to L.
 *
 * ance_first_rows_gather / _scatter -- the first row of every sequence out of a row matrix [R, H] and its backward; H = 768 or 1024,
 *   dtype ANCE_DTYPE_F32, _F16 or _BF16, 16-byte pieces, one wave per sequence, ONE launch each:
 *   gather   first[s] = rows_matrix[d_seq_off[s]] when d_seq_kept[s] > 0; zeros when it is 0 (an empty sequence); a QUIET NaN in
 *            every element when it is negative (a dropped sequence: it must not go unnoticed, and nothing may wait for the host)
 *   scatter  rows_matrix[d_seq_off[s]] = first[s] for every s with d_seq_kept[s] > 0 -- distinct rows, one owner each, plain vector
 *            stores; nothing else is written: the CALLER zero-fills rows_matrix.
 *   d_seq_off is clamped into [0, rows - 1] before a row is addressed.  Refuses a null or unaligned pointer, H, dtype, n_seq outside
 *   1 .. 65535, rows < 1, a stride that is not a multiple of a 16-byte piece or below H. */
typedef struct AncePackArgs {
    const int32_t *ids;           /* [n_seq, L]                                                   */
    const int32_t *type_ids;      /* [n_seq, L] or NULL                                           */
    const int32_t *d_seq_len;     /* [n_seq] on the device                                        */
    int32_t *d_seq_off;           /* [n_seq + 1] out                                              */
    int32_t *d_seq_kept;          /* [n_seq] out                                                  */
    int64_t *d_dropped;           /* device counter, added to                                     */
    int32_t *packed_ids;          /* [rows] out                                                   */
    int32_t *packed_type_ids;     /* [rows] out, with type_ids                                    */
    int32_t *packed_positions;    /* [rows] out                                                   */
    int32_t n_seq, L, rows;
    int32_t position_mode;        /* ANCE_EMBED_POSITION_*                                        */
    int32_t padding_idx;          /* -1: none                                                     */
    int32_t vocab, max_pos;
    int32_t reserved;             /* 0 */
} AncePackArgs;
typedef struct AnceFirstRowsArgs {
    void *rows_matrix;            /* [rows, H]: read by the gather, written by the scatter        */
    void *first;                  /* [n_seq, H]: written by the gather, read by the scatter       */
    const int32_t *d_seq_off;     /* [n_seq + 1] (the last entry is not read)                     */
    const int32_t *d_seq_kept;    /* [n_seq]                                                      */
    int32_t ld_rows, ld_first;    /* row strides in elements                                      */
    int32_t n_seq, rows, H;
    int32_t dtype;                /* ANCE_DTYPE_*                                                 */
} AnceFirstRowsArgs;
typedef struct AncePackByIdArgs {
    const int32_t *ids;           /* [n_seq, L]                                                   */
    int32_t *d_seq_len;           /* [n_seq] on the device, WRITTEN: the non-pad counts, -1: a leading pad */
    int32_t *d_seq_off;           /* [n_seq + 1] out                                              */
    int32_t *d_seq_kept;          /* [n_seq] out                                                  */
    int64_t *d_dropped;           /* device counter, added to                                     */
    int32_t *packed_ids;          /* [rows] out                                                   */
    int32_t *packed_positions;    /* [rows] out                                                   */
    int32_t n_seq, L, rows;
    int32_t padding_idx;          /* 0 .. vocab - 1                                               */
    int32_t vocab, max_pos;
} AncePackByIdArgs;
int ance_pack_tokens(const AncePackArgs *args, void *stream);
int ance_pack_tokens_by_id(const AncePackByIdArgs *args, void *stream);
int ance_embed_rows_forward(const AnceEmbedArgs *args, void *stream);
int ance_embed_rows_backward(const AnceEmbedArgs *args, const AnceEmbedGradArgs *grads, void *stream);
int ance_embed_rows_forward_dstream(const AnceEmbedArgs *args, const uint64_t *d_stream, void *stream);
int ance_embed_rows_backward_dstream(const AnceEmbedArgs *args, const AnceEmbedGradArgs *grads, const uint64_t *d_stream, void *stream);
int ance_first_rows_gather(const AnceFirstRowsArgs *args, void *stream);
int ance_first_rows_scatter(const AnceFirstRowsArgs *args, void *stream);

/* Test hook: the SPLIT (fp32-grade) GEMM of the encoder with one of its epilogues.  acc[m][n] = sum_k a[m][k] b[n][k] with
 * a = a_hi + a_lo (b likewise; the lo x lo products are left out); d_a_pair [M, 2K] / d_b_pair [N, 2K] fp16 PAIR ROWS -- 32-column
 * blocks [hi (32) | lo (32)], lo = fp16(v - hi) unscaled: ance_pair_layout gives the positions; (mu_m, r_m) = mean and
 * 1 / sqrt(var + ln_eps) of row m combined from d_part [M][12][2], the (mean, M2) of its twelve 64-column slices (EPI_S_RESLN at
 * N = 1024: [M][24] floats holding the (mean, M2) of eight 128-column slices, in and out -- the hidden-1024 format);
 * w = *d_wscale_inv (device scalar; NULL: 1), the inverse of the power of two b was stored with.
 *   epi 8   d_out fp32 [M, N]      = r_m (w acc - mu_m vec1[n]) + bias[n]                             (vec1 = csum)
 *   epi 9   d_out fp16 pair [M, 2N] = pair(gelu_erf(r_m (w acc - mu_m vec1[n]) + bias[n]))
 *   epi 10  d_out fp16 pair [M, 2N] = pair(w acc + bias[n] + (res[m][n] - mu_m) r_m vec1[n] + vec2[n])   (vec1 = gamma, vec2 = beta,
 *           res = d_res_pair [M, 2N] pair rows; N = 768 or 1024), d_part_out [M][24] = slice statistics of the output rows
 * M, N multiples of 256, K of 64, >= 128. */
int ance_debug_gemm_split(int epi, const void *d_a_pair, const void *d_b_pair, int M, int N, int K, const float *d_bias,
                          const float *d_vec1, const float *d_vec2, const float *d_part, float ln_eps, const void *d_res_pair,
                          void *d_out, float *d_part_out, const float *d_wscale_inv, void *stream);

/* Test hook: ONE instance of the encoder's GEMM (epilogues 4-10 at hidden width hw = 768 or 1024) with every field the encoder
 * sets, on caller data -- what ance_debug_gemm / ance_debug_gemm_split cannot reach: the fp16 mode's folded epilogues, the
 * hidden-1024 instances of the split epilogues, tok_lo and n_split.  Field names are the encoder's (csrc/gemm_f16.h: GemmArgs);
 * row strides are in elements; M, N multiples of 256, K of 64, >= 128; the token / feature arrays hold 256-row tiles.
 *   part_in  [tokens][24]: (mean, M2) of the slices of each token's pre-LayerNorm row -- twelve 64-column slices at hw 768, eight
 *            128-column slices (16 of the 24 floats) at hw 1024; tokens are the rows m, the columns n for epi 7
 *   epi 4  EPI_RESLN    out / out_lo fp16 [M, ldc] = (hi, lo) of acc + bias[n] + LayerNorm(res_hi + res_lo) (res rows at stride ldc,
 *                       statistics from part_in, res_gamma / res_beta); part_out [M][24] = output slice statistics; N = hw
 *   epi 5  EPI_QK_F     out fp16 [M, ldc] = (r_m (acc - mu_m csum[n]) + bias[n]) * (n < scale_cols ? scale : 1); scale_cols % 64 == 0
 *   epi 6  EPI_GELU_F   out fp16 [M, ldc] = gelu(r_m (acc - mu_m csum[n]) + bias[n])
 *   epi 7  EPI_VT_F     out fp16 [M, ldc]: column col_map[n] = r_n (acc - mu_n csum[m]) + bias[m], tokens n < n_valid only
 *   epi 5-7: tok_lo (nullable) = the lo halves of the token operand (A for 5 / 6, B for 7, same stride): a tile with a token
 *            whose |mean| rstd > 2 adds acc += lo . W^T for those tokens
 *   epi 8-10 the split epilogues of ance_debug_gemm_split (pair rows; epi 10: residual pair rows at stride ldr, N = hw) with
 *            wscale_inv (nullable) and the partials in the hw format
 *   n_split  0, or 2: the N-split tile order (N / 256 even)
 * Refuses (ANCE_E_INVALID, before any launch) hw outside {768, 1024}, epi outside 4..10, a null pointer the epilogue reads and
 * n_split outside {0, 2}. */
typedef struct AnceGemmDebugArgs {
    const void *a, *b;            /* fp16 [M, lda] / [N, ldb] (split: pair rows)                 */
    int32_t lda, ldb, M, N, K;
    const float *bias, *csum, *part_in;
    float ln_eps;
    const void *tok_lo;
    float scale;
    int32_t scale_cols;
    const int32_t *col_map;
    int32_t n_valid, ldc;
    void *out;                    /* fp16 (epi 4-7, 9, 10) or fp32 (epi 8)                      */
    const void *res_hi, *res_lo;
    const float *res_gamma, *res_beta;
    void *out_lo;
    float *part_out;
    int32_t ldr;
    const float *wscale_inv;
    int32_t n_split;
} AnceGemmDebugArgs;
int ance_debug_gemm_hw(int epi, int hw, const AnceGemmDebugArgs *args, void *stream);

/* Test hook: ONE launch of one of the encoder's three attention kernels on caller data, through the encoder's own launchers
 * (csrc/attention.hip: launch_attention, launch_attention_split; csrc/precise32.h: launch_attention32).  Head dim 64, H = 64 n_heads.
 *   kind 0  fp16 fast mode (AttnArgs): qk fp16 [qk_rows, ld_qk] = Q (pre-scaled by log2(e) / 8) | K; vt fp16 [H, ld_vt] = V^T with
 *           the keys of a sequence at columns vcol .. vcol + len; ctx fp16 [ctx_rows, ld_ctx].  cls_only: query 0 of every sequence
 *           only, its output row is s; q_compact (with cls_only): that query is row s of the Q columns
 *   kind 1  split mode: qk fp32 [qk_rows, 3 H] = Q | K | V (unscaled); ctx fp16 PAIR rows [ctx_rows, 2 H] (ance_pair_layout);
 *           cls_only: the query of sequence s is row s of the Q columns and its output row is s (q_compact must equal cls_only)
 *   kind 2  fp32 mode: qk fp32 [qk_rows, 3 H] = Q | K | V; ctx fp32 [ctx_rows, H]; no cls_only
 * h_desc is HOST memory: kinds 0, 1 int32[n_seq][4] = (first token, length, first V^T column, sequence index s), kind 2 int32
 * [n_seq + 1] = token offsets (sequence s = rows seq_off[s] .. seq_off[s + 1]).  The hook validates it, then copies it with
 * hipMemcpyAsync on the stream into d_desc (d_desc_bytes long); h_desc must stay valid until the stream has run the copy.
 * Refuses (ANCE_E_INVALID, before any copy or launch) a kind outside 0..2, n_heads outside {12, 16}, n_seq < 1,
 * max_seq_len outside 1..512, a length outside 1..max_seq_len, a sequence whose token rows, Q row s (q_compact), output row or V^T
 * columns vcol + roundup8(len) fall outside the allocation, vcol % 8 != 0, strides or pointers that break the kernels' 16-byte
 * accesses (kinds 1, 2: the strides are fixed at 3 H and 2 H / H), a repeated or out-of-range sequence index, cls_only on
 * kind 2, q_compact without cls_only (kind 1: q_compact != cls_only), a d_desc too small and a null pointer the kind reads. */
typedef struct AnceAttnDebugArgs {
    int32_t kind, n_heads, n_seq, max_seq_len, cls_only, q_compact;
    const int32_t *h_desc;        /* HOST: int4 descriptors (kinds 0, 1) or seq_off (kind 2)      */
    void *d_desc;
    int64_t d_desc_bytes;
    const void *qk;               /* fp16 (kind 0) or fp32 Q | K | V (kinds 1, 2)                 */
    int32_t ld_qk, qk_rows;
    const void *vt;               /* fp16 [H, ld_vt], kind 0 only                                 */
    int32_t ld_vt;
    void *ctx;                    /* fp16 (kind 0), fp16 pair rows (kind 1) or fp32 (kind 2)      */
    int32_t ld_ctx, ctx_rows;
} AnceAttnDebugArgs;
int ance_debug_attention(const AnceAttnDebugArgs *args, void *stream);

/* Layout of the split mode's pair rows (for tests and tools that build or read them): column n of a W-wide fp32 row has its hi
 * half at *hi_col and its lo half at *lo_col of the 2 W-half pair row, lo = fp16((v - hi) * *lo_scale).  Product library:
 * hi_col = 64 (n / 32) + n % 32, lo_col = hi_col + 32, lo_scale = 1. */
void ance_pair_layout(int n, int W, int *hi_col, int *lo_col, float *lo_scale);

/* ---------------------------------------------------------------------------------------------
 * Fused multi-tensor LAMB step (csrc/lamb.hip; the reference's utils/lamb.py Lamb.step, which drivers/run_ann.py and
 * drivers/run_warmup.py train with).  Per tensor p with gradient g, state m, v and its group's lr, beta1, beta2, eps, wd:
 *   m <- beta1 m + (1 - beta1) g ;  v <- beta2 v + (1 - beta2) g^2          (no bias correction)
 *   u  = m / (sqrt(v) + eps) [+ wd p when wd != 0]
 *   wn = min(|p|_2, 10) (p before the update) ;  an = |u|_2 ;  tr = 1 if wn == 0 or an == 0 else wn / an
 *   p <- p - lr tr u    (tr = 1 in the update when adam != 0; the recorded tr is the LAMB one either way)
 * Every tensor of the call in three launches and no host synchronisation: pass 1 updates m, v and stores per-chunk partial
 * sums of p^2 and u^2 (fp64), a per-tensor kernel sums them in a fixed order into d_out, pass 2 recomputes u and writes p.
 * The same inputs give the same bits (no atomics).  40 bytes of HBM traffic per element.
 *
 * h_tensors and h_groups are HOST tables; they are staged into d_workspace on the stream through a pinned buffer of the library
 * (reused only once an event shows its previous copy has run), so the caller may overwrite or free them when the call returns.
 * The workspace must not be shared by two calls that can run at the same time (streams run a call's copy and kernels in order).
 * d_out: fp32 [n_tensors][3] = (wn, an, tr) per tensor.  Every device pointer fp32; p, m, v may not overlap one another
 * or another tensor's.  numel == 0 is allowed (any pointers; wn = an = 0, tr = 1).  n_tensors == 0: nothing is enqueued.
 * Refuses (ANCE_E_INVALID, before any copy or launch) a null table, n_tensors < 0, n_groups < 1, a group index out of range,
 * numel < 0, a null p / g / m / v of a tensor with numel > 0, a null d_out and a null, unaligned (16 B) or too small workspace;
 * ANCE_E_NOMEM when no pinned staging buffer can be allocated. */
typedef struct AnceLambTensor {
    float *p;                     /* parameter, updated in place                                  */
    const float *g;               /* gradient                                                     */
    float *m, *v;                 /* exp_avg, exp_avg_sq, updated in place                        */
    int64_t numel;
    int32_t group, reserved;
} AnceLambTensor;
typedef struct AnceLambGroup {
    double lr, beta1, beta2, eps, weight_decay;
} AnceLambGroup;
/* Bytes of workspace ance_lamb_step needs for n_tensors tensors of total_numel elements in n_groups groups (0: invalid). */
size_t ance_lamb_workspace_bytes(int n_tensors, int n_groups, int64_t total_numel);
int ance_lamb_step(const AnceLambTensor *h_tensors, int n_tensors, const AnceLambGroup *h_groups, int n_groups, int adam,
                   float *d_out, void *d_workspace, size_t workspace_bytes, void *stream);

/* ance_lamb_step with torch.nn.utils.clip_grad_norm_(params, max_grad_norm) (norm_type 2, error_if_nonfinite=False) over every
 * tensor of the call fused in front: total = the 2-norm of all gradients (per-chunk fp64 sums added in chunk order, one sqrt,
 * rounded to fp32) -> *d_grad_norm (DEVICE fp32, the norm before clipping); coef = min(max_grad_norm / (total + 1e-6), 1) in fp32;
 * every gradient element enters m and v as the fp32 product g coef (bit-neutral when coef == 1).  The gradients in memory are NOT
 * rescaled.  A NaN total makes coef NaN and poisons every tensor of the call, as torch's function does.  Five launches, 44 bytes
 * per element, no host synchronisation.  Workspace: ance_lamb_clipped_workspace_bytes (larger than ance_lamb_workspace_bytes).
 * Refuses what ance_lamb_step refuses, a max_grad_norm that is not a positive finite number and a null d_grad_norm. */
size_t ance_lamb_clipped_workspace_bytes(int n_tensors, int n_groups, int64_t total_numel);
int ance_lamb_step_clipped(const AnceLambTensor *h_tensors, int n_tensors, const AnceLambGroup *h_groups, int n_groups, int adam,
                           double max_grad_norm, float *d_grad_norm, float *d_out, void *d_workspace, size_t workspace_bytes,
                           void *stream);

/* Either step under loss scaling -- torch.amp.GradScaler's contract for an optimizer that sets _step_supports_amp_scaling: the
 * scale and the overflow flag are DEVICE fp32 scalars and the step is called unconditionally.  max_grad_norm == 0: ance_lamb_step,
 * else ance_lamb_step_clipped, with:
 *   unscale  d_grad_scale != NULL: inv = (float)(1.0 / (double)*d_grad_scale), formed on the device (the value
 *            GradScaler.unscale_ forms).  Every gradient element enters the step as the single fp32 product g inv, formed in
 *            registers: with clipping the 2-norm is taken over those products (squared and summed in fp64 in chunk order),
 *            coef is formed as in ance_lamb_step_clipped, and the element enters m, v as (g inv) coef -- two fp32 roundings in that
 *            order.  The gradients in memory are never rewritten.  A scale of 0 or a non-finite scale cannot be checked on the
 *            host and POISONS the step (inv is inf, 0 or NaN); a power-of-two scale is bit-neutral.
 *   skip     d_found_inf != NULL and !(*d_found_inf == 0) (NaN skips too): no bit of any p, m, v changes -- the workgroups of
 *            both passes read the flag and return before any store.  *d_grad_norm is still written when clipping and may be inf
 *            or NaN.  Row t of d_out is row t of d_prev_out when that is given (fp32 [n_tensors][3], e.g. the previous step's
 *            d_out; it may be d_out itself), else (0, 0, 1).  *d_skipped (DEVICE int64, nullable) is incremented by one.
 * Launches: three without clipping, five with it -- none more than the step it extends -- no atomics, a fixed summation order,
 * no host synchronisation.  With d_grad_scale == NULL and d_found_inf == NULL the result has the bits of ance_lamb_step /
 * ance_lamb_step_clipped.  Workspace: ance_lamb_amp_workspace_bytes (>= ance_lamb_clipped_workspace_bytes; 0 where that is 0).
 * Refuses (ANCE_E_INVALID, before any copy or launch) everything ance_lamb_step refuses, a negative, NaN or infinite
 * max_grad_norm, and clipping with a null d_grad_norm.  n_tensors == 0: nothing is enqueued (and nothing counted). */
size_t ance_lamb_amp_workspace_bytes(int n_tensors, int n_groups, int64_t total_numel);
int ance_lamb_step_amp(const AnceLambTensor *h_tensors, int n_tensors, const AnceLambGroup *h_groups, int n_groups, int adam,
                       double max_grad_norm,            /* 0: no clipping; else positive finite */
                       const float *d_grad_scale,       /* nullable: no unscale */
                       const float *d_found_inf,        /* nullable: never skip */
                       const float *d_prev_out,         /* nullable, [n_tensors][3] */
                       float *d_grad_norm,              /* required iff max_grad_norm != 0 */
                       int64_t *d_skipped,              /* nullable */
                       float *d_out, void *d_workspace, size_t workspace_bytes, void *stream);

/* The resident plan of a LAMB step: a caller that steps the same tensors again and again builds the device tables ONCE and then only
 * launches.  ance_lamb_plan_build checks the host tables as ance_lamb_step does and fills h_tables (HOST memory of at least
 * ance_lamb_plan_table_bytes bytes; pinned memory the caller owns and never refills while the plan lives) with the device layout;
 * d_lrs (nullable; n_groups entries, each nullable) gives a group's learning rate as a DEVICE fp64 scalar that the kernels read at
 * every step -- neg_lr = (float)(-*d_lr), the bits of a host lr of the same value -- and h_groups[i].lr is then ignored.  The caller
 * copies *table_bytes_out bytes of h_tables to the HEAD of a device workspace of ance_lamb_amp_workspace_bytes bytes that the plan
 * owns (one copy, with its own allocator and on its own stream: a copy captured into a graph re-reads identical bytes), and
 * ance_lamb_step_planned on that workspace is ance_lamb_step_amp without tables, checks of them, staging or copy: it enqueues only
 * its kernels (3, or 5 with max_grad_norm != 0), touches no event and allocates nothing, so it can be captured.  The plan is
 * valid as long as every pointer, numel and hyper-parameter it was built from is (a device lr may change in place). */
size_t ance_lamb_plan_table_bytes(int n_tensors, int n_groups, int64_t total_numel);
int ance_lamb_plan_build(const AnceLambTensor *h_tensors, int n_tensors, const AnceLambGroup *h_groups, const double *const *d_lrs,
                         int n_groups, void *h_tables, size_t h_tables_bytes, int64_t *n_chunks_out, size_t *table_bytes_out);
int ance_lamb_step_planned(int n_tensors, int n_groups, int64_t n_chunks, int adam, double max_grad_norm, const float *d_grad_scale,
                           const float *d_found_inf, const float *d_prev_out, float *d_grad_norm, int64_t *d_skipped, float *d_out,
                           void *d_workspace, size_t workspace_bytes, void *stream);

/* A planned step that FINDS ITS OWN OVERFLOW (for a loss scaler whose state lives on the device: ance_amd.optim.LossScaler).  Same
 * leading arguments, plan and workspace as ance_lamb_step_planned, but d_grad_scale is required and d_found_inf is a required
 * OUTPUT that nobody hands in: the step writes it and is its only reader.
 *   flag     the gradient-norm pass over the products g inv runs with and without max_grad_norm, and the one workgroup that adds its
 *            per-chunk fp64 sums (in the fixed chunk order of the clipped step, no atomics) stores, by one thread and an ordinary
 *            store, *d_found_inf = 1.0f when the total is not finite and 0.0f otherwise.  RULE: the flag is set iff some product
 *            g inv is not finite.  (The total is a sum of squares of fp32 values in fp64: the square of the largest fp32 is 1.2e77
 *            and 2^31 chunks of 16,384 such terms stay far inside the fp64 range, so the total is finite exactly when every term
 *            is.)  For any scale >= 1 that is torch's rule -- some g is not finite -- since |inv| <= 1 cannot overflow a finite g.
 *            For a scale below 1 it ALSO catches a finite g whose unscaled product overflows, which torch's check (of g itself)
 *            lets through into the moments.
 *   skip     every later kernel of the call reads the flag as ance_lamb_step_planned reads d_found_inf: on a non-finite total no
 *            bit of any p, m, v changes, *d_skipped grows by one, d_out takes the rows of d_prev_out ((0, 0, 1) without it; it may
 *            be d_out itself) and *d_grad_norm (when clipping) holds the inf / NaN norm.
 *   no clip  max_grad_norm == 0: the clip factor is not applied, d_grad_norm may be null and only the flag is taken from the total.
 * With a finite total the results have the bits of ance_lamb_step_planned called with the same d_grad_scale and a d_found_inf of 0.
 * Five launches with or without the clip (gnorm, total + flag, pass 1, reduce, pass 2), capturable like the planned step.
 * Workspace: ance_lamb_amp_workspace_bytes in both cases (the per-chunk fp64 area is used without the clip too).  Refuses
 * (ANCE_E_INVALID, before any launch) what ance_lamb_step_planned refuses, a null d_grad_scale and a null d_found_inf. */
int ance_lamb_step_scaled(int n_tensors, int n_groups, int64_t n_chunks, int adam, double max_grad_norm, const float *d_grad_scale,
                          float *d_found_inf, const float *d_prev_out, float *d_grad_norm, int64_t *d_skipped, float *d_out,
                          void *d_workspace, size_t workspace_bytes, void *stream);

/* The dynamic loss scale's update (csrc/loss_scale.hip): the arithmetic of torch._amp_update_scale_, which
 * torch.amp.GradScaler.update() runs, roundings included, on three DEVICE scalars -- *d_scale fp32, *d_growth_tracker int32,
 * *d_found_inf fp32 (e.g. what ance_*_step_scaled left).  !(*d_found_inf == 0) (NaN included):
 * scale <- float32(float64(scale) * backoff_factor), tracker <- 0.  Otherwise n = tracker + 1; at n == growth_interval
 * scale <- float32(float64(scale) * growth_factor) unless that is not finite (the scale is then kept) and tracker <- 0; else
 * tracker <- n.  One launch of one thread, no host synchronisation, capturable.  Refuses (ANCE_E_INVALID, before the launch) a null
 * or unaligned (4 B) pointer, a factor that is not a positive finite number and growth_interval < 1. */
int ance_loss_scale_update(float *d_scale, int32_t *d_growth_tracker, const float *d_found_inf, double growth_factor,
                           double backoff_factor, int32_t growth_interval, void *stream);

/* transformers' get_linear_schedule_with_warmup as one launch on device scalars (csrc/lr_schedule.hip): *d_n += 1, then
 * d_lrs[g] = d_base_lrs[g] * lambda(*d_n) in fp64 for every group, lambda(n) = n / max(1, warm) below warm, else
 * max(0, (total - n) / max(1, total - warm)): the values torch.optim.lr_scheduler.LambdaLR holds after its step(), bit for bit.
 * d_n is a DEVICE int64, the two arrays DEVICE fp64 [n_groups]; the entries of d_lrs are what the plans' d_lrs point to. */
int ance_linear_warmup_step(int64_t *d_n, const double *d_base_lrs, double *d_lrs, int n_groups, int64_t num_warmup_steps,
                            int64_t num_training_steps, void *stream);

/* ---------------------------------------------------------------------------------------------
 * Fused multi-tensor AdamW step (csrc/adamw.hip; transformers 2.3.0 optimization.py AdamW.step, which drivers/run_ann_dpr.py
 * trains with by default and run_ann.py / run_warmup.py with --optimizer adamW).  Per tensor p with gradient g, state m, v, a
 * DEVICE step counter and its group's lr, beta1, beta2, eps, wd:
 *   g' = g [inv, then coef: below]
 *   m <- beta1 m + (1 - beta1) g' ;  v <- beta2 v + (1 - beta2) g' g'
 *   t  = *step + 1
 *   ss = float32(lr sqrt(1 - beta2^t) / (1 - beta1^t))   in fp64 on the device; float32(lr) when correct_bias == 0
 *   p <- p - ss (m / (sqrt(v) + eps))
 *   p <- p + float32(-lr wd) p   when wd > 0: on the UPDATED p -- the decay comes after the update (torch.optim.AdamW decays
 *                                before it, and puts eps inside the bias correction: it is another arithmetic)
 *   *step <- t
 * beta1, beta2, 1 - beta1, 1 - beta2 and eps enter the moment updates rounded to fp32 as torch rounds a scalar; ss and the decay
 * factor are formed from the doubles.  *step is an fp32 scalar per tensor (exact up to 2^24 steps): tensors of one call may
 * carry different counts and each uses its own bias correction.
 *   clip     max_grad_norm != 0: the 2-norm of all gradients -> *d_grad_norm and coef = min(max_grad_norm / (total + 1e-6), 1)
 *            exactly as ance_lamb_step_clipped forms them; g' = g coef.
 *   unscale  d_grad_scale != NULL: inv = (float)(1.0 / (double)*d_grad_scale) formed on the device; g' = (g inv) coef, two fp32
 *            roundings in that order; the norm is taken over the products g inv.  The gradients in memory are never rewritten.
 *   skip     d_found_inf != NULL and !(*d_found_inf == 0) (NaN skips too): no bit of any p, m, v or *step changes -- every
 *            workgroup returns before any store -- and *d_skipped (DEVICE int64, nullable) grows by one.  *d_grad_norm is still
 *            written when clipping.  The next step therefore uses the bias correction of the steps that were applied.
 * Launches: two without clipping (a per-tensor kernel that forms t, ss and the decay factor and advances *step; one elementwise
 * pass, 28 bytes per element), three with it (the gradient-norm pass in front, 32 bytes per element; its total shares the
 * per-tensor launch).  No atomics, a fixed summation order, no host synchronisation: the same inputs give the same bits.
 * Tables, staging and workspace rules as ance_lamb_step; the groups are AnceLambGroup rows.  numel == 0 is allowed (any pointers:
 * that tensor's step is neither read nor written).  n_tensors == 0: nothing is enqueued.  Refuses (ANCE_E_INVALID, before any copy
 * or launch) everything ance_lamb_step_amp refuses (it has no d_out) and a null step of a tensor with numel > 0. */
typedef struct AnceAdamwTensor {
    float *p;                     /* parameter, updated in place                                  */
    const float *g;               /* gradient                                                     */
    float *m, *v;                 /* exp_avg, exp_avg_sq, updated in place                        */
    float *step;                  /* DEVICE fp32 scalar: applied steps, advanced in place         */
    int64_t numel;
    int32_t group, reserved;
} AnceAdamwTensor;
/* Bytes of workspace ance_adamw_step needs (0: invalid); larger with clip != 0. */
size_t ance_adamw_workspace_bytes(int n_tensors, int n_groups, int64_t total_numel, int clip);
int ance_adamw_step(const AnceAdamwTensor *h_tensors, int n_tensors, const AnceLambGroup *h_groups, int n_groups, int correct_bias,
                    double max_grad_norm,            /* 0: no clipping; else positive finite */
                    const float *d_grad_scale,       /* nullable: no unscale */
                    const float *d_found_inf,        /* nullable: never skip */
                    float *d_grad_norm,              /* required iff max_grad_norm != 0 */
                    int64_t *d_skipped,              /* nullable */
                    void *d_workspace, size_t workspace_bytes, void *stream);
/* The resident plan of an AdamW step, as ance_lamb_plan_*: h_tables of ance_adamw_plan_table_bytes bytes, a workspace of
 * ance_adamw_workspace_bytes(.., clip) bytes with the tables at its head, and a step that enqueues only its kernels (2, or 3 with
 * max_grad_norm != 0).  With a group's d_lr the per-tensor kernel forms ss and -lr wd from *d_lr in fp64 exactly as from the host
 * double. */
long long ance_debug_staging_sends(void); /* table uploads through the shared pinned staging pool so far (the unplanned steps') */
size_t ance_adamw_plan_table_bytes(int n_tensors, int n_groups, int64_t total_numel);
int ance_adamw_plan_build(const AnceAdamwTensor *h_tensors, int n_tensors, const AnceLambGroup *h_groups, const double *const *d_lrs,
                          int n_groups, void *h_tables, size_t h_tables_bytes, int64_t *n_chunks_out, size_t *table_bytes_out);
int ance_adamw_step_planned(int n_tensors, int n_groups, int64_t n_chunks, int correct_bias, double max_grad_norm,
                            const float *d_grad_scale, const float *d_found_inf, float *d_grad_norm, int64_t *d_skipped,
                            void *d_workspace, size_t workspace_bytes, void *stream);
/* The planned AdamW step that finds its own overflow: the flag, its rule, the skip and the refusals of ance_lamb_step_scaled (there
 * is no d_out).  The per-tensor workgroup forms the gradient total and stores *d_found_inf BEFORE it decides whether the step counts
 * advance: on a non-finite total no bit of any p, m, v or *step changes and *d_skipped grows by one.  With a finite total the
 * results have the bits of ance_adamw_step_planned with the same d_grad_scale and a d_found_inf of 0.  Three launches with or
 * without the clip (gnorm, total + flag + per-tensor scalars, update).  Workspace: ance_adamw_workspace_bytes(.., clip = 1) in both
 * cases. */
int ance_adamw_step_scaled(int n_tensors, int n_groups, int64_t n_chunks, int correct_bias, double max_grad_norm,
                           const float *d_grad_scale, float *d_found_inf, float *d_grad_norm, int64_t *d_skipped,
                           void *d_workspace, size_t workspace_bytes, void *stream);

/* ---------------------------------------------------------------------------------------------
 * Training batches gathered on the device (csrc/batch_gather.hip): what the reference's loaders build per item in Python
 * (data/msmarco_data.py:275-362, data/DPR_data.py:276-344), collate, copy and cast (drivers/run_ann.py:237-254).  A segment is one
 * tower's share of a batch: item first + b of its index names the record whose tokens become row b of its outputs.
 *   d_records  the token cache file's bytes on the device: n_records rows of 4 + 4 L bytes (big-endian passage_len, L little-endian
 *              int32), 4-byte aligned
 *   d_index    int64 [n_index]: one record index per item of the plan.  The host validates it when the plan is made; the kernel
 *              clamps every value into [0, n_records), so no value makes it read outside the records
 *   mask_rule  ANCE_GATHER_MASK_LENGTH: 1 x min(passage_len, L) then 0 (MS MARCO); ANCE_GATHER_MASK_NONZERO: ids != 0 (DPR)
 *   type_rule  ANCE_GATHER_TYPES_ZERO (MS MARCO query, both DPR towers); ANCE_GATHER_TYPES_LENGTH: 1 x min(passage_len, L) then 0
 *   outputs    [B, L] each, every byte written (pad region included).  width ANCE_GATHER_REFERENCE: int32 ids, 1-byte bool mask;
 *              ANCE_GATHER_WIDE: int64 ids and mask (what the trainers' .long() makes).  d_types (nullable): uint8 in both.
 * ONE launch for all segments; no host/device copy, no allocation, no synchronisation.  Refuses (ANCE_E_INVALID, before any launch):
 * a null table or a null pointer other than d_types; n_segs outside 1..3; L < 1; n_records < 1; B < 1; first < 0; first + B past
 * n_index; an unknown mask, type or width code; d_records or an output not 4-byte aligned (int64 outputs and d_index: 8-byte). */
#define ANCE_GATHER_MASK_LENGTH 0
#define ANCE_GATHER_MASK_NONZERO 1
#define ANCE_GATHER_TYPES_ZERO 0
#define ANCE_GATHER_TYPES_LENGTH 1
#define ANCE_GATHER_REFERENCE 0
#define ANCE_GATHER_WIDE 1
typedef struct AnceGatherSegment {
    const void *d_records;
    int64_t n_records;
    const int64_t *d_index;
    int64_t n_index;
    void *d_ids, *d_mask;
    void *d_types;                /* nullable: no token types written */
    int32_t L, mask_rule, type_rule, reserved;
} AnceGatherSegment;
int ance_gather_batch(const AnceGatherSegment *h_segs, int n_segs, int64_t first, int64_t B, int width, void *stream);

/* Packed batches straight from the token caches (csrc/batch_gather_packed.hip): the gather above followed by ance_pack_tokens in
 * every tower, as ONE launch for all towers, with the scan of the lengths moved to the time the pass's plan is made.
 *
 * ance_record_lengths -- int32 d_out [n_records, L / chunk_len], once per cache: entry (r, c) is the length of chunk c of record r.
 *   rule ANCE_GATHER_MASK_LENGTH: len = min(bswap(header), L), chunk c gets clamp(len - c chunk_len, 0, chunk_len);
 *   ANCE_GATHER_MASK_NONZERO: the number of non-zero ids in the chunk (what the lengths of the DPR loaders' mask are, holes
 *   included).  chunk_len == L is the ordinary one-sequence record.  Refuses (ANCE_E_INVALID, before any launch): a null or not
 *   4-byte aligned pointer; n_records < 1; L < 1; chunk_len outside 1 .. 512 or not dividing L; an unknown rule.
 *
 * ance_gather_batch_packed -- a segment is one tower's share of a batch of B items, each C = L / chunk_len sequences:
 *   d_cum      int64 [n_index * C + 1], made with the plan: the exclusive running sum of the sequence lengths (ance_record_lengths
 *              of the records d_index names) in item-then-chunk order.  Sequence s = item * C + c of the batch, s0 = first * C:
 *              off_s = cum[s0 + s] - cum[s0], len_s = clamp(cum[s0 + s + 1] - cum[s0 + s], 0, chunk_len), KEPT iff
 *              off_s + len_s <= rows.  off_s + len_s never decreases, so the dropped sequences are a suffix; T = the rows in use.
 *   outputs    packed_ids, packed_positions [rows]; d_seq_off [B C + 1]; d_seq_kept [B C]; d_dropped: exactly what ance_pack_tokens
 *              writes for the padded batch the segment stands for -- the ids as they are, the positions with their clamps, off_s and
 *              len_s for a kept sequence, T and -1 for a dropped one, T in the last entry, the slack rows T .. rows - 1 as stated
 *              there -- EXCEPT d_dropped, which is STORED, not added to: this batch's number of dropped sequences, by the one lane
 *              of the grid that also stores T (no read-modify-write: the segments share a grid).  No token types are produced.
 *              Every byte of the five outputs is written on every call, and no row >= rows ever.
 *   position_mode, padding_idx, vocab, max_pos   as in AncePackArgs
 *   first, d_first   the first item of the batch; with d_first != NULL it is read from that int64 device scalar when the kernel
 *              starts and `first` is ignored (a cursor that lives on the device: the call can be captured and replayed).  The item
 *              is clamped into [0, n_index] and every read of d_cum and d_index stays inside them whatever the scalar holds; an
 *              item at or beyond n_index is C empty sequences (kept with length 0 if they fit) and reads no record.
 *   The record index is clamped into [0, n_records) and every offset into [0, rows] before an address is formed.
 * ONE launch for all segments; no copy, no allocation, no synchronisation, no atomics.  Refuses (ANCE_E_INVALID, before any launch): a
 * null table or pointer (d_first aside); n_segs outside 1..3; B < 1; without d_first: first < 0 or first + B past n_index; L < 1;
 * chunk_len outside 1 .. 512 or not dividing L; B C above 65535; n_records < 1; n_index < 0; rows < 1; vocab or max_pos < 1; a
 * position_mode other than the two; padding_idx outside -1 .. vocab - 1 (roberta: 0 .. vocab - 1); d_records or an int32 output not
 * 4-byte aligned; d_index, d_cum, d_dropped or d_first not 8-byte aligned. */
typedef struct AncePackedGatherSegment {
    const void *d_records;
    int64_t n_records;
    const int64_t *d_index;
    int64_t n_index;
    const int64_t *d_cum;         /* [n_index * (L / chunk_len) + 1]                              */
    int32_t *packed_ids;          /* [rows] out                                                   */
    int32_t *packed_positions;    /* [rows] out                                                   */
    int32_t *d_seq_off;           /* [B * (L / chunk_len) + 1] out                                */
    int32_t *d_seq_kept;          /* [B * (L / chunk_len)] out                                    */
    int64_t *d_dropped;           /* out: this batch's dropped sequences (stored)                 */
    int32_t L, chunk_len, rows;
    int32_t position_mode;        /* ANCE_EMBED_POSITION_*                                        */
    int32_t padding_idx;          /* -1: none                                                     */
    int32_t vocab, max_pos;
    int32_t reserved;             /* 0 */
} AncePackedGatherSegment;
int ance_record_lengths(const void *d_records, int64_t n_records, int L, int chunk_len, int rule, int32_t *d_out, void *stream);
int ance_gather_batch_packed(const AncePackedGatherSegment *h_segs, int n_segs, int64_t first, int64_t B, const int64_t *d_first,
                             void *stream);

/* Re-reads every ANCE_* tuning knob from the environment (they are otherwise read once per process).  For tests and
 * sweeps that change a knob between two calls; not thread-safe against concurrent searches. */
void ance_reload_env(void);

/*
 * Measurement hook of the two-precision search -- a no-op in the product library; the instrumented kernel builds exist
 * only in the measurement library (`make -C ance_amd/csrc measure` -> libance_amd_measure.so, -DANCE_MEASURE; load it
 * with ANCE_AMD_LIB=<path>).  There: while d_stamps != NULL, the filter kernel runs as its instrumented
 * build and every workgroup of a launch chunk leaves uint64[8] at d_stamps + 8 * blockIdx: ticks of the 100 MHz
 * counter spent in {prologue, fp16 main loop, filter, prune, window waits, hand-over to the re-scoring kernel},
 * then (query tile << 32 | split) and the XCC id it ran on.  The buffer needs 8 * 8 * 2048 bytes.  NULL switches it off.
 */
void ance_debug_search_stamps(void *d_stamps);

/* Introspection for tests / bench: algorithmic FLOPs of the last ance_encode_* call cannot be
 * known without a sync, so the library exposes the pure function instead:
 * F_enc(T) = 169,869,312 T + 36,864 T^2 + 1,179,648 per sequence of T tokens. */
double ance_encoder_flops_per_sequence(int T);

/* ---------------------------------------------------------------------------------------------
 * Host-side post-search stage.  Pure host code, HOST pointers, no GPU work:
 * replaces the per-element Python of GenerateNegativePassaageID
 * (drivers/run_ann_data_gen.py:339-396) and of the ann_training_data_N writer (:314-327).
 *
 * mt_state: uint32[625] = CPython `random.getstate()[1]` (624 Mersenne-Twister words + index).
 * The functions draw exactly what the reference's `random.shuffle` calls would draw and leave the
 * advanced state in place (install it with `random.setstate`), so a seeded run produces the
 * reference's files byte for byte.
 * ------------------------------------------------------------------------------------------- */

/* out[0..n) = list(range(n)) after random.shuffle (the line order of ann_training_data_N, :316-317). */
int ance_host_py_shuffle(uint32_t *mt_state, int64_t n, int64_t *out);

/*
 * Negative selection for every query row r with active[r] != 0 (query id in effective_q_id):
 * candidates = I[r, order] with order = random.shuffle(range(k)) (select_topk == 0; one shuffle per
 * active row, row order) or I[r, :negative_sample+1] (select_topk != 0, --ann_measure_topk_mrr);
 * walk them as the reference does: pid = p2id[row] (negative row ids index from the end like
 * NumPy), skip pid == pos_pid[r] (rank <= 10 adds 1/rank to *out_mrr), skip pids already taken,
 * stop at negative_sample.  out_neg [nq, negative_sample] (-1 padded), out_cnt [nq] (-1 for
 * inactive rows).  *out_mrr = the reference's `mrr` accumulator (before the division), summed in
 * its order.  n_threads <= 0: up to 16.  mt_state may be NULL when select_topk != 0.
 */
int ance_host_select_negatives(uint32_t *mt_state, const int64_t *I, int64_t nq, int k, const int64_t *p2id,
                               int64_t n_rows, const int64_t *pos_pid, const uint8_t *active, int negative_sample,
                               int select_topk, int n_threads, int64_t *out_neg, int32_t *out_cnt, double *out_mrr);

/*
 * Writes "qid \t pos_pid \t neg,neg,...\n" for rows order[0..n_order) whose src_row[row] >= 0, taking
 * the negatives of row src_row[row] (the reference keys them by query id, so a repeated id shows
 * the negatives of its last row).  *out_lines = lines written.
 */
int ance_host_write_ann_training(const char *path, const int64_t *order, int64_t n_order, const int64_t *qid,
                                 const int64_t *pos_pid, const int64_t *src_row, const int64_t *neg, const int32_t *cnt,
                                 int negative_sample, int64_t *out_lines);

#ifdef __cplusplus
}
#endif
#endif /* ANCE_AMD_H */
