// Dual-encoder forward for gfx950: RoBERTa-base / BERT-base stack + ANCE head, variable-length
// packed (pad tokens are never materialised).  Replaces, on the reference's hot path,
//   model.module.query_emb / body_emb  (drivers/run_ann_data_gen.py:171-180)
//   = transformers RobertaModel/BertModel forward + embeddingHead + norm (model/models.py:149-157,
//     165-199, 235-259).
//
// Three arithmetic modes (AnceEncoderDesc.precision), one forward each: forward_fp16, forward_split, forward_fp32.  encode_impl
// plans the micro-batches (<= max_tokens real tokens; encoder_plan.h), packs their tokens and hands each one to the forward of the
// handle's mode on one of two lanes (activation sets) and streams.  The small kernels the forwards launch: encoder_kernels.h.
//
// fp16 mode: fp16 MFMA operands, fp32 accumulation, fp32 LayerNorm statistics and softmax.  The residual stream of a layer is
// never normalised by a kernel of its own ("LayerNorm without a kernel"): a LayerNorm pass would read 3 KB and write 1.5 KB per
// token at the HBM roofline for arithmetic every consumer can do on the fly.  Instead
//   * the RES GEMM epilogue (EPI_RESLN) writes its output row v as an fp16 pair (hi = fp16(v), lo = fp16(v - hi): the same
//     3 KB the fp32 row took, 22 mantissa bits) and the (mean, M2) of every 64-column slice (96 bytes per row);
//   * the consumer GEMMs take hi AS IT IS for their token operand and finish the normalisation algebraically:
//       LN(v) W^T + b = r (v (gamma (.) W)^T - mu c) + (b + W beta),   c[n] = sum_k fp16(gamma_k W[n][k])
//     with gamma folded into the fp16 weight when it is loaded (fold_weight_kernel), c summed over the ROUNDED weights (so that
//     the identity is exact for the products the MFMA actually forms) and b' in fp32;
//   * every consumer combines the 12 slices of a row into (mean, rstd) itself (Chan): a GEMM tile gets the partials of
//     its 256 tokens, with its bias / csum / gamma / beta vectors, by LDS-DMA ahead of its main loop and combines them
//     when its epilogue starts -- there is no LayerNorm kernel and no statistics kernel at all;
//   * the consumers of the fp32 value (next RES epilogue, [CLS] gather, head) recompute LN(hi + lo) from the pair.
// Per layer, x_b = the (hi, lo) pair of the previous layer's pre-LayerNorm output (or of the embeddings, embed_kernel):
//   QK   = LN(x_b) Wqk^T + b          (gemm EPI_QK_F, Q pre-scaled by log2(e) / 8)   [T, 1536] f16
//   V^T  = Wv LN(x_b)^T + b           (gemm EPI_VT_F, key-contiguous)                 [768, cols] f16
//   ctx  = softmax(Q K^T) V           (attention.hip)                                 [T, 768] f16
//   x_a  = ctx Wo^T + b + LN(x_b)     (gemm EPI_RESLN: pair + slice statistics)       [T, 768] (hi, lo)
//   f    = gelu(LN(x_a) W1^T + b)     (gemm EPI_GELU_F)                               [T, 3072] f16
//   x_b  = f W2^T + b + LN(x_a)       (gemm EPI_RESLN)                                [T, 768] (hi, lo)
// then  emb = LayerNorm(Wh LN(x_b)[cls] + bh)  (fp32: head_gemm_kernel, head_ln_kernel)  or LN(x_b)[cls] for DPR's BERT
// (head_kernel).  The last layer runs its Q projection and everything after the attention on the [CLS] rows only (the CLS-only
// tail; ANCE_CLS_TAIL=0 runs it in full, bit-identically).  Rounding points against the fp32 forward: the token operand is
// fp16(v) instead of fp16(LN(v)) -- the same relative rounding of every element, taken before the mean is removed -- and
// gamma (.) W is rounded once instead of W.  Measured parity: DESIGN.md 4.
//
// SPLIT mode (the default; round 4-5): an fp32-GRADE result on the fp16 matrix cores instead of the sixteenth of their rate the
// fp32-input ones run at (precise32.h).  Every GEMM operand is an fp16 pair row (common.h), a product is three fp16 MFMAs per
// k-step on the pipeline of the fp16 mode (gemm256_f16.hip: gemm256_split_kernel), with the same LayerNorm fold; the attention
// runs on fp32 Q | K | V (attention.hip: attention_split_kernel), the GELU is the exact erf form and the head is fp32 -- the
// reference's arithmetic.  Stated tolerance 2e-5 (tests/test_split_model.py: 3.3e-6 on the CPU model).
//
// fp32 mode: fp32 operands throughout (precise32.h), the audit path.
#include <stdlib.h>
#include <type_traits>
#include <vector>

#include "attention.h"
#include "common.h"
#include "encoder_kernels.h"
#include "encoder_plan.h"
#include "gemm_f16.h"
#include "precise32.h"

namespace ance {
namespace {

// The hidden width H is a template parameter of every kernel and forward that depends on it: 768 (RoBERTa-base, BERT-base, SEED)
// or 1024 (RoBERTa-large: ANCE_ARCH_ROBERTA with the head only, desc_ok).  with_hidden calls f with the width of a descriptor as
// a compile-time constant (constexpr int H = decltype(h)::value): the one place that picks a template instance from desc.hidden.
template <typename F>
auto with_hidden(int hidden, F &&f) {
    return hidden == 1024 ? f(std::integral_constant<int, 1024>()) : f(std::integral_constant<int, 768>());
}

constexpr int S_CAP_MAX = 8192; // sequences per micro-batch
constexpr int FETCH_CHUNK = 262144;
constexpr int MAX_LANES = 2;     // activation sets / internal streams (3 and 4 lanes measured no gain: DESIGN.md 9)

// ------------------------------------------------------------------------------- host layout --

// AnceEncoderDesc.precision names the arithmetic of a handle; ANCE_PRECISION_DEFAULT defers to these environment switches.
// ANCE_ENCODER_PRECISE=1: the fp32 path of precise32.h (the arena and workspace sizes grow by the fp32 weights and activations, so
// the size queries resolve the mode the same way)
bool precise_env() {
    const char *p = getenv("ANCE_ENCODER_PRECISE");
    return p && p[0] == '1';
}

// The encoder arithmetic of a handle, read from the environment when it is created (and by the two size queries: the modes differ
// in arena and workspace size).  DEFAULT = the split (fp32-grade) path: the reference runs its encoder in fp32
// (drivers/run_ann_data_gen.py:158,176-180, model/models.py:149-157 -- no .half()), and it is the mode in which the refresh
// reproduces the reference's negative ids (tests/test_gpu_config1.py).  ANCE_ENCODER_PRECISE=1 selects the fp32-operand audit
// path and wins over everything; ANCE_ENCODER_FP16=1 (or ANCE_ENCODER_SPLIT=0) selects the fp16-operand fast mode (3e-3 on the
// embeddings, 2.2 x the throughput); ANCE_ENCODER_SPLIT=1 names the default explicitly and wins over ANCE_ENCODER_FP16.
bool split_env() {
    if (precise_env()) return false;
    const char *s = getenv("ANCE_ENCODER_SPLIT");
    if (s && s[0] == '1') return true;
    if (s && s[0] == '0') return false;
    const char *f = getenv("ANCE_ENCODER_FP16");
    return !(f && f[0] == '1');
}

// The arithmetic of a descriptor: AnceEncoderDesc.precision, or -- ANCE_PRECISION_DEFAULT -- what the environment says.
int resolve_precision(const AnceEncoderDesc *d) {
    if (d->precision == ANCE_PRECISION_SPLIT || d->precision == ANCE_PRECISION_FP16 || d->precision == ANCE_PRECISION_FP32)
        return d->precision;
    if (precise_env()) return ANCE_PRECISION_FP32;
    return split_env() ? ANCE_PRECISION_SPLIT : ANCE_PRECISION_FP16;
}

// Per-layer weights.  Every mode's buffers have a place in the arena (layout_weights), but ance_encoder_create fills only those the
// handle's forward reads: fp16 mode the fp16 / folded ones, split mode the *_s ones, fp32 mode the *32 ones and b1; all modes bo,
// b2 and the LayerNorm parameters.
struct LayerW {
    _Float16 *wqk, *wv, *wo, *w1, *w2;  // fp16 path
    _Float16 *wqkv_s, *wo_s, *w1_s, *w2_s;  // split path: pair rows [hi (K) | lo' (K)]
    float *bqkv_s, *cqkv_s, *b1_s, *c1_s;   // split path: folded biases and row sums
    float *sc_s;  // split path: [0..3] max |g (.) W| of Wqkv, Wo, W1, W2 as float bits (weight load), [4..7] the inverse of their power-of-two scales
    float *bqk, *bv, *bo, *b1, *b2, *ln1w, *ln1b, *ln2w, *ln2b;
    float *cqk, *cv, *c1;  // folded LayerNorm: per-feature sums of the folded fp16 weight rows
    float *wqkv32, *bqkv32, *wo32, *w132, *w232;  // fp32 path only
};

struct Arena {
    size_t off = 0;
    char *base = nullptr;
    template <typename T>
    T *take(size_t n) {
        T *p = base ? reinterpret_cast<T *>(base + off) : nullptr;
        off = align_up(off + n * sizeof(T), 256);
        return p;
    }
};

}  // namespace
}  // namespace ance

using namespace ance;

struct AnceEncoder {
    AnceEncoderDesc d;
    // weights
    float *word, *pos, *type0, *eln_w, *eln_b;
    std::vector<LayerW> layers;
    float *head_w, *head_b, *norm_w, *norm_b;
    // workspace: two independent "lanes" (activation sets) so that consecutive micro-batches can run
    // on two streams -- the MFMA-bound GEMMs of one overlap the HBM-bound LayerNorm / attention /
    // epilogue phases of the other
    int tcap, vcap, scap;
    int *lens_fetch;
    unsigned *faults;  // device: [0] out-of-range stores of the split mode, [1] NaN output rows
    struct Lane {
        int *seq_off, *seq_vtcol, *seq_len, *tok_id, *tok_pos, *tok_vtcol;
        int4 *desc;  // attention descriptors in length-bucket order
        // The activation buffers as each mode's forward sees them (layout_workspace: three views of the same bytes).  xa / xb: the
        // two pre-LayerNorm streams -- attention block output / FFN block output (or embeddings) -- as Rows of the mode's form.
        // cls(S_pad): the scratch of the CLS-only tail -- S_pad compact [CLS] rows and their partials, at the start of the FFN
        // activation buffer (dead until FFN1 of the last layer, which runs after the scratch's last reader).
        struct Fp16 {
            Rows<FORM_PLANES> xa, xb;
            _Float16 *qk, *vt, *ctx, *ffn;  // Q | K, V^T, attention output, FFN activation
            Rows<FORM_PLANES> cls(int S_pad, int H) const {
                _Float16 *const lo = ffn + (size_t)S_pad * H;
                return {ffn, lo, reinterpret_cast<float *>(lo + (size_t)S_pad * H)};
            }
        } f16;
        struct Split {
            Rows<FORM_PAIR> xa, xb;
            float *qkv;           // fp32 Q | K | V
            _Float16 *ctx, *ffn;  // pair rows of the attention output / FFN activation
            Rows<FORM_PAIR> cls(int S_pad, int H) const { return {ffn, reinterpret_cast<float *>(ffn + (size_t)S_pad * 2 * H)}; }
        } sp;
        struct Fp32 {
            Rows<FORM_F32> xa, xb;  // (stats: xb's, of the last layer)
            float *h, *ha, *qkv, *ctx, *ffn;  // hidden states LN(xb) / LN(xa), Q | K | V, attention output, FFN activation
        } f32;
    } lane[MAX_LANES];
    int n_lanes;
    hipStream_t side[MAX_LANES];
    hipEvent_t ev_fork, ev_join[MAX_LANES];
    std::vector<int32_t> host_lens;
    bool cls_tail;  // run the last layer's post-attention part on the [CLS] rows only (ANCE_CLS_TAIL=0 disables)
    int mode;       // ANCE_PRECISION_FP16 / SPLIT / FP32 (resolve_precision)
};

namespace {

// Shapes (include/ance_amd.h): head dimension 64 and hidden 768 (every arch), or hidden 1024 for RoBERTa with the ANCE head only --
// DPR's BiEncoder is BERT-base and SEED's config is base width; a head-less large tower would change the output width.  At 1024 the
// FFN GEMMs also need intermediate % 256 (N of FFN1 is a whole number of 256-column tiles).
bool desc_ok(const AnceEncoderDesc *d) {
    if (!d || d->n_heads <= 0 || d->hidden != 64 * d->n_heads || (d->hidden != 768 && d->hidden != 1024)) return false;
    if (d->hidden == 1024 && (d->arch != ANCE_ARCH_ROBERTA || d->has_head != 1 || d->intermediate % 256 != 0)) return false;
    return d->intermediate > 0 && d->intermediate % 128 == 0 &&
           d->n_layers >= 1 && d->vocab_size > 0 && d->max_position > 0 && d->max_seq_len >= 1 &&
           d->max_seq_len <= 512 && d->max_tokens >= 512 && d->max_tokens % 256 == 0 && d->precision >= 0 && d->precision <= 3 &&
           (d->arch == ANCE_ARCH_ROBERTA || d->arch == ANCE_ARCH_BERT || d->arch == ANCE_ARCH_SEED);
}

void layout_weights(const AnceEncoderDesc *d, Arena &a, AnceEncoder *e) {
    const size_t I = d->intermediate;
    const int H = d->hidden, HP = 2 * H;
    const int mode = resolve_precision(d);
    float *word = a.take<float>((size_t)d->vocab_size * H);
    float *pos = a.take<float>((size_t)d->max_position * H);
    float *type0 = a.take<float>(H);
    float *ew = a.take<float>(H), *eb = a.take<float>(H);
    if (e) { e->word = word; e->pos = pos; e->type0 = type0; e->eln_w = ew; e->eln_b = eb; e->layers.resize(d->n_layers); }
    for (int i = 0; i < d->n_layers; ++i) {
        LayerW w;
        w.wqk = a.take<_Float16>((size_t)2 * H * H);
        w.bqk = a.take<float>(2 * H);
        w.wv = a.take<_Float16>((size_t)H * H);
        w.bv = a.take<float>(H);
        w.wo = a.take<_Float16>((size_t)H * H);
        w.bo = a.take<float>(H);
        w.ln1w = a.take<float>(H);
        w.ln1b = a.take<float>(H);
        w.w1 = a.take<_Float16>(I * H);
        w.b1 = a.take<float>(I);
        w.w2 = a.take<_Float16>((size_t)H * I);
        w.b2 = a.take<float>(H);
        w.ln2w = a.take<float>(H);
        w.ln2b = a.take<float>(H);
        w.cqk = a.take<float>(2 * H);
        w.cv = a.take<float>(H);
        w.c1 = a.take<float>(I);
        w.wqkv_s = w.wo_s = w.w1_s = w.w2_s = nullptr;
        w.bqkv_s = w.cqkv_s = w.b1_s = w.c1_s = w.sc_s = nullptr;
        if (mode == ANCE_PRECISION_SPLIT) {
            w.sc_s = a.take<float>(8);
            w.wqkv_s = a.take<_Float16>((size_t)3 * H * HP);
            w.bqkv_s = a.take<float>(3 * H);
            w.cqkv_s = a.take<float>(3 * H);
            w.wo_s = a.take<_Float16>((size_t)H * HP);
            w.w1_s = a.take<_Float16>(I * HP);
            w.b1_s = a.take<float>(I);
            w.c1_s = a.take<float>(I);
            w.w2_s = a.take<_Float16>((size_t)H * 2 * I);
        }
        w.wqkv32 = w.bqkv32 = w.wo32 = w.w132 = w.w232 = nullptr;
        if (mode == ANCE_PRECISION_FP32) {
            w.wqkv32 = a.take<float>((size_t)3 * H * H);
            w.bqkv32 = a.take<float>(3 * H);
            w.wo32 = a.take<float>((size_t)H * H);
            w.w132 = a.take<float>(I * H);
            w.w232 = a.take<float>((size_t)H * I);
        }
        if (e) e->layers[i] = w;
    }
    float *hw = nullptr, *hb = nullptr, *nw = nullptr, *nb = nullptr;
    if (d->has_head) {
        hw = a.take<float>((size_t)HEAD_OUT * H);
        hb = a.take<float>(HEAD_OUT);
        nw = a.take<float>(HEAD_OUT);
        nb = a.take<float>(HEAD_OUT);
    }
    if (e) { e->head_w = hw; e->head_b = hb; e->norm_w = nw; e->norm_b = nb; }
}

void layout_workspace(const AnceEncoderDesc *d, Arena &a, AnceEncoder *e) {
    const int tcap = d->max_tokens;
    const int scap = tcap < S_CAP_MAX ? tcap : S_CAP_MAX;
    const int vcap = (int)align_up((size_t)tcap + tcap / 4 + 256, 256);
    const int mode = resolve_precision(d);
    const size_t H = d->hidden, I = d->intermediate;
    unsigned *faults = a.take<unsigned>(64);  // [0] out-of-range stores of the split mode, [1] NaN output rows (ance_encoder_range_faults)
    int *lens_fetch = a.take<int>(FETCH_CHUNK);
    if (e) { e->tcap = tcap; e->scap = scap; e->vcap = vcap; e->lens_fetch = lens_fetch; e->faults = faults; }
    // an fp16 pair -- two planes or a pair row -- is as many bytes as the fp32 row: such buffers are taken as fp32 rows
    auto halves = [](float *p) { return reinterpret_cast<_Float16 *>(p); };
    for (int ln = 0; ln < MAX_LANES; ++ln) {
        AnceEncoder::Lane L;
        L.seq_off = a.take<int>(scap + 1); L.seq_vtcol = a.take<int>(scap); L.seq_len = a.take<int>(scap);
        L.tok_id = a.take<int>(tcap); L.tok_pos = a.take<int>(tcap); L.tok_vtcol = a.take<int>(tcap);
        L.desc = a.take<int4>(scap);
        float *const preB = a.take<float>(tcap * H), *const preA = a.take<float>(tcap * H);
        float *const statsA = a.take<float>((size_t)tcap * 2), *const statsB = a.take<float>((size_t)tcap * 2);
        (void)a.take<_Float16>(tcap * H);  // (read by no mode: kept so that the workspace layout does not change)
        _Float16 *const qk16 = a.take<_Float16>(tcap * 2 * H);
        _Float16 *const vt16 = a.take<_Float16>(H * vcap);
        _Float16 *const ctx16 = a.take<_Float16>(tcap * H);
        _Float16 *const ffn16 = a.take<_Float16>(tcap * I);
        float *const partA = a.take<float>((size_t)tcap * PART_FLOATS), *const partB = a.take<float>((size_t)tcap * PART_FLOATS);
        const bool f32 = mode == ANCE_PRECISION_FP32, wide = f32 || mode == ANCE_PRECISION_SPLIT;  // (fp32 rows or pair rows)
        float *const h32 = f32 ? a.take<float>(tcap * H) : nullptr, *const ha32 = f32 ? a.take<float>(tcap * H) : nullptr;
        float *const qkv32 = wide ? a.take<float>(tcap * 3 * H) : nullptr, *const ctx32 = wide ? a.take<float>(tcap * H) : nullptr;
        float *const ffn32 = wide ? a.take<float>(tcap * I) : nullptr;
        if (!e) continue;  // (a size query)
        // fp16 mode: the two planes of a stream share the fp32 row's bytes, hi first
        L.f16 = {{halves(preA), halves(preA) + tcap * H, partA}, {halves(preB), halves(preB) + tcap * H, partB}, qk16, vt16, ctx16, ffn16};
        L.sp = {{halves(preA), partA}, {halves(preB), partB}, qkv32, halves(ctx32), halves(ffn32)};
        L.f32 = {{preA, statsA}, {preB, statsB}, h32, ha32, qkv32, ctx32, ffn32};
        e->lane[ln] = L;
    }
}

void cvt16(const void *src, _Float16 *dst, size_t n, hipStream_t st) {
    const unsigned blocks = (unsigned)((n + 256 * 8 - 1) / (256 * 8));
    hipLaunchKernelGGL(cvt_f32_f16_kernel, dim3(blocks > 4096 ? 4096 : (blocks ? blocks : 1)), dim3(256), 0, st,
                       (const float *)src, dst, n);
}
void cpy32(const void *src, float *dst, size_t n, hipStream_t st) {
    (void)hipMemcpyAsync(dst, src, n * sizeof(float), hipMemcpyDeviceToDevice, st);
}

// The output of the encoder from the last layer's LayerNorm of the [CLS] rows of the stream `pre`: the embeddingHead as one MFMA
// GEMM + its LayerNorm (has_head), or those rows as they are (DPR's BERT).  compact: row s already is the [CLS] row of sequence s.
template <int H, int FORM>
void encoder_output(AnceEncoder *e, const AnceEncoder::Lane &LN, hipStream_t st, const MicroPlan &mb, float *out,
                    const Rows<FORM> &pre, int compact) {
    const AnceEncoderDesc &D = e->d;
    const LayerW &WL = e->layers[D.n_layers - 1];
    ProfScope ps(PC_HEAD, st);
    if (D.has_head) {
        hipLaunchKernelGGL((head_gemm_kernel<H, FORM>), dim3((mb.S + 31) / 32, HEAD_OUT / 128), dim3(256), HEAD_LDS_BYTES<H>, st, pre,
                           D.ln_eps, WL.ln2w, WL.ln2b, LN.seq_off, compact, mb.S, e->head_w, e->head_b, out);
        hipLaunchKernelGGL(head_ln_kernel, dim3((mb.S + 3) / 4), dim3(256), 0, st, out, mb.S, e->norm_w, e->norm_b, e->faults);
    } else {
        hipLaunchKernelGGL((head_kernel<H, FORM>), dim3(mb.S), dim3(256), 0, st, pre, D.ln_eps, WL.ln2w, WL.ln2b, LN.seq_off, compact,
                           out, e->faults);
    }
}

// ---- fp32 mode (precise32.h): plain sequence of fp32 kernels, every layer on every token ----
template <int H>
int forward_fp32(AnceEncoder *e, const AnceEncoder::Lane &LN, hipStream_t st, const MicroPlan &mb, float *out) {
    const AnceEncoderDesc &D = e->d;
    const AnceEncoder::Lane::Fp32 &V = LN.f32;
    const int I = D.intermediate, T = mb.T, Tpad = mb.Tpad;
    float *const no_stats = nullptr;
    {
        ProfScope pe(PC_EMBED, st);
        hipLaunchKernelGGL(embed32_kernel<H>, dim3(Tpad / 4), dim3(256), 0, st, LN.tok_id, LN.tok_pos, Tpad, e->word, e->pos,
                           e->type0, D.vocab_size, D.max_position, V.xb.x);
        hipLaunchKernelGGL(ln32_kernel<H>, dim3(Tpad / 4), dim3(256), 0, st, V.xb.x, Tpad, e->eln_w, e->eln_b, D.ln_eps, V.h, no_stats);
    }
    for (int li = 0; li < D.n_layers; ++li) {
        const LayerW &W = e->layers[li];
        const bool last = li == D.n_layers - 1;
        if (ProfScope ps(PC_GEMM_QK, st, 2.0 * T * (3.0 * H) * H);
            int rc = launch_gemm32(P_EPI_BIAS, V.h, H, W.wqkv32, H, W.bqkv32, nullptr, 0, V.qkv, 3 * H, Tpad, 3 * H, H, st))
            return rc;
        if (ProfScope ps(PC_ATTN, st); int rc = launch_attention32(V.qkv, V.ctx, LN.seq_off, mb.S, D.n_heads, st)) return rc;
        if (ProfScope ps(PC_GEMM_OUT, st, 2.0 * T * (double)H * H);
            int rc = launch_gemm32(P_EPI_RES, V.ctx, H, W.wo32, H, W.bo, V.h, H, V.xa.x, H, Tpad, H, H, st))
            return rc;
        {
            ProfScope ps(PC_LN, st);
            hipLaunchKernelGGL(ln32_kernel<H>, dim3(Tpad / 4), dim3(256), 0, st, V.xa.x, Tpad, W.ln1w, W.ln1b, D.ln_eps, V.ha, no_stats);
        }
        if (ProfScope ps(PC_GEMM_FFN1, st, 2.0 * T * (double)I * H);
            int rc = launch_gemm32(P_EPI_GELU, V.ha, H, W.w132, H, W.b1, nullptr, 0, V.ffn, I, Tpad, I, H, st))
            return rc;
        if (ProfScope ps(PC_GEMM_FFN2, st, 2.0 * T * (double)I * H);
            int rc = launch_gemm32(P_EPI_RES, V.ffn, I, W.w232, I, W.b2, V.ha, H, V.xb.x, H, Tpad, H, I, st))
            return rc;
        {
            ProfScope ps(PC_LN, st);
            hipLaunchKernelGGL(ln32_kernel<H>, dim3(Tpad / 4), dim3(256), 0, st, V.xb.x, Tpad, W.ln2w, W.ln2b, D.ln_eps, V.h,
                               last ? V.xb.stats : no_stats);
        }
    }
    encoder_output<H>(e, LN, st, mb, out, V.xb, 0);
    return ANCE_OK;
}

// ---- GemmArgs of the folded forwards' GEMM roles (gemm_f16.h; a field that is not named stays zero) ----
// One constructor per role, for both stream forms: planes (fp16 mode; operand rows of K halves) or pair rows (split mode; operand rows
// of 2 K halves, the weight's scale wscale_inv and the range guard).  Which fields each epilogue reads: tests/test_gpu_gemm_fold.py,
// ance_debug_gemm_hw.

// Folded projection (EPI_QK_F / EPI_GELU_F; EPI_S_QKV / EPI_S_GELU): M rows of the pre-LayerNorm stream x as the token operand, the
// LayerNorm finished in the epilogue from x's partials; B [N, H]: weight rows with gamma folded in, bias and csum per row of B.
template <int H, int FORM>
GemmArgs folded_args(const Rows<FORM> &x, int M, float eps, const _Float16 *B, int N, const float *bias, const float *csum,
                     const float *wscale_inv = nullptr, unsigned *faults = nullptr) {
    constexpr int ld = FORM == FORM_PAIR ? 2 * H : H;
    GemmArgs G = {};
    if constexpr (FORM == FORM_PAIR) G.A = x.xp;
    else { G.A = x.hi; G.tok_lo = x.lo; }
    G.lda = ld; G.B = B; G.ldb = ld; G.M = M; G.N = N; G.K = H;
    G.bias = bias; G.csum = csum; G.part_in = x.part; G.ln_eps = eps; G.wscale_inv = wscale_inv; G.range_faults = faults;
    return G;
}

// Columns [c0, c0 + n) of the Q | K projection (fp16 mode; Q = the first H columns, pre-scaled by 1/sqrt(64) and log2(e): the softmax
// runs on exp2) or of the Q | K | V projection (split mode, fp32 out).  The CLS-only tail asks for the K (| V) columns of every token
// and for the Q columns of the compact [CLS] rows; every element is the same arithmetic as in the one full launch.
template <int H>
GemmArgs qk_args(const Rows<FORM_PLANES> &x, int M, float eps, const LayerW &W, int c0, int n, _Float16 *qk) {
    GemmArgs G = folded_args<H>(x, M, eps, W.wqk + (size_t)c0 * H, n, W.bqk + c0, W.cqk + c0);
    G.out16 = qk + c0; G.ldc = 2 * H;
    G.scale = 0.125f * 1.44269504088896340736f; G.scale_cols = c0 == 0 ? H : 0;
    return G;
}
template <int H>
GemmArgs qkv_args(const Rows<FORM_PAIR> &x, int M, float eps, const LayerW &W, int c0, int n, float *qkv, unsigned *faults) {
    GemmArgs G = folded_args<H>(x, M, eps, W.wqkv_s + (size_t)c0 * 2 * H, n, W.bqkv_s + c0, W.cqkv_s + c0, W.sc_s + 4, faults);
    G.out32 = qkv + c0; G.ldc = 3 * H;
    return G;
}

// V^T = Wv LN(x)^T (fp16 mode, EPI_VT_F): the weight is the A operand, the Tpad token rows the B operand; token n < T goes to column
// col_map[n] of vt (row stride ldvt)
template <int H>
GemmArgs vt_args(const Rows<FORM_PLANES> &x, int Tpad, int T, float eps, const LayerW &W, _Float16 *vt, int ldvt, const int *col_map) {
    GemmArgs G = {};
    G.A = W.wv; G.lda = H; G.B = x.hi; G.tok_lo = x.lo; G.ldb = H; G.M = H; G.N = Tpad; G.K = H;
    G.bias = W.bv; G.csum = W.cv; G.part_in = x.part; G.ln_eps = eps;
    G.out16 = vt; G.ldc = ldvt; G.col_map = col_map; G.n_valid = T;
    return G;
}

// FFN1: intermediate.dense + GELU of LN(xa) (attention.output.LayerNorm folded in); n_split: gemm256_tile.h, tile_of_block
template <int H, int FORM>
GemmArgs ffn1_args(const Rows<FORM> &xa, int M, float eps, const LayerW &W, int I, _Float16 *ffn, int n_split, unsigned *faults) {
    constexpr bool P = FORM == FORM_PAIR;
    GemmArgs G = folded_args<H>(xa, M, eps, P ? W.w1_s : W.w1, I, P ? W.b1_s : W.b1, P ? W.c1_s : W.c1, P ? W.sc_s + 6 : nullptr, faults);
    G.out16 = ffn; G.ldc = P ? 2 * I : I; G.n_split = n_split;
    return G;
}

// Residual + LayerNorm (EPI_RESLN / EPI_S_RESLN), the role of attention.output.dense (K = H) and of FFN2, output.dense (K = I):
// out = A B^T + bias + LN(res), M rows; gamma / beta: the LayerNorm whose input the stream res is, finished from res's partials;
// out: rows + partials of the new stream
template <int H, int FORM>
GemmArgs resln_args(const _Float16 *A, const _Float16 *B, int K, const float *bias, int M, const Rows<FORM> &res, const float *gamma,
                    const float *beta, float eps, const Rows<FORM> &out, const float *wscale_inv, unsigned *faults) {
    constexpr int w = FORM == FORM_PAIR ? 2 : 1;  // halves per element of a row
    GemmArgs G = {};
    G.A = A; G.lda = w * K; G.B = B; G.ldb = w * K; G.M = M; G.N = H; G.K = K; G.bias = bias; G.ldc = w * H;
    G.res_gamma = gamma; G.res_beta = beta; G.part_in = res.part; G.ln_eps = eps; G.part_out = out.part;
    G.wscale_inv = wscale_inv; G.range_faults = faults;
    if constexpr (FORM == FORM_PAIR) { G.res_hi = res.xp; G.ldr = 2 * H; G.out16 = out.xp; }
    else { G.res_hi = res.hi; G.res_lo = res.lo; G.out16 = out.hi; G.out_lo = out.lo; }
    return G;
}

// ---- split (fp32-grade) mode: the fp16 mode's schedule with pair operands and the fp32 attention ----
template <int H>
int forward_split(AnceEncoder *e, const AnceEncoder::Lane &LN, hipStream_t st, const MicroPlan &mb, float *out) {
    constexpr int HP = 2 * H;
    const AnceEncoderDesc &D = e->d;
    const AnceEncoder::Lane::Split &V = LN.sp;
    const int I = D.intermediate, S = mb.S, T = mb.T, Tpad = mb.Tpad;
    {
        ProfScope pe(PC_EMBED, st);
        hipLaunchKernelGGL((embed_kernel<H, FORM_PAIR>), dim3(Tpad / 4), dim3(256), 0, st, LN.tok_id, LN.tok_pos, Tpad, e->word,
                           e->pos, e->type0, D.vocab_size, D.max_position, V.xb, e->faults);
    }
    const bool cls_tail = e->cls_tail;
    const int S_pad = (int)align_up((size_t)S, 256);
    const Rows<FORM_PAIR> cls = V.cls(S_pad, H);
    const int n_split = (I / 256) % 2 == 0 ? 2 : 0;  // FFN1: N-split tile order (gemm256_tile.h: tile_of_block)
    for (int li = 0; li < D.n_layers; ++li) {
        const LayerW &W = e->layers[li];
        const bool tail = cls_tail && li == D.n_layers - 1;
        const int Mrows = tail ? S_pad : Tpad;
        const double Mwork = tail ? (double)S : (double)T;
        // layer 0 reads the embedding stream, stored times EMB_SCALE: its LayerNorm runs with eps EMB_SCALE^2 (embed_kernel)
        const float eps_b = li == 0 ? D.ln_eps * (EMB_SCALE * EMB_SCALE) : D.ln_eps;
        // the LayerNorm of x_b, the previous layer's output (or the embeddings)
        const float *const gamma_b = li == 0 ? e->eln_w : e->layers[li - 1].ln2w, *const beta_b = li == 0 ? e->eln_b : e->layers[li - 1].ln2b;
        // CLS-only tail: the last layer's attention has ONE query per sequence.  K | V of every token, but Q of the [CLS]
        // rows only: their pair rows and slice partials are compacted first (they are also the residual of the
        // attention-output GEMM below) and projected by a second, small launch into the Q columns of rows 0 .. S_pad of
        // qkv -- row s = the query of sequence s (attention_split_kernel, cls_only).  A third of this GEMM's work in one
        // layer of twelve.
        if (tail) {
            ProfScope ps(PC_LN, st);
            hipLaunchKernelGGL((gather_cls_kernel<H, FORM_PAIR>), dim3(S_pad / 4), dim3(256), 0, st, V.xb, LN.seq_off, S, S_pad, cls);
        }
        // Q | K | V projection -> fp32 (the LayerNorm that produces this layer's input is folded in)
        {
            ProfScope ps(PC_GEMM_QK, st, tail ? 2.0 * T * (2.0 * H) * H + 2.0 * S * (double)H * H : 2.0 * T * (3.0 * H) * H);
            const int c0 = tail ? H : 0;  // (tail: K | V here, Q of the compact rows by the second launch)
            int rc = launch_gemm_f16(EPI_S_QKV, qkv_args<H>(V.xb, Tpad, eps_b, W, c0, 3 * H - c0, V.qkv, e->faults), st, H);
            if (tail && !rc) rc = launch_gemm_f16(EPI_S_QKV, qkv_args<H>(cls, S_pad, eps_b, W, 0, H, V.qkv, e->faults), st, H);
            if (rc) return rc;
        }
        {
            ProfScope ps(PC_ATTN, st);
            if (tail && S_pad > S)  // rows S..S_pad of the compact attention output feed the GEMM tile: keep them finite
                (void)hipMemsetAsync(V.ctx + (size_t)S * HP, 0, (size_t)(S_pad - S) * HP * sizeof(_Float16), st);
            // (cls_only: one query per sequence, read from row s of the Q columns -- the tail's compact Q projection above)
            if (int rc = launch_attention_split(V.qkv, V.ctx, LN.desc, S, D.n_heads, mb.maxlen, tail ? 1 : 0, st)) return rc;
        }
        // attention.output.dense + residual LayerNorm(x_b); tail: of the compact [CLS] rows
        if (ProfScope ps(PC_GEMM_OUT, st, 2.0 * Mwork * (double)H * H);
            int rc = launch_gemm_f16(EPI_S_RESLN, resln_args<H>(V.ctx, W.wo_s, H, W.bo, Mrows, tail ? cls : V.xb, gamma_b, beta_b, eps_b,
                                                                V.xa, W.sc_s + 5, e->faults), st, H))
            return rc;
        // intermediate.dense + exact GELU (attention.output.LayerNorm folded in)
        if (ProfScope ps(PC_GEMM_FFN1, st, 2.0 * Mwork * (double)I * H);
            int rc = launch_gemm_f16(EPI_S_GELU, ffn1_args<H>(V.xa, Mrows, D.ln_eps, W, I, V.ffn, n_split, e->faults), st, H))
            return rc;
        // output.dense + residual LayerNorm(x_a)
        if (ProfScope ps(PC_GEMM_FFN2, st, 2.0 * Mwork * (double)I * H);
            int rc = launch_gemm_f16(EPI_S_RESLN, resln_args<H>(V.ffn, W.w2_s, I, W.b2, Mrows, V.xa, W.ln1w, W.ln1b, D.ln_eps, V.xb,
                                                                W.sc_s + 7, e->faults), st, H))
            return rc;
    }
    encoder_output<H>(e, LN, st, mb, out, V.xb, cls_tail ? 1 : 0);
    return ANCE_OK;
}

// ---- fp16 mode: the folded-LayerNorm forward of the file header ----
template <int H>
int forward_fp16(AnceEncoder *e, const AnceEncoder::Lane &LN, hipStream_t st, const MicroPlan &mb, float *out) {
    const AnceEncoderDesc &D = e->d;
    const AnceEncoder::Lane::Fp16 &V = LN.f16;
    const int I = D.intermediate, S = mb.S, T = mb.T, Tpad = mb.Tpad;
    {
        ProfScope pe(PC_EMBED, st);
        hipLaunchKernelGGL((embed_kernel<H, FORM_PLANES>), dim3(Tpad / 4), dim3(256), 0, st, LN.tok_id, LN.tok_pos, Tpad, e->word,
                           e->pos, e->type0, D.vocab_size, D.max_position, V.xb, (unsigned *)nullptr);
    }
    // Only the [CLS] row of the last layer reaches the head (model/models.py:49,152): after the
    // last layer's K / V projections everything runs on the S compact [CLS] rows.
    const bool cls_tail = e->cls_tail;
    const int S_pad = (int)align_up((size_t)S, 256);
    const Rows<FORM_PLANES> cls = V.cls(S_pad, H);
    const int n_split = (I / 256) % 2 == 0 ? 2 : 0;  // FFN1: N-split tile order (gemm256_tile.h: tile_of_block)
    for (int li = 0; li < D.n_layers; ++li) {
        const LayerW &W = e->layers[li];
        const bool tail = cls_tail && li == D.n_layers - 1;
        const int Mrows = tail ? S_pad : Tpad;   // rows of the post-attention GEMMs
        const double Mwork = tail ? (double)S : (double)T;
        // the LayerNorm that produced this layer's input x_b: the previous layer's output.LayerNorm, or the embedding LayerNorm
        const float *const gamma_b = li == 0 ? e->eln_w : e->layers[li - 1].ln2w, *const beta_b = li == 0 ? e->eln_b : e->layers[li - 1].ln2b;
        // CLS-only tail: K of every token, Q of the compact [CLS] rows only -- row s of the Q columns is the query of sequence s
        // (attention_kernel, q_compact; split mode: above)
        if (tail) {
            ProfScope ps(PC_LN, st);
            hipLaunchKernelGGL((gather_cls_kernel<H, FORM_PLANES>), dim3(S_pad / 4), dim3(256), 0, st, V.xb, LN.seq_off, S, S_pad, cls);
        }
        // Q | K projection
        {
            ProfScope ps(PC_GEMM_QK, st, tail ? 2.0 * T * (double)H * H + 2.0 * S * (double)H * H : 2.0 * T * (2.0 * H) * H);
            const int c0 = tail ? H : 0;  // (tail: K here, Q of the compact rows by the second launch)
            int rc = launch_gemm_f16(EPI_QK_F, qk_args<H>(V.xb, Tpad, D.ln_eps, W, c0, 2 * H - c0, V.qk), st, H);
            if (tail && !rc) rc = launch_gemm_f16(EPI_QK_F, qk_args<H>(cls, S_pad, D.ln_eps, W, 0, H, V.qk), st, H);
            if (rc) return rc;
        }
        // V^T = Wv h^T
        if (ProfScope ps(PC_GEMM_VT, st, 2.0 * T * (double)H * H);
            int rc = launch_gemm_f16(EPI_VT_F, vt_args<H>(V.xb, Tpad, T, D.ln_eps, W, V.vt, mb.ldvt, LN.tok_vtcol), st, H))
            return rc;
        AttnArgs A;
        A.qk = V.qk; A.vt = V.vt; A.ctx = V.ctx; A.desc = LN.desc;
        A.ld_qk = 2 * H; A.ld_vt = mb.ldvt; A.ld_ctx = H; A.n_heads = D.n_heads; A.cls_only = tail ? 1 : 0; A.q_compact = tail ? 1 : 0;
        if (ProfScope ps(PC_ATTN, st, 0.0); int rc = launch_attention(A, S, mb.maxlen, st)) return rc;
        // attention.output.dense + residual LayerNorm(x_b); tail: of the compact [CLS] rows
        if (ProfScope ps(PC_GEMM_OUT, st, 2.0 * Mwork * (double)H * H);
            int rc = launch_gemm_f16(EPI_RESLN, resln_args<H>(V.ctx, W.wo, H, W.bo, Mrows, tail ? cls : V.xb, gamma_b, beta_b, D.ln_eps,
                                                              V.xa, nullptr, nullptr), st, H))
            return rc;
        // intermediate.dense + GELU
        if (ProfScope ps(PC_GEMM_FFN1, st, 2.0 * Mwork * (double)I * H);
            int rc = launch_gemm_f16(EPI_GELU_F, ffn1_args<H>(V.xa, Mrows, D.ln_eps, W, I, V.ffn, n_split, nullptr), st, H))
            return rc;
        // output.dense + residual LayerNorm(x_a)
        if (ProfScope ps(PC_GEMM_FFN2, st, 2.0 * Mwork * (double)I * H);
            int rc = launch_gemm_f16(EPI_RESLN, resln_args<H>(V.ffn, W.w2, I, W.b2, Mrows, V.xa, W.ln1w, W.ln1b, D.ln_eps, V.xb,
                                                              nullptr, nullptr), st, H))
            return rc;
    }
    encoder_output<H>(e, LN, st, mb, out, V.xb, cls_tail ? 1 : 0);
    return ANCE_OK;
}

// The fork of encode_impl onto the side streams.  Once they have started, no path leaves encode_impl -- an error return included --
// before join_lanes has ordered the caller's stream after every one of them.
struct LaneFork {
    AnceEncoder *e;
    hipStream_t caller_st;
    bool forked = false;
    void fork() {  // side streams start after everything already queued by the caller
        (void)hipEventRecord(e->ev_fork, caller_st);
        for (int ln = 0; ln < e->n_lanes; ++ln) (void)hipStreamWaitEvent(e->side[ln], e->ev_fork, 0);
        forked = true;
    }
    void join_lanes() {
        for (int ln = 0; forked && ln < e->n_lanes; ++ln) {
            (void)hipEventRecord(e->ev_join[ln], e->side[ln]);
            (void)hipStreamWaitEvent(caller_st, e->ev_join[ln], 0);
        }
        forked = false;
    }
    ~LaneFork() { join_lanes(); }
};

int encode_impl(AnceEncoder *e, const int32_t *base, int64_t ld, const int32_t *d_lens, const int32_t *h_lens, int hdr,
                int64_t n, int L, int n_chunks, float *d_out, hipStream_t caller_st) {
    if (!e || !base || !d_out || n < 0 || L < 1 || n_chunks < 1 || L % n_chunks) {
        set_last_error("ance_encode: invalid argument");
        return ANCE_E_INVALID;
    }
    const int Lc = L / n_chunks;
    if (Lc > e->d.max_seq_len) {
        set_last_error("ance_encode: chunk length exceeds desc.max_seq_len");
        return ANCE_E_INVALID;
    }
    const AnceEncoderDesc &D = e->d;
    const bool seed = D.arch == ANCE_ARCH_SEED;
    if (seed && n_chunks != 1) {
        set_last_error("ance_encode: ANCE_ARCH_SEED encodes whole records (n_chunks must be 1)");
        return ANCE_E_INVALID;
    }
    int mb_index = 0;
    LaneFork lanes{e, caller_st};

    for (int64_t r0 = 0; r0 < n; r0 += FETCH_CHUNK) {
        const int nr = (int)((n - r0) < FETCH_CHUNK ? (n - r0) : FETCH_CHUNK);
        const int32_t *hl;
        if (h_lens) {
            hl = h_lens + r0;
        } else {
            // no host copy of the lengths: read them back once (the only synchronising path)
            e->host_lens.resize(nr);
            hipLaunchKernelGGL(fetch_lens_kernel, dim3((nr + 255) / 256), dim3(256), 0, caller_st, base, ld, d_lens, r0, nr, L,
                               e->lens_fetch);
            if (hipMemcpyAsync(e->host_lens.data(), e->lens_fetch, (size_t)nr * 4, hipMemcpyDeviceToHost, caller_st) != hipSuccess ||
                hipStreamSynchronize(caller_st) != hipSuccess)
                return check_launch("ance_encode: length read-back");
            hl = e->host_lens.data();
        }
        if (seed)
            for (int i = 0; i < nr; ++i)
                if (hl[i] <= 0) {
                    // no [CLS]: the reference reads a pad row or NaN there (a record that starts with the pad id is caught on the
                    // device: seed_count_kernel)
                    set_last_error("ance_encode: empty record under ANCE_ARCH_SEED (the reference defines no output for it)");
                    return ANCE_E_INVALID;
                }
        if (e->n_lanes > 1 && !lanes.forked) lanes.fork();
        // ---- greedy micro-batches over the sequences (record, chunk) of this block of records ---
        const int64_t gs_end = (int64_t)nr * n_chunks;
        int64_t gs = 0;
        while (gs < gs_end) {
            const AnceEncoder::Lane &LN = e->lane[mb_index % e->n_lanes];
            hipStream_t st = e->n_lanes > 1 ? e->side[mb_index % e->n_lanes] : caller_st;
            ++mb_index;
            const MicroPlan mb = plan_micro_batch(hl, gs, gs_end, n_chunks, L, Lc, e->scap, e->tcap, e->vcap, seed);
            if (mb.S == 0) {
                set_last_error("ance_encode: max_tokens too small for one sequence");
                return ANCE_E_INVALID;
            }
            PlanArgs P;
            P.base = base; P.ld = ld; P.lens = d_lens; P.hdr = hdr;
            P.g0 = r0 * n_chunks + gs; P.S = mb.S; P.L = L; P.n_chunks = n_chunks; P.Lc = Lc;
            P.pad_id = D.pad_token_id; P.arch = D.arch; P.T = mb.T; P.Tpad = mb.Tpad; P.vt_spare = mb.V;
            P.seq_off = LN.seq_off; P.seq_vtcol = LN.seq_vtcol; P.seq_len = LN.seq_len;
            P.tok_id = LN.tok_id; P.tok_pos = LN.tok_pos; P.tok_vtcol = LN.tok_vtcol;
            P.desc = LN.desc; P.faults = e->faults;
            {
                ProfScope ps(PC_PLAN, st);
                if (seed) hipLaunchKernelGGL(seed_count_kernel, dim3((mb.S + 3) / 4), dim3(256), 0, st, P);
                hipLaunchKernelGGL(plan_kernel, dim3(1), dim3(1024), 0, st, P);
                const int nb_seq = (mb.S + 3) / 4, nb_pad = ((seed ? mb.Tpad : mb.Tpad - mb.T) + 255) / 256;
                hipLaunchKernelGGL(pack_kernel, dim3(nb_seq > nb_pad ? nb_seq : nb_pad), dim3(256), 0, st, P);
            }
            float *const out = d_out + (size_t)(r0 * n_chunks + gs) * HEAD_OUT;
            const int rc = with_hidden(D.hidden, [&](auto h) {
                constexpr int H = decltype(h)::value;
                return e->mode == ANCE_PRECISION_FP32    ? forward_fp32<H>(e, LN, st, mb, out)
                       : e->mode == ANCE_PRECISION_SPLIT ? forward_split<H>(e, LN, st, mb, out)
                                                         : forward_fp16<H>(e, LN, st, mb, out);
            });
            if (rc) return rc;
            gs = mb.next;
        }
        // the next block of records needs a length read-back on the caller's stream: join first
        if (r0 + FETCH_CHUNK < n && !h_lens) lanes.join_lanes();
    }
    lanes.join_lanes();
    return check_launch("ance_encode");
}

}  // namespace

extern "C" size_t ance_encoder_weight_bytes(const AnceEncoderDesc *desc) {
    if (!desc_ok(desc)) return 0;
    Arena a;
    layout_weights(desc, a, nullptr);
    return a.off + 256;
}

extern "C" size_t ance_encoder_workspace_bytes(const AnceEncoderDesc *desc) {
    if (!desc_ok(desc)) return 0;
    Arena a;
    layout_workspace(desc, a, nullptr);
    return a.off + 256;
}

extern "C" int ance_encoder_create(const AnceEncoderDesc *desc, const void *const *w, int n_weights, void *d_weight_arena,
                                   size_t weight_bytes, void *d_workspace, size_t workspace_bytes, void *stream,
                                   AnceEncoder **out) {
    if (!desc_ok(desc) || !w || !out || !d_weight_arena || !d_workspace ||
        n_weights != ANCE_ENCODER_N_WEIGHTS(desc->n_layers, desc->has_head)) {
        set_last_error("ance_encoder_create: invalid descriptor or weight list");
        return ANCE_E_INVALID;
    }
    for (int i = 0; i < n_weights; ++i)
        if (!w[i]) {
            set_last_error("ance_encoder_create: null weight pointer");
            return ANCE_E_INVALID;
        }
    if (weight_bytes < ance_encoder_weight_bytes(desc) || workspace_bytes < ance_encoder_workspace_bytes(desc)) {
        set_last_error("ance_encoder_create: arena or workspace too small");
        return ANCE_E_WORKSPACE;
    }
    AnceEncoder *e = new (std::nothrow) AnceEncoder();
    if (!e) return ANCE_E_NOMEM;
    e->d = *desc;
    {
        const char *ct = getenv("ANCE_CLS_TAIL");
        e->cls_tail = !(ct && ct[0] == '0');
        e->mode = resolve_precision(desc);
        const char *ns = getenv("ANCE_ENCODER_STREAMS");
        e->n_lanes = (ns && ns[0] >= '1' && ns[0] <= '0' + MAX_LANES) ? ns[0] - '0' : 2;
    }
    for (int ln = 0; ln < MAX_LANES; ++ln) {
        e->side[ln] = nullptr;
        e->ev_join[ln] = nullptr;
    }
    e->ev_fork = nullptr;
    if (e->n_lanes > 1) {
        bool ok = hipEventCreateWithFlags(&e->ev_fork, hipEventDisableTiming) == hipSuccess;
        for (int ln = 0; ln < e->n_lanes && ok; ++ln)
            ok = hipStreamCreateWithFlags(&e->side[ln], hipStreamNonBlocking) == hipSuccess &&
                 hipEventCreateWithFlags(&e->ev_join[ln], hipEventDisableTiming) == hipSuccess;
        if (!ok) {
            delete e;
            return check_launch("ance_encoder_create: streams");
        }
    }
    const int H = desc->hidden, HP = 2 * H;
    // per device: set for the device this handle lives on
    const hipError_t head_attr = with_hidden(H, [&](auto h) {
        constexpr int HW = decltype(h)::value;
        const void *k = e->mode == ANCE_PRECISION_FP32    ? reinterpret_cast<const void *>(head_gemm_kernel<HW, FORM_F32>)
                        : e->mode == ANCE_PRECISION_SPLIT ? reinterpret_cast<const void *>(head_gemm_kernel<HW, FORM_PAIR>)
                                                          : reinterpret_cast<const void *>(head_gemm_kernel<HW, FORM_PLANES>);
        return hipFuncSetAttribute(k, hipFuncAttributeMaxDynamicSharedMemorySize, (int)HEAD_LDS_BYTES<HW>);
    });
    if (head_attr != hipSuccess) {
        delete e;
        return check_launch("ance_encoder_create: head attr");
    }
    Arena wa, xa;
    wa.base = reinterpret_cast<char *>(align_up((uintptr_t)d_weight_arena, 256));
    xa.base = reinterpret_cast<char *>(align_up((uintptr_t)d_workspace, 256));
    layout_weights(desc, wa, e);
    layout_workspace(desc, xa, e);
    hipStream_t st = (hipStream_t)stream;
    (void)hipMemsetAsync(xa.base, 0, xa.off, st);  // pad rows must never hold NaN bit patterns

    const size_t I = desc->intermediate;
    cpy32(w[0], e->word, (size_t)desc->vocab_size * H, st);
    cpy32(w[1], e->pos, (size_t)desc->max_position * H, st);
    cpy32(w[2], e->type0, H, st);
    cpy32(w[3], e->eln_w, H, st);
    cpy32(w[4], e->eln_b, H, st);
    // each mode prepares only the weights its forward reads (the arena layout is the same for all three: layout_weights)
    for (int i = 0; i < desc->n_layers; ++i) {
        const void *const *p = w + 5 + 16 * i;
        LayerW &L = e->layers[i];
        // the LayerNorm that produces this layer's input: embeddings.LayerNorm or the previous output.LayerNorm
        const float *gin = (const float *)(i == 0 ? w[3] : w[5 + 16 * (i - 1) + 14]);
        const float *bin = (const float *)(i == 0 ? w[4] : w[5 + 16 * (i - 1) + 15]);
        cpy32(p[7], L.bo, H, st);
        cpy32(p[8], L.ln1w, H, st);
        cpy32(p[9], L.ln1b, H, st);
        cpy32(p[13], L.b2, H, st);
        cpy32(p[14], L.ln2w, H, st);
        cpy32(p[15], L.ln2b, H, st);
        if (e->mode == ANCE_PRECISION_FP16) {
            auto foldw = [&](const void *W, const void *b, const float *g, const float *be, int N, _Float16 *W16, float *cs,
                             float *bo) {
                with_hidden(H, [&](auto h) {
                    hipLaunchKernelGGL(fold_weight_kernel<decltype(h)::value>, dim3((N + 3) / 4), dim3(256), 0, st, (const float *)W,
                                       (const float *)b, g, be, N, W16, cs, bo);
                });
            };
            foldw(p[0], p[1], gin, bin, H, L.wqk, L.cqk, L.bqk);                                     // query
            foldw(p[2], p[3], gin, bin, H, L.wqk + (size_t)H * H, L.cqk + H, L.bqk + H);            // key
            foldw(p[4], p[5], gin, bin, H, L.wv, L.cv, L.bv);                                        // value
            foldw(p[10], p[11], (const float *)p[8], (const float *)p[9], (int)I, L.w1, L.c1, L.b1);  // intermediate.dense
            cvt16(p[6], L.wo, (size_t)H * H, st);
            cvt16(p[12], L.w2, (size_t)H * I, st);
        } else if (e->mode == ANCE_PRECISION_SPLIT) {
            unsigned *slots = reinterpret_cast<unsigned *>(L.sc_s);
            (void)hipMemsetAsync(L.sc_s, 0, 4 * sizeof(float), st);
            auto mx = [&](const void *W, const float *g, int N, int K, int slot) {
                hipLaunchKernelGGL(wabsmax_kernel, dim3(256), dim3(256), 0, st, (const float *)W, g, N, K, slots + slot);
            };
            auto sw = [&](const void *W, const void *b, const float *g, const float *be, int N, int K, int slot, _Float16 *Wp, float *cs,
                          float *bo) {
                hipLaunchKernelGGL(split_weight_kernel, dim3((N + 3) / 4), dim3(256), 0, st, (const float *)W, (const float *)b, g, be,
                                   N, K, (const unsigned *)(slots + slot), Wp, cs, bo, L.sc_s + 4 + slot);
            };
            mx(p[0], gin, H, H, 0);  // Q, K and V are one operand matrix: one scale
            mx(p[2], gin, H, H, 0);
            mx(p[4], gin, H, H, 0);
            mx(p[6], nullptr, H, H, 1);
            mx(p[10], (const float *)p[8], (int)I, H, 2);
            mx(p[12], nullptr, H, (int)I, 3);
            sw(p[0], p[1], gin, bin, H, H, 0, L.wqkv_s, L.cqkv_s, L.bqkv_s);                                             // query
            sw(p[2], p[3], gin, bin, H, H, 0, L.wqkv_s + (size_t)H * HP, L.cqkv_s + H, L.bqkv_s + H);                    // key
            sw(p[4], p[5], gin, bin, H, H, 0, L.wqkv_s + (size_t)2 * H * HP, L.cqkv_s + 2 * H, L.bqkv_s + 2 * H);        // value
            sw(p[6], nullptr, nullptr, nullptr, H, H, 1, L.wo_s, nullptr, nullptr);                                      // attention.output.dense
            sw(p[10], p[11], (const float *)p[8], (const float *)p[9], (int)I, H, 2, L.w1_s, L.c1_s, L.b1_s);            // intermediate.dense
            sw(p[12], nullptr, nullptr, nullptr, H, (int)I, 3, L.w2_s, nullptr, nullptr);                                // output.dense
        } else {
            cpy32(p[0], L.wqkv32, (size_t)H * H, st);
            cpy32(p[2], L.wqkv32 + (size_t)H * H, (size_t)H * H, st);
            cpy32(p[4], L.wqkv32 + (size_t)2 * H * H, (size_t)H * H, st);
            cpy32(p[1], L.bqkv32, H, st);
            cpy32(p[3], L.bqkv32 + H, H, st);
            cpy32(p[5], L.bqkv32 + 2 * H, H, st);
            cpy32(p[6], L.wo32, (size_t)H * H, st);
            cpy32(p[10], L.w132, I * H, st);
            cpy32(p[11], L.b1, I, st);
            cpy32(p[12], L.w232, (size_t)H * I, st);
        }
    }
    if (desc->has_head) {
        const void *const *p = w + 5 + 16 * desc->n_layers;
        cpy32(p[0], e->head_w, (size_t)HEAD_OUT * H, st);
        cpy32(p[1], e->head_b, HEAD_OUT, st);
        cpy32(p[2], e->norm_w, HEAD_OUT, st);
        cpy32(p[3], e->norm_b, HEAD_OUT, st);
    }
    int rc = check_launch("ance_encoder_create");
    if (rc) {
        delete e;
        return rc;
    }
    *out = e;
    return ANCE_OK;
}

extern "C" void ance_encoder_destroy(AnceEncoder *enc) {
    if (!enc) return;
    for (int ln = 0; ln < MAX_LANES; ++ln) {
        if (enc->side[ln]) {
            (void)hipStreamSynchronize(enc->side[ln]);
            (void)hipStreamDestroy(enc->side[ln]);
        }
        if (enc->ev_join[ln]) (void)hipEventDestroy(enc->ev_join[ln]);
    }
    if (enc->ev_fork) (void)hipEventDestroy(enc->ev_fork);
    delete enc;
}

extern "C" int ance_encoder_precision(const AnceEncoder *enc) {
    if (!enc) return ANCE_E_INVALID;
    return enc->mode;
}

extern "C" int ance_encoder_range_faults(AnceEncoder *enc, uint32_t *h_out, int reset, void *stream) {
    if (!enc || !h_out) {
        set_last_error("ance_encoder_range_faults: invalid argument");
        return ANCE_E_INVALID;
    }
    hipStream_t st = (hipStream_t)stream;
    if (hipMemcpyAsync(h_out, enc->faults, 2 * sizeof(uint32_t), hipMemcpyDeviceToHost, st) != hipSuccess)
        return check_launch("ance_encoder_range_faults");
    if (reset) (void)hipMemsetAsync(enc->faults, 0, 2 * sizeof(uint32_t), st);
    return check_launch("ance_encoder_range_faults");
}

extern "C" int ance_encode_records(AnceEncoder *enc, const void *d_records, const int32_t *h_lens, int64_t n, int L,
                                   int n_chunks, float *d_out, void *stream) {
    return encode_impl(enc, (const int32_t *)d_records, (int64_t)L + 1, nullptr, h_lens, 1, n, L, n_chunks, d_out,
                       (hipStream_t)stream);
}

extern "C" int ance_encode_ids(AnceEncoder *enc, const int32_t *d_ids, int64_t ld_ids, const int32_t *d_lens,
                               const int32_t *h_lens, int64_t n, int L, int n_chunks, float *d_out, void *stream) {
    if (!d_lens) {
        set_last_error("ance_encode_ids: d_lens is required");
        return ANCE_E_INVALID;
    }
    return encode_impl(enc, d_ids, ld_ids, d_lens, h_lens, 0, n, L, n_chunks, d_out, (hipStream_t)stream);
}

extern "C" double ance_encoder_flops_per_sequence(int T) {
    const double t = T;
    return 169869312.0 * t + 36864.0 * t * t + 1179648.0;
}
