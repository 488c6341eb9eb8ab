// C-ABI test hooks of the 256 x 256 GEMM (include/ance_amd.h): host-side marshalling of caller-provided buffers into a GemmArgs.
// The kernels and their launch are gemm256_f16.hip's (launch_gemm_f16); nothing here runs on the device.
#include "common.h"
#include "gemm_f16.h"
#include <string.h>

// Test hook (include/ance_amd.h): the fp16 GEMM kernel on caller-provided data.  ablate is kept for the ABI and must be 0.
extern "C" int ance_debug_gemm(int ablate, int epi, const void *d_a_f16, const void *d_b_f16, int M, int N, int K,
                               const float *d_bias, void *d_out, const float *d_res32, void *stream) {
    using namespace ance;
    if (ablate != 0 || !d_a_f16 || !d_b_f16 || !d_bias || !d_out || epi < 0 || epi > 2 || (epi == EPI_RES32 && !d_res32)) {
        set_last_error("ance_debug_gemm: invalid argument");
        return ANCE_E_INVALID;
    }
    GemmArgs G;
    memset(&G, 0, sizeof(G));
    G.A = (const _Float16 *)d_a_f16; G.lda = K; G.B = (const _Float16 *)d_b_f16; G.ldb = K;
    G.M = M; G.N = N; G.K = K; G.bias = d_bias; G.ldc = N; G.scale = 1.0f; G.scale_cols = 0;
    if (epi == EPI_RES32) { G.out32 = (float *)d_out; G.res32 = d_res32; }
    else G.out16 = (_Float16 *)d_out;
    ProfScope ps(PC_GEMM_FFN1, (hipStream_t)stream, 2.0 * M * (double)N * K);
    int rc = launch_gemm_f16(epi, G, (hipStream_t)stream);
    return rc ? rc : check_launch("ance_debug_gemm");
}

// Test hook (include/ance_amd.h): the SPLIT GEMM with each of its three epilogues on caller-provided pair operands (blocked pair
// rows: ance_pair_layout); d_wscale_inv: optional device scalar the accumulators are multiplied by (the inverse of the power of
// two the B operand was stored with).
extern "C" int ance_debug_gemm_split(int epi, const void *d_a_pair, const void *d_b_pair, int M, int N, int K, const float *d_bias,
                                     const float *d_vec1, const float *d_vec2, const float *d_part, float ln_eps,
                                     const void *d_res_pair, void *d_out, float *d_part_out, const float *d_wscale_inv, void *stream) {
    using namespace ance;
    if (!d_a_pair || !d_b_pair || !d_bias || !d_vec1 || !d_part || !d_out || epi < EPI_S_QKV || epi > EPI_S_RESLN ||
        (epi == EPI_S_RESLN && (!d_vec2 || !d_res_pair || !d_part_out || (N != 768 && N != 1024))) || K % 64 != 0) {
        set_last_error("ance_debug_gemm_split: invalid argument");
        return ANCE_E_INVALID;
    }
    GemmArgs G;
    memset(&G, 0, sizeof(G));
    G.A = (const _Float16 *)d_a_pair; G.lda = 2 * K; G.B = (const _Float16 *)d_b_pair; G.ldb = 2 * K;
    G.M = M; G.N = N; G.K = K; G.bias = d_bias; G.part_in = d_part; G.ln_eps = ln_eps; G.wscale_inv = d_wscale_inv;
    if (epi == EPI_S_QKV) {
        G.csum = d_vec1; G.out32 = (float *)d_out; G.ldc = N;
    } else if (epi == EPI_S_GELU) {
        G.csum = d_vec1; G.out16 = (_Float16 *)d_out; G.ldc = 2 * N;
    } else {
        G.res_gamma = d_vec1; G.res_beta = d_vec2; G.res_hi = (const _Float16 *)d_res_pair; G.ldr = 2 * N;
        G.out16 = (_Float16 *)d_out; G.ldc = 2 * N; G.part_out = d_part_out;
    }
    // EPI_S_RESLN at N = 1024: the partials (in and out) are the hidden-1024 format (gemm_f16.h: PartFormat)
    int rc = launch_gemm_f16(epi, G, (hipStream_t)stream, epi == EPI_S_RESLN && N == 1024 ? 1024 : 768);
    return rc ? rc : check_launch("ance_debug_gemm_split");
}

// Test hook (include/ance_amd.h): one GEMM instance the encoder dispatches (epilogues EPI_RESLN .. EPI_S_RESLN at hidden 768 or
// 1024) with every GemmArgs field the encoder sets (encoder.hip: forward_split, forward_fp16).  Host code only: the kernels and
// their launch are the encoder's own.
extern "C" int ance_debug_gemm_hw(int epi, int hw, const AnceGemmDebugArgs *a, void *stream) {
    using namespace ance;
    const bool fold = epi == EPI_QK_F || epi == EPI_GELU_F || epi == EPI_VT_F;   // bias, csum (per feature)
    const bool bad = !a || (hw != 768 && hw != 1024) || epi < EPI_RESLN || epi > EPI_S_RESLN || (a->n_split != 0 && a->n_split != 2) ||
                     !a->a || !a->b || !a->bias || !a->part_in || !a->out ||
                     ((fold || epi == EPI_S_QKV || epi == EPI_S_GELU) && !a->csum) ||
                     (epi == EPI_QK_F && a->scale_cols % 64 != 0) ||
                     (epi == EPI_VT_F && !a->col_map) ||
                     (epi == EPI_RESLN && (!a->res_hi || !a->res_lo || !a->out_lo)) ||
                     ((epi == EPI_RESLN || epi == EPI_S_RESLN) && (!a->res_gamma || !a->res_beta || !a->part_out || a->N != hw)) ||
                     (epi == EPI_S_RESLN && !a->res_hi);
    if (bad) {
        set_last_error("ance_debug_gemm_hw: invalid argument");
        return ANCE_E_INVALID;
    }
    GemmArgs G;
    memset(&G, 0, sizeof(G));
    G.A = (const _Float16 *)a->a; G.B = (const _Float16 *)a->b; G.lda = a->lda; G.ldb = a->ldb;
    G.M = a->M; G.N = a->N; G.K = a->K;
    G.bias = a->bias; G.csum = a->csum; G.part_in = a->part_in; G.ln_eps = a->ln_eps; G.tok_lo = (const _Float16 *)a->tok_lo;
    G.scale = a->scale; G.scale_cols = a->scale_cols; G.col_map = a->col_map; G.n_valid = a->n_valid; G.ldc = a->ldc;
    if (epi == EPI_S_QKV) G.out32 = (float *)a->out;
    else G.out16 = (_Float16 *)a->out;
    G.res_hi = (const _Float16 *)a->res_hi; G.res_lo = (const _Float16 *)a->res_lo; G.res_gamma = a->res_gamma; G.res_beta = a->res_beta;
    G.out_lo = (_Float16 *)a->out_lo; G.part_out = a->part_out;
    G.ldr = a->ldr; G.wscale_inv = a->wscale_inv; G.n_split = a->n_split;
    int rc = launch_gemm_f16(epi, G, (hipStream_t)stream, hw);
    return rc ? rc : check_launch("ance_debug_gemm_hw");
}

// Layout of the split mode's pair rows for tests and tools: column n of a W-wide row -> positions of its hi and lo halves in the
// 2 W-half row, and the factor lo was multiplied by (1: unscaled; the round-4 A/B build reports 2048 and rows [hi (W) | lo' (W)]).
extern "C" void ance_pair_layout(int n, int W, int *hi_col, int *lo_col, float *lo_scale) {
    if (hi_col) *hi_col = ance::pair_hi_col(n, W);
    if (lo_col) *lo_col = ance::pair_lo_col(n, W);
    if (lo_scale) *lo_scale = ance::PAIR_LO_SCALE;
}
