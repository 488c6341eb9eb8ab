// Exact re-scoring of the lists the filter left (ip_topk_fast.hip, step 5) and the hand-over of overflowed queries to the
// exact scan.  Included by ip_topk_fast.hip only (after its shape constants), into its anonymous namespace.
#pragma once
#include "search_filter.h"

namespace ance {
namespace {

// ---- exact re-scoring of the lists the filter kernel left: one wave (= one workgroup) per (query, split) ---------------
// A buffer ends the scan with a few hundred rows (everything above the LAST threshold), but only the rows within 2 eps
// of the final k-th best approximate score (about k + 66 per query) can be in the exact top-k.  The band is cut first: the
// k-th approximate score by radix select over this list and the next split's, the survivors' buffer positions compacted into an LDS list.  Then, 64 rows per
// round (one per lane), 256 floats of every row at a time: the wave copies the 64 row pieces into LDS with one
// 1 KiB LDS-DMA each -- every lane reading its own row straight from memory made 64 scattered 16-byte requests per
// load instruction and ran at 1.3 TB/s -- and each lane runs the canonical fmaf chain (k ascending) over its row's
// piece from LDS (row stride 1040 bytes: conflict-free ds_read_b128).  Exact keys stay in registers for the selection.
struct RescoreParams {
    const float *q32, *x32, *qnorm_c, *qnorm_o;
    const QueryStat *qstat;
    const DedupHeader *hdr;
    const uint32_t *live2row;
    const u64 *cand;     // [n_qt * S][FQ][F_C]
    const int *cnt_g;    // [n_qt * S][FQ]
    const float *thr_g;  // [n_qt * S][FQ] final filter thresholds
    u64 *part;           // [nq][S][k]
    uint32_t nq;
    int d, k, S;
    EpsConst eps;
};
constexpr int RS_CHUNK = 256;            // floats of a row staged per step
constexpr int RS_STRIDE = RS_CHUNK + 4;  // floats between the staged pieces of consecutive rows
inline size_t rescore_lds_bytes(int d) { return ((size_t)d + F_C / 2 + 64 * RS_STRIDE) * sizeof(float); }

__global__ void __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(1, 1))) rescore_kernel(const RescoreParams P) {  // LDS allows 2 waves per CU
    extern __shared__ __attribute__((aligned(16))) float rs_smem[];
    if (P.qstat->bad_image) return;
    const int l = threadIdx.x;
    const int d = P.d;
    float *qrow_lds = rs_smem;                                                   // d floats
    unsigned short *list = reinterpret_cast<unsigned short *>(qrow_lds + d);    // F_C buffer positions (4 KiB)
    float *stage = qrow_lds + d + F_C / 2;                                       // 64 x RS_STRIDE floats
    // list id -> (query tile, split, query): lists of one query tile and split are consecutive
    const size_t lid = blockIdx.x;
    const int ql = (int)(lid % FQ);
    const size_t ts = lid / FQ;  // qt * S + split
    const int split = (int)(ts % P.S);
    const uint32_t qg = (uint32_t)(ts / P.S) * FQ + ql;
    if (qg >= P.nq) return;
    const int n_c = P.cnt_g[lid];
    const u64 *cq = P.cand + lid * (size_t)F_C;
    u64 *dst = P.part + ((size_t)qg * P.S + split) * (size_t)P.k;
    const float *qsrc = P.q32 + (size_t)qg * d;
    for (int k4 = l * 4; k4 < d; k4 += 256) *reinterpret_cast<f32x4 *>(qrow_lds + k4) = *reinterpret_cast<const f32x4 *>(qsrc + k4);
    const float eps2 = two_eps(P.eps, P.qnorm_c[qg], P.qnorm_o[qg], P.qstat, P.hdr);  // as in the filter kernel
    const u64 lt_mask = (1ull << l) - 1ull;
    u64 keys[F_NPL];
#pragma unroll
    for (int j = 0; j < F_NPL; ++j) {
        const int idx = j * 64 + l;
        keys[j] = (idx < n_c) ? cq[idx] : 0ull;
    }
    float thr_band = P.thr_g[lid];  // rows buffered before the threshold rose (own prunes, other splits) are out as well
    if (!(thr_band == thr_band)) thr_band = -INFINITY;
    // The k-th best approximate score is taken over this list AND the list of the next split of the same query (with two
    // splits: over everything the filter kept for the query): a threshold from any subset of the rows is valid for all of
    // them, and the union's k-th is what the merged answer is cut at -- each list then keeps its share of the ~k + 66
    // band rows instead of k + 66 of its own.  Only the score halves of the keys take part (32 radix steps).
    const int n_own = (n_c + 63) >> 6;  // registers in use (wave-uniform)
    uint32_t sib[F_NPL];
    int n_c2 = 0, n_sib = 0;
    if (P.S > 1) {
        const size_t lid2 = (ts - split + (size_t)((split + 1) % P.S)) * FQ + ql;
        n_c2 = min(P.cnt_g[lid2], F_C);
        n_sib = (n_c2 + 63) >> 6;
        const u64 *cq2 = P.cand + lid2 * (size_t)F_C;
#pragma unroll
        for (int j = 0; j < F_NPL; ++j) {
            const int idx = j * 64 + l;
            sib[j] = (idx < n_c2) ? (uint32_t)(cq2[idx] >> 32) : 0u;
        }
    } else {
#pragma unroll
        for (int j = 0; j < F_NPL; ++j) sib[j] = 0u;
    }
    if (n_c + n_c2 >= P.k) {
        uint32_t T = 0;  // score half of the k-th largest approximate key of the union
        for (int bit = 31; bit >= 0; --bit) {
            const uint32_t t2 = T | (1u << bit);
            int ge = 0;
#pragma unroll
            for (int j = 0; j < F_NPL; ++j) {
                if (j < n_own) ge += __popcll(__ballot((uint32_t)(keys[j] >> 32) >= t2));
            }
#pragma unroll
            for (int j = 0; j < F_NPL; ++j) {
                if (j < n_sib) ge += __popcll(__ballot(sib[j] >= t2));
            }
            if (ge >= P.k) T = t2;
        }
        if (T != 0u) thr_band = fmaxf(thr_band, key_score((u64)T << 32) - eps2);
    }
    int n_band = 0;
#pragma unroll
    for (int j = 0; j < F_NPL; ++j) {
        const bool keep = keys[j] != 0ull && !(key_score(keys[j]) < thr_band);
        const u64 m = __ballot(keep);
        if (keep) list[n_band + __popcll(m & lt_mask)] = (unsigned short)(j * 64 + l);
        n_band += __popcll(m);
    }
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
#pragma unroll
    for (int j = 0; j < F_NPL; ++j) keys[j] = 0ull;
    for (int r0 = 0, rnd = 0; r0 < n_band; r0 += 64, ++rnd) {
        const int e = r0 + l;
        const bool valid = e < n_band;
        const uint32_t prow = valid ? P.live2row[key_row(cq[list[e]])] : 0u;  // image row -> shard row
        const int rows = min(64, n_band - r0);  // wave-uniform
        float sc = 0.0f;
        for (int c0 = 0; c0 < d; c0 += RS_CHUNK) {
            const int len = min(RS_CHUNK, d - c0);         // 256, or 128 for the last piece when d % 256 == 128
            const int lsrc = l * 4 < len ? l * 4 : 0;      // lanes past a short piece re-read its head (never past the row)
            for (int r = 0; r < rows; ++r) {
                const uint32_t row = __builtin_amdgcn_readlane(prow, r);
                const float *src = P.x32 + ((size_t)row * d + c0) + lsrc;
                __builtin_amdgcn_global_load_lds((pipe_glb_t *)src, (pipe_lds_t *)(stage + r * RS_STRIDE), 16, 0, 0);
            }
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
            __builtin_amdgcn_wave_barrier();
            if (valid) {
                const float *xs = stage + l * RS_STRIDE;
                const float *qs = qrow_lds + c0;
#pragma unroll 16
                for (int j = 0; j < len / 4; ++j) {
                    const f32x4 xv = *reinterpret_cast<const f32x4 *>(xs + 4 * j);
                    const f32x4 a = *reinterpret_cast<const f32x4 *>(qs + 4 * j);
                    sc = __builtin_fmaf(a[0], xv[0], sc);
                    sc = __builtin_fmaf(a[1], xv[1], sc);
                    sc = __builtin_fmaf(a[2], xv[2], sc);
                    sc = __builtin_fmaf(a[3], xv[3], sc);
                }
            }
            asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");  // the next pieces overwrite the stage
            __builtin_amdgcn_wave_barrier();
        }
        const u64 v = valid ? pack_key(sc, prow) : 0ull;
#pragma unroll
        for (int j = 0; j < F_NPL; ++j) keys[j] = (j == rnd) ? v : keys[j];  // rnd is wave-uniform: register file stays static
    }
    if (n_band > P.k) {
        float tau_new;
        select_topk_regs<F_NPL>(keys, P.k, dst, &tau_new);
    } else {
#pragma unroll
        for (int j = 0; j < F_NPL; ++j) {
            const int e = j * 64 + l;
            if (e < P.k) dst[e] = keys[j];
        }
    }
}

// after the filter launch: turn the overflow list into the input of the per-query exact scan
__global__ void __launch_bounds__(256) gather_overflow_kernel(FastCtl *ctl, const QueryStat *qs, const int *ovf_list, const float *q32,
                                                              int d, float *qfb, int *fb_slot) {
    const int cnt = ctl->ovf_count, i = blockIdx.x;
    if (qs->bad_image || cnt > OVF_CAP) {  // nothing was filtered, or too many queries to redo one by one: the whole chunk
        if (i == 0 && threadIdx.x == 0) {  // goes to the exact scan
            ctl->fb_all = 1;
            ctl->fb_nq = 0;
        }
        return;
    }
    if (i == 0 && threadIdx.x == 0) ctl->fb_nq = cnt;
    if (i >= cnt) return;
    const int q = ovf_list[i];
    for (int k = threadIdx.x * 4; k < d; k += 1024)
        *reinterpret_cast<f32x4 *>(qfb + (size_t)i * d + k) = *reinterpret_cast<const f32x4 *>(q32 + (size_t)q * d + k);
    if (threadIdx.x == 0) fb_slot[q] = i;
}

}  // namespace
}  // namespace ance
