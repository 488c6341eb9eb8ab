// Two-precision exact inner-product top-k for gfx950: the fast path behind ance_ip_topk.
//
// gfx950 has no reduced-precision path for fp32 inputs (no xf32), and the exact fp32 MFMA runs at
// 1/16 of the fp16 rate.  This kernel gets the fp16 rate WITHOUT giving up bit-exact results:
//
//   1. the corpus shard is turned ONCE into a search image (ance_ip_index_build): the shard's mean row mu, every row as
//      fp16(x - mu), the maximum norms of x - mu and of x, and -- when a sample of the shard shows heavy duplicate
//      classes (the all-pad MaxP chunks of model/models.py:165-199 are millions of bit-identical rows)
//      -- every class collapsed to its smallest row id; the image is compacted, `live2row` maps image
//      rows back to shard rows and the first ids of every class are kept for the expansion in step 6;
//   2. an approximate score  s~ = b + fp16(q - mq) . fp16(x - mu)  (b, mq: "Error bound" in search_query.h) is an fp16 GEMM on the
//      256 x 256 x 64 direct-to-LDS main loop of pipe256.h (queries are the "m" side, so a lane owns a query), streamed
//      across the corpus tiles of a workgroup;
//   3. with eps a rigorous bound on the error of s~ (search_query.h) and t~ the k-th best APPROXIMATE score seen so
//      far, a row with s~ < t~ - 2 eps can never be in the exact top-k (k rows have s >= t~ - eps
//      > its s), so the per-query buffers keep exactly the rows with s~ >= t~ - 2 eps: about
//      k + 2 eps * density rows (~270 for k = 200 on LayerNorm-distributed rows).  The bound holds for
//      t~ taken over ANY subset of rows, so the workgroups that scan different corpus splits for the same
//      queries exchange their thresholds through global memory (stale values are merely weaker bounds);
//   4. the corpus is scanned in WINDOWS of ~100 MB that every workgroup of the launch finishes before any
//      moves on (a counter with a bounded spin: a scheduling hint, no data depends on it), and every list of every
//      workgroup is pruned at the same geometrically spaced tile counts: the workgroups stay within microseconds of each
//      other, the 16 of an XCD that scan the same corpus split find its tiles in their L2 (hit rate 15 % -> 58 %) and the
//      256 MB Infinity Cache serves the other XCDs;
//   5. when the scan is over, rescore_kernel (one wave per list) re-scores the rows within 2 eps of the final k-th best
//      approximate score (k-th over the list and its neighbour split's list together) with the exact fp32 fmaf chain over k ascending (the contract of oracle/ip_topk_ref.c) -- 64 rows
//      per round, one per lane, their fp32 data staged through LDS by coalesced 1 KiB LDS-DMAs -- and selects the exact
//      top-k under (score desc, row asc) from exact keys;
//   6. topk_finalize merges the splits and, for every duplicate class whose representative survived, adds
//      the class members (same exact score, ascending ids) before the final sort.
//   A query whose buffer cannot be pruned below its capacity (more than ~1,800 rows inside one 2 eps
//   band: pathologically clustered scores, fp16 overflow of that query) is appended to a device-side list
//   and redone by the exact fp32 scan -- only those queries; above 1,024 such queries per launch chunk the
//   whole chunk is redone.  Both are device-side conditionals, no host synchronisation.
//
// This file is the host side: shape limits, knobs, launch plan, workspace, orchestration.  The device code of the one
// translation unit lives in search_image.h (step 1), search_query.h (the bound; per-call query preparation),
// search_filter.h (steps 2-4) and search_rescore.h (step 5).
#include "common.h"
#include "topk_common.h"
#include "pipe256.h"
#include <stdlib.h>

namespace ance {
namespace {

constexpr int FQ = 256, FP = 256, FK = 64;
constexpr int F_OPER_HALVES = 256 * FK;
constexpr int F_STAGE_HALVES = 2 * F_OPER_HALVES;
constexpr int F_THREADS = 512;
constexpr int F_NPL = 32;
constexpr int F_C = F_NPL * 64;  // 2048 buffered rows per (block, query); a tile can add 256
constexpr size_t F_LDS_BYTES = (size_t)2 * F_STAGE_HALVES * sizeof(_Float16) + 3 * FQ * 4 + 16 + 2 * FP * 4;
constexpr int F_MAX_D = 2048;    // rescore_kernel's dynamic LDS is requested for rows of this length (rescore_lds_bytes)
constexpr int F_MAX_K = 1024;
constexpr int OVF_CAP = 1024;    // overflowing queries per launch chunk that are redone one by one

}  // namespace
}  // namespace ance

#include "search_image.h"
#include "search_query.h"
#include "search_filter.h"
#include "search_rescore.h"

namespace ance {
namespace {

int env_int(const char *name, int dflt) {
    const char *e = getenv(name);
    return e && *e ? atoi(e) : dflt;
}

// Tuning knobs of the fast path (include/ance_amd.h lists them): read from the environment ONCE, when the library first
// needs them; ance_reload_env() re-reads (tests and sweeps that change a knob inside one process call it).
struct FastKnobs {
    int splits, window_tiles, dedup, center, share, wait_us, prune_at, prune_growth;
    void load() {
        splits = env_int("ANCE_FAST_SPLITS", 0);
        window_tiles = env_int("ANCE_FAST_WINDOW_TILES", 256);
        dedup = env_int("ANCE_FAST_DEDUP", 1) != 0;
        center = env_int("ANCE_FAST_CENTER", 1) != 0;
        share = env_int("ANCE_FAST_SHARE", 1);
        wait_us = env_int("ANCE_FAST_WINDOW_WAIT_US", 200);
        prune_at = env_int("ANCE_FAST_PRUNE_AT", 512);
        prune_growth = env_int("ANCE_FAST_PRUNE_GROWTH", 150);
        if (prune_growth < 105) prune_growth = 105;
    }
};
FastKnobs &fast_knobs() {
    static FastKnobs k = [] { FastKnobs x; x.load(); return x; }();
    return k;
}

bool fast_shape_ok(int64_t n, int d, int k) {
    return d >= 128 && d % 128 == 0 && d <= F_MAX_D && k >= 1 && k <= F_MAX_K && n >= 4096 && n < (1ll << 32);
}

struct FastPlan {
    int S, Ws;
    int64_t qc;  // queries per launch
    size_t fb_bytes, fball_bytes;  // workspaces of the two exact-scan redos (OVF_CAP queries; a whole launch chunk)
};
bool make_fast_plan(int64_t n, int64_t nq, int d, int k, FastPlan *pl) {
    if (!fast_shape_ok(n, d, k) || nq < 1) return false;
    const int n_tiles = (int)((n + FP - 1) / FP);
    const int64_t nqt = (nq + FQ - 1) / FQ;
    // One workgroup per CU: (query tiles per launch) x (corpus splits) = 256.  More splits = fewer query tiles per
    // XCD (better L2 reuse of the query side) but one more candidate list per query; ANCE_FAST_SPLITS overrides.
    int S = fast_knobs().splits;
    if (S < 1 || S > 32 || (S & (S - 1))) S = 2;
    while (nqt * S < 256 && S < 32) S <<= 1;
    while (S > 1 && (S * 8 > n_tiles || next_pow2((S + DEDUP_MAXC) * k) > 8192)) S >>= 1;
    pl->S = S;
    const int64_t qct = nqt < 256 / S ? nqt : 256 / S;
    pl->qc = qct * FQ;
    // window: ANCE_FAST_WINDOW_TILES corpus tiles of 256 rows (default 256 = 100 MB of fp16 rows at d = 768; 0 = one
    // window, i.e. every split scans its contiguous share as the first version of this kernel did)
    int Wt = fast_knobs().window_tiles;
    if (Wt <= 0 || Wt > n_tiles) Wt = n_tiles;
    pl->Ws = (Wt + S - 1) / S;
    pl->fb_bytes = exact_scan_fallback_bytes(n, OVF_CAP, k);
    pl->fball_bytes = exact_scan_fallback_bytes(n, nq < pl->qc ? nq : pl->qc, k);
    return pl->fb_bytes > 0 && pl->fball_bytes > 0;
}

// The search workspace, every area in its order in memory: the one description behind both its size and its pointers
// (d_workspace = NULL: the sizes alone).  Shapes as in FastParams, with qc queries and lists = qc / FQ * S * FQ.
struct FastWorkspace {
    _Float16 *q2;
    float *qn_c, *qn_o;        // [qc] |q - mq|, |q|
    QueryStat *qstat;
    float *mq, *qpart, *bias;  // [d] mean query, [1024, d] its column-sum partials, [n + FP]
    u64 *part, *cand;
    float *thr_g;              // [lists]  \ 0xFF-filled before every launch chunk, ff_bytes from thr_g:
    int *fb_slot;              // [qc]     / NaN = no threshold yet, -1 = query not redone
    int *cnt_g;
    FastCtl *ctl;              // 256 bytes, then ovf_flag [qc] and ovf_list [OVF_CAP]: zeroed before every launch chunk,
    int *ovf_flag, *ovf_list;  // zero_bytes from ctl
    float *qfb;                // [OVF_CAP, d] the queries redone one by one
    u64 *fb_keys;              // [OVF_CAP][k] their top-k keys
    void *fb_ws, *fball_ws;    // workspaces of the two exact-scan redos
    void *image;               // where the call's own image goes when the caller brought none
    size_t bias_bytes, ff_bytes, zero_bytes;
    size_t bytes;              // everything but the image, alignment slack included
};
FastWorkspace fast_workspace(const FastPlan &pl, int64_t n, int d, int k, void *d_workspace) {
    const size_t qc = (size_t)pl.qc, lists = (size_t)(pl.qc / FQ) * pl.S * FQ;
    Carver c(d_workspace);
    FastWorkspace W;
    W.q2 = c.take<_Float16>(qc * d * sizeof(_Float16)); c.end_area();
    W.qn_c = c.take<float>(qc * sizeof(float));
    W.qn_o = c.take<float>(qc * sizeof(float)); c.end_area();
    W.qstat = c.take<QueryStat>(256);
    W.mq = c.take<float>((size_t)d * sizeof(float)); c.end_area();
    W.qpart = c.take<float>((size_t)1024 * d * sizeof(float)); c.end_area();
    W.bias = c.take<float>(((size_t)n + FP) * sizeof(float)); W.bias_bytes = c.end_area();
    W.part = c.take<u64>(qc * pl.S * k * sizeof(u64)); c.end_area();
    W.cand = c.take<u64>(lists * F_C * sizeof(u64)); c.end_area();
    W.thr_g = c.take<float>(lists * sizeof(float));
    W.fb_slot = c.take<int>(qc * sizeof(int)); W.ff_bytes = c.end_area();
    W.cnt_g = c.take<int>(lists * sizeof(int)); c.end_area();
    W.ctl = c.take<FastCtl>(256);
    W.ovf_flag = c.take<int>(qc * sizeof(int));
    W.ovf_list = c.take<int>(OVF_CAP * sizeof(int)); W.zero_bytes = c.end_area();
    W.qfb = c.take<float>((size_t)OVF_CAP * d * sizeof(float)); c.end_area();
    W.fb_keys = c.take<u64>((size_t)OVF_CAP * k * sizeof(u64)); c.end_area();
    W.fb_ws = c.take<void>(pl.fb_bytes); c.end_area();
    W.fball_ws = c.take<void>(pl.fball_bytes); c.end_area();
    W.image = c.take<void>(0);
    W.bytes = 256 + c.o;
    return W;
}

template <bool STAMPS>
void launch_filter(unsigned blocks, const FastParams &P, hipStream_t st) {  // both builds, see BIAS (search_filter.h)
    hipLaunchKernelGGL((ip_topk_fast_kernel<STAMPS, false>), dim3(blocks), dim3(F_THREADS), F_LDS_BYTES, st, P);
    hipLaunchKernelGGL((ip_topk_fast_kernel<STAMPS, true>), dim3(blocks), dim3(F_THREADS), F_LDS_BYTES, st, P);
}

unsigned long long *g_fast_stamps = nullptr;

}  // namespace

// measurement hook: while d_stamps != NULL the filter kernel is the instrumented build and every workgroup of the LAST launch
// chunk leaves uint64[8] = {prologue, main loop, filter, prune, sync, block end} ticks of the 100 MHz counter, (qt << 32 | split), XCC id
void set_fast_stamps(unsigned long long *d_stamps) { g_fast_stamps = d_stamps; }  // read by ANCE_MEASURE builds only
void reload_fast_knobs() { fast_knobs().load(); }

// ---- search image --------------------------------------------------------------------------------------
size_t ip_index_bytes(int64_t n, int d) {
    if (!fast_shape_ok(n, d, 1)) return 0;
    return image_view(nullptr, n, d).bytes + 256;
}

int ip_index_build(const float *d_x, int64_t n, int d, void *d_index, size_t index_bytes, hipStream_t st) {
    if (!fast_shape_ok(n, d, 1) || !d_x || !d_index || ((uintptr_t)d_x & 15)) {
        set_last_error("ance_ip_index_build: shape not eligible (d % 128 == 0, 128 <= d <= 2048, 4096 <= n < 2^32)");
        return ANCE_E_INVALID;
    }
    if (index_bytes < ip_index_bytes(n, d)) {
        set_last_error("ance_ip_index_build: index buffer too small");
        return ANCE_E_WORKSPACE;
    }
    const ImageView V = image_view(d_index, n, d);
    DedupHeader *H = V.hdr;
    ProfScope ps(PC_PLAN, st);
    (void)hipMemsetAsync(H, 0, 256, st);
    hipLaunchKernelGGL(idx_colsum_kernel, dim3((unsigned)V.n_part), dim3(256), 0, st, d_x, n, d, V.part);
    hipLaunchKernelGGL(idx_mean_kernel, dim3((unsigned)((d + 255) / 256)), dim3(256), 0, st, V.part, V.n_part, n, d,
                       fast_knobs().center, V.mu);
    if (fast_knobs().dedup) {
        hipLaunchKernelGGL(idx_sample_hash_kernel, dim3(IDX_SAMPLES / 4), dim3(256), 0, st, d_x, n, d, V.samp);
        hipLaunchKernelGGL(idx_find_classes_kernel, dim3(1), dim3(256), 0, st, V.samp, n, H);
        const unsigned cb = (unsigned)(((n + 63) / 64 + 3) / 4 < 4096 ? ((n + 63) / 64 + 3) / 4 : 4096);
        hipLaunchKernelGGL(idx_classify_kernel, dim3(cb), dim3(256), 0, st, d_x, n, d, H, V.cls);
        hipLaunchKernelGGL(idx_count_kernel, dim3((unsigned)V.nb), dim3(256), 0, st, n, V.nb, H, V.cls, V.blk);
        hipLaunchKernelGGL(idx_scan_kernel, dim3(1), dim3(1024), 0, st, V.nb, H, V.blk);
    }
    hipLaunchKernelGGL(idx_compact_round_kernel, dim3((unsigned)V.nb), dim3(256), 0, st, d_x, n, d, V.nb, H, V.cls, V.blk, V.mu, V.x2,
                       V.live2row, V.members);
    hipLaunchKernelGGL(idx_stamp_kernel, dim3(1), dim3(64), 0, st, H, n, d, d_x);  // last: marks the build complete
    return check_launch("ance_ip_index_build");
}

size_t ip_topk_fast_workspace_bytes(int64_t n, int64_t nq, int d, int k, bool with_index) {
    FastPlan pl;
    if (!make_fast_plan(n, nq, d, k, &pl)) return 0;
    return fast_workspace(pl, n, d, k, nullptr).bytes + (with_index ? ip_index_bytes(n, d) : 0);
}

int ip_topk_fast(const float *d_x, int64_t n, int64_t row_base, const void *d_index, const float *d_q, int64_t nq, int d, int k,
                 float *d_out_d, int64_t *d_out_i, void *d_workspace, size_t workspace_bytes, hipStream_t st) {
    FastPlan pl;
    if (!make_fast_plan(n, nq, d, k, &pl)) {
        set_last_error("ip_topk_fast: shape not eligible");
        return ANCE_E_INVALID;
    }
    if (workspace_bytes < ip_topk_fast_workspace_bytes(n, nq, d, k, d_index == nullptr)) {
        set_last_error("ip_topk_fast: workspace too small");
        return ANCE_E_WORKSPACE;
    }
    const FastWorkspace W = fast_workspace(pl, n, d, k, d_workspace);
    if (!d_index) {
        const int rc = ip_index_build(d_x, n, d, W.image, ip_index_bytes(n, d), st);
        if (rc) return rc;
        d_index = W.image;
    }
    const ImageView V = image_view(d_index, n, d);  // read only from here on

    static unsigned long long attr_done = 0;
    if (attr_needed(&attr_done)) {
        bool ok = true;
        for (const void *fn : {reinterpret_cast<const void *>(ip_topk_fast_kernel<false, false>),
#ifdef ANCE_MEASURE
                               reinterpret_cast<const void *>(ip_topk_fast_kernel<true, false>),
                               reinterpret_cast<const void *>(ip_topk_fast_kernel<true, true>),
#endif
                               reinterpret_cast<const void *>(ip_topk_fast_kernel<false, true>)})
            ok = ok && hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)F_LDS_BYTES) == hipSuccess;
        if (!ok)
            return check_launch("ip_topk_fast attr");
        if (hipFuncSetAttribute(reinterpret_cast<const void *>(rescore_kernel), hipFuncAttributeMaxDynamicSharedMemorySize,
                                (int)rescore_lds_bytes(F_MAX_D)) != hipSuccess)
            return check_launch("rescore attr");
        attr_mark(&attr_done);
    }
    const EpsConst eps = make_eps(d);
    const FastKnobs &kn = fast_knobs();
    // ---- the mean query of this call and its per-row share of every score (skipped on the device when |mq| is small) ----
    {
        const int n_part_q = (int)(nq < 1024 ? nq : 1024);
        ProfScope ps(PC_PLAN, st);
        hipLaunchKernelGGL(idx_colsum_kernel, dim3((unsigned)n_part_q), dim3(256), 0, st, d_q, nq, d, W.qpart);
        hipLaunchKernelGGL(idx_mean_kernel, dim3((unsigned)((d + 255) / 256)), dim3(256), 0, st, W.qpart, n_part_q, nq, d, kn.center,
                           W.mq);
        hipLaunchKernelGGL(query_mean_decide_kernel, dim3(1), dim3(256), 0, st, W.mq, d, V.hdr, W.qstat, n, d_x);
        (void)hipMemsetAsync(W.bias, 0, W.bias_bytes, st);
        hipLaunchKernelGGL(row_bias_kernel, dim3(4096), dim3(256), 0, st, d_x, d, V.hdr,
                           V.live2row, V.mu, W.mq, W.qstat, W.bias);
    }
    for (int64_t q0 = 0; q0 < nq; q0 += pl.qc) {
        const int64_t nqc = (nq - q0) < pl.qc ? (nq - q0) : pl.qc;
        const float *q32 = d_q + (size_t)q0 * d;
        (void)hipMemsetAsync(W.thr_g, 0xFF, W.ff_bytes, st);
        (void)hipMemsetAsync(W.ctl, 0, W.zero_bytes, st);
        {
            ProfScope ps(PC_PLAN, st);
            hipLaunchKernelGGL(round_rows_kernel, dim3((unsigned)((nqc + 3) / 4 < 8192 ? (nqc + 3) / 4 : 8192)), dim3(256), 0, st,
                               q32, nqc, d, W.mq, W.q2, W.qn_c, W.qn_o);
        }
        FastParams P;
        P.q2 = W.q2; P.x2 = V.x2; P.q32 = q32; P.x32 = d_x; P.qnorm_c = W.qn_c; P.qnorm_o = W.qn_o; P.qstat = W.qstat; P.bias = W.bias;
        P.hdr = V.hdr; P.live2row = V.live2row;
        P.nq = (uint32_t)nqc; P.d = d; P.k = k; P.S = pl.S; P.Ws = pl.Ws;
        P.n_qt = (int)((nqc + FQ - 1) / FQ);
        P.share = kn.share && pl.S > 1; P.wait_ticks = (unsigned)(kn.wait_us > 0 ? kn.wait_us * 100 : 0);
        P.eps = eps; P.cand = W.cand; P.part = W.part; P.thr_g = W.thr_g; P.ctl = W.ctl;
        P.ovf_flag = W.ovf_flag; P.ovf_list = W.ovf_list; P.cnt_g = W.cnt_g;
        P.prune_at = kn.prune_at > k + 64 ? kn.prune_at : k + 64;
        if (P.prune_at > F_C - FP) P.prune_at = F_C - FP;
        P.prune_growth = kn.prune_growth;
        P.stamps = nullptr;
        const int gq = 32 / pl.S;
        const int groups = (P.n_qt + gq - 1) / gq;
        const unsigned blocks = (unsigned)((groups + 7) / 8 * 8) * 32u;
        {
            ProfScope ps(PC_SCAN, st, 2.0 * (double)nqc * (double)n * (double)d);
#ifdef ANCE_MEASURE  // the instrumented builds (per-workgroup time stamps) exist in the measurement library only
            P.stamps = g_fast_stamps;  // measurement hook (ance_debug_search_stamps)
            if (P.stamps) launch_filter<true>(blocks, P, st);
            else
#endif
                launch_filter<false>(blocks, P, st);
        }
        {
            RescoreParams R;
            R.q32 = q32; R.x32 = d_x; R.qnorm_c = W.qn_c; R.qnorm_o = W.qn_o; R.qstat = W.qstat; R.hdr = V.hdr; R.live2row = V.live2row;
            R.cand = W.cand; R.cnt_g = W.cnt_g; R.thr_g = W.thr_g; R.part = W.part; R.nq = P.nq; R.d = d; R.k = k; R.S = pl.S; R.eps = eps;
            ProfScope ps(PC_RESCORE, st);
            hipLaunchKernelGGL(rescore_kernel, dim3((unsigned)(P.n_qt * pl.S * FQ)), dim3(64), rescore_lds_bytes(d), st, R);
        }
        // queries whose buffers overflowed: redone by the exact scan, one by one (<= OVF_CAP) or as a whole chunk
        hipLaunchKernelGGL(gather_overflow_kernel, dim3(OVF_CAP), dim3(256), 0, st, W.ctl, W.qstat,
                           W.ovf_list, q32, d, W.qfb, W.fb_slot);
        const u64 *fb_part = nullptr, *fball_part = nullptr;
        int fb_m = 0, fball_m = 0;
        int rc = exact_scan_fallback(d_x, n, W.qfb, OVF_CAP, OVF_CAP, d, k, W.fb_ws, nullptr, &W.ctl->fb_nq, &fb_part, &fb_m, st);
        if (rc) return rc;
        rc = launch_reduce_keys(fb_part, OVF_CAP, fb_m, k, W.fb_keys, &W.ctl->fb_nq, st);
        if (rc) return rc;
        rc = exact_scan_fallback(d_x, n, q32, nqc, nq < pl.qc ? nq : pl.qc, d, k, W.fball_ws, &W.ctl->fb_all, nullptr, &fball_part,
                                 &fball_m, st);
        if (rc) return rc;
        FinalizeAlt alt;
        alt.sel_all = &W.ctl->fb_all; alt.all_keys = fball_part; alt.all_m = fball_m;
        alt.slot = W.fb_slot; alt.slot_keys = W.fb_keys; alt.slot_m = k;
        alt.dd = V.hdr; alt.members = V.members;
        rc = launch_finalize_keys(W.part, nqc, pl.S * k, k, row_base, d_out_d + (size_t)q0 * k, d_out_i + (size_t)q0 * k, st, &alt);
        if (rc) return rc;
    }
    return check_launch("ip_topk_fast");
}

}  // namespace ance

// include/ance_amd.h: how many ance_ip_topk_indexed calls (per launch chunk) on the current device ignored their image.
// Synchronises the device (a diagnostic, not a data-path call).
extern "C" int ance_search_bad_image_calls(unsigned long long *out) {
    using namespace ance;
    if (!out) {
        set_last_error("ance_search_bad_image_calls: invalid argument");
        return ANCE_E_INVALID;
    }
    if (hipMemcpyFromSymbol(out, HIP_SYMBOL(g_bad_image_calls), sizeof(*out)) != hipSuccess) return check_launch("ance_search_bad_image_calls");
    return ANCE_OK;
}
