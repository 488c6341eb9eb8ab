// The streaming filter of the two-precision search (ip_topk_fast.hip, steps 2-4): the fp16 GEMM of pipe256.h over the
// corpus tiles of a workgroup, the 2 eps filter into per-query candidate lists, their prunes and the window hand-shake.
// Included by ip_topk_fast.hip only (after its shape constants), into its anonymous namespace.
#pragma once
#include "pipe256.h"
#include "search_query.h"

namespace ance {
namespace {

// ---- per-launch control block (device, zeroed before every launch chunk) ------------------------------
struct FastCtl {
    unsigned int win_arrived;  // workgroups that finished a corpus window (monotonic over the launch)
    int ovf_count;             // queries appended to ovf_list (may exceed OVF_CAP)
    int fb_nq;                 // queries the per-query exact scan redoes (0 when the whole chunk is redone)
    int fb_all;                // != 0: the whole chunk is redone by the exact scan
};

struct FastParams {
    const _Float16 *q2;  // [nq, d]  fp16(q - mq)
    const _Float16 *x2;  // [n_live, d] fp16 image rows
    const float *q32;    // [nq, d]
    const float *x32;    // [n, d] shard rows
    const float *qnorm_c, *qnorm_o;  // [nq] |q - mq|, |q|
    const QueryStat *qstat;
    const float *bias;   // [n_live + 256] mq . x' per image row (read only when qstat->use_bias)
    const DedupHeader *hdr;
    const uint32_t *live2row;
    uint32_t nq;
    int d, k, S, n_qt;
    int Ws;              // corpus tiles per split per window (a window is S * Ws tiles)
    int share;           // exchange thresholds between the splits of a query tile
    unsigned int wait_ticks;  // bound of the window wait (100 MHz ticks)
    EpsConst eps;
    u64 *cand;     // [n_qt * S][FQ][F_C]
    u64 *part;     // [nq][S][k]
    float *thr_g;  // [n_qt * S][FQ] published thresholds (NaN = none yet)
    int *cnt_g;    // [n_qt * S][FQ] rows left in every buffer (for rescore_kernel)
    FastCtl *ctl;
    int *ovf_flag;  // [nq] 0 / 1
    int *ovf_list;  // [OVF_CAP]
    int prune_at;           // first scheduled prune once every list has this many rows (<= F_C - FP)
    int prune_growth;       // percent: the tile count between scheduled prunes grows by this factor (150 = 1.5x)
    unsigned long long *stamps;  // measurement: [workgroup][8] accumulated 100 MHz ticks (STAMPS kernel only)
};

// Source policy of the streamed main loop (pipe256.h).  Both operands go through buffer descriptors (wave-uniform
// SGPRs) + one 32-bit per-lane byte offset per staged piece that never changes during the kernel, + the K offset in an
// SGPR: 8 address VGPRs in all.  (With flat 64-bit addresses hipcc keeps a pointer pair per piece for the current AND
// the next corpus tile, spills, and every spill reload in the tile loop is a vmcnt(0) that drains the prefetch.)
// The descriptor of a corpus tile covers exactly its rows that exist (<= 256), the one of the query tile its real
// queries: rows past the end read as zeros (hardware range check) and are masked in the filter.
// K-tile t >= NK belongs to the NEXT corpus tile of this workgroup's sequence (descriptor rx1).
struct FastSrc {
    __amdgpu_buffer_rsrc_t rq, rx0, rx1;
    uint32_t voff[4][2];  // [A-half0, A-half1, B-half0, B-half1][piece]: (row of the 256-row tile) * d * 2 + chunk * 2 bytes
    int NK;
    template <int TYPE, int J>
    __device__ __forceinline__ void issue(int t, pipe_lds_t *dst) const {
        const bool nxt = t >= NK;
        const int so = (nxt ? t - NK : t) * (FK * 2);
        if constexpr (TYPE < 2) __builtin_amdgcn_raw_ptr_buffer_load_lds(rq, dst, 16, voff[TYPE][J], so, 0, 0);
        else __builtin_amdgcn_raw_ptr_buffer_load_lds(nxt ? rx1 : rx0, dst, 16, voff[TYPE][J], so, 0, 0);
    }
    // PRECOMPUTE (pipe256.h): the K offsets of the eight LDS-DMAs of a K-tile and the corpus descriptor of K-tile t + 2 are
    // computed ONCE per K-tile, in the read half-phase -- the compare / select / shift chains (and the four s_cselect of the descriptor)
    // used to sit in front of each DMA, between the MFMAs, fenced there by the schedule's sched_barriers: ~25 scalar instructions per
    // K-tile in the matrix pipe's shadow.
    static constexpr bool PRECOMPUTE = true;
    int so_1, so_2;                // K offset (bytes) of K-tile t + 1 (A-half1) and of K-tile t + 2 (A-half0, B-half0, B-half1)
    __amdgpu_buffer_rsrc_t rx_2;   // corpus descriptor of K-tile t + 2
    __device__ __forceinline__ void prepare(int t) {
        const int t1 = t + 1, t2 = t + 2;
        so_1 = (t1 >= NK ? t1 - NK : t1) * (FK * 2);
        so_2 = (t2 >= NK ? t2 - NK : t2) * (FK * 2);
        rx_2 = t2 >= NK ? rx1 : rx0;
    }
    template <int TYPE, int J>
    __device__ __forceinline__ void issue_pre(pipe_lds_t *dst) const {
        if constexpr (TYPE == 1) __builtin_amdgcn_raw_ptr_buffer_load_lds(rq, dst, 16, voff[TYPE][J], so_1, 0, 0);
        else if constexpr (TYPE == 0) __builtin_amdgcn_raw_ptr_buffer_load_lds(rq, dst, 16, voff[TYPE][J], so_2, 0, 0);
        else __builtin_amdgcn_raw_ptr_buffer_load_lds(rx_2, dst, 16, voff[TYPE][J], so_2, 0, 0);
    }
};

__device__ __forceinline__ __amdgpu_buffer_rsrc_t tile_rsrc(const _Float16 *base, uint32_t first_row, uint32_t n_rows, int d) {
    return pipe_rows_rsrc(base, first_row, d, first_row < n_rows ? min(n_rows - first_row, 256u) : 0u);
}

// v_max3_f32 without the canonicalisation (v_max_f32 x, x) hipcc puts in front of every fmaxf operand it cannot prove quiet.
// NaN operands lose against numbers, like fmaxf.  The caller pads the MFMA -> VALU hazard of the first use.
__device__ __forceinline__ float max3_f32(float a, float b, float c) {
    float r;
    asm volatile("v_max3_f32 %0, %1, %2, %3" : "=v"(r) : "v"(a), "v"(b), "v"(c));
    return r;
}

__device__ __forceinline__ float load_thr(const float *p) {
    return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

#define STAMP(acc)                                      \
    if constexpr (STAMPS) {                             \
        const unsigned long long now_ = wall_clock64(); \
        acc += now_ - t_last;                           \
        t_last = now_;                                  \
    }

// One wave prunes one list in place: the k-th largest approximate key by radix select, then every row whose approximate
// score is below max(that score - 2 eps, thr_other) goes.  Returns the rows kept; *thr_out = the new filter threshold.
template <int NPL>
__device__ __forceinline__ int prune_list(u64 *cq, int n_c, int lp, int k, float eps2, float thr_other, float *thr_out) {
    u64 keys[NPL];
#pragma unroll
    for (int j = 0; j < NPL; ++j) {
        const int idx = j * 64 + lp;
        keys[j] = (idx < n_c) ? cq[idx] : 0ull;
    }
    u64 T = 0;  // k-th largest approximate key
    for (int bit = 63; bit >= 0; --bit) {
        const u64 t2 = T | (1ull << bit);
        int ge = 0;
#pragma unroll
        for (int j = 0; j < NPL; ++j) ge += __popcll(__ballot(keys[j] >= t2));
        if (ge >= k) T = t2;
    }
    const float thr_new = fmaxf(key_score(T) - eps2, thr_other);
    int base = 0;
    const u64 lt_mask = (1ull << lp) - 1ull;
#pragma unroll
    for (int j = 0; j < NPL; ++j) {
        const bool keep = keys[j] != 0ull && !(key_score(keys[j]) < thr_new);
        const u64 m = __ballot(keep);
        if (keep) cq[base + __popcll(m & lt_mask)] = keys[j];
        base += __popcll(m);
    }
    *thr_out = thr_new;
    return base;
}

// BIAS: the build that starts every corpus tile's accumulators from the per-row share of the mean query (search_query.h).  Both
// builds are launched for every chunk and the one the device-side decision (QueryStat) did not pick returns at once: the
// choice needs no host synchronisation, and the common case keeps the leaner kernel (the bias build is ~5 % slower).
template <bool STAMPS, bool BIAS>
__global__ void __launch_bounds__(F_THREADS, 2) ip_topk_fast_kernel(const FastParams P) {
    if ((P.qstat->use_bias != 0) != BIAS || P.qstat->bad_image) return;
    extern __shared__ __attribute__((aligned(16))) float smem_f[];
    _Float16 *smem = reinterpret_cast<_Float16 *>(smem_f);
    float *thr_s = smem_f + (2 * F_STAGE_HALVES) / 2;  // after the 128 KiB of stages: filter threshold t~ - 2 eps
    float *eps2_s = thr_s + FQ;                         // 2 eps per query
    int *cnt_s = reinterpret_cast<int *>(eps2_s + FQ);

    // block -> (query tile, corpus split).  32 blocks of an XCD run at once (1 per CU): a group is
    // 32/S query tiles x S splits, so an XCD keeps few query tiles hot and shares each corpus tile.
    const int b = blockIdx.x, xcd = b & 7, jx = b >> 3;
    const int gq = 32 / P.S;
    const int grp = (jx >> 5) * 8 + xcd;
    const int r32 = jx & 31;
    const int qt = grp * gq + r32 / P.S;
    const int split = r32 % P.S;
    if (qt >= P.n_qt) return;

    const int tid = threadIdx.x;
    const int w = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int l = tid & 63;
    const int wm = w >> 2, wn = w & 3;  // wave tile: 128 queries x 64 passages
    const uint32_t q0 = (uint32_t)qt * FQ;
    const int d = P.d;
    const uint32_t n = P.hdr->n_live;  // rows of the image (device side: duplicates were collapsed there)
    const int n_tiles = (int)((n + FP - 1) / FP);
    const int W = P.Ws * P.S;
    const int n_win = (n_tiles + W - 1) / W;
    const unsigned n_part = (unsigned)(P.n_qt * P.S);
    u64 *cand = P.cand + ((size_t)qt * P.S + split) * (size_t)FQ * F_C;
    float *thr_mine = P.thr_g + ((size_t)qt * P.S + split) * FQ;
    const float *thr_tile = P.thr_g + (size_t)qt * P.S * FQ;

    if (tid < FQ) {
        const uint32_t qg = q0 + tid;
        thr_s[tid] = -INFINITY;
        cnt_s[tid] = 0;
        // the bound assumes no fp16 overflow: |x_j| <= ||x||, so norms <= 65504 exclude it.  Otherwise eps = inf
        // keeps every row until the buffer overflows and the query is redone by the exact scan.
        eps2_s[tid] = two_eps(P.eps, qg < P.nq ? P.qnorm_c[qg] : 0.0f, qg < P.nq ? P.qnorm_o[qg] : 0.0f, P.qstat, P.hdr);
    }

    // ---- main loop: the ping-pong pipeline of pipe256.h, streamed across this workgroup's corpus tiles ----
    // A operand = the block's 256 queries (re-read from L2 for every corpus tile), B operand = image rows.
    // Tile sequence: window by window, inside a window the Ws tiles of this split.  K-tile index t of the tile
    // being computed; t >= NK addresses the next tile of the sequence, so the LDS-DMA prefetch (5-6 phases
    // ahead) runs through the filter step into the next tile.
    Pipe256T<FastSrc> pipe;
    pipe.init(smem, w, l);
    {
        FastSrc &S = pipe.S;
        S.NK = d / FK;
        S.rq = tile_rsrc(P.q2, q0, P.nq, d);
        // (pipe_fill_voff would do; written out because this kernel's instruction stream comes out different with it: profiles/README.md, r10)
        const int ch = pipe_stage_chunk(pipe_stage_row(w, l, 0), l);  // rows of piece 1 are 64 further: same swizzle
#pragma unroll
        for (int h = 0; h < 2; ++h)
#pragma unroll
            for (int j = 0; j < 2; ++j) {
                const int r = pipe_stage_row(w, l, j);
                S.voff[h][j] = (uint32_t)(pipe_a_tile_row(h, r) * d + ch) * 2u;
                S.voff[2 + h][j] = (uint32_t)(pipe_b_tile_row(h, r) * d + ch) * 2u;
            }
    }
    const int NK = d / FK;
    // Prune schedule.  The filter threshold is only as fresh as the last prune, and for most of the scan the insertion
    // rate is (rows kept at the last prune) / (rows seen at the last prune) per row: waiting for a full buffer (1,792
    // rows) lets the rows seen grow 6.6x between prunes and has ~1 insertion per (wave, query group) per tile.  Every
    // list of the workgroup is therefore pruned at the SAME geometrically spaced tile counts (x P.prune_growth / 100:
    // ~24 episodes over 17 k tiles at 1.5x): thresholds stay within 1.5x of fresh, and because every workgroup of the
    // launch follows the same schedule the episodes (a vmcnt(0) drain + ~0.3 ms of selection) coincide instead of
    // making a different workgroup the straggler of every window.  A buffer that fills up in between is pruned at once.
    int *epoch_s = cnt_s + FQ;  // last tile (1-based) in which some wave asked for an unscheduled prune
    if (tid == 0) *epoch_s = 0;
    // Per-row bias b = mq . x' of the corpus tile (search_query.h: the mean query's share of every score): two 1 KiB LDS slots,
    // filled by ONE LDS-DMA of wave 0 a whole tile ahead -- the instruction is older than every staging DMA the pipeline
    // counts, so the pipeline's own waits and barriers retire and publish it -- and read back as the accumulators' start.
    float *bias_s = reinterpret_cast<float *>(epoch_s + 4);
    int bbuf = 0;
    auto stage_bias = [&](int tile, int buf) {
        if (w == 0) {
            int lb = l;  // (laundered: keeps the per-lane address out of the tile loop's live registers, see the filter)
            asm volatile("" : "+v"(lb));
            __builtin_amdgcn_global_load_lds((pipe_glb_t *)(P.bias + (size_t)tile * FP + lb * 4), (pipe_lds_t *)(bias_s + buf * FP), 16, 0, 0);
        }
    };
    int n_done = 0, next_sched = max(1, (P.prune_at + FP - 1) / FP);

    unsigned long long t_last = 0, a_main = 0, a_filter = 0, a_prune = 0, a_sync = 0, a_end = 0, a_pro = 0;
    if constexpr (STAMPS) t_last = wall_clock64();

    int t = split * P.Ws, jw = 0, win = 0;
    bool have = t < n_tiles;
    if (have) {
        if constexpr (BIAS) stage_bias(t, 0);
        pipe.S.rx0 = tile_rsrc(P.x2, (uint32_t)t * FP, n, d);
        pipe.S.rx1 = pipe.S.rx0;
        pipe.prologue();  // also publishes thr_s / cnt_s / eps2_s / epoch_s
    } else {
        __syncthreads();
    }
    STAMP(a_pro)

    while (have) {
        int tn, jn = jw + 1, winn = win;
        if (jn < P.Ws) {
            tn = t + 1;
        } else {
            jn = 0;
            winn = win + 1;
            tn = winn * W + split * P.Ws;
        }
        const bool have_n = tn < n_tiles;
        const uint32_t p0 = (uint32_t)t * FP;
        pipe.S.rx0 = tile_rsrc(P.x2, p0, n, d);
        pipe.S.rx1 = tile_rsrc(P.x2, (uint32_t)tn * FP, n, d);
        f32x16 acc[2][4];
        if constexpr (BIAS) {
            if (have_n) stage_bias(tn, bbuf ^ 1);
            // acc[x][y][4 rq + j] <- b[row p0 + wn*64 + x*32 + 8 rq + 4 g + j], the same for the four query groups y
            int lb = l;
            asm volatile("" : "+v"(lb));
            const float *bs = bias_s + bbuf * FP + wn * 64 + 4 * (lb >> 5);
#pragma unroll
            for (int x = 0; x < 2; ++x)
#pragma unroll
                for (int rq = 0; rq < 4; ++rq) {
                    const f32x4 v = *reinterpret_cast<const f32x4 *>(bs + x * 32 + 8 * rq);
#pragma unroll
                    for (int y = 0; y < 4; ++y)
#pragma unroll
                        for (int j = 0; j < 4; ++j) acc[x][y][4 * rq + j] = v[j];
                }
            bbuf ^= 1;
        } else {
#pragma unroll
            for (int x = 0; x < 2; ++x)
#pragma unroll
                for (int y = 0; y < 4; ++y) acc[x][y] = f32x16{0};
        }
        pipe.enter();
        if (have_n) pipe.tiles_streaming(NK, acc);
        else pipe.tiles_final(NK, acc);
        pipe.leave();
        STAMP(a_main)

        // ---- filter: keep every row whose approximate score is within 2 eps of the k-th best -------
        // acc[x][y][r]: passage = p0 + wn*64 + x*32 + (r&3) + 8 (r>>2) + 4 g ; query = q0 + wm*128 + y*32 + i
        // (the lane id is laundered through an empty asm: hipcc otherwise hoists every lane-derived address of this
        // section out of the tile loop, runs out of registers and reloads them from scratch here -- and a scratch
        // reload is a vmcnt(0) wait that drains the LDS-DMA prefetch of the next tile)
        int lf = l;
        asm volatile("" : "+v"(lf));
        const int gf = lf >> 5, qf = wm * 128 + (lf & 31);
        const uint32_t pw0 = p0 + wn * 64 + 4 * gf;
        const bool ragged = p0 + FP > n;  // uniform: rows past n were staged as zeros
        // MFMA results -> VALU reads inside asm statements: the compiler does not pad that hazard for us
        __builtin_amdgcn_sched_barrier(0);
        asm volatile("s_nop 15\n\ts_nop 15" ::: "memory");
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int y = 0; y < 4; ++y) {
            const int ql = qf + y * 32;
            const bool qv = (q0 + ql) < P.nq;
            const float thr = thr_s[ql];  // -inf until the first prune
            // Once the threshold is set few rows pass: take the maximum of the lane's 32 scores first and skip the whole
            // group when no lane of the wave has a candidate.  Scores are finite (fp16_ok above), so the maximum loses
            // nothing.  Not on a ragged last tile (clamped rows).  Quarter maxima (8 scores each) come out of the same
            // max tree (v_max3_f32: 18 instructions per 32 scores): the per-score compare-and-insert code only runs for
            // the quarters that hold a candidate somewhere in the wave.
            float mq[4];
#pragma unroll
            for (int qd = 0; qd < 4; ++qd) {
                const int x = qd >> 1, rb = (qd & 1) * 8;
                float m = max3_f32(acc[x][y][rb], acc[x][y][rb + 1], acc[x][y][rb + 2]);
                m = max3_f32(m, acc[x][y][rb + 3], acc[x][y][rb + 4]);
                m = max3_f32(m, acc[x][y][rb + 5], acc[x][y][rb + 6]);
                mq[qd] = max3_f32(m, acc[x][y][rb + 7], acc[x][y][rb + 7]);
            }
            if (!ragged) {
                const float mx = max3_f32(max3_f32(mq[0], mq[1], mq[2]), mq[3], mq[3]);
                if (__ballot(qv && !(mx < thr)) == 0ull) continue;
            }
            u64 *cq = cand + (size_t)ql * F_C;
#pragma unroll
            for (int qd = 0; qd < 4; ++qd) {
                if (!ragged && __ballot(qv && !(mq[qd] < thr)) == 0ull) continue;
                const int x = qd >> 1, rb = (qd & 1) * 8;
#pragma unroll
                for (int r = rb; r < rb + 8; ++r) {
                    const uint32_t prow = pw0 + x * 32 + (r & 3) + 8 * (r >> 2);
                    const float sc = acc[x][y][r];
                    if (qv && prow < n && !(sc < thr)) {
                        const int sl = atomicAdd(&cnt_s[ql], 1);
                        cq[sl] = pack_key(sc, prow);
                    }
                }
            }
        }
        // ---- prune buffers that could overflow on the next tile (approximate keys) --------------------
        // Barriers here are raw s_barriers: a __syncthreads would drain the LDS-DMA prefetch of the next
        // tile (vmcnt(0)).  Only when some buffer really needs a prune (a few times per query, early in
        // the scan) do all waves retire their candidate stores before anybody reads them back.
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
        __builtin_amdgcn_s_barrier();
        STAMP(a_filter)
        ++n_done;
        const bool sched = n_done == next_sched;  // uniform
        if (sched) next_sched = max(next_sched + 1, (int)(((long long)next_sched * P.prune_growth) / 100));
        {
            const int c32 = cnt_s[w * 32 + (l & 31)];
            if (__ballot(c32 > F_C - FP) != 0ull && l == 0) *epoch_s = t + 1;
        }
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
        __builtin_amdgcn_s_barrier();
        if (sched || *epoch_s == t + 1) {  // block-uniform
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
            __builtin_amdgcn_s_barrier();
            int lp = l;  // laundered like lf above: keeps the 32 buffer positions j * 64 + lane out of the tile loop's registers
            asm volatile("" : "+v"(lp));
            // queries of this wave whose buffer passed its trigger (lane q < 32 looks at query w * 32 + q)
            u64 need = __ballot(lp < 32 && cnt_s[w * 32 + (lp & 31)] > (sched ? P.k + 32 : F_C - FP));
            while (need) {
                const int qq = __builtin_ctzll(need);
                need &= need - 1;
                const int ql = w * 32 + qq;
                const int n_c = __builtin_amdgcn_readfirstlane(cnt_s[ql]);
                {
                    u64 *cq = cand + (size_t)ql * F_C;
                    float thr_other = -INFINITY;
                    if (P.share) {  // what the other splits of this query have established is just as valid here
                        float o = (lp < P.S && lp != split) ? load_thr(thr_tile + (size_t)lp * FQ + ql) : -INFINITY;
#pragma unroll
                        for (int off = 16; off > 0; off >>= 1) o = fmaxf(o, __shfl_xor(o, off));  // S <= 32; NaN = none
                        thr_other = __shfl(o, 0);
                    }
                    float thr_new;
                    int base;  // (scheduled prunes see a few hundred rows: 8 keys per lane instead of 32)
                    if (n_c <= 8 * 64) base = prune_list<8>(cq, n_c, lp, P.k, eps2_s[ql], thr_other, &thr_new);
                    else if (n_c <= 16 * 64) base = prune_list<16>(cq, n_c, lp, P.k, eps2_s[ql], thr_other, &thr_new);
                    else base = prune_list<F_NPL>(cq, n_c, lp, P.k, eps2_s[ql], thr_other, &thr_new);
                    if (lp == 0) {
                        if (base > F_C - FP) {  // more than 1,792 rows inside one 2 eps band: this query is redone exactly
                            if (atomicExch(&P.ovf_flag[q0 + ql], 1) == 0) {
                                const int slot = atomicAdd(&P.ctl->ovf_count, 1);
                                if (slot < OVF_CAP) P.ovf_list[slot] = (int)(q0 + ql);
                            }
                            base = F_C - FP;
                        }
                        cnt_s[ql] = base;
                        thr_s[ql] = thr_new;
                        if (P.share) __hip_atomic_store(thr_mine + ql, thr_new, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                    }
                }
            }
        }
        STAMP(a_prune)
        // ---- window boundary: wait (bounded) for the other workgroups, adopt their thresholds ----------
        if (winn != win && winn < n_win) {  // block-uniform
            if (tid == 0) {
                __hip_atomic_fetch_add(&P.ctl->win_arrived, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                if (have_n && P.wait_ticks) {
                    const unsigned target = (unsigned)(win + 1) * n_part;
                    const unsigned long long t_in = wall_clock64();
                    while (__hip_atomic_load(&P.ctl->win_arrived, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) < target) {
                        __builtin_amdgcn_s_sleep(64);
                        if (wall_clock64() - t_in > P.wait_ticks) break;
                    }
                }
            }
            asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
            __builtin_amdgcn_s_barrier();
            if (P.share && tid < FQ) {
                float m = thr_s[tid];
                for (int s2 = 0; s2 < P.S; ++s2)
                    if (s2 != split) m = fmaxf(m, load_thr(thr_tile + (size_t)s2 * FQ + tid));
                thr_s[tid] = m;
            }
        }
        // thr_s / cnt_s updates are published by the barriers of the next tile's main loop
        t = tn; jw = jn; win = winn; have = have_n;
        STAMP(a_sync)
    }
    __syncthreads();

    // ---- hand the lists to rescore_kernel: rows buffered, final threshold --------------------------------------
    if (tid < FQ) {
        P.cnt_g[((size_t)qt * P.S + split) * FQ + tid] = cnt_s[tid];
        thr_mine[tid] = thr_s[tid];  // (thr_g doubles as the final-threshold array: nobody reads it during the scan any more
                                     //  once every split of this query tile is done, and a stale read is only a weaker bound)
    }
    if constexpr (STAMPS) {
        STAMP(a_end)
        if (tid == 0) {
            unsigned long long *o = P.stamps + (size_t)blockIdx.x * 8;
            o[0] = a_pro; o[1] = a_main; o[2] = a_filter; o[3] = a_prune; o[4] = a_sync; o[5] = a_end;
            o[6] = (unsigned long long)qt << 32 | (unsigned)split;
            o[7] = __builtin_amdgcn_s_getreg(0x1814) /* XCC_ID */;
        }
    }
}

}  // namespace
}  // namespace ance
