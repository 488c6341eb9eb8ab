// The 256 x 256 output tile of the encoder GEMMs (gemm256_f16.hip): which tile a workgroup computes, the LDS maps, and the epilogue's
// parameter block (slice partials of the tile's 256 tokens, bias / csum / gamma / beta of its 256 features) next to them.
#pragma once
#include "common.h"
#include "gemm_f16.h"
#include "pipe256.h"

namespace ance {

constexpr int TM = 256, TN = 256, TK = 64;      // TK halves = 128 B per LDS row
constexpr int G256_THREADS = 512;
constexpr size_t G256_LDS_BYTES = PIPE_LDS_BYTES;  // two K-tile buffers of A-rows tile + B-rows tile: 128 KiB

// XCD-aware tile order (speed only).  Blocks b, b + 8, ... share an XCD (and its 4 MiB L2).  The dimension with more tiles
// is dealt round-robin to the XCDs, the other one is swept fastest, so the panel of the outer dimension stays in that XCD's L2
// while the inner panels stream through it.  N-SPLIT (round 4): when the inner dimension's operand does not fit the L2 -- FFN1:
// 12 weight tiles x 384 KiB = 4.5 MiB, re-fetched for every token panel: 994 MB of L2 fills + writes per launch against
// 510 MB algorithmic (profiles/pmc_traffic.json, r03) -- the XCDs pair up: XCD x sweeps only the N-tiles of half x & 1 (2.25 MiB,
// resident) for the token panels = x >> 1 (mod 4).  A token panel is then fetched by two XCDs instead of one, the weights
// by every XCD once.
// The order runs over VIRTUAL blocks: the dealt dimension is padded to a multiple of the 8 XCDs (N-split: of the 4 XCD pairs),
// tile_of_block says no for a block in the padding.  Their number: the launch-per-tile grid, the end of a persistent sequence.
__host__ __device__ __forceinline__ int gemm256_virtual_blocks(const GemmArgs &G) {
    const int NT = G.N / TN, MT = G.M / TM;
    return G.n_split == 2 ? (MT + 3) / 4 * 4 * NT : MT >= NT ? (MT + 7) / 8 * 8 * NT : (NT + 7) / 8 * 8 * MT;
}
__device__ __forceinline__ bool tile_of_block(const GemmArgs &G, int b, int *mt_, int *nt_) {
    const int NT = G.N / TN, MT = G.M / TM;
    const int xcd = b & 7, jx = b >> 3;
    int mt, nt;
    if (G.n_split == 2) {
        const int nh = NT >> 1;
        mt = (jx / nh) * 4 + (xcd >> 1);
        nt = (xcd & 1) * nh + jx % nh;
    } else if (MT >= NT) {
        mt = (jx / NT) * 8 + xcd;
        nt = jx % NT;
    } else {
        nt = (jx / MT) * 8 + xcd;
        mt = jx % MT;
    }
    *mt_ = mt;
    *nt_ = nt;
    return mt < MT && nt < NT;
}

// ---- LDS of the launch-per-tile kernels -------------------------------------------------------------------------------------
// [0, 128 KiB) stage buffers, reused by the epilogue as wave-private slabs of 16 KiB; above them the epilogue parameter block (floats)
constexpr int EPB_OFF = 32768;           // = 128 KiB
constexpr int EPB_PART = 0;              // [256 tokens][PART_FLOATS]: slice partials (24 KiB)
constexpr int EPB_STATS = 256 * PART_FLOATS;  // [256][2]: (mean, rstd), filled when the epilogue starts
constexpr int EPB_VEC = EPB_STATS + 512; // three vectors of 256 floats: bias, csum | gamma, beta
constexpr int EPB_FLOATS = EPB_VEC + 768;
constexpr size_t G256_EPB_LDS_BYTES = G256_LDS_BYTES + (size_t)EPB_FLOATS * sizeof(float);
static_assert(EPB_OFF * sizeof(float) == G256_LDS_BYTES, "the parameter block starts where the stage buffers end");

// ---- LDS of the persistent streaming kernel (gemm256_split_stream_kernel) ------------------------------------------------------
// The stage buffers are busy during the epilogue (the next tile's first K-tiles are in flight), so the epilogue lives in a quarter
// of the slab space (gemm256_epilogue_split.h: gemm256_epilogue_split32, 32 x 32 passes) --
//   [0, 128 KiB)          stage buffers; the A-half1 slot of buffer 1 is free between two tiles (K-tile 1's A-half1 is staged by
//                         P0 of K-tile 0): slabs of waves 0-2
//   STATS 2 KiB, VEC 3 KiB   (mean, rstd) of the tile's 256 tokens; bias | csum of its 256 features
//   R 27 KiB              during the K loop the slice partials of the tile's tokens (24 KiB at either hidden width: PART_FLOATS
//                         floats per token; LDS-DMA issued after the previous epilogue, retired by the pipeline's counted
//                         waits); during the epilogue the slabs of waves 3-7
// = 160 KiB exactly.
constexpr int EPS_LS = 36;                       // slab row stride (floats): [32 m][32 n] fp32
constexpr int EPS_SLAB_FLOATS = 32 * EPS_LS;     // 4,608 bytes per wave
constexpr int EPS_STATS = 32768;                 // floats: above the 128 KiB of stage buffers
constexpr int EPS_VEC = EPS_STATS + 512;
constexpr int EPS_R = EPS_VEC + 768;             // 27,648 bytes: slice partials (24 KiB) | slabs of waves 3-7 (5 x 4,608 B)
constexpr int EPS_R_FLOATS = 256 * PART_FLOATS + 768;
constexpr size_t GS_LDS_BYTES = (size_t)(EPS_R + EPS_R_FLOATS) * sizeof(float);  // 163,840
static_assert(GS_LDS_BYTES == 160 * 1024, "the streaming kernel uses the whole LDS of a CU");
static_assert(2 * PartFormat<768>::N <= PART_FLOATS && 2 * PartFormat<1024>::N <= PART_FLOATS,
              "the slice partials of 256 tokens fill R at hidden 768 and fit it at hidden 1024");
static_assert(5 * EPS_SLAB_FLOATS <= EPS_R_FLOATS && 3 * EPS_SLAB_FLOATS * 4 <= 16384, "slab layout");
// slab of a wave: waves 0-2 in the A-half1 slot of stage buffer 1, waves 3-7 in R
__device__ __forceinline__ float *eps_slab(float *smem_f, int w) {
    return w < 3 ? smem_f + (PIPE_BUF_HALVES + PIPE_HALF_HALVES) / 2 + w * EPS_SLAB_FLOATS : smem_f + EPS_R + (w - 3) * EPS_SLAB_FLOATS;
}

#ifndef ANCE_STREAM_LOOSE_FIRST
#define ANCE_STREAM_LOOSE_FIRST 1  // 1: K-tile 0 of a prefetched tile does not wait for the previous epilogue's stores (pipe256.h: tile2); 0: steady-state waits
#endif
// vector-memory operations EVERY wave issues between the hand-over's last LDS-DMA and K-tile 0 of the next output tile: the
// epilogue's stores (gemm256_epilogue_split32: 8 passes x 4 16-byte stores of fp32 rows for QKV, 8 x 2 x (hi + lo) for the pair rows of
// GELU: 32 either way) and the three LDS-DMAs of the slice partials (pb_issue below; the vector DMAs are issued by two waves only
// and do not count)
constexpr int EPS_FOREIGN_OPS = 32 + 3;

// ---- parameter block ---------------------------------------------------------------------------------------------------------------
// LDS-DMA of a tile's parameter block, issued by all 512 threads: the slice partials of its 256 tokens to `part` (24 pieces of
// 1 KiB, three per wave), the vectors the epilogue EPI_ wants to `vec` (bias; csum, or gamma and beta for the RESLN forms; one
// wave each).  Tokens are the tile's rows m and features its columns n, EPI_VT_F has them the other way round.  Launch-per-tile
// kernels issue it BEFORE the main loop (EPB_*): older than every LDS-DMA of the pipeline, whose first counted wait retires it and
// whose first barrier publishes it.  The streaming kernel issues the next tile's (EPS_*) after an epilogue: EPS_FOREIGN_OPS.
template <int EPI_>
__device__ __forceinline__ void pb_issue(const GemmArgs &G, float *part, float *vec, int m0, int n0, int w, int l) {
    const int tok0 = EPI_ == EPI_VT_F ? n0 : m0;  // first of the tile's 256 tokens
    const float *psrc = G.part_in + (size_t)tok0 * PART_FLOATS;
#pragma unroll
    for (int j = 0; j < 3; ++j) {
        const int piece = w + 8 * j;
        __builtin_amdgcn_global_load_lds((pipe_glb_t *)(psrc + piece * 256 + l * 4), (pipe_lds_t *)(part + piece * 256), 16, 0, 0);
    }
    const int f0 = EPI_ == EPI_VT_F ? m0 : n0;    // first of the tile's 256 features
    if (w == 0) __builtin_amdgcn_global_load_lds((pipe_glb_t *)(G.bias + f0 + l * 4), (pipe_lds_t *)vec, 16, 0, 0);
    if (EPI_ == EPI_RESLN || EPI_ == EPI_S_RESLN) {
        if (w == 1) __builtin_amdgcn_global_load_lds((pipe_glb_t *)(G.res_gamma + f0 + l * 4), (pipe_lds_t *)(vec + 256), 16, 0, 0);
        if (w == 2) __builtin_amdgcn_global_load_lds((pipe_glb_t *)(G.res_beta + f0 + l * 4), (pipe_lds_t *)(vec + 512), 16, 0, 0);
    } else {
        if (w == 1) __builtin_amdgcn_global_load_lds((pipe_glb_t *)(G.csum + f0 + l * 4), (pipe_lds_t *)(vec + 256), 16, 0, 0);
    }
}
template <int EPI_>
__device__ __forceinline__ void epb_issue(const GemmArgs &G, float *smem_f, int m0, int n0, int w, int l) {
    pb_issue<EPI_>(G, smem_f + EPB_OFF + EPB_PART, smem_f + EPB_OFF + EPB_VEC, m0, n0, w, l);
}

// Thread t < 256 of a folded epilogue's first step: the slice partials of token t combined into (mean, rstd) at stats[2 t]; the
// caller's barrier publishes them.  Returns whether the token has |mean| rstd > FOLD_WIDE_MEAN: the single-fp16 token operand of
// the folded GEMMs rounds v, not v - mean, so its error grows with |mean| / std (20-80 x at an offset of 5-30 std);
// a tile with such a token adds a second pass over the lo halves.
constexpr float FOLD_WIDE_MEAN = 2.0f;
template <int HW>
__device__ __forceinline__ bool pb_token_stats(const float *part, float *stats, int t, float ln_eps) {
    float mean, rstd;
    stats_from_parts<HW>(part + t * PART_FLOATS, ln_eps, &mean, &rstd);
    stats[2 * t] = mean;
    stats[2 * t + 1] = rstd;
    return __builtin_fabsf(mean) * rstd > FOLD_WIDE_MEAN;
}
// launch-per-tile kernels (all 512 threads, after the main loop): one workgroup barrier publishes the statistics.  Returns
// (uniformly) whether any token of the tile is wide.
template <int HW>
__device__ __forceinline__ bool epb_stats(const GemmArgs &G, float *smem_f, int tid) {
    float *pb = smem_f + EPB_OFF;
    int wide = 0;
    if (tid < 256) wide = pb_token_stats<HW>(pb + EPB_PART, pb + EPB_STATS, tid, G.ln_eps);
    return __builtin_amdgcn_readfirstlane(__syncthreads_or(wide)) != 0;  // (readfirstlane: the compiler must know it is uniform)
}

// Hidden 1024 (PartFormat<1024>): the RES epilogues leave 128-column slice statistics, but a wave owns 64 columns.  Each wave parks
// the (mean, M2) of its 64 columns of every row in the parameter block's partial area (dead once epb_stats has run: its barrier
// comes after the last read), and after one workgroup barrier thread t merges the two halves of slice t & 1 of tile row t >> 1.
__device__ __forceinline__ void epb_park_part(float *smem_f, int row_local, int wn, float mean, float m2) {
    *reinterpret_cast<float2 *>(smem_f + EPB_OFF + EPB_PART + (row_local * 4 + wn) * 2) = make_float2(mean, m2);
}
__device__ __forceinline__ void epb_merge_parts(const GemmArgs &G, const float *smem_f, int m0, int n0, int tid) {
    __syncthreads();
    const int r = tid >> 1, hf = tid & 1;
    const f32x4 ab = *reinterpret_cast<const f32x4 *>(smem_f + EPB_OFF + EPB_PART + (r * 4 + 2 * hf) * 2);
    float m, q;
    part_merge(ab[0], ab[1], ab[2], ab[3], &m, &q);
    *reinterpret_cast<float2 *>(G.part_out + (size_t)(m0 + r) * PART_FLOATS + ((n0 >> 7) + hf) * 2) = make_float2(m, q);
}

// workgroup barrier that does NOT drain the vector-memory counter (the next tile's LDS-DMAs and this tile's stores stay in flight)
__device__ __forceinline__ void eps_barrier() {
    __builtin_amdgcn_sched_barrier(0);
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    __builtin_amdgcn_s_barrier();
    __builtin_amdgcn_sched_barrier(0);
}

// the kernel's GemmArgs re-read from the kernarg segment (first argument) behind an opaque pointer: see the call site
__device__ __forceinline__ GemmArgs kernarg_reload(const GemmArgs &G) {
#if defined(__HIP_DEVICE_COMPILE__)
    typedef const __attribute__((address_space(4))) GemmArgs *kernarg_ptr_t;
    kernarg_ptr_t gp = (kernarg_ptr_t)__builtin_amdgcn_kernarg_segment_ptr();
    asm volatile("" : "+s"(gp));
    (void)G;
    return *gp;
#else
    return G;
#endif
}

}  // namespace ance
