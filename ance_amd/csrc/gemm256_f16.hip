// 256 x 256 x 64 fp16 MFMA GEMM with fused epilogues for the encoder (gfx950):
//   C[m][n] = sum_k A[m][k] * B[n][k],  A [M,K] and B [N,K] row-major f16 (nn.Linear weight layout,
//   so y = x W^T needs no transpose), fp32 accumulation.
// Epilogues (what the reference computes after each nn.Linear, fused here):
//   EPI_QK     out16 = (acc + bias[n]) * (n < scale_cols ? scale : 1)      Q | K projection, Q/8
//   EPI_GELU   out16 = gelu_erf(acc + bias[n])                            intermediate.dense
//   EPI_RES32  out32 = acc + bias[n] + res32[m][n]                        attention.output.dense / output.dense
//   (ance_debug_gemm reaches the main loop through these three; the encoder runs the folded-LayerNorm forms EPI_*_F /
//   EPI_RESLN of gemm_f16.h and the split GEMM below)
// This file: the three kernels, their table and their launch.  gemm256_tile.h: tile order, LDS maps, parameter block.  pipe256.h:
// the main loop.  gemm256_epilogue.h / gemm256_epilogue_split.h: the epilogues.  gemm256_hooks.hip: the C-ABI test hooks.
//
// Why this tile: a 128 x 128 tile has 64 FLOP per staged byte, i.e. 39 TB/s of L2 traffic at the
// 2.5 PFLOP/s MFMA rate -- more than the 34.5 TB/s the eight L2s deliver -- so it is L2-bound by
// construction.  256 x 256 halves that.  8 waves (2 per SIMD), one workgroup per CU, 128 KiB of LDS.
// The main loop is the ping-pong pipeline of pipe256.h (half-tile staging with counted vmcnt, the
// two waves of a SIMD alternating between LDS reads and MFMAs).
//
// MFMA orientation is SWAPPED with respect to the output: MFMA rows (A operand) are B-matrix rows
// n, MFMA columns (B operand) are A-matrix rows m.  In the C-layout a lane then owns one output
// row m and, per register quad, 4 CONSECUTIVE n -- so the epilogue writes 8/16-byte pieces into a
// wave-private row-major LDS slab and reads it back as whole 16-byte row segments: global stores
// (and the residual read) are full-width and coalesced instead of 4-byte scalars.
//
// Staging is direct-to-LDS (global_load_lds_dwordx4): the LDS image is lane-linear, so the XOR
// swizzle is applied to the per-lane SOURCE address.  Measured alternatives on MI355X are listed in
// DESIGN.md section 9 (register staging, a BK=32 ring, LDS-DMA placements, staggered starts, ...).
#include "common.h"
#include "gemm_f16.h"
#include "gemm256_epilogue.h"
#include "gemm256_epilogue_split.h"
#include "gemm256_tile.h"
#include "pipe256.h"
#include <stdlib.h>

namespace ance {
namespace {

// fp16 GEMM: operands through buffer descriptors (PipeSrcDesc), epilogue passes ordered inside the wave instead of by workgroup
// barriers.
#ifdef ANCE_MEASURE
// measurement library: per-workgroup 100 MHz stamps of the folded kernels (ance_debug_gemm_stamps): [block][8] =
// start, main loop done, statistics ready, epilogue done, and for EPI_RESLN the end of each of its four passes
__device__ unsigned long long *g_gemm_stamps = nullptr;
#define GSTAMP(slot) do { if (stamps_ && tid == 0) stamps_[(size_t)blockIdx.x * 8 + (slot)] = __builtin_amdgcn_s_memrealtime(); } while (0)
#else
#define GSTAMP(slot) do { } while (0)
#endif

// HW: the hidden width of the slice partials the folded epilogues read and write (gemm_f16.h: PartFormat)
template <int EPI, int HW = 768>
__global__ void __launch_bounds__(G256_THREADS, 2) gemm256_f16_desc_kernel(const GemmArgs G) {
    extern __shared__ __attribute__((aligned(16))) float smem_f[];
    _Float16 *smem = reinterpret_cast<_Float16 *>(smem_f);
    int mt, nt;
    if (!tile_of_block(G, blockIdx.x, &mt, &nt)) return;
    const int m0 = mt * TM, n0 = nt * TN;
    const int tid = threadIdx.x;
    const int w = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int l = tid & 63;
    f32x16 acc[2][4];
#pragma unroll
    for (int x = 0; x < 2; ++x)
#pragma unroll
        for (int y = 0; y < 4; ++y) acc[x][y] = f32x16{0};
    Pipe256T<PipeSrcDesc> P;
    P.init(smem, w, l);
    // descriptors of this tile's 256 rows of each operand (bases are wave-uniform: kernel arguments and blockIdx), staging offsets
    P.S.ra = pipe_rows_rsrc(G.A, m0, G.lda);
    P.S.rb = pipe_rows_rsrc(G.B, n0, G.ldb);
    pipe_fill_voff(P.S.voff, w, l, G.lda, G.ldb);
    constexpr bool EPB = EPI >= EPI_RESLN;  // folded-LayerNorm epilogues: parameter block by LDS-DMA, ahead of the pipeline's own
#ifdef ANCE_MEASURE
    unsigned long long *stamps_ = (EPI == EPI_RESLN && G.stamp) ? g_gemm_stamps : nullptr;
#endif
    GSTAMP(0);
    if constexpr (EPB) epb_issue<EPI>(G, smem_f, m0, n0, w, l);
    constexpr bool FOLDK = EPI == EPI_QK_F || EPI == EPI_GELU_F || EPI == EPI_VT_F;
    if constexpr (FOLDK) {
        // A tile with a token whose |mean| >> std runs the K loop a second time over the lo halves of the token operand:
        // acc += lo . W^T (the identity  r (acc - mu c) + b'  holds for any operand, so nothing else changes).  Uniform branch,
        // taken by no tile of a random-init model.  The second pass is MASKED per row: only the wide-mean tokens feed their lo
        // halves, every other lane feeds zeros -- the bits of a row therefore depend on that row alone, not on which tokens
        // share its tile (micro-batch composition, shard boundaries, stale pad rows): ADVICE r4, tests/test_gpu_encoder.py::
        // test_fp16_rows_do_not_depend_on_their_tile_mates.
        P.run(G.K / TK, acc);
        GSTAMP(1);
        const bool wide = epb_stats<HW>(G, smem_f, tid);
        if (wide && G.tok_lo) {
            Pipe256T<PipeSrcDesc, false, true> P2;
            P2.init(smem, w, l);
            P2.S = P.S;
            const float *st = smem_f + EPB_OFF + EPB_STATS;
            const int i = l & 31;
            auto tok_wide = [&](int t) { return __builtin_fabsf(st[2 * t]) * st[2 * t + 1] > FOLD_WIDE_MEAN; };
            if constexpr (EPI == EPI_VT_F) {  // tokens are the B-operand rows n = wn * 64 + x * 32 + i
                P2.S.rb = pipe_rows_rsrc(G.tok_lo, n0, G.ldb);
                P2.keep_b = (tok_wide((w & 3) * 64 + i) ? 1u : 0u) | (tok_wide((w & 3) * 64 + 32 + i) ? 2u : 0u);
            } else {                          // tokens are the A-operand rows m = wm * 128 + y * 32 + i
                P2.S.ra = pipe_rows_rsrc(G.tok_lo, m0, G.lda);
                unsigned k = 0;
#pragma unroll
                for (int y = 0; y < 4; ++y) k |= tok_wide((w >> 2) * 128 + y * 32 + i) ? (1u << y) : 0u;
                P2.keep_a = k;
            }
            P2.run(G.K / TK, acc);
        }
    } else {
        P.run(G.K / TK, acc);
        GSTAMP(1);
        if constexpr (EPB) (void)epb_stats<HW>(G, smem_f, tid);
    }
    GSTAMP(2);
#ifdef ANCE_MEASURE
    gemm256_epilogue<EPI, HW>(G, acc, smem_f, m0, n0, w, l, stamps_ ? stamps_ + (size_t)blockIdx.x * 8 + 4 : nullptr);
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
#else
    gemm256_epilogue<EPI, HW>(G, acc, smem_f, m0, n0, w, l);
#endif
    GSTAMP(3);
}

// SPLIT (fp32-grade) GEMM: C = A B^T with both operands as fp16 (hi, lo) pair rows (common.h; v = hi + lo),
//   C = sum_k  A_hi B_hi + A_lo B_hi + A_hi B_lo                  (the dropped lo x lo term is 2^-22 relative)
// Round 5: the pair rows are BLOCKED -- 32 columns of hi, then the same 32 columns of lo -- so the operand matrices look like
// plain [rows, 2 K] fp16 matrices to the staging side (PipeSrcDesc, 128 contiguous bytes per row and K-tile, exactly the fp16
// GEMM's access pattern) and a K-tile in LDS holds a 32-deep k-slice of hi AND lo of both operands: FOUR operand tiles staged
// and read once for THREE products (Pipe256T<.., PAIR3>: 96 v_mfma_f32_16x16x32_f16 per K-tile and wave, the work of 48 of 32x32x16), all into one accumulator
// set.  Round 4 ran three passes over [hi | lo'] rows (six staged tiles per three products, a 2^-11 rescale between the
// passes): per MFMA this loop issues two thirds of the LDS-DMAs, ds_reads and barriers -- the resources the K loop is bound by
// (DESIGN.md 3.2).  One accumulator means one scale: lo is NOT multiplied by 2^11 any more; activations are O(1) (their
// elements below 2^-3 have subnormal lo halves: at most 2^-25 absolute), weights are stored times a per-matrix power of two
// (G.wscale_inv undoes it in the epilogue).  Every partial product is exact in fp32 (11 x 11 bits); fp32 accumulation is what
// is left.  tests/test_split_model.py restates the rounding points on the CPU (3.0e-6 against the fp64 oracle at 12 layers;
// plain fp32: 2.8e-6).
template <int EPI, int HW = 768>
__global__ void __launch_bounds__(G256_THREADS, 2) gemm256_split_kernel(const GemmArgs G) {
    extern __shared__ __attribute__((aligned(16))) float smem_f[];
    _Float16 *smem = reinterpret_cast<_Float16 *>(smem_f);
    int mt, nt;
    if (!tile_of_block(G, blockIdx.x, &mt, &nt)) return;
    const int m0 = mt * TM, n0 = nt * TN;
    const int tid = threadIdx.x;
    const int w = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int l = tid & 63;
    f32x4 acc[4][8];  // 16 x 16 blocks of v_mfma_f32_16x16x32_f16 (pipe256.h)
#pragma unroll
    for (int x = 0; x < 4; ++x)
#pragma unroll
        for (int y = 0; y < 8; ++y) acc[x][y] = f32x4{0.f, 0.f, 0.f, 0.f};
    Pipe256T<PipeSrcDesc, true> P;
    P.init(smem, w, l);
    P.S.ra = pipe_rows_rsrc(G.A, m0, G.lda);
    P.S.rb = pipe_rows_rsrc(G.B, n0, G.ldb);
    pipe_fill_voff(P.S.voff, w, l, G.lda, G.ldb);
    const float winv = G.wscale_inv ? *G.wscale_inv : 1.0f;  // wave-uniform: a scalar load, long back when the epilogue starts
#ifdef ANCE_MEASURE
    unsigned long long *stamps_ = G.stamp ? g_gemm_stamps : nullptr;  // [block][8]: start, main loop done, statistics, end
#endif
    GSTAMP(0);
    epb_issue<EPI>(G, smem_f, m0, n0, w, l);
    P.run(G.K / 32, acc);  // K-tile = 64 halves of a blocked pair row = 32 k of hi and lo
    GSTAMP(1);
    (void)epb_stats<HW>(G, smem_f, tid);
    GSTAMP(2);
    gemm256_epilogue_split<EPI, HW>(G, acc, smem_f, m0, n0, w, l, winv);
#ifdef ANCE_MEASURE
    if (stamps_) asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
#endif
    GSTAMP(3);
}

// PERSISTENT, STREAMING form of the split GEMM (round 6): the product's kernel for the QKV and FFN1 GEMMs (ANCE_GEMM_STREAM, below).
// One workgroup per CU walks its own sequence of output tiles; the K loop of tile i ends as Pipe256T::tiles_streaming -- its last
// two K-tiles stage K-tile 0 and A0 / B0 / B1 of K-tile 1 of tile i + 1 in the steady-state rhythm -- so tile i's epilogue runs with
// the next tile's first operand bytes in flight and the next K loop starts where a steady-state K-tile starts: no pipeline fill
// (3 us of a 58-62 us tile at K = 768), no workgroup launch between two tiles, no launch ramp; the epilogue's stores drain under
// the next tile's first MFMA phase.  What that costs is LDS: the stage buffers are busy during the epilogue, so the epilogue lives
// in a quarter of the slab space (gemm256_epilogue_split32: 32 x 32 passes; LDS map, EPS_*: gemm256_tile.h), 160 KiB in all.
// Tile order: workgroup b is on XCD b & 7 (round-robin dispatch) and takes the virtual blocks
// ((i * slots + (b >> 3)) << 3) | xcd, i = 0, 1, ... of tile_of_block's order -- at any time the 32 CUs of an XCD work on the 32
// consecutive blocks the launch-per-tile kernel would have had in flight there, so the L2 behaviour (and the N-split order of FFN1)
// carries over.  Results are bit-identical to the kernel above (same K order, same epilogue arithmetic, same reduction trees).
template <int EPI, int HW = 768>
__global__ void __launch_bounds__(G256_THREADS, 2) gemm256_split_stream_kernel(const GemmArgs G) {
    extern __shared__ __attribute__((aligned(16))) float smem_f[];
    _Float16 *smem = reinterpret_cast<_Float16 *>(smem_f);
    const int tid = threadIdx.x;
    const int w = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int l = tid & 63;
    const int xcd = blockIdx.x & 7, slot = blockIdx.x >> 3, nslots = gridDim.x >> 3;
    const int n_blocks = gemm256_virtual_blocks(G);
    int round = 0;
    // next valid tile of this workgroup's sequence (virtual blocks past the matrix -- the padding of tile_of_block's order -- are skipped)
    auto next_tile = [&](int *mt, int *nt) -> bool {
        for (;;) {
            const int b = ((round * nslots + slot) << 3) | xcd;
            if (b >= n_blocks) return false;
            ++round;
            if (tile_of_block(G, b, mt, nt)) return true;
        }
    };
    int mt, nt;
    if (!next_tile(&mt, &nt)) return;
    Pipe256T<PipeSrcStream, true> P;
    P.init(smem, w, l);
    P.S.ra = pipe_rows_rsrc(G.A, 0, G.lda, (uint32_t)G.M);  // the whole matrices: tiles are SGPR offsets (PipeSrcStream)
    P.S.rb = pipe_rows_rsrc(G.B, 0, G.ldb, (uint32_t)G.N);
    pipe_fill_voff(P.S.voff, w, l, G.lda, G.ldb);
    const int NK = G.K / 32;  // K-tile = 64 halves of a blocked pair row = 32 k of hi and lo
    P.S.NK = NK;
    P.S.a_cur = P.S.a_nxt = (uint32_t)mt * 256u * (uint32_t)G.lda * 2u;
    P.S.b_cur = P.S.b_nxt = (uint32_t)nt * 256u * (uint32_t)G.ldb * 2u;
    const float winv = G.wscale_inv ? *G.wscale_inv : 1.0f;
    pb_issue<EPI>(G, smem_f + EPS_R, smem_f + EPS_VEC, mt * TM, nt * TN, w, l);
    if constexpr (ANCE_STREAM_LOOSE_FIRST) P.prologue_landed(); else P.prologue();
    P.enter();
    for (;;) {
        int mtn = 0, ntn = 0;
        const bool have_n = next_tile(&mtn, &ntn);
        f32x4 acc[4][8];
#pragma unroll
        for (int x = 0; x < 4; ++x)
#pragma unroll
            for (int y = 0; y < 8; ++y) acc[x][y] = f32x4{0.f, 0.f, 0.f, 0.f};
        if (have_n) {
            P.S.a_nxt = (uint32_t)mtn * 256u * (uint32_t)G.lda * 2u;
            P.S.b_nxt = (uint32_t)ntn * 256u * (uint32_t)G.ldb * 2u;
        }
        constexpr int F = ANCE_STREAM_LOOSE_FIRST ? EPS_FOREIGN_OPS : 0;
        constexpr int VM0F = 6 + F > 63 ? 63 : 6 + F, VM1F = 2 + F > 63 ? 63 : 2 + F;
        // (the first tile of the workgroup comes from prologue_landed: nothing in flight, the loose waits of its K-tile 0 are trivially enough)
        if (have_n) P.template tiles_streaming<VM0F, VM1F>(NK, acc); else P.template tiles_final<VM0F, VM1F>(NK, acc);
        P.leave();
        // (the lane id is laundered through an empty asm: hipcc otherwise hoists every lane-derived address of the epilogue out of the
        // tile loop, runs out of registers next to the 128 accumulators and reloads them from scratch here -- and a scratch reload is a
        // vmcnt(0) wait that drains the next tile's prefetch; ip_topk_fast.hip found the same)
        int lf = l;
        asm volatile("" : "+v"(lf));
        const int tf = (w << 6) | lf;
        // (the same for the kernel arguments: ~50 SGPRs of pointers and strides that only the epilogue uses would otherwise stay live
        // across the K loop -- re-read from the kernarg segment per tile instead)
        const GemmArgs Ge = kernarg_reload(G);
        // (mean, rstd) of the tile's tokens from their slice partials (in R since before this K loop), published by one barrier;
        // after it R belongs to the slabs
        if (tf < 256) (void)pb_token_stats<HW>(smem_f + EPS_R, smem_f + EPS_STATS, tf, Ge.ln_eps);
        eps_barrier();
        gemm256_epilogue_split32<EPI>(Ge, acc, eps_slab(smem_f, w), smem_f + EPS_STATS, smem_f + EPS_VEC, mt * TM, nt * TN, w, lf, winv);
        if (!have_n) break;
        eps_barrier();  // every wave is done with STATS, VEC and its slab: R and the A-half1 slot may be refilled
        mt = mtn;
        nt = ntn;
        P.S.a_cur = P.S.a_nxt;
        P.S.b_cur = P.S.b_nxt;
        pb_issue<EPI>(Ge, smem_f + EPS_R, smem_f + EPS_VEC, mt * TM, nt * TN, w, lf);
        P.enter();
    }
}

#ifdef ANCE_MEASURE
unsigned long long *g_gemm_stamps_host = nullptr;
int g_gemm_stamps_epi = EPI_RESLN;  // which epilogue's launches are stamped (ance_debug_gemm_stamps_epi)
#endif

// ANCE_GEMM_STREAM: 1 (default) = the persistent streaming kernel for the QKV and FFN1 GEMMs (same-box A/Bs: -0.6 .. -1.3 % and
// -1.7 .. -3.0 % per launch), the launch-per-tile kernel for the two RESLN GEMMs (streaming them measured +1.0 % / +1.5 %:
// DESIGN_REJECTED.md round 6); 0 = launch-per-tile everywhere (A/B).  Read once per process, ance_reload_env re-reads it.
int g_gemm_stream = -1;
int gemm_stream_mode() {
    if (g_gemm_stream < 0) {
        const char *e = getenv("ANCE_GEMM_STREAM");
        g_gemm_stream = (e && e[0] == '0') ? 0 : 1;
    }
    return g_gemm_stream;
}
int device_cu_count() {
    static int cus[64] = {0};
    int dev = 0;
    (void)hipGetDevice(&dev);
    if (dev < 0 || dev >= 64) dev = 0;
    if (cus[dev] == 0) {
        int n = 0;
        if (hipDeviceGetAttribute(&n, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || n < 8) n = 256;
        cus[dev] = n;
    }
    return cus[dev];
}

// the kernels of one hidden width (gemm_f16.h: PartFormat); the plain epilogues (ance_debug_gemm) read no partials: 768 only.
// stream: the persistent streaming form (EPI_S_QKV and EPI_S_GELU have one)
typedef void (*gemm_kernel_t)(const GemmArgs);
template <int HW>
gemm_kernel_t gemm_kernel_of(int epi, bool stream) {
    if (stream) {
        switch (epi) {
            case EPI_S_QKV: return gemm256_split_stream_kernel<EPI_S_QKV, HW>;
            case EPI_S_GELU: return gemm256_split_stream_kernel<EPI_S_GELU, HW>;
            default: return nullptr;
        }
    }
    switch (epi) {
        case EPI_QK: return HW == 768 ? gemm256_f16_desc_kernel<EPI_QK> : nullptr;
        case EPI_GELU: return HW == 768 ? gemm256_f16_desc_kernel<EPI_GELU> : nullptr;
        case EPI_RES32: return HW == 768 ? gemm256_f16_desc_kernel<EPI_RES32> : nullptr;
        case EPI_RESLN: return gemm256_f16_desc_kernel<EPI_RESLN, HW>;
        case EPI_QK_F: return gemm256_f16_desc_kernel<EPI_QK_F, HW>;
        case EPI_GELU_F: return gemm256_f16_desc_kernel<EPI_GELU_F, HW>;
        case EPI_VT_F: return gemm256_f16_desc_kernel<EPI_VT_F, HW>;
        case EPI_S_QKV: return gemm256_split_kernel<EPI_S_QKV, HW>;
        case EPI_S_GELU: return gemm256_split_kernel<EPI_S_GELU, HW>;
        case EPI_S_RESLN: return gemm256_split_kernel<EPI_S_RESLN, HW>;
        default: return nullptr;
    }
}

// the dynamic-LDS limit of a kernel instance, set once per instance AND per device (common.h: attr_needed / attr_mark)
bool dynamic_lds_ready(gemm_kernel_t k, unsigned long long *done, size_t bytes) {
    if (!attr_needed(done)) return true;
    if (hipFuncSetAttribute(reinterpret_cast<const void *>(k), hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes) != hipSuccess) return false;
    attr_mark(done);
    return true;
}

int launch256(int epi, const GemmArgs &G, hipStream_t st, int hw) {
    if (G.n_split != 0 && (G.n_split != 2 || ((G.N / TN) & 1) || epi < EPI_RESLN)) {
        set_last_error("gemm256: n_split needs an even number of N tiles and a descriptor-form kernel");
        return ANCE_E_INVALID;
    }
    const unsigned blocks = (unsigned)gemm256_virtual_blocks(G);
    const int wi = hw == 1024 ? 1 : 0;  // instance set
    const bool known = epi >= 0 && epi < EPI_COUNT && (hw == 768 || hw == 1024);
    bool stream = (epi == EPI_S_QKV || epi == EPI_S_GELU) && gemm_stream_mode() == 1 && G.K >= 96 &&
                  (uint64_t)G.M * (uint64_t)G.lda * 2u < (1ull << 31) && (uint64_t)G.N * (uint64_t)G.ldb * 2u < (1ull << 31);
#ifdef ANCE_MEASURE
    const bool stamped = epi == g_gemm_stamps_epi && g_gemm_stamps_host;
    stream = stream && !stamped;
#endif
    const gemm_kernel_t k = !known ? nullptr : wi ? gemm_kernel_of<1024>(epi, stream) : gemm_kernel_of<768>(epi, stream);
    if (!k) {
        set_last_error("gemm256: bad epilogue or hidden width");
        return ANCE_E_INVALID;
    }
    const size_t lds = stream ? GS_LDS_BYTES : epi >= EPI_RESLN ? G256_EPB_LDS_BYTES : G256_LDS_BYTES;
    static unsigned long long attr_done[2][2][EPI_COUNT] = {{{0}}};  // [stream][instance set][epilogue]
    // (the launch-per-tile instances always ask for the parameter block's room, the plain epilogues launch without it)
    if (!dynamic_lds_ready(k, &attr_done[stream][wi][epi], stream ? GS_LDS_BYTES : G256_EPB_LDS_BYTES)) return check_launch("gemm256 attr");
    if (stream) {
        const unsigned cus = (unsigned)device_cu_count() & ~7u;  // one workgroup per CU (160 KiB of LDS each), a multiple of the 8 XCDs
        hipLaunchKernelGGL(k, dim3(blocks < cus ? blocks : cus), dim3(G256_THREADS), lds, st, G);
        return ANCE_OK;
    }
#ifdef ANCE_MEASURE
    if (stamped) {
        GemmArgs G2 = G;
        G2.stamp = 1;
        hipLaunchKernelGGL(k, dim3(blocks), dim3(G256_THREADS), lds, st, G2);
        return ANCE_OK;
    }
#endif
    hipLaunchKernelGGL(k, dim3(blocks), dim3(G256_THREADS), lds, st, G);
    return ANCE_OK;
}

}  // namespace

void reload_gemm_knobs() { g_gemm_stream = -1; }

bool gemm256_applicable(const GemmArgs &G) {
    return G.M > 0 && G.N > 0 && G.K >= 2 * TK && G.M % TM == 0 && G.N % TN == 0 && G.K % TK == 0;
}

int launch_gemm_f16(int epi, const GemmArgs &G, hipStream_t st, int hw) {
    if (!gemm256_applicable(G)) {
        set_last_error("gemm_f16: M,N must be multiples of 256 and K a multiple of 64, >= 128");
        return ANCE_E_INVALID;
    }
    return launch256(epi, G, st, hw);
}

}  // namespace ance

#ifdef ANCE_MEASURE
// measurement library only: while d_stamps != NULL the RES GEMMs of the encoder leave uint64[8] per workgroup at d_stamps
extern "C" void ance_debug_gemm_stamps(void *d_stamps) {
    ance::g_gemm_stamps_host = reinterpret_cast<unsigned long long *>(d_stamps);
    unsigned long long *p = ance::g_gemm_stamps_host;
    (void)hipMemcpyToSymbol(HIP_SYMBOL(ance::g_gemm_stamps), &p, sizeof(p));
}
// measurement library only: the epilogue (gemm_f16.h: EPI_*) whose launches leave stamps; default EPI_RESLN.  The split kernels
// (EPI_S_QKV 8, EPI_S_GELU 9, EPI_S_RESLN 10) fill slots 0..3: start, main loop done, statistics ready, stores drained
extern "C" void ance_debug_gemm_stamps_epi(int epi) { ance::g_gemm_stamps_epi = epi; }
#endif
