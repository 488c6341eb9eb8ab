// Micro-batch planner of the encoder (encoder.hip: encode_impl): the length rule of a sequence, the host function that cuts the
// next micro-batch out of the host lengths, and the kernels that lay the same micro-batch out on the device.  The rule is written
// ONCE, below, as __host__ __device__ functions: the host sizes grids and buffers with it, the device fills them with it.
#pragma once
#include "common.h"

namespace ance {
namespace {

// ---- the length rule -----------------------------------------------------------------------------
__host__ __device__ inline int clamp_len(int full, int L) { return full < 0 ? 0 : (full > L ? L : full); }  // record length -> [0, L]
__host__ __device__ inline int chunk_len(int full, int c, int Lc) {  // tokens of chunk c (Lc tokens per chunk) of a record of `full`
    const int lc = full - c * Lc;
    return lc < 0 ? 0 : (lc > Lc ? Lc : lc);
}
// an all-pad chunk runs as one pad token attending to itself
__host__ __device__ inline int eff_len(int lc) { return lc > 0 ? lc : 1; }
__host__ __device__ inline int vt_width(int eff) { return (eff + 7) & ~7; }  // V^T columns of a sequence: 8-aligned
__host__ __device__ inline int len_bucket(int eff) {  // ceil(eff / 32) - 1, everything above 96 tokens in bucket 3
    const int b = (eff + 31) >> 5;
    return b > 4 ? 3 : b - 1;
}

// One micro-batch: sequences [first, next) of a block of records, cut greedily from the host lengths hl (one per record; sequence g
// is chunk g % n_chunks of record g / n_chunks) under the lane's capacities -- scap sequences, tcap tokens, vcap - 256 V^T columns.
// SEED: the lengths here are upper bounds of the compacted ones (they size grids, LDS and buffers only); column V (never part of
// a sequence) takes the V^T stores of the pad rows below T, V + 8 <= vcap - 256.  S == 0: not even one sequence fits.
struct MicroPlan {
    int S, T, V;    // sequences, real tokens, V^T columns
    int maxlen;     // longest sequence
    int Tpad, ldvt; // tokens padded to the GEMM tile (256); row stride of V^T
    int64_t next;   // first sequence of the next micro-batch
};
inline MicroPlan plan_micro_batch(const int32_t *hl, int64_t first, int64_t end, int n_chunks, int L, int Lc, int scap, int tcap,
                                  int vcap, bool seed) {
    MicroPlan p = {0, 0, 0, 1, 0, 0, first};
    while (p.next < end && p.S < scap) {
        const int64_t rec = p.next / n_chunks;
        const int eff = eff_len(chunk_len(clamp_len(hl[rec], L), (int)(p.next - rec * n_chunks), Lc));
        if (p.T + eff > tcap || p.V + vt_width(eff) > vcap - 256) break;
        p.T += eff; p.V += vt_width(eff); ++p.S; ++p.next;
        if (eff > p.maxlen) p.maxlen = eff;
    }
    p.Tpad = (int)align_up((size_t)p.T, 256);
    p.ldvt = (int)align_up((size_t)p.V + (seed ? 8 : 0), 256);
    return p;
}

// ---- kernels ---------------------------------------------------------------------------------------

__device__ __forceinline__ int record_len(const int32_t *ids_or_rec, int64_t ld, const int32_t *lens, int64_t rec, int L) {
    int full;
    if (lens) full = lens[rec];
    else full = (int)__builtin_bswap32((uint32_t)ids_or_rec[rec * ld]);  // 4-byte big-endian header
    return clamp_len(full, L);
}

// lengths of records [r0, r0 + n) -> out (for the host-side planner when it has no host copy)
__global__ void fetch_lens_kernel(const int32_t *base, int64_t ld, const int32_t *lens, int64_t r0, int n, int L, int32_t *out) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) out[i] = record_len(base, ld, lens, r0 + i, L);
}

struct PlanArgs {
    const int32_t *base;  // records (header mode: row = [len_be, ids...]) or ids
    int64_t ld;           // row stride in int32
    const int32_t *lens;  // nullptr in header mode
    int hdr;              // 1: ids start at column 1
    int64_t g0;           // first global sequence (record * n_chunks + chunk) of this micro-batch
    int S;                // sequences in this micro-batch
    int L, n_chunks, Lc;
    int pad_id, arch;
    int T, Tpad;          // real tokens / padded to 256 (plan_micro_batch; SEED: T is an upper bound, the device total is seq_off[S])
    int vt_spare;         // SEED: V^T column the pad rows below T write to (no sequence reads it)
    int *seq_off, *seq_vtcol, *seq_len;
    int *tok_id, *tok_pos, *tok_vtcol;
    int4 *desc;           // attention descriptors (first token, length, V^T column, sequence), longest length bucket first
    unsigned *faults;     // ance_encoder_range_faults; SEED: [1] counts sequences that are empty or start with the pad id
};

// SEED (ANCE_ARCH_SEED): the encoder masks every key whose id is the pad id, inside the record's length too.  Positions skip pad
// ids already, so dropping those tokens leaves every other token's output unchanged: seq_len[s] = the number of non-pad ids in
// [0, len), which plan_kernel / pack_kernel then treat as the sequence's length.  One wave per sequence (no MaxP: n_chunks = 1).
// A record that is empty or starts with the pad id has no defined output in the reference (a pad row or NaN): counted in faults[1].
__global__ void __launch_bounds__(256) seed_count_kernel(const PlanArgs P) {
    const int s = blockIdx.x * 4 + (threadIdx.x >> 6);
    const int l = threadIdx.x & 63;
    if (s >= P.S) return;
    const int64_t rec = P.g0 + s;
    const int full = record_len(P.base, P.ld, P.lens, rec, P.L);
    const int32_t *src = P.base + rec * P.ld + P.hdr;
    int cnt = 0;
    for (int j0 = 0; j0 < full; j0 += 64) {
        const int j = j0 + l;
        cnt += __popcll(__ballot(j < full && src[j] != P.pad_id));
    }
    if (l == 0) {
        P.seq_len[s] = cnt;
        if (full == 0 || src[0] == P.pad_id) atomicAdd(P.faults + 1, 1u);
    }
}

// effective lengths + exclusive scans (token offsets; 8-aligned V^T columns; rank inside the length bucket).  One block.
__global__ void __launch_bounds__(1024) plan_kernel(const PlanArgs P) {
    __shared__ int s_tot[1024], s_tot8[1024];
    __shared__ unsigned long long s_bk[1024];  // four 16-bit bucket counts (a micro-batch has at most 8,192 sequences)
    const int tid = threadIdx.x;
    const int per = (P.S + 1023) / 1024;
    const int b0 = tid * per;
    int sum = 0, sum8 = 0;
    unsigned long long bk = 0;
    for (int j = 0; j < per; ++j) {
        const int s = b0 + j;
        if (s < P.S) {
            int lc;
            if (P.arch == ANCE_ARCH_SEED) {
                lc = P.seq_len[s];  // seed_count_kernel
            } else {
                const int64_t gs = P.g0 + s;
                const int64_t rec = gs / P.n_chunks;
                const int c = (int)(gs - rec * P.n_chunks);
                lc = chunk_len(record_len(P.base, P.ld, P.lens, rec, P.L), c, P.Lc);
                P.seq_len[s] = lc;
            }
            const int eff = eff_len(lc);
            sum += eff;
            sum8 += vt_width(eff);
            bk += 1ull << (16 * len_bucket(eff));
        }
    }
    s_tot[tid] = sum;
    s_tot8[tid] = sum8;
    s_bk[tid] = bk;
    __syncthreads();
    // Hillis-Steele inclusive scan over 1024 partials
    for (int off = 1; off < 1024; off <<= 1) {
        int a = 0, a8 = 0;
        unsigned long long ab = 0;
        if (tid >= off) {
            a = s_tot[tid - off];
            a8 = s_tot8[tid - off];
            ab = s_bk[tid - off];
        }
        __syncthreads();
        s_tot[tid] += a;
        s_tot8[tid] += a8;
        s_bk[tid] += ab;
        __syncthreads();
    }
    int run = s_tot[tid] - sum, run8 = s_tot8[tid] - sum8;
    unsigned long long rbk = s_bk[tid] - bk;  // sequences of each bucket before this thread's
    // first descriptor of each bucket, longest sequences first, from the totals (SEED's lengths are known on the device only)
    const unsigned long long tbk = s_bk[1023];
    for (int j = 0; j < per; ++j) {
        const int s = b0 + j;
        if (s < P.S) {
            const int eff = eff_len(P.seq_len[s]);
            P.seq_off[s] = run;
            P.seq_vtcol[s] = run8;
            const int b = len_bucket(eff);
            int bstart = 0;
            for (int bb = 3; bb > b; --bb) bstart += (int)((tbk >> (16 * bb)) & 0xFFFF);
            P.desc[bstart + (int)((rbk >> (16 * b)) & 0xFFFF)] = make_int4(run, eff, run8, s);
            rbk += 1ull << (16 * b);
            run += eff;
            run8 += vt_width(eff);
        }
    }
    if (tid == 1023) P.seq_off[P.S] = s_tot[1023];
}

// one wave per sequence: packed token ids, position ids, V^T columns
__global__ void __launch_bounds__(256) pack_kernel(const PlanArgs P) {
    const int s = blockIdx.x * 4 + (threadIdx.x >> 6);
    const int l = threadIdx.x & 63;
    if (s < P.S) {
        const int64_t gs = P.g0 + s;
        const int64_t rec = gs / P.n_chunks;
        const int c = (int)(gs - rec * P.n_chunks);
        const int lc = P.seq_len[s];
        const int t0 = P.seq_off[s], v0 = P.seq_vtcol[s];
        if (lc == 0) {
            // all-pad chunk == one pad token attending to itself (eff_len)
            if (l == 0) {
                P.tok_id[t0] = P.pad_id;
                P.tok_pos[t0] = P.arch == ANCE_ARCH_BERT ? 0 : P.pad_id;
                P.tok_vtcol[t0] = v0;
            }
        } else if (P.arch == ANCE_ARCH_SEED) {
            // the non-pad ids of [0, len) back to back: rank r gets position pad + 1 + r (RoBERTa's rule on the kept tokens)
            const int32_t *src = P.base + rec * P.ld + P.hdr;
            const int full = record_len(P.base, P.ld, P.lens, rec, P.L);
            int before = 0;
            for (int j0 = 0; j0 < full; j0 += 64) {
                const int j = j0 + l;
                const int id = j < full ? src[j] : P.pad_id;
                const bool keep = j < full && id != P.pad_id;
                const u64 m = __ballot(keep);
                const int r = before + __popcll(m & ((1ull << l) - 1ull));
                if (keep) {
                    P.tok_id[t0 + r] = id;
                    P.tok_pos[t0 + r] = P.pad_id + 1 + r;
                    P.tok_vtcol[t0 + r] = v0 + r;
                }
                before += __popcll(m);
            }
        } else {
            const int32_t *src = P.base + rec * P.ld + P.hdr + c * P.Lc;
            int before = 0;  // non-pad tokens seen so far (RoBERTa position ids)
            for (int j0 = 0; j0 < lc; j0 += 64) {
                const int j = j0 + l;
                const bool in = j < lc;
                const int id = in ? src[j] : P.pad_id;
                const bool nonpad = in && id != P.pad_id;
                const u64 m = __ballot(nonpad);
                if (in) {
                    int pos;
                    if (P.arch == ANCE_ARCH_ROBERTA)
                        pos = nonpad ? before + __popcll(m & ((2ull << l) - 1ull)) + P.pad_id : P.pad_id;
                    else
                        pos = j;
                    P.tok_id[t0 + j] = id;
                    P.tok_pos[t0 + j] = pos;
                    P.tok_vtcol[t0 + j] = v0 + j;
                }
                before += __popcll(m);
            }
        }
    }
    // rows T..Tpad exist only to fill the last GEMM tile.  SEED: from the device total on; the V^T GEMM stores rows below the host's
    // T, so those write the spare column
    const bool seed = P.arch == ANCE_ARCH_SEED;
    const int T = seed ? P.seq_off[P.S] : P.T;
    const int gt = blockIdx.x * blockDim.x + threadIdx.x;
    if (gt < P.Tpad - T) {
        P.tok_id[T + gt] = P.pad_id;
        P.tok_pos[T + gt] = P.arch == ANCE_ARCH_BERT ? 0 : P.pad_id;
        P.tok_vtcol[T + gt] = seed ? P.vt_spare : 0;
    }
}

}  // namespace
}  // namespace ance
