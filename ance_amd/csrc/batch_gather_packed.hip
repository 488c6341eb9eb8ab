// Packed training batches straight from the token caches (include/ance_amd.h: ance_record_lengths, ance_gather_batch_packed).
// ance_gather_batch writes padded [B, L] ids and masks, and every tower then rebuilds the lengths from the mask, scans them and packs
// (csrc/pack_rows.hip).  The lengths are in the cache all along, and the item list of a pass is known when its plan is made, so the
// scan moves to plan time: the host side builds cum[n_items * C + 1], the exclusive running sum of the sequence lengths in item-then-
// chunk order, ONCE per pass, and a batch is ONE launch that reads its offsets from cum.
//   record lengths   a wave per (record, chunk): the header rule needs the header only, the nonzero rule counts ids != 0 by ballot
//   gather           grid (x, y), y = segment (tower).  The first seq_blocks workgroups of a segment hold a wave per sequence
//                    s = item * C + c of the batch: off = cum[s0 + s] - cum[s0], len = cum[s0 + s + 1] - cum[s0 + s], kept iff
//                    off + len <= rows; the wave copies the ids raw and forms the positions as pack_fill_kernel does.  The further
//                    workgroups write the slack rows T .. rows - 1.
//   T and dropped    off + len never decreases with s, so whether a sequence is the FIRST dropped one is decidable from cum alone
//                    (it is not kept and its predecessor is kept or absent), and T is found by a binary search over cum: no scan,
//                    no cooperation between workgroups.  Exactly one lane per segment -- lane 0 of the first dropped sequence's
//                    wave, or of the last sequence's when none is dropped -- stores T into seq_off[n_seq] and this batch's dropped
//                    count into *dropped: a plain store, never a read-modify-write, as three segments share the grid.
//   the cursor       with d_first the first item is read from that int64 device scalar.  The item is clamped into [0, n_index] and
//                    every cum index into [0, n_index * C], so neither index nor cum is read past its end whatever the cursor
//                    holds; an item at or beyond n_index is an empty sequence that reads no record.
// Every record index is clamped into [0, n_records), every offset into [0, rows], and no row >= rows is ever written.
// Plain C++: no inline assembly, no atomics, no shared memory, no state shared between segments.
#include "common.h"

namespace ance {
namespace {

constexpr int PG_THREADS = 256, PG_WAVES = PG_THREADS / 64;
constexpr int PG_MAX_CHUNK = 512, PG_MAX_SEQS = 65535;

__device__ __forceinline__ int pg_clamp(int v, int lo, int hi) { return v < lo ? lo : (v > hi ? hi : v); }
__device__ __forceinline__ int64_t pg_clamp64(int64_t v, int64_t lo, int64_t hi) { return v < lo ? lo : (v > hi ? hi : v); }

// ---------------------------------------------------------------------------------------------------------------- record lengths
struct LengthsParams {
    const uint32_t *rec;  // records as dwords: row stride 1 + L
    int *out;             // [n_records, C]
    int64_t n_entries;    // n_records * C
    int L, chunk_len, C, rule;
};

__global__ void __launch_bounds__(PG_THREADS) record_lengths_kernel(const LengthsParams P) {
    const int lane = threadIdx.x & 63;
    const int64_t e = (int64_t)blockIdx.x * PG_WAVES + (threadIdx.x >> 6);
    if (e >= P.n_entries) return;
    const int64_t record = e / P.C;
    const int c = (int)(e - record * P.C);
    const uint32_t *r = P.rec + record * (int64_t)(P.L + 1);
    int len;
    if (P.rule == ANCE_GATHER_MASK_LENGTH) {
        const int whole = (int)min(__builtin_bswap32(r[0]), (uint32_t)P.L);
        len = pg_clamp(whole - c * P.chunk_len, 0, P.chunk_len);
    } else {
        const uint32_t *src = r + 1 + c * P.chunk_len;
        len = 0;
        for (int l0 = 0; l0 < P.chunk_len; l0 += 64) {
            const int l = l0 + lane;
            len += __builtin_popcountll(__ballot(l < P.chunk_len && src[l] != 0u));
        }
    }
    if (lane == 0) P.out[e] = len;
}

// ---------------------------------------------------------------------------------------------------------------- the packed gather
struct PackedSeg {
    const uint32_t *rec;
    const int64_t *index, *cum;
    int *ids, *pos, *seq_off, *seq_kept;
    long long *dropped;
    int64_t n_records, n_index;
    int L, chunk_len, C, rows, roberta, pad, vocab, max_pos;
    int n_seq, seq_blocks;  // B * C; the workgroups that hold its waves
};
struct PackedArgs {
    PackedSeg seg[3];
    const long long *d_first;  // nullable: the cursor
    int64_t first;
};

// The batch's view of cum: sequence s of the batch begins at cum index base + s; indices past the plan's end repeat its last entry,
// which makes every sequence beyond the plan an empty one.
struct CumView {
    const int64_t *cum;
    int64_t base, last;  // last = n_index * C, the largest valid index
    int64_t origin;      // cum[base]
    int chunk_len, rows;
    __device__ __forceinline__ int64_t at(int64_t s) const { return cum[pg_clamp64(base + s, 0, last)] - origin; }
    __device__ __forceinline__ int len(int s) const { return (int)pg_clamp64(at((int64_t)s + 1) - at(s), 0, chunk_len); }
    __device__ __forceinline__ bool kept(int s) const { return at(s) + len(s) <= (int64_t)rows; }
    // the rows in use: the offset of the first dropped sequence, or the end of the last one
    __device__ int total(int n_seq) const {
        int lo = 0, hi = n_seq;  // the first s in [0, n_seq] that is not kept (n_seq: none)
        while (lo < hi) {
            const int mid = (lo + hi) >> 1;
            if (kept(mid)) lo = mid + 1; else hi = mid;
        }
        return (int)pg_clamp64(at(lo), 0, rows);
    }
};

__device__ __forceinline__ CumView cum_view(const PackedSeg &S, int64_t first) {
    CumView V;
    V.cum = S.cum;
    V.last = S.n_index * S.C;
    V.base = pg_clamp64(first, 0, S.n_index) * S.C;
    V.origin = S.cum[V.base];
    V.chunk_len = S.chunk_len;
    V.rows = S.rows;
    return V;
}

__global__ void __launch_bounds__(PG_THREADS) gather_batch_packed_kernel(const PackedArgs A) {
    const PackedSeg S = A.seg[blockIdx.y];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int64_t first = pg_clamp64(A.d_first ? (int64_t)*A.d_first : A.first, 0, S.n_index);
    const CumView V = cum_view(S, first);
    if ((int)blockIdx.x >= S.seq_blocks) {  // the slack rows
        const long long row = (long long)((int)blockIdx.x - S.seq_blocks) * PG_THREADS + threadIdx.x;
        if (row >= S.rows) return;
        const int T = V.total(S.n_seq);
        if (row >= T) {
            S.ids[row] = S.pad >= 0 ? S.pad : 0;
            S.pos[row] = S.roberta ? S.pad : 0;
        }
        return;
    }
    const int s = (int)blockIdx.x * PG_WAVES + wave;
    if (s >= S.n_seq) return;
    const int len = V.len(s);
    const int64_t off64 = V.at(s);
    const bool kept = off64 + len <= (int64_t)S.rows;
    const int off = (int)pg_clamp64(off64, 0, S.rows);
    const bool first_dropped = !kept && (s == 0 || V.kept(s - 1));
    // T: a kept sequence needs it only as the writer of the last entry; a dropped one has it as its offset
    int T = off;
    if (!kept && !first_dropped) T = V.total(S.n_seq);
    if (lane == 0) {
        S.seq_kept[s] = kept ? len : -1;
        S.seq_off[s] = kept ? off : T;
        if (first_dropped) {
            S.seq_off[S.n_seq] = T;
            *S.dropped = (long long)(S.n_seq - s);
        } else if (kept && s == S.n_seq - 1) {
            S.seq_off[S.n_seq] = off + len;  // off + len <= rows
            *S.dropped = 0;
        }
    }
    if (!kept || len <= 0) return;
    const int64_t item = first + s / S.C;
    if (item >= S.n_index) return;  // len is 0 there already: cum repeats its last entry
    int64_t ix = S.index[item];
    ix = ix < 0 ? 0 : (ix >= S.n_records ? S.n_records - 1 : ix);  // no index value reads outside the records
    const uint32_t *src = S.rec + ix * (int64_t)(S.L + 1) + 1 + (s % S.C) * S.chunk_len;
    int count = 0;  // roberta: the non-pad ids in the columns before this round's
    for (int l0 = 0; l0 < len; l0 += 64) {
        const int l = l0 + lane;
        const bool in = l < len;
        const int raw = in ? (int)src[l] : 0;
        const int id = pg_clamp(raw, 0, S.vocab - 1);
        int p = l;
        if (S.roberta) {
            const bool tok = in && id != S.pad;
            const u64 b = __ballot(tok);
            const int n = count + __builtin_popcountll(b & (~0ull >> (63 - lane)));  // columns 0 .. l
            count += __builtin_popcountll(b);
            p = S.pad + (tok ? n : 0);
        }
        const long long row = (long long)off + l;
        if (in && row < S.rows) {
            S.ids[row] = raw;
            S.pos[row] = pg_clamp(p, 0, S.max_pos - 1);
        }
    }
}

const char *check_aligned(const void *p, uintptr_t to, const char *why) {
    if (!p) return "null pointer";
    return (uintptr_t)p % to ? why : nullptr;
}

}  // namespace
}  // namespace ance

extern "C" int ance_record_lengths(const void *d_records, int64_t n_records, int L, int chunk_len, int rule, int32_t *d_out, void *stream) {
    using namespace ance;
    const char *fn = "ance_record_lengths";
    if (!d_records || !d_out) return refuse(fn, "null pointer");
    if ((uintptr_t)d_records % 4) return refuse(fn, "d_records not 4-byte aligned");
    if ((uintptr_t)d_out % 4) return refuse(fn, "d_out not 4-byte aligned");
    if (n_records < 1) return refuse(fn, "n_records < 1");
    if (L < 1) return refuse(fn, "L < 1");
    if (chunk_len < 1 || chunk_len > PG_MAX_CHUNK) return refuse(fn, "chunk_len outside 1 .. 512");
    if (L % chunk_len) return refuse(fn, "chunk_len does not divide L");
    if (rule != ANCE_GATHER_MASK_LENGTH && rule != ANCE_GATHER_MASK_NONZERO) return refuse(fn, "unknown length rule");
    const int C = L / chunk_len;
    if (n_records > ((int64_t)INT32_MAX * PG_WAVES) / C) return refuse(fn, "n_records * (L / chunk_len) too large");
    LengthsParams P = {};
    P.rec = (const uint32_t *)d_records;
    P.out = d_out;
    P.n_entries = n_records * C;
    P.L = L; P.chunk_len = chunk_len; P.C = C; P.rule = rule;
    const unsigned blocks = (unsigned)((P.n_entries + PG_WAVES - 1) / PG_WAVES);
    hipLaunchKernelGGL(record_lengths_kernel, dim3(blocks), dim3(PG_THREADS), 0, (hipStream_t)stream, P);
    return check_launch(fn);
}

extern "C" int ance_gather_batch_packed(const AncePackedGatherSegment *h_segs, int n_segs, int64_t first, int64_t B,
                                        const int64_t *d_first, void *stream) {
    using namespace ance;
    const char *fn = "ance_gather_batch_packed";
    if (!h_segs) return refuse(fn, "null segment table");
    if (n_segs < 1 || n_segs > 3) return refuse(fn, "n_segs outside 1..3");
    if (B < 1) return refuse(fn, "B < 1");
    if ((uintptr_t)d_first % 8) return refuse(fn, "d_first not 8-byte aligned");
    if (!d_first && first < 0) return refuse(fn, "first < 0");
    PackedArgs A = {};
    A.d_first = (const long long *)d_first;
    A.first = first;
    int64_t blocks = 0;
    for (int s = 0; s < n_segs; ++s) {
        const AncePackedGatherSegment &h = h_segs[s];
        if (const char *why = check_aligned(h.d_records, 4, "d_records not 4-byte aligned")) return refuse(fn, why);
        if (const char *why = check_aligned(h.d_index, 8, "d_index not 8-byte aligned")) return refuse(fn, why);
        if (const char *why = check_aligned(h.d_cum, 8, "d_cum not 8-byte aligned")) return refuse(fn, why);
        if (const char *why = check_aligned(h.d_dropped, 8, "d_dropped not 8-byte aligned")) return refuse(fn, why);
        for (const void *p : {(const void *)h.packed_ids, (const void *)h.packed_positions, (const void *)h.d_seq_off, (const void *)h.d_seq_kept})
            if (const char *why = check_aligned(p, 4, "an output not 4-byte aligned")) return refuse(fn, why);
        if (h.n_records < 1) return refuse(fn, "n_records < 1");
        if (h.n_index < 0) return refuse(fn, "n_index < 0");
        if (!d_first && (first > h.n_index || B > h.n_index - first)) return refuse(fn, "first + B past the item index");
        if (h.L < 1) return refuse(fn, "L < 1");
        if (h.chunk_len < 1 || h.chunk_len > PG_MAX_CHUNK) return refuse(fn, "chunk_len outside 1 .. 512");
        if (h.L % h.chunk_len) return refuse(fn, "chunk_len does not divide L");
        const int C = h.L / h.chunk_len;
        if (B > PG_MAX_SEQS / C) return refuse(fn, "B * (L / chunk_len) outside 1 .. 65535");
        if (h.n_index > (INT64_MAX / 16) / C) return refuse(fn, "n_index * (L / chunk_len) too large");
        if (h.rows < 1) return refuse(fn, "rows < 1");
        if (h.vocab < 1 || h.max_pos < 1) return refuse(fn, "an empty table");
        if (h.position_mode == ANCE_EMBED_POSITION_ABSOLUTE) {
            if (h.padding_idx < -1 || h.padding_idx >= h.vocab) return refuse(fn, "padding_idx outside -1 .. vocab - 1");
        } else if (h.position_mode == ANCE_EMBED_POSITION_ROBERTA) {
            if (h.padding_idx < 0 || h.padding_idx >= h.vocab) return refuse(fn, "roberta positions: padding_idx outside 0 .. vocab - 1");
        } else {
            return refuse(fn, "position_mode not 0 or 1");
        }
        PackedSeg &S = A.seg[s];
        S.rec = (const uint32_t *)h.d_records;
        S.index = h.d_index;
        S.cum = h.d_cum;
        S.ids = h.packed_ids; S.pos = h.packed_positions; S.seq_off = h.d_seq_off; S.seq_kept = h.d_seq_kept;
        S.dropped = (long long *)h.d_dropped;
        S.n_records = h.n_records; S.n_index = h.n_index;
        S.L = h.L; S.chunk_len = h.chunk_len; S.C = C; S.rows = h.rows;
        S.roberta = h.position_mode == ANCE_EMBED_POSITION_ROBERTA; S.pad = h.padding_idx;
        S.vocab = h.vocab; S.max_pos = h.max_pos;
        S.n_seq = (int)(B * C);
        S.seq_blocks = (S.n_seq + PG_WAVES - 1) / PG_WAVES;
        const int64_t nb = S.seq_blocks + ((int64_t)h.rows + PG_THREADS - 1) / PG_THREADS;
        blocks = nb > blocks ? nb : blocks;
    }
    hipLaunchKernelGGL(gather_batch_packed_kernel, dim3((unsigned)blocks, (unsigned)n_segs), dim3(PG_THREADS), 0, (hipStream_t)stream, A);
    return check_launch(fn);
}
