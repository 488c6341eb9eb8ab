// Packed token rows of a fixed capacity (include/ance_amd.h: ance_pack_tokens, ance_first_rows_*): what turns a right-padded batch
// [n_seq, L] into R rows that hold the sequences back to back, and what carries the first row of every sequence out of them again.
//   plan      one workgroup walks the sequences in tiles of PLAN_THREADS: len = clamp(d_seq_len, 0, L), an exclusive scan (wave
//             shuffles, the sixteen wave totals through LDS, a carry from tile to tile), kept iff off + len <= R.  off + len never
//             decreases, so the dropped sequences are a suffix and T, the rows in use, is the first dropped sequence's offset.
//   fill      a wave per sequence copies its ids and types to rows off .. off + len - 1 and forms the positions (roberta: the
//             running count of non-pad ids, a ballot per 64 columns and a carry); further workgroups write the slack rows T .. R - 1.
//   first rows  a wave per sequence copies row off_s of x to out[s] (gather) or dout[s] to row off_s of dx (scatter) in 16-byte
//             pieces, whatever the element type.
// Every offset read back from memory is clamped into [0, R] before a row is addressed with it, and no row >= R is ever written.
// No atomics: the dropped-sequence counter is one thread's plain read, add and store.
// By id (ance_pack_tokens_by_id): the lengths are not given but counted -- a wave per sequence ballots id != pad over all L columns
// (-1 for a sequence that BEGINS with the pad id) -- the plan treats -1 as a dropped sequence of no rows that keeps its running
// offset, and the fill walks all L columns and sends every non-pad id to row off + its rank among them: three launches.
#include "common.h"

namespace ance {
namespace {

constexpr int PLAN_THREADS = 1024, PLAN_WAVES = PLAN_THREADS / 64;
constexpr int FILL_THREADS = 256, FILL_WAVES = FILL_THREADS / 64;

struct PackParams {
    const int *ids, *type_ids, *seq_len;
    int *seq_off, *seq_kept, *out_ids, *out_types, *out_pos;
    long long *dropped;
    int n_seq, L, rows, roberta, pad, vocab, max_pos, seq_blocks;
};

__device__ __forceinline__ int clamp_to(int v, int lo, int hi) { return v < lo ? lo : (v > hi ? hi : v); }

// BY_ID: a length of -1 (a sequence that begins with the pad id) scans as 0 rows, is dropped (seq_kept -1, counted) and, unlike a
// sequence dropped for capacity, keeps its own running offset in seq_off while that is <= R: -2 marks it between the two loops.
template <bool BY_ID>
__global__ void __launch_bounds__(PLAN_THREADS) pack_plan_kernel(const PackParams P) {
    __shared__ int wave_tot[PLAN_WAVES];
    __shared__ int red[2][PLAN_WAVES];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    int carry = 0, used = 0, n_drop = 0;  // carry: the same in every thread; used, n_drop: this thread's share
    for (int s0 = 0; s0 < P.n_seq; s0 += PLAN_THREADS) {
        const int s = s0 + (int)threadIdx.x;
        const int given = s < P.n_seq ? P.seq_len[s] : 0;
        const bool lead = BY_ID && given < 0;
        const int len = clamp_to(given, 0, P.L);
        int inc = len;  // the inclusive scan inside the wave
#pragma unroll
        for (int d = 1; d < 64; d <<= 1) {
            const int up = __shfl_up(inc, d);
            if (lane >= d) inc += up;
        }
        if (lane == 63) wave_tot[wave] = inc;
        __syncthreads();
        int before = 0, tile = 0;
#pragma unroll
        for (int w = 0; w < PLAN_WAVES; ++w) {
            const int t = wave_tot[w];
            before += w < wave ? t : 0;
            tile += t;
        }
        __syncthreads();  // wave_tot is written again by the next tile
        const int off = carry + before + inc - len;
        const bool kept = off + len <= P.rows;  // at most 65535 * 512 rows: no overflow
        if (s < P.n_seq) {
            P.seq_kept[s] = kept && !lead ? len : (kept ? -2 : -1);
            if (kept) P.seq_off[s] = off;
            if (kept && !lead) {
                used = off + len;  // the thread's sequences ascend, and so do their ends
            } else {
                ++n_drop;
            }
        }
        carry += tile;
    }
    // T = the largest end of a kept sequence; the number of dropped ones
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) {
        const int u = __shfl_xor(used, d), n = __shfl_xor(n_drop, d);
        used = used > u ? used : u;
        n_drop += n;
    }
    if (lane == 0) {
        red[0][wave] = used;
        red[1][wave] = n_drop;
    }
    __syncthreads();
    int T = 0, dropped = 0;
#pragma unroll
    for (int w = 0; w < PLAN_WAVES; ++w) {
        T = T > red[0][w] ? T : red[0][w];
        dropped += red[1][w];
    }
    for (int s = (int)threadIdx.x; s < P.n_seq; s += PLAN_THREADS) {  // the thread's own stores above: s has the same owner in both loops
        const int k = P.seq_kept[s];
        if (BY_ID && k == -2) P.seq_kept[s] = -1;
        else if (k < 0) P.seq_off[s] = T;
    }
    if (threadIdx.x == 0) {
        P.seq_off[P.n_seq] = T;
        *P.dropped = *P.dropped + dropped;
    }
}

__global__ void __launch_bounds__(FILL_THREADS) pack_fill_kernel(const PackParams P) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    if ((int)blockIdx.x >= P.seq_blocks) {  // the slack rows
        const int T = clamp_to(P.seq_off[P.n_seq], 0, P.rows);
        const long long row = (long long)((int)blockIdx.x - P.seq_blocks) * FILL_THREADS + threadIdx.x;
        if (row >= T && row < P.rows) {
            P.out_ids[row] = P.pad >= 0 ? P.pad : 0;
            if (P.out_types) P.out_types[row] = 0;
            P.out_pos[row] = P.roberta ? P.pad : 0;
        }
        return;
    }
    const int s = (int)blockIdx.x * FILL_WAVES + wave;
    if (s >= P.n_seq) return;
    const int len = clamp_to(P.seq_kept[s], -1, P.L);
    if (len <= 0) return;
    const int off = clamp_to(P.seq_off[s], 0, P.rows);
    const int *src = P.ids + (size_t)s * P.L, *tsrc = P.type_ids ? P.type_ids + (size_t)s * P.L : nullptr;
    int count = 0;  // roberta: the non-pad ids in the columns before this round's
    for (int l0 = 0; l0 < len; l0 += 64) {
        const int l = l0 + lane;
        const bool in = l < len;
        const int raw = in ? src[l] : 0;
        const int id = clamp_to(raw, 0, P.vocab - 1);
        int p = l;
        if (P.roberta) {
            const bool tok = in && id != P.pad;
            const u64 b = __ballot(tok);
            const int n = count + __builtin_popcountll(b & (~0ull >> (63 - lane)));  // columns 0 .. l
            count += __builtin_popcountll(b);
            p = P.pad + (tok ? n : 0);
        }
        const long long row = (long long)off + l;
        if (in && row < P.rows) {
            P.out_ids[row] = raw;
            if (P.out_types) P.out_types[row] = tsrc[l];
            P.out_pos[row] = clamp_to(p, 0, P.max_pos - 1);
        }
    }
}

// d_seq_len[s] = #{l < L : ids[s, l] != pad}, or -1 when ids[s, 0] == pad (an all-pad row included): a wave per sequence, one ballot
// per 64 columns.
__global__ void __launch_bounds__(FILL_THREADS) pack_count_by_id_kernel(const int *ids, int *seq_len, int n_seq, int L, int pad) {
    const int lane = threadIdx.x & 63, s = (int)blockIdx.x * FILL_WAVES + (threadIdx.x >> 6);
    if (s >= n_seq) return;
    const int *src = ids + (size_t)s * L;
    int count = 0;
    for (int l0 = 0; l0 < L; l0 += 64) {
        const int l = l0 + lane;
        count += __builtin_popcountll(__ballot(l < L && src[l] != pad));
    }
    if (lane == 0) seq_len[s] = src[0] == pad ? -1 : count;
}

// pack_fill_kernel by id: the wave of a kept sequence walks ALL L columns; a non-pad id goes to row off + rank, rank = the non-pad
// ids before it (the ballot's prefix popcount plus the carry of the earlier rounds), with position pad + 1 + rank.
__global__ void __launch_bounds__(FILL_THREADS) pack_fill_by_id_kernel(const PackParams P) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    if ((int)blockIdx.x >= P.seq_blocks) {  // the slack rows
        const int T = clamp_to(P.seq_off[P.n_seq], 0, P.rows);
        const long long row = (long long)((int)blockIdx.x - P.seq_blocks) * FILL_THREADS + threadIdx.x;
        if (row >= T && row < P.rows) {
            P.out_ids[row] = P.pad;
            P.out_pos[row] = P.pad;
        }
        return;
    }
    const int s = (int)blockIdx.x * FILL_WAVES + wave;
    if (s >= P.n_seq) return;
    const int len = clamp_to(P.seq_kept[s], -1, P.L);
    if (len <= 0) return;
    const int off = clamp_to(P.seq_off[s], 0, P.rows);
    const int *src = P.ids + (size_t)s * P.L;
    int count = 0;  // the non-pad ids in the columns before this round's
    for (int l0 = 0; l0 < P.L; l0 += 64) {
        const int l = l0 + lane;
        const int raw = l < P.L ? src[l] : P.pad;
        const bool tok = raw != P.pad;
        const u64 b = __ballot(tok);
        const int rank = count + __builtin_popcountll(b & ((1ull << lane) - 1));  // columns 0 .. l - 1
        count += __builtin_popcountll(b);
        const long long row = (long long)off + rank;
        if (tok && rank < len && row < P.rows) {  // rank < len: the plan's count is the bound, whatever the ids hold by now
            P.out_ids[row] = raw;
            P.out_pos[row] = clamp_to(P.pad + 1 + rank, 0, P.max_pos - 1);
        }
    }
}

struct FirstRowsParams {
    const uint4 *src;
    uint4 *dst;
    const int *seq_off, *seq_kept;
    int n_seq, rows, pieces;  // pieces: 16-byte pieces per row
    long long ld_src, ld_dst;  // in pieces
    unsigned nan_word;
};

__global__ void __launch_bounds__(FILL_THREADS) first_rows_gather_kernel(const FirstRowsParams P) {
    const int lane = threadIdx.x & 63, s = (int)blockIdx.x * FILL_WAVES + (threadIdx.x >> 6);
    if (s >= P.n_seq) return;
    const int kept = P.seq_kept[s];
    const int row = clamp_to(P.seq_off[s], 0, P.rows - 1);
    const uint4 *x = P.src + (size_t)row * P.ld_src;
    uint4 *o = P.dst + (size_t)s * P.ld_dst;
    const unsigned fill = kept < 0 ? P.nan_word : 0u;
    for (int c = lane; c < P.pieces; c += 64) o[c] = kept > 0 ? x[c] : make_uint4(fill, fill, fill, fill);
}

__global__ void __launch_bounds__(FILL_THREADS) first_rows_scatter_kernel(const FirstRowsParams P) {
    const int lane = threadIdx.x & 63, s = (int)blockIdx.x * FILL_WAVES + (threadIdx.x >> 6);
    if (s >= P.n_seq) return;
    if (P.seq_kept[s] <= 0) return;  // kept sequences of length >= 1 start at distinct rows: one owner per row
    const int row = clamp_to(P.seq_off[s], 0, P.rows - 1);
    const uint4 *g = P.src + (size_t)s * P.ld_src;
    uint4 *o = P.dst + (size_t)row * P.ld_dst;
    for (int c = lane; c < P.pieces; c += 64) o[c] = g[c];
}

const char *check_ints4(const void *p, bool nullable = false) {
    if (!p) return nullable ? nullptr : "null pointer";
    if ((uintptr_t)p % 4) return "alignment: an integer array is not 4-byte aligned";
    return nullptr;
}

const char *check_first_rows(const AnceFirstRowsArgs *a) {
    if (!a) return "null pointer";
    if (a->H != 768 && a->H != 1024) return "width H not 768 or 1024";
    if (a->dtype != ANCE_DTYPE_F32 && a->dtype != ANCE_DTYPE_F16 && a->dtype != ANCE_DTYPE_BF16) return "dtype not ANCE_DTYPE_F32, _F16 or _BF16";
    if (a->n_seq < 1 || a->n_seq > 65535) return "n_seq outside 1 .. 65535";
    if (a->rows < 1) return "rows < 1";
    if (!a->rows_matrix || !a->first) return "null pointer";
    if ((uintptr_t)a->rows_matrix % 16 || (uintptr_t)a->first % 16) return "alignment: a base is not 16-byte aligned";
    const int piece = a->dtype == ANCE_DTYPE_F32 ? 4 : 8;
    if (a->ld_rows % piece || a->ld_rows < a->H || a->ld_first % piece || a->ld_first < a->H)
        return "stride: not a multiple of a 16-byte piece or below the width";
    if (const char *why = check_ints4(a->d_seq_off)) return why;
    if (const char *why = check_ints4(a->d_seq_kept)) return why;
    return nullptr;
}

FirstRowsParams first_rows_params(const AnceFirstRowsArgs *a, bool gather) {
    FirstRowsParams P = {};
    const int piece = a->dtype == ANCE_DTYPE_F32 ? 4 : 8;
    P.src = (const uint4 *)(gather ? a->rows_matrix : a->first);
    P.dst = (uint4 *)(gather ? a->first : a->rows_matrix);
    P.ld_src = (gather ? a->ld_rows : a->ld_first) / piece;
    P.ld_dst = (gather ? a->ld_first : a->ld_rows) / piece;
    P.seq_off = a->d_seq_off; P.seq_kept = a->d_seq_kept;
    P.n_seq = a->n_seq; P.rows = a->rows; P.pieces = a->H / piece;
    P.nan_word = a->dtype == ANCE_DTYPE_F32 ? 0x7FC00000u : (a->dtype == ANCE_DTYPE_F16 ? 0x7E007E00u : 0x7FC07FC0u);  // quiet NaNs
    return P;
}

}  // namespace
}  // namespace ance

extern "C" int ance_pack_tokens(const AncePackArgs *a, void *stream) {
    using namespace ance;
    const char *fn = "ance_pack_tokens";
    if (!a) return refuse(fn, "null pointer");
    if (a->n_seq < 1 || a->n_seq > 65535) return refuse(fn, "n_seq outside 1 .. 65535");
    if (a->L < 1 || a->L > 512) return refuse(fn, "L outside 1 .. 512");
    if (a->rows < 1) return refuse(fn, "rows < 1");
    if (a->vocab < 1 || a->max_pos < 1) return refuse(fn, "an empty table");
    if (a->position_mode == ANCE_EMBED_POSITION_ABSOLUTE) {
        if (a->padding_idx < -1 || a->padding_idx >= a->vocab) return refuse(fn, "padding_idx outside -1 .. vocab - 1");
    } else if (a->position_mode == ANCE_EMBED_POSITION_ROBERTA) {
        if (a->padding_idx < 0 || a->padding_idx >= a->vocab) return refuse(fn, "roberta positions: padding_idx outside 0 .. vocab - 1");
    } else {
        return refuse(fn, "position_mode not 0 or 1");
    }
    for (const void *p : {(const void *)a->ids, (const void *)a->d_seq_len, (const void *)a->d_seq_off, (const void *)a->d_seq_kept,
                          (const void *)a->packed_ids, (const void *)a->packed_positions})
        if (const char *why = check_ints4(p)) return refuse(fn, why);
    if (const char *why = check_ints4(a->type_ids, true)) return refuse(fn, why);
    if (a->type_ids && !a->packed_type_ids) return refuse(fn, "null pointer: type_ids without packed_type_ids");
    if (const char *why = check_ints4(a->packed_type_ids, true)) return refuse(fn, why);
    if (!a->d_dropped) return refuse(fn, "null pointer");
    if ((uintptr_t)a->d_dropped % 8) return refuse(fn, "alignment: d_dropped is not 8-byte aligned");

    PackParams P = {};
    P.ids = a->ids; P.type_ids = a->type_ids; P.seq_len = a->d_seq_len;
    P.seq_off = a->d_seq_off; P.seq_kept = a->d_seq_kept;
    P.out_ids = a->packed_ids; P.out_types = a->type_ids ? a->packed_type_ids : nullptr; P.out_pos = a->packed_positions;
    P.dropped = (long long *)a->d_dropped;
    P.n_seq = a->n_seq; P.L = a->L; P.rows = a->rows;
    P.roberta = a->position_mode == ANCE_EMBED_POSITION_ROBERTA; P.pad = a->padding_idx;
    P.vocab = a->vocab; P.max_pos = a->max_pos;
    P.seq_blocks = (a->n_seq + FILL_WAVES - 1) / FILL_WAVES;
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(pack_plan_kernel<false>, dim3(1), dim3(PLAN_THREADS), 0, st, P);
    const unsigned slack_blocks = (unsigned)(((int64_t)a->rows + FILL_THREADS - 1) / FILL_THREADS);
    hipLaunchKernelGGL(pack_fill_kernel, dim3((unsigned)P.seq_blocks + slack_blocks), dim3(FILL_THREADS), 0, st, P);
    return check_launch(fn);
}

extern "C" int ance_pack_tokens_by_id(const AncePackByIdArgs *a, void *stream) {
    using namespace ance;
    const char *fn = "ance_pack_tokens_by_id";
    if (!a) return refuse(fn, "null pointer");
    if (a->n_seq < 1 || a->n_seq > 65535) return refuse(fn, "n_seq outside 1 .. 65535");
    if (a->L < 1 || a->L > 512) return refuse(fn, "L outside 1 .. 512");
    if (a->rows < 1) return refuse(fn, "rows < 1");
    if (a->vocab < 1 || a->max_pos < 1) return refuse(fn, "an empty table");
    if (a->padding_idx < 0 || a->padding_idx >= a->vocab) return refuse(fn, "padding_idx outside 0 .. vocab - 1");
    for (const void *p : {(const void *)a->ids, (const void *)a->d_seq_len, (const void *)a->d_seq_off, (const void *)a->d_seq_kept,
                          (const void *)a->packed_ids, (const void *)a->packed_positions})
        if (const char *why = check_ints4(p)) return refuse(fn, why);
    if (!a->d_dropped) return refuse(fn, "null pointer");
    if ((uintptr_t)a->d_dropped % 8) return refuse(fn, "alignment: d_dropped is not 8-byte aligned");

    PackParams P = {};
    P.ids = a->ids; P.seq_len = a->d_seq_len;
    P.seq_off = a->d_seq_off; P.seq_kept = a->d_seq_kept;
    P.out_ids = a->packed_ids; P.out_pos = a->packed_positions;
    P.dropped = (long long *)a->d_dropped;
    P.n_seq = a->n_seq; P.L = a->L; P.rows = a->rows;
    P.roberta = 1; P.pad = a->padding_idx;
    P.vocab = a->vocab; P.max_pos = a->max_pos;
    P.seq_blocks = (a->n_seq + FILL_WAVES - 1) / FILL_WAVES;
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(pack_count_by_id_kernel, dim3((unsigned)P.seq_blocks), dim3(FILL_THREADS), 0, st, a->ids, a->d_seq_len, a->n_seq,
                       a->L, a->padding_idx);
    hipLaunchKernelGGL(pack_plan_kernel<true>, dim3(1), dim3(PLAN_THREADS), 0, st, P);
    const unsigned slack_blocks = (unsigned)(((int64_t)a->rows + FILL_THREADS - 1) / FILL_THREADS);
    hipLaunchKernelGGL(pack_fill_by_id_kernel, dim3((unsigned)P.seq_blocks + slack_blocks), dim3(FILL_THREADS), 0, st, P);
    return check_launch(fn);
}

extern "C" int ance_first_rows_gather(const AnceFirstRowsArgs *a, void *stream) {
    using namespace ance;
    const char *fn = "ance_first_rows_gather";
    if (const char *why = check_first_rows(a)) return refuse(fn, why);
    const FirstRowsParams P = first_rows_params(a, true);
    hipLaunchKernelGGL(first_rows_gather_kernel, dim3((unsigned)((a->n_seq + FILL_WAVES - 1) / FILL_WAVES)), dim3(FILL_THREADS), 0,
                       (hipStream_t)stream, P);
    return check_launch(fn);
}

extern "C" int ance_first_rows_scatter(const AnceFirstRowsArgs *a, void *stream) {
    using namespace ance;
    const char *fn = "ance_first_rows_scatter";
    if (const char *why = check_first_rows(a)) return refuse(fn, why);
    const FirstRowsParams P = first_rows_params(a, false);
    hipLaunchKernelGGL(first_rows_scatter_kernel, dim3((unsigned)((a->n_seq + FILL_WAVES - 1) / FILL_WAVES)), dim3(FILL_THREADS), 0,
                       (hipStream_t)stream, P);
    return check_launch(fn);
}
