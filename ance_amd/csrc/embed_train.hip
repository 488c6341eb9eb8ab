// The input end of a trainable tower with its gradients (include/ance_amd.h: ance_embed_*): what transformers' eager BertEmbeddings /
// RobertaEmbeddings compute, fp32 throughout.
//   forward   id, tt, p clamped into their tables FIRST;  v = (word[id] + type[tt]) + pos[p];  mean, var two-pass over the row in
//             registers, rstd = 1 / sqrtf(var + eps);  y = keep o (xhat gamma + beta) / (1 - p_drop)
//             p = column (absolute) or pad + (id != pad ? number of ids != pad in columns 0 .. l of the sequence : 0) (roberta: the
//             wave reads its sequence's prefix and counts; the position is saved for the backward)
//   backward  row kernel: v and xhat recomputed from the tables and the saved (mean, rstd), the mask regenerated;
//             d = keep o dy / (1 - p_drop);  g = d o gamma;  dv = rstd (g - mean_H(g) - xhat mean_H(g o xhat)) -> workspace [T, H];
//             partial rows of dgamma = sum d o xhat, dbeta = sum d and sum dv per 16-row workgroup, then row_kernels.h's tree
//             table gradients: dTable[key] = sum of dv over the rows with that key, a segmented sum over the rows in the order of a
//             STABLE sort of the keys (see seg_piece_kernel below).  No atomics.
//   rows forms  (ance_embed_rows_*: packed rows, pack_rows.hip) the same kernels over T rows with L = 1 whose position is the CALLER's
//             positions[row], read in both directions; dpos then always goes through the sorted keys
// One wave owns a token row, as in layer_tail.hip; the reductions, the partial rows and the tree are row_kernels.h's.
#include "common.h"
#include "philox.h"
#include "row_kernels.h"

#include <math.h>

namespace ance {
namespace {

constexpr int SEG_C = ANCE_EMBED_SEGMENT_CHUNK;  // sorted positions per chunk: one per lane of a wave
static_assert(SEG_C == 64, "a chunk is one key per lane");

struct EmbedParams {
    const int *ids, *type_ids;
    const float *word, *pos, *type, *gamma, *beta, *dy;
    float *y, *g, *mean, *rstd, *part;
    int *positions;
    int64_t n_rows;
    int L, vocab, max_pos, n_types, roberta, pad;
    int given;  // the rows forms (ance_embed_rows_*): the position of a row is positions[row], in both directions
    float eps, keep_scale;
    uint32_t seed_lo, seed_hi, off_lo, off_hi, keep_thr;
    const uint64_t *d_stream;  // null, or the device stream {seed, base} (philox.h: drop_stream)
};

__device__ __forceinline__ int clampi(int v, int n) { return v < 0 ? 0 : (v >= n ? n - 1 : v); }

// (id, tt, p) of a row, each clamped into its table before anything is addressed with it.  FWD: the roberta position is counted from
// the sequence's prefix; otherwise it is read back from the saved buffer (and clamped again: the buffer is memory like any other).
// given (the rows forms): the caller's positions are read, forward and backward, and the forward writes none.
template <bool FWD>
__device__ __forceinline__ void row_keys(const EmbedParams &P, int64_t row, int lane, int &id, int &tt, int &p) {
    id = clampi(P.ids[row], P.vocab);
    tt = P.type_ids ? clampi(P.type_ids[row], P.n_types) : 0;
    const int l = (int)(row % P.L);
    if (P.given) {
        p = clampi(P.positions[row], P.max_pos);
    } else if (!P.roberta) {
        p = clampi(l, P.max_pos);
    } else if (FWD) {
        const int *seq = P.ids + (row - l);
        int n = 0;
        for (int t = lane; t <= l; t += 64) n += clampi(seq[t], P.vocab) != P.pad ? 1 : 0;
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) n += __shfl_xor(n, off);
        p = clampi(P.pad + (id != P.pad ? n : 0), P.max_pos);
    } else {
        p = clampi(P.positions[row], P.max_pos);
    }
}

// v = (word[id] + type[tt]) + pos[p]: no multiplication, so the forward and the backward form the same bits
template <int NV>
__device__ __forceinline__ void embed_sum(const EmbedParams &P, int id, int tt, int p, int lane, f32x4 (&v)[NV]) {
    constexpr int H = 256 * NV;
    const float *w = P.word + (size_t)id * H, *t = P.type + (size_t)tt * H, *q = P.pos + (size_t)p * H;
#pragma unroll
    for (int i = 0; i < NV; ++i) {
        const int c = 4 * (64 * i + lane);
        v[i] = (load4(w + c) + load4(t + c)) + load4(q + c);
    }
}

// keep bits of four columns (bit e: column 4 c4 + e) under the layer tail's counter contract
__device__ __forceinline__ uint32_t keep_bits(const EmbedParams &P, const DropStream &D, int64_t row, int c4) {
    uint32_t w[4], k = 0;
    philox4((uint32_t)row, (uint32_t)c4, D.off_lo, D.off_hi, D.seed_lo, D.seed_hi, w);
#pragma unroll
    for (int e = 0; e < 4; ++e) k |= (w[e] >= P.keep_thr ? 1u : 0u) << e;
    return k;
}

template <int NV, int DROP>
__global__ void __launch_bounds__(LT_THREADS) embed_fwd_kernel(const EmbedParams P) {
    const DropStream D = drop_stream<DROP>(P);
    constexpr float H = (float)(256 * NV);
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    f32x4 ga[NV], be[NV];
    load_vec(ga, P.gamma, lane);
    load_vec(be, P.beta, lane);
    const int64_t r0 = (int64_t)blockIdx.x * LT_ROWS + wave * LT_RPW;
    for (int j = 0; j < LT_RPW; ++j) {
        const int64_t row = r0 + j;
        if (row >= P.n_rows) break;  // the same in every lane of the wave
        int id, tt, p;
        row_keys<true>(P, row, lane, id, tt, p);
        f32x4 z[NV];
        embed_sum<NV>(P, id, tt, p, lane, z);
        float s = 0.f;
#pragma unroll
        for (int i = 0; i < NV; ++i) s += (z[i][0] + z[i][1]) + (z[i][2] + z[i][3]);
        const float mean = wave_sum(s) / H;
        float q = 0.f;
#pragma unroll
        for (int i = 0; i < NV; ++i) {
            z[i] -= mean;
            q += (z[i][0] * z[i][0] + z[i][1] * z[i][1]) + (z[i][2] * z[i][2] + z[i][3] * z[i][3]);
        }
        const float rstd = 1.0f / sqrtf(wave_sum(q) / H + P.eps);
        float *yr = P.y + row * (256 * NV);
#pragma unroll
        for (int i = 0; i < NV; ++i) {
            const int c4 = 64 * i + lane;
            f32x4 y = z[i] * rstd * ga[i] + be[i];
            if (DROP) {
                const uint32_t k = keep_bits(P, D, row, c4);
#pragma unroll
                for (int e = 0; e < 4; ++e) y[e] = (k >> e) & 1u ? y[e] * P.keep_scale : 0.f;
            }
            store4(yr + 4 * c4, y);
        }
        if (lane == 0) {
            P.mean[row] = mean;
            P.rstd[row] = rstd;
            if (P.roberta && !P.given) P.positions[row] = p;
        }
    }
}

template <int NV, int DROP>
__global__ void __launch_bounds__(LT_THREADS) embed_bwd_kernel(const EmbedParams P) {
    const DropStream D = drop_stream<DROP>(P);
    __shared__ __attribute__((aligned(16))) f32x4 sm[2 * 3 * NV * 64];
    constexpr float H = (float)(256 * NV);
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    f32x4 ga[NV];
    load_vec(ga, P.gamma, lane);
    f32x4 acc[3 * NV];  // dgamma, dbeta, sum of dv (the gradient of a one-row type table)
#pragma unroll
    for (int a = 0; a < 3 * NV; ++a) acc[a] = f32x4{0.f, 0.f, 0.f, 0.f};
    const int64_t r0 = (int64_t)blockIdx.x * LT_ROWS + wave * LT_RPW;
    for (int j = 0; j < LT_RPW; ++j) {
        const int64_t row = r0 + j;
        if (row >= P.n_rows) break;  // the same in every lane of the wave
        int id, tt, p;
        row_keys<false>(P, row, lane, id, tt, p);
        f32x4 xh[NV], g[NV];
        embed_sum<NV>(P, id, tt, p, lane, xh);
        const float mean = P.mean[row], rstd = P.rstd[row];
        const float *gr = P.dy + row * (256 * NV);
        float s1 = 0.f, s2 = 0.f;
#pragma unroll
        for (int i = 0; i < NV; ++i) {
            const int c4 = 64 * i + lane;
            f32x4 d = load4(gr + 4 * c4);
            if (DROP) {
                const uint32_t k = keep_bits(P, D, row, c4);
#pragma unroll
                for (int e = 0; e < 4; ++e) d[e] = (k >> e) & 1u ? d[e] * P.keep_scale : 0.f;
            }
            xh[i] = (xh[i] - mean) * rstd;
            g[i] = d * ga[i];
            const f32x4 gx = g[i] * xh[i];
            s1 += (g[i][0] + g[i][1]) + (g[i][2] + g[i][3]);
            s2 += (gx[0] + gx[1]) + (gx[2] + gx[3]);
            acc[i] += d * xh[i];
            acc[NV + i] += d;
        }
        const float m1 = wave_sum(s1) / H, m2 = wave_sum(s2) / H;
        float *go = P.g + row * (256 * NV);
#pragma unroll
        for (int i = 0; i < NV; ++i) {
            const f32x4 dv = (g[i] - m1 - xh[i] * m2) * rstd;
            store4(go + 4 * (64 * i + lane), dv);
            acc[2 * NV + i] += dv;
        }
    }
    write_partial(sm, acc, P.part + (int64_t)blockIdx.x * (3 * 256 * NV));
}

// ---- the segmented row sum -------------------------------------------------------------------------------------------------------
// dTable[key] = sum of g[row] over the rows with that key.  The rows stand in the order of a stable sort of the keys (sorted position
// j: key(j), row(j)), so the rows of one key are a run of consecutive j in ascending row order.  The sorted positions are cut into
// aligned chunks of SEG_C; a PIECE is a maximal run of one key inside a chunk.  First launch: a workgroup per chunk, a wave per piece
// (wave w of four takes the pieces w, w + 4, ..), which adds the piece's rows in ascending j.  A piece that is its key's whole run
// is stored into the table; any other goes to the chunk's partial rows (slot 0: the piece starts the chunk; slot 1: it does not,
// and so ends it).  Second launch: a wave per chunk; the one whose chunk holds the START of a run that goes on into the next chunk
// adds that run's partial rows in ascending chunk order and stores the table row.  Which rows are added in which order is a function
// of the sorted keys alone -- not of the grid, not of timing.  The longest serial chain is SEG_C + n / SEG_C row additions for a key
// with n rows.  Rows of the key `pad` are skipped: their table row keeps the caller's zeros.
// Three tables ride in one launch (blockIdx.y).  mode 1: keys and rows come from arrays (the raw sorted keys are clamped here, which
// keeps them sorted; a row index is clamped into [0, T)).  mode 2, analytic: key(j) = j / n_seq, row(j) = (j % n_seq) L + j / n_seq
// -- the absolute positions, which need no sort.
struct SegTable {
    const int *keys;
    const int64_t *perm;
    float *out, *part;  // [n_keys][H]; [n_chunks][2][H]
    int mode, n_keys, pad, n_seq, L;
};
struct SegParams {
    SegTable t[3];
    const float *g;
    int64_t n_rows;
};

__device__ __forceinline__ int seg_key(const SegTable &S, int64_t j) {
    return S.mode == 2 ? (int)(j / S.n_seq) : clampi(S.keys[j], S.n_keys);
}
__device__ __forceinline__ int64_t seg_row(const SegTable &S, int64_t j, int64_t T) {
    if (S.mode == 2) return (j % S.n_seq) * S.L + j / S.n_seq;
    const int64_t r = S.perm[j];
    return r < 0 ? 0 : (r >= T ? T - 1 : r);
}

template <int NV>
__global__ void __launch_bounds__(256) seg_piece_kernel(const SegParams P) {
    constexpr int H = 256 * NV;
    const SegTable &S = P.t[blockIdx.y];
    if (S.mode == 0) return;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int64_t T = P.n_rows, j0 = (int64_t)blockIdx.x * SEG_C;
    const int nvalid = (int)(T - j0 < SEG_C ? T - j0 : SEG_C);  // >= 1: the grid is ceil(T / SEG_C)
    const bool valid = lane < nvalid;
    const int key = valid ? seg_key(S, j0 + lane) : -2;
    const int row = valid ? (int)seg_row(S, j0 + lane, T) : 0;
    const int prev = __shfl_up(key, 1);
    u64 heads = __ballot(valid && (lane == 0 || key != prev));
    const int key_before = j0 > 0 ? seg_key(S, j0 - 1) : -3, key_after = j0 + SEG_C < T ? seg_key(S, j0 + SEG_C) : -3;
    for (int idx = 0; heads; ++idx) {
        const int s = __builtin_ctzll(heads);
        heads &= heads - 1;
        const int e = heads ? __builtin_ctzll(heads) : nvalid;
        if ((idx & 3) != wave) continue;
        const int k = __shfl(key, s);
        if (k == S.pad) continue;
        f32x4 acc[NV];
        load_vec(acc, P.g + (size_t)__shfl(row, s) * H, lane);
        for (int t = s + 1; t < e; ++t) {
            const float *gr = P.g + (size_t)__shfl(row, t) * H;
#pragma unroll
            for (int i = 0; i < NV; ++i) acc[i] += load4(gr + 4 * (64 * i + lane));
        }
        const bool whole = !(s == 0 && key_before == k) && !(e == SEG_C && key_after == k);
        float *dst = whole ? S.out + (size_t)k * H : S.part + ((size_t)blockIdx.x * 2 + (s == 0 ? 0 : 1)) * H;
#pragma unroll
        for (int i = 0; i < NV; ++i) store4(dst + 4 * (64 * i + lane), acc[i]);
    }
}

template <int NV>
__global__ void __launch_bounds__(256) seg_join_kernel(const SegParams P) {
    constexpr int H = 256 * NV;
    const SegTable &S = P.t[blockIdx.y];
    if (S.mode == 0) return;
    const int lane = threadIdx.x & 63;
    const int64_t T = P.n_rows, n_chunks = (T + SEG_C - 1) / SEG_C;
    const int64_t c = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6), j0 = c * SEG_C;
    if (c + 1 >= n_chunks) return;               // the last chunk's runs go nowhere; every chunk before it is full
    const int k = seg_key(S, j0 + SEG_C - 1);
    if (seg_key(S, j0 + SEG_C) != k) return;     // the chunk's last run ends with it
    if (k == S.pad) return;
    const int s = __builtin_ctzll(__ballot(seg_key(S, j0 + lane) == k));
    if (s == 0 && c > 0 && seg_key(S, j0 - 1) == k) return;  // the run started earlier: its first chunk's wave does it
    f32x4 acc[NV];
    load_vec(acc, S.part + ((size_t)c * 2 + (s == 0 ? 0 : 1)) * H, lane);
    for (int64_t cc = c + 1;; ++cc) {
        const float *pr = S.part + (size_t)cc * 2 * H;
#pragma unroll
        for (int i = 0; i < NV; ++i) acc[i] += load4(pr + 4 * (64 * i + lane));
        if (cc + 1 >= n_chunks) break;
        if (seg_key(S, cc * SEG_C + SEG_C - 1) != k || seg_key(S, (cc + 1) * SEG_C) != k) break;
    }
    float *dst = S.out + (size_t)k * H;
#pragma unroll
    for (int i = 0; i < NV; ++i) store4(dst + 4 * (64 * i + lane), acc[i]);
}

// ---- host ------------------------------------------------------------------------------------------------------------------------
size_t seg_chunks(int64_t n_rows) { return (size_t)((n_rows + SEG_C - 1) / SEG_C); }
size_t g_bytes(int64_t n_rows, int H) { return (size_t)n_rows * H * sizeof(float); }
size_t part_bytes(int64_t n_rows, int H) { return n_part(n_rows) * 3 * (size_t)H * sizeof(float); }
size_t seg_bytes(int64_t n_rows, int H) { return seg_chunks(n_rows) * 2 * (size_t)H * sizeof(float); }
size_t embed_ws_bytes(int64_t n_rows, int H) {
    return stats_bytes(n_rows) + g_bytes(n_rows, H) + part_bytes(n_rows, H) + 3 * seg_bytes(n_rows, H);
}

const char *check_ints(const void *p, bool nullable = false) {
    if (!p) return nullable ? nullptr : "null pointer";
    if ((uintptr_t)p % 4) return "alignment: an integer array is not 4-byte aligned";
    return nullptr;
}

const char *check_embed(const AnceEmbedArgs *a, bool backward, bool rows = false) {
    if (!a) return "null pointer";
    if (a->H != 768 && a->H != 1024) return "width H not 768 or 1024";
    if (rows && a->L != 1) return "the rows form takes L = 1: n_seq is the number of rows";
    if (a->L < 1 || a->L > 512) return "L outside 1 .. 512";
    if (a->n_seq < 1 || (int64_t)a->n_seq * a->L > 0x7fffffff) return "n_seq < 1 or more than 2^31 - 1 rows";
    if (a->vocab < 1 || a->max_pos < 1) return "an empty table";
    if (a->n_types != 1 && a->n_types != 2) return "n_types not 1 or 2";
    if (rows) {  // the positions are given: the mode only says whether the position table has a padding row
        if (a->position_mode != ANCE_EMBED_POSITION_ABSOLUTE && a->position_mode != ANCE_EMBED_POSITION_ROBERTA) return "position_mode not 0 or 1";
        const int lo = a->position_mode == ANCE_EMBED_POSITION_ROBERTA ? 0 : -1;
        if (a->padding_idx < lo || a->padding_idx >= a->vocab) return "padding_idx outside its range";
        if (const char *why = check_ints(a->positions)) return why;
    } else if (a->position_mode == ANCE_EMBED_POSITION_ABSOLUTE) {
        if (a->L > a->max_pos) return "absolute positions: L > max_pos";
        if (a->padding_idx < -1 || a->padding_idx >= a->vocab) return "padding_idx outside -1 .. vocab - 1";
    } else if (a->position_mode == ANCE_EMBED_POSITION_ROBERTA) {
        if (a->padding_idx < 0 || a->padding_idx >= a->vocab) return "roberta positions: padding_idx outside 0 .. vocab - 1";
        if ((int64_t)a->L + a->padding_idx + 1 > a->max_pos) return "roberta positions: L + padding_idx + 1 > max_pos";
        if (const char *why = check_ints(a->positions)) return why;
    } else {
        return "position_mode not 0 or 1";
    }
    if (const char *why = check_ints(a->ids)) return why;
    if (const char *why = check_ints(a->type_ids, true)) return why;
    if (const char *why = check_vector(a->word)) return why;
    if (const char *why = check_vector(a->pos)) return why;
    if (const char *why = check_vector(a->type)) return why;
    if (const char *why = check_vector(a->gamma)) return why;
    if (!backward) {  // the backward touches neither y nor beta
        if (const char *why = check_vector(a->y)) return why;
        if (const char *why = check_vector(a->beta)) return why;
    }
    if (!(a->dropout_p >= 0.0f && a->dropout_p < 1.0f)) return "dropout_p outside [0, 1)";
    if (!(a->eps > 0.0f)) return "eps <= 0";
    const int64_t n_rows = (int64_t)a->n_seq * a->L;
    return check_workspace(a->d_workspace, a->workspace_bytes, backward ? embed_ws_bytes(n_rows, a->H) : stats_bytes(n_rows));
}

EmbedParams embed_params(const AnceEmbedArgs *a, const uint64_t *d_stream, bool rows = false) {
    EmbedParams P = {};
    const int64_t n_rows = (int64_t)a->n_seq * a->L;
    P.ids = a->ids; P.type_ids = a->type_ids;
    P.word = a->word; P.pos = a->pos; P.type = a->type; P.gamma = a->gamma; P.beta = a->beta;
    P.y = a->y; P.positions = a->positions;
    P.n_rows = n_rows;
    P.L = a->L; P.vocab = a->vocab; P.max_pos = a->max_pos; P.n_types = a->n_types;
    P.roberta = !rows && a->position_mode == ANCE_EMBED_POSITION_ROBERTA; P.pad = a->padding_idx;
    P.given = rows ? 1 : 0;
    char *ws = (char *)a->d_workspace;
    P.mean = (float *)ws;
    P.rstd = (float *)(ws + stats_bytes(n_rows) / 2);
    P.g = (float *)(ws + stats_bytes(n_rows));
    P.part = (float *)(ws + stats_bytes(n_rows) + g_bytes(n_rows, a->H));
    P.eps = a->eps;
    P.seed_lo = (uint32_t)a->seed; P.seed_hi = (uint32_t)(a->seed >> 32);
    P.off_lo = (uint32_t)a->offset; P.off_hi = (uint32_t)(a->offset >> 32);
    P.d_stream = d_stream;  // given: seed and base come from the device, a->offset is added to the base
    P.keep_thr = (uint32_t)((double)a->dropout_p * 4294967296.0);  // floor(p 2^32), p < 1
    P.keep_scale = 1.0f / (1.0f - a->dropout_p);
    return P;
}
bool drops(const AnceEmbedArgs *a) { return a->training != 0 && a->dropout_p > 0.0f; }

template <int DROP>
void launch_embed_fwd(int H, dim3 grid, dim3 block, hipStream_t st, const EmbedParams &P) {
    if (H == 768) hipLaunchKernelGGL((embed_fwd_kernel<3, DROP>), grid, block, 0, st, P);
    else hipLaunchKernelGGL((embed_fwd_kernel<4, DROP>), grid, block, 0, st, P);
}
template <int DROP>
void launch_embed_bwd(int H, dim3 grid, dim3 block, hipStream_t st, const EmbedParams &P) {
    if (H == 768) hipLaunchKernelGGL((embed_bwd_kernel<3, DROP>), grid, block, 0, st, P);
    else hipLaunchKernelGGL((embed_bwd_kernel<4, DROP>), grid, block, 0, st, P);
}

}  // namespace
}  // namespace ance

extern "C" int ance_embed_segment_chunk(void) {
    return ance::SEG_C;
}

extern "C" size_t ance_embed_workspace_bytes(int64_t n_rows, int H) {
    using namespace ance;
    return rows_ok(n_rows) && (H == 768 || H == 1024) ? embed_ws_bytes(n_rows, H) : 0;
}

static int ance_embed_forward_impl(const char *fn, const AnceEmbedArgs *args, const uint64_t *d_stream, void *stream, bool rows = false) {
    using namespace ance;
    if (!stream_aligned(d_stream)) return refuse(fn, "alignment: d_stream is not 16-byte aligned");
    if (const char *why = check_embed(args, false, rows)) return refuse(fn, why);
    const EmbedParams P = embed_params(args, d_stream, rows);
    const dim3 grid((unsigned)n_part(P.n_rows)), block(LT_THREADS);
    hipStream_t st = (hipStream_t)stream;
    const int mode = drop_mode(drops(args), d_stream);
    if (mode == DROP_DEVICE) launch_embed_fwd<DROP_DEVICE>(args->H, grid, block, st, P);
    else if (mode == DROP_HOST) launch_embed_fwd<DROP_HOST>(args->H, grid, block, st, P);
    else launch_embed_fwd<DROP_NONE>(args->H, grid, block, st, P);
    return check_launch(fn);
}

static int ance_embed_backward_impl(const char *fn, const AnceEmbedArgs *args, const AnceEmbedGradArgs *grads, const uint64_t *d_stream,
                                    void *stream, bool rows = false) {
    using namespace ance;
    if (!stream_aligned(d_stream)) return refuse(fn, "alignment: d_stream is not 16-byte aligned");
    if (const char *why = check_embed(args, true, rows)) return refuse(fn, why);
    if (!grads) return refuse(fn, "null pointer");
    if (const char *why = check_vector(grads->dy)) return refuse(fn, why);
    for (const float *p : {(const float *)grads->dword, (const float *)grads->dpos, (const float *)grads->dtype,
                           (const float *)grads->dgamma, (const float *)grads->dbeta})
        if (const char *why = check_vector(p, true)) return refuse(fn, why);
    const bool roberta = args->position_mode == ANCE_EMBED_POSITION_ROBERTA;
    // which table gradients go through the segmented sum, and with which grouping
    const bool seg_word = grads->dword != nullptr, seg_pos = grads->dpos != nullptr;
    const bool seg_type = grads->dtype != nullptr && args->n_types == 2 && args->type_ids != nullptr;
    if (seg_word && (!grads->word_keys || !grads->word_perm)) return refuse(fn, "null pointer: dword without word_keys / word_perm");
    if (seg_pos && (roberta || rows) && (!grads->pos_keys || !grads->pos_perm)) return refuse(fn, "null pointer: dpos without pos_keys / pos_perm");
    if (seg_type && (!grads->type_keys || !grads->type_perm)) return refuse(fn, "null pointer: dtype without type_keys / type_perm");
    for (const void *p : {(const void *)grads->word_keys, (const void *)grads->pos_keys, (const void *)grads->type_keys})
        if (const char *why = check_ints(p, true)) return refuse(fn, why);
    for (const void *p : {(const void *)grads->word_perm, (const void *)grads->pos_perm, (const void *)grads->type_perm})
        if (p && (uintptr_t)p % 8) return refuse(fn, "alignment: a permutation is not 8-byte aligned");

    EmbedParams P = embed_params(args, d_stream, rows);
    P.dy = grads->dy;
    const int H = args->H;
    const dim3 grid((unsigned)n_part(P.n_rows)), block(LT_THREADS);
    hipStream_t st = (hipStream_t)stream;
    const int mode = drop_mode(drops(args), d_stream);
    if (mode == DROP_DEVICE) launch_embed_bwd<DROP_DEVICE>(H, grid, block, st, P);
    else if (mode == DROP_HOST) launch_embed_bwd<DROP_HOST>(H, grid, block, st, P);
    else launch_embed_bwd<DROP_NONE>(H, grid, block, st, P);
    // a type table that needs no grouping: every row has type 0, whose gradient is the column sum of dv
    float *dtype0 = grads->dtype && !seg_type ? grads->dtype : nullptr;
    hipLaunchKernelGGL(colsum_tree_kernel, dim3((unsigned)(3 * H / 64)), dim3(256), 0, st, (const float *)P.part,
                       (int64_t)n_part(P.n_rows), 3 * H, H, grads->dgamma, grads->dbeta, dtype0);
    if (seg_word || seg_pos || seg_type) {
        SegParams S = {};
        S.g = P.g;
        S.n_rows = P.n_rows;
        char *seg = (char *)P.part + part_bytes(P.n_rows, H);
        const size_t sb = seg_bytes(P.n_rows, H);
        if (seg_word) S.t[0] = SegTable{grads->word_keys, grads->word_perm, grads->dword, (float *)seg, 1, args->vocab, args->padding_idx, 0, 0};
        if (seg_pos && (roberta || rows))  // rows: sorted keys in absolute mode too (a row is no longer s * L + p), and no padding row there
            S.t[1] = SegTable{grads->pos_keys, grads->pos_perm, grads->dpos, (float *)(seg + sb), 1, args->max_pos,
                              roberta ? args->padding_idx : -1, 0, 0};
        else if (seg_pos)
            S.t[1] = SegTable{nullptr, nullptr, grads->dpos, (float *)(seg + sb), 2, args->L, -1, args->n_seq, args->L};
        if (seg_type) S.t[2] = SegTable{grads->type_keys, grads->type_perm, grads->dtype, (float *)(seg + 2 * sb), 1, 2, -1, 0, 0};
        const unsigned chunks = (unsigned)seg_chunks(P.n_rows);
        if (H == 768) {
            hipLaunchKernelGGL(seg_piece_kernel<3>, dim3(chunks, 3), dim3(256), 0, st, S);
            hipLaunchKernelGGL(seg_join_kernel<3>, dim3((chunks + 3) / 4, 3), dim3(256), 0, st, S);
        } else {
            hipLaunchKernelGGL(seg_piece_kernel<4>, dim3(chunks, 3), dim3(256), 0, st, S);
            hipLaunchKernelGGL(seg_join_kernel<4>, dim3((chunks + 3) / 4, 3), dim3(256), 0, st, S);
        }
    }
    return check_launch(fn);
}

// The entry points: each with its sibling that takes the device dropout stream (include/ance_amd.h); the plain one passes none.
extern "C" int ance_embed_forward(const AnceEmbedArgs *args, void *stream) {
    return ance_embed_forward_impl("ance_embed_forward", args, nullptr, stream);
}
extern "C" int ance_embed_forward_dstream(const AnceEmbedArgs *args, const uint64_t *d_stream, void *stream) {
    return ance_embed_forward_impl("ance_embed_forward_dstream", args, d_stream, stream);
}
extern "C" int ance_embed_backward(const AnceEmbedArgs *args, const AnceEmbedGradArgs *grads, void *stream) {
    return ance_embed_backward_impl("ance_embed_backward", args, grads, nullptr, stream);
}
extern "C" int ance_embed_backward_dstream(const AnceEmbedArgs *args, const AnceEmbedGradArgs *grads, const uint64_t *d_stream,
                                           void *stream) {
    return ance_embed_backward_impl("ance_embed_backward_dstream", args, grads, d_stream, stream);
}

// The rows forms: n_seq rows (L = 1) whose positions are the caller's (include/ance_amd.h) -- the same kernels, the same launches.
extern "C" int ance_embed_rows_forward(const AnceEmbedArgs *args, void *stream) {
    return ance_embed_forward_impl("ance_embed_rows_forward", args, nullptr, stream, true);
}
extern "C" int ance_embed_rows_forward_dstream(const AnceEmbedArgs *args, const uint64_t *d_stream, void *stream) {
    return ance_embed_forward_impl("ance_embed_rows_forward_dstream", args, d_stream, stream, true);
}
extern "C" int ance_embed_rows_backward(const AnceEmbedArgs *args, const AnceEmbedGradArgs *grads, void *stream) {
    return ance_embed_backward_impl("ance_embed_rows_backward", args, grads, nullptr, stream, true);
}
extern "C" int ance_embed_rows_backward_dstream(const AnceEmbedArgs *args, const AnceEmbedGradArgs *grads, const uint64_t *d_stream,
                                                void *stream) {
    return ance_embed_backward_impl("ance_embed_rows_backward_dstream", args, grads, d_stream, stream, true);
}
