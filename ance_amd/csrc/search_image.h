// The search image of a corpus shard (ip_topk_fast.hip, step 1): its layout in device memory and the kernels of
// ance_ip_index_build -- mean row, duplicate-class detection, compaction, fp16 rounding, completion stamp.
// Included by ip_topk_fast.hip only, into its anonymous namespace.
#pragma once
#include "topk_common.h"

namespace ance {
namespace {

constexpr int IDX_BLOCK_ROWS = 1024;
constexpr int IDX_SAMPLES = 2048;
constexpr int IDX_MIN_CLASS = 8;  // a duplicate class is collapsed when >= 8 of the 2,048 sampled rows fall in it

// Carves consecutive areas out of a device buffer from its 256-byte aligned start; a NULL buffer yields the sizes alone.
struct Carver {
    uintptr_t base;
    size_t o = 0, mark = 0;
    explicit Carver(const void *buf) : base(align_up((uintptr_t)buf, 256)) {}
    template <typename T>
    T *take(size_t bytes) {
        T *p = reinterpret_cast<T *>(base + o);
        o += bytes;
        return p;
    }
    size_t end_area() {  // pads to 256 bytes; returns the bytes taken since the previous call
        o = align_up(o, 256);
        const size_t bytes = o - mark;
        mark = o;
        return bytes;
    }
};

// Typed view of an image; the build's scratch areas (cls .. part) are part of it.  d_index = NULL: nb, n_part and bytes only.
struct ImageView {
    DedupHeader *hdr;    // first 256 bytes
    float *mu;           // [d] mean row of the shard
    _Float16 *x2;        // [n_live, d] fp16(x - mu)
    uint32_t *live2row;  // [n_live] image row -> shard row
    uint32_t *members;   // [DEDUP_MAXC][DEDUP_MEMCAP] smallest ids of every collapsed class
    uint8_t *cls;        // [n] class of a row, 0xFF: none
    uint32_t *blk;       // [1 + DEDUP_MAXC][nb] rows per counter field and block of 1,024 rows
    u64 *samp;           // [IDX_SAMPLES] sample hashes
    float *part;         // [n_part, d] column-sum partials
    int64_t nb;
    int n_part;          // row ranges of the column-sum pass
    size_t bytes;        // of the image, from its 256-byte aligned start
};
ImageView image_view(const void *d_index, int64_t n, int d) {
    ImageView V;
    V.nb = (n + IDX_BLOCK_ROWS - 1) / IDX_BLOCK_ROWS;
    V.n_part = (int)(V.nb < 1024 ? V.nb : 1024);
    Carver c(d_index);
    V.hdr = c.take<DedupHeader>(256);
    V.mu = c.take<float>(align_up((size_t)d * sizeof(float), 256));
    V.x2 = c.take<_Float16>(align_up((size_t)n * d * sizeof(_Float16), 256));
    V.live2row = c.take<uint32_t>(align_up((size_t)n * 4, 256));
    V.members = c.take<uint32_t>((size_t)DEDUP_MAXC * DEDUP_MEMCAP * 4);
    V.cls = c.take<uint8_t>(align_up((size_t)n + 4, 256));
    V.blk = c.take<uint32_t>(align_up((size_t)(1 + DEDUP_MAXC) * V.nb * 4, 256));
    V.samp = c.take<u64>((size_t)IDX_SAMPLES * sizeof(u64));
    V.part = c.take<float>(align_up((size_t)V.n_part * d * sizeof(float), 256));
    V.bytes = c.o;
    return V;
}

__device__ __forceinline__ u64 mix64(u64 z) {
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}

// mean row of the shard, pass 1: block b sums the rows b, b + gridDim.x, ... per column (fp32 partials; the mean only has to be a
// fixed vector near the centre of the rows -- its own accuracy never enters the error bound)
__global__ void __launch_bounds__(256) idx_colsum_kernel(const float *x, int64_t n, int d, float *part) {
    for (int c4 = threadIdx.x; c4 * 4 < d; c4 += 256) {
        f32x4 acc = {0.f, 0.f, 0.f, 0.f};
        for (int64_t r = blockIdx.x; r < n; r += gridDim.x) acc += *reinterpret_cast<const f32x4 *>(x + (size_t)r * d + c4 * 4);
        *reinterpret_cast<f32x4 *>(part + (size_t)blockIdx.x * d + c4 * 4) = acc;
    }
}
// pass 2: mu[c] = sum of the partials / n (double), or 0 when centring is off or a partial is not finite
__global__ void __launch_bounds__(256) idx_mean_kernel(const float *part, int n_part, int64_t n, int d, int center, float *mu) {
    const int c = blockIdx.x * 256 + threadIdx.x;
    if (c >= d) return;
    double s = 0.0;
    for (int p = 0; p < n_part; ++p) s += (double)part[(size_t)p * d + c];
    const float m = (float)(s / (double)n);
    mu[c] = (center && m == m && fabsf(m) < 3.0e38f) ? m : 0.0f;
}

// one wave per sampled row: position-mixed 64-bit hash of the row's bits; low 11 bits carry the sample index
__global__ void __launch_bounds__(256) idx_sample_hash_kernel(const float *x, int64_t n, int d, u64 *samp) {
    const int l = threadIdx.x & 63, w = threadIdx.x >> 6;
    const int j = blockIdx.x * 4 + w;
    if (j >= IDX_SAMPLES) return;
    const int64_t row = (int64_t)(((unsigned __int128)(unsigned long long)j * (unsigned long long)n) / IDX_SAMPLES);
    const uint32_t *s = reinterpret_cast<const uint32_t *>(x + (size_t)row * d);
    u64 h = 0;
    for (int k = l; k < d; k += 64) h += mix64(((u64)s[k] << 20) ^ (u64)(k + 1) * 0x9E3779B97F4A7C15ull);
    h = wave_sum(h);
    if (l == 0) samp[j] = (h & ~2047ull) | (u64)j;
}

// one block: sort the sample keys, every run of >= IDX_MIN_CLASS equal hashes defines a duplicate class
__global__ void __launch_bounds__(256) idx_find_classes_kernel(const u64 *samp, int64_t n, DedupHeader *H) {
    __shared__ u64 s[IDX_SAMPLES];
    __shared__ int ncls;
    for (int i = threadIdx.x; i < IDX_SAMPLES; i += 256) s[i] = samp[i];
    if (threadIdx.x == 0) ncls = 0;
    __syncthreads();
    bitonic_sort_desc(s, IDX_SAMPLES);
    for (int i = threadIdx.x; i < IDX_SAMPLES; i += 256) {
        if (i > 0 && (s[i] >> 11) == (s[i - 1] >> 11)) continue;  // not a run start
        int len = 1;
        while (i + len < IDX_SAMPLES && (s[i + len] >> 11) == (s[i] >> 11)) ++len;
        if (len >= IDX_MIN_CLASS) {
            const int c = atomicAdd(&ncls, 1);
            if (c < DEDUP_MAXC) {
                const int j = (int)(s[i] & 2047ull);
                H->guess[c] = (uint32_t)(((unsigned __int128)(unsigned long long)j * (unsigned long long)n) / IDX_SAMPLES);
                H->rep[c] = 0xFFFFFFFFu;
                H->csize[c] = 0;
            }
        }
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        H->n_classes = ncls < DEDUP_MAXC ? ncls : DEDUP_MAXC;
        H->n_live = (uint32_t)n;
    }
}

// class of every row (0xFF: none): a row belongs to class c when it is BIT-identical to the class's sample row.
// A lane first compares the leading 16 bytes of its own row; only matches are compared in full by the wave.
__global__ void __launch_bounds__(256) idx_classify_kernel(const float *x, int64_t n, int d, DedupHeader *H, uint8_t *cls) {
    const int nc = H->n_classes;
    if (nc == 0) return;
    __shared__ uint32_t wmin[4][DEDUP_MAXC];
    const int l = threadIdx.x & 63, w = threadIdx.x >> 6;
    typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));
    u32x4 head[DEDUP_MAXC];
    uint32_t mn[DEDUP_MAXC];
    for (int c = 0; c < DEDUP_MAXC; ++c) {
        mn[c] = 0xFFFFFFFFu;
        head[c] = *reinterpret_cast<const u32x4 *>(x + (size_t)H->guess[c < nc ? c : 0] * d);
    }
    const int64_t n_chunks = (n + 63) / 64;
    for (int64_t ch = (int64_t)blockIdx.x * 4 + w; ch < n_chunks; ch += (int64_t)gridDim.x * 4) {
        const int64_t row = ch * 64 + l;
        const bool rv = row < n;
        const u32x4 hv = *reinterpret_cast<const u32x4 *>(x + (size_t)(rv ? row : n - 1) * d);
        uint8_t mine = 0xFF;
        for (int c = 0; c < nc; ++c) {
            u64 m = __ballot(rv && hv[0] == head[c][0] && hv[1] == head[c][1] && hv[2] == head[c][2] && hv[3] == head[c][3]);
            const uint32_t *g = reinterpret_cast<const uint32_t *>(x + (size_t)H->guess[c] * d);
            while (m) {
                const int b = __builtin_ctzll(m);
                m &= m - 1;
                const uint32_t *r = reinterpret_cast<const uint32_t *>(x + (size_t)(ch * 64 + b) * d);
                bool ne = false;
                for (int k = l * 4; k < d; k += 256) {
                    const u32x4 a = *reinterpret_cast<const u32x4 *>(r + k), bb = *reinterpret_cast<const u32x4 *>(g + k);
                    ne |= a[0] != bb[0] || a[1] != bb[1] || a[2] != bb[2] || a[3] != bb[3];
                }
                if (__ballot(ne) == 0ull && l == b && mine == 0xFF) {
                    mine = (uint8_t)c;
                    mn[c] = min(mn[c], (uint32_t)row);
                }
            }
        }
        if (rv) cls[row] = mine;
    }
    for (int c = 0; c < nc; ++c) {
        const uint32_t v = wave_min(mn[c]);
        if (l == 0) wmin[w][c] = v;
    }
    __syncthreads();
    if (threadIdx.x < nc) {
        const int c = threadIdx.x;
        const uint32_t v = min(min(wmin[0][c], wmin[1][c]), min(wmin[2][c], wmin[3][c]));
        if (v != 0xFFFFFFFFu) atomicMin(&H->rep[c], v);
    }
}

// counter field of a row: 0 = stays in the image (no class, or the representative of its class), 1 + c = duplicate of class c
__device__ __forceinline__ int idx_row_field(const DedupHeader *H, uint8_t c, uint32_t row) {
    return (c == 0xFF || H->rep[c] == row) ? 0 : 1 + c;
}

// blk[f * nb + b] = rows of field f in block b (1,024 rows per block)
__global__ void __launch_bounds__(256) idx_count_kernel(int64_t n, int64_t nb, const DedupHeader *H, const uint8_t *cls,
                                                        uint32_t *blk) {
    if (H->n_classes == 0) return;
    __shared__ u64 ws[4];
    const int64_t r0 = (int64_t)blockIdx.x * IDX_BLOCK_ROWS + threadIdx.x * 4;
    u64 v = 0;  // five 12-bit fields (each <= 1024)
    for (int j = 0; j < 4; ++j)
        if (r0 + j < n) v += 1ull << (12 * idx_row_field(H, cls[r0 + j], (uint32_t)(r0 + j)));
    v = wave_sum(v);
    if ((threadIdx.x & 63) == 0) ws[threadIdx.x >> 6] = v;
    __syncthreads();
    if (threadIdx.x <= DEDUP_MAXC) {
        const u64 t = ws[0] + ws[1] + ws[2] + ws[3];
        blk[(size_t)threadIdx.x * nb + blockIdx.x] = (uint32_t)((t >> (12 * threadIdx.x)) & 4095ull);
    }
}

// one block: exclusive scan of every field over the blocks, in place; totals go to the header
__global__ void __launch_bounds__(1024) idx_scan_kernel(int64_t nb, DedupHeader *H, uint32_t *blk) {
    if (H->n_classes == 0) return;
    __shared__ uint32_t sh[1024];
    __shared__ uint32_t carry;
    const int tid = threadIdx.x;
    for (int f = 0; f <= DEDUP_MAXC; ++f) {
        if (tid == 0) carry = 0;
        __syncthreads();
        for (int64_t b0 = 0; b0 < nb; b0 += 1024) {
            const int64_t b = b0 + tid;
            const uint32_t mine = b < nb ? blk[(size_t)f * nb + b] : 0u;
            sh[tid] = mine;
            __syncthreads();
            for (int s = 1; s < 1024; s <<= 1) {
                const uint32_t t = tid >= s ? sh[tid - s] : 0u;
                __syncthreads();
                sh[tid] += t;
                __syncthreads();
            }
            if (b < nb) blk[(size_t)f * nb + b] = carry + sh[tid] - mine;
            __syncthreads();
            if (tid == 0) carry += sh[1023];
            __syncthreads();
        }
        if (tid == 0) {
            if (f == 0) H->n_live = carry;
            else H->csize[f - 1] = carry;
        }
        __syncthreads();
    }
}

// One wave centres a row on a mean vector and rounds it to fp16: dst = fp16(c), c = fl32(src - mean) -- x' of an image row,
// dq of a query.  *norm_c and *norm_o get upper bounds of |c| and |src| (they only feed an upper bound, hence the 1.0001),
// in every lane.  Image rows and queries share this routine because the error bound (search_query.h) rests on both
// sides doing this arithmetic; what a NaN norm means is the caller's business.
__device__ __forceinline__ void center_round_row(const float *src, const float *mean, int d, int l, _Float16 *dst, float *norm_c,
                                                 float *norm_o) {
    float q = 0.f, qo = 0.f;
    for (int k = l * 4; k < d; k += 256) {
        const f32x4 v = *reinterpret_cast<const f32x4 *>(src + k), m4 = *reinterpret_cast<const f32x4 *>(mean + k);
        f16x4 h;
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const float c = v[e] - m4[e];
            h[e] = (_Float16)c;
            q = fmaf(c, c, q);
            qo = fmaf(v[e], v[e], qo);
        }
        *reinterpret_cast<f16x4 *>(dst + k) = h;
    }
    *norm_c = sqrtf(wave_sum(q)) * 1.0001f;
    *norm_o = sqrtf(wave_sum(qo)) * 1.0001f;
}

// Builds the image: block b owns rows [1024 b, 1024 b + 1024).  Phase A ranks the block's rows inside their field
// (image position of a kept row, ordinal of a duplicate inside its class); phase B rounds the kept rows to fp16 at
// their image position (one wave per row) and folds their norms into the shard maximum.
__global__ void __launch_bounds__(256) idx_compact_round_kernel(const float *x, int64_t n, int d, int64_t nb, DedupHeader *H,
                                                                const uint8_t *cls, const uint32_t *blk, const float *mu,
                                                                _Float16 *x2, uint32_t *live2row, uint32_t *members) {
    __shared__ uint32_t pos_s[IDX_BLOCK_ROWS];  // image row of the block's rows, 0xFFFFFFFF for collapsed duplicates
    __shared__ u64 wtot[4];
    __shared__ float wmax[4], wmaxo[4];
    const int tid = threadIdx.x, l = tid & 63, w = tid >> 6;
    const int64_t r0 = (int64_t)blockIdx.x * IDX_BLOCK_ROWS;
    const int nc = H->n_classes;
    if (nc == 0) {
        if (blockIdx.x == 0 && tid == 0) H->n_live = (uint32_t)n;  // (not set by anyone when the class search is off)
        for (int j = tid; j < IDX_BLOCK_ROWS; j += 256) {
            const int64_t row = r0 + j;
            pos_s[j] = row < n ? (uint32_t)row : 0xFFFFFFFFu;
            if (row < n) live2row[row] = (uint32_t)row;
        }
    } else {
        int fld[4];
        u64 v = 0;
        for (int j = 0; j < 4; ++j) {
            const int64_t row = r0 + tid * 4 + j;
            fld[j] = row < n ? idx_row_field(H, cls[row], (uint32_t)row) : -1;
            if (fld[j] >= 0) v += 1ull << (12 * fld[j]);
        }
        // exclusive prefix of the packed counters over the block's 256 threads (rows are in thread order)
        u64 inc = v;
#pragma unroll
        for (int off = 1; off < 64; off <<= 1) {
            const u64 t = __shfl_up(inc, off);
            if (l >= off) inc += t;
        }
        if (l == 63) wtot[w] = inc;
        __syncthreads();
        u64 base = 0;
        for (int ww = 0; ww < w; ++ww) base += wtot[ww];
        u64 run = base + inc - v;
        for (int j = 0; j < 4; ++j) {
            if (fld[j] < 0) {  // past the end of the shard
                pos_s[tid * 4 + j] = 0xFFFFFFFFu;
                continue;
            }
            const uint32_t row = (uint32_t)(r0 + tid * 4 + j);
            const uint32_t rank = (uint32_t)((run >> (12 * fld[j])) & 4095ull);
            const uint32_t at = blk[(size_t)fld[j] * nb + blockIdx.x] + rank;
            if (fld[j] == 0) {
                pos_s[tid * 4 + j] = at;
                live2row[at] = row;
            } else {
                pos_s[tid * 4 + j] = 0xFFFFFFFFu;
                if (at < (uint32_t)DEDUP_MEMCAP) members[(size_t)(fld[j] - 1) * DEDUP_MEMCAP + at] = row;
            }
            run += 1ull << (12 * fld[j]);
        }
    }
    __syncthreads();
    float mymax = 0.0f, mymaxo = 0.0f;
    for (int j = w; j < IDX_BLOCK_ROWS; j += 4) {
        const uint32_t at = pos_s[j];
        if (at == 0xFFFFFFFFu) continue;  // wave-uniform
        const float *s = x + (size_t)(r0 + j) * d;
        _Float16 *hi = x2 + (size_t)at * d;
        float nr, nro;
        center_round_row(s, mu, d, l, hi, &nr, &nro);
        if (!(nr == nr)) nr = INFINITY;  // a NaN row must not hide from the fp16-trust test of the filter
        if (!(nro == nro)) nro = INFINITY;
        mymax = fmaxf(mymax, nr);
        mymaxo = fmaxf(mymaxo, nro);
    }
    // ONE atomic per block and maximum (a single word saturates near 88 atomics/us)
    if (l == 0) {
        wmax[w] = mymax;
        wmaxo[w] = mymaxo;
    }
    __syncthreads();
    if (tid == 0) {
        atomicMax(&H->xmax_bits, __builtin_bit_cast(unsigned int, fmaxf(fmaxf(wmax[0], wmax[1]), fmaxf(wmax[2], wmax[3]))));
        atomicMax(&H->xmax_orig_bits, __builtin_bit_cast(unsigned int, fmaxf(fmaxf(wmaxo[0], wmaxo[1]), fmaxf(wmaxo[2], wmaxo[3]))));
    }
}

// last kernel of a build: marks the image complete and names the matrix it belongs to (DedupHeader)
__global__ void __launch_bounds__(64) idx_stamp_kernel(DedupHeader *H, int64_t n, int d, const float *x) {
    if (threadIdx.x == 0) {
        H->d = (unsigned int)d;
        H->n = (unsigned long long)n;
        H->x_ptr = (unsigned long long)(uintptr_t)x;
        H->magic = DEDUP_MAGIC;
    }
}

}  // namespace
}  // namespace ance
