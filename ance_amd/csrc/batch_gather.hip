// Training batches gathered on the device (include/ance_amd.h: ance_gather_batch): the head of a trainer's step.  The reference
// builds a batch in Python -- per item three seek + read calls on the token caches (utils/util.py:292-298), twelve torch.tensor
// constructions (data/msmarco_data.py:275-303), then default collation, nine host-to-device copies and six .long() casts
// (drivers/run_ann.py:237-254).  Here the caches are resident as the files' own bytes (rows of 4 + 4 L bytes: big-endian
// passage_len, L little-endian int32) and the item list of the whole ann_training_data file is on the device, so a batch is ONE
// launch for up to three segments (query, first passage, second passage), with no copy, allocation or synchronisation.
//   grid (x, y)   y = segment; x covers the segment's B L output tokens as one flat array, four consecutive tokens per thread
//   per thread    row = token / L, t = token % L (four tokens may straddle rows when L is no multiple of 4); the record index of
//                 item first + row, CLAMPED into [0, n_records); the header, byte-swapped and clamped to L; one dword load per
//                 token id (a record is only 4-byte aligned: stride 84 at L = 20, 516 at L = 128)
//   stores        ids 16 bytes per store where the output is 16-byte aligned, else per element; a byte mask and the token types as
//                 one packed dword per four tokens (the outputs are 4-byte aligned and a thread's tokens start at a multiple of
//                 4); the last tokens of an output whose size is no multiple of 4 per element.  Every byte of [B, L] is written.
// Plain C++: no inline assembly, no atomics, no shared memory.
#include "common.h"

namespace ance {
namespace {

constexpr int GATHER_THREADS = 256, GATHER_TOKENS = 4;

struct GatherSeg {
    const uint32_t *rec;   // records as dwords: row stride 1 + L
    const int64_t *index;  // record index per item of the plan
    void *ids, *mask;
    uint8_t *types;        // nullable
    int64_t n_records;
    int32_t L, mask_rule, type_rule, vec;  // vec: ids and mask 16-byte aligned
};
struct GatherArgs {
    GatherSeg seg[3];
    int64_t first, B;
};

typedef int32_t i32x4 __attribute__((ext_vector_type(4)));
typedef long long i64x2 __attribute__((ext_vector_type(2)));

__device__ __forceinline__ uint32_t pack4(const uint32_t v[4]) { return v[0] | (v[1] << 8) | (v[2] << 16) | (v[3] << 24); }

// WIDE: int64 ids and mask (what the trainers' .long() makes); else int32 ids and a 1-byte bool mask.  Types are uint8 in both.
template <bool WIDE>
__global__ void __launch_bounds__(GATHER_THREADS) gather_batch_kernel(const GatherArgs A) {
    const GatherSeg S = A.seg[blockIdx.y];
    const int64_t total = A.B * (int64_t)S.L;
    const int64_t j0 = ((int64_t)blockIdx.x * GATHER_THREADS + threadIdx.x) * GATHER_TOKENS;
    if (j0 >= total) return;
    const int n = (int)min((int64_t)GATHER_TOKENS, total - j0);
    int64_t row = j0 / S.L;
    int t = (int)(j0 - row * S.L);
    const uint32_t *r = nullptr;
    uint32_t len = 0;
    bool fresh = true;
    uint32_t id[4] = {0, 0, 0, 0}, mk[4] = {0, 0, 0, 0}, ty[4] = {0, 0, 0, 0};
#pragma unroll
    for (int k = 0; k < GATHER_TOKENS; ++k) {
        if (k < n) {
            if (fresh) {
                int64_t ix = S.index[A.first + row];
                ix = ix < 0 ? 0 : (ix >= S.n_records ? S.n_records - 1 : ix);  // no index value reads outside the records
                r = S.rec + ix * (int64_t)(S.L + 1);
                len = min(__builtin_bswap32(r[0]), (uint32_t)S.L);
                fresh = false;
            }
            const uint32_t v = r[1 + t];
            const uint32_t in_len = (uint32_t)t < len ? 1u : 0u;
            id[k] = v;
            mk[k] = S.mask_rule == ANCE_GATHER_MASK_LENGTH ? in_len : (v != 0u ? 1u : 0u);
            ty[k] = S.type_rule == ANCE_GATHER_TYPES_LENGTH ? in_len : 0u;
            if (++t == S.L) {
                t = 0;
                ++row;
                fresh = true;
            }
        }
    }
    const bool full = n == GATHER_TOKENS;
    if (WIDE) {
        long long *ids = (long long *)S.ids + j0, *mask = (long long *)S.mask + j0;
        if (full && S.vec) {
            ((i64x2 *)ids)[0] = i64x2{(long long)(int32_t)id[0], (long long)(int32_t)id[1]};
            ((i64x2 *)ids)[1] = i64x2{(long long)(int32_t)id[2], (long long)(int32_t)id[3]};
            ((i64x2 *)mask)[0] = i64x2{(long long)mk[0], (long long)mk[1]};
            ((i64x2 *)mask)[1] = i64x2{(long long)mk[2], (long long)mk[3]};
        } else {
#pragma unroll
            for (int k = 0; k < GATHER_TOKENS; ++k) {
                if (k < n) {
                    ids[k] = (long long)(int32_t)id[k];
                    mask[k] = (long long)mk[k];
                }
            }
        }
    } else {
        int32_t *ids = (int32_t *)S.ids + j0;
        uint8_t *mask = (uint8_t *)S.mask + j0;
        if (full && S.vec) {
            *(i32x4 *)ids = i32x4{(int32_t)id[0], (int32_t)id[1], (int32_t)id[2], (int32_t)id[3]};
        } else {
#pragma unroll
            for (int k = 0; k < GATHER_TOKENS; ++k)
                if (k < n) ids[k] = (int32_t)id[k];
        }
        if (full) {
            *(uint32_t *)mask = pack4(mk);
        } else {
#pragma unroll
            for (int k = 0; k < GATHER_TOKENS; ++k)
                if (k < n) mask[k] = (uint8_t)mk[k];
        }
    }
    if (S.types) {
        uint8_t *types = S.types + j0;
        if (full) {
            *(uint32_t *)types = pack4(ty);
        } else {
#pragma unroll
            for (int k = 0; k < GATHER_TOKENS; ++k)
                if (k < n) types[k] = (uint8_t)ty[k];
        }
    }
}

int gather_refuse(const char *why) {
    char buf[160];
    snprintf(buf, sizeof(buf), "ance_gather_batch: invalid argument (%s)", why);
    set_last_error(buf);
    return ANCE_E_INVALID;
}

}  // namespace
}  // namespace ance

extern "C" int ance_gather_batch(const AnceGatherSegment *h_segs, int n_segs, int64_t first, int64_t B, int width, void *stream) {
    using namespace ance;
    if (!h_segs) return gather_refuse("null segment table");
    if (n_segs < 1 || n_segs > 3) return gather_refuse("n_segs outside 1..3");
    if (B < 1) return gather_refuse("B < 1");
    if (first < 0) return gather_refuse("first < 0");
    if (width != ANCE_GATHER_REFERENCE && width != ANCE_GATHER_WIDE) return gather_refuse("unknown width code");
    const bool wide = width == ANCE_GATHER_WIDE;
    const uintptr_t wide_align = wide ? 8 : 4;  // int64 outputs at their natural alignment
    GatherArgs A = {};
    A.first = first;
    A.B = B;
    int64_t blocks = 0;
    for (int s = 0; s < n_segs; ++s) {
        const AnceGatherSegment &h = h_segs[s];
        if (!h.d_records || !h.d_index || !h.d_ids || !h.d_mask) return gather_refuse("null pointer");
        if (h.L < 1) return gather_refuse("L < 1");
        if (h.n_records < 1) return gather_refuse("n_records < 1");
        if (h.n_index < 0 || first > h.n_index || B > h.n_index - first) return gather_refuse("first + B past the item index");
        if (h.mask_rule != ANCE_GATHER_MASK_LENGTH && h.mask_rule != ANCE_GATHER_MASK_NONZERO) return gather_refuse("unknown mask code");
        if (h.type_rule != ANCE_GATHER_TYPES_ZERO && h.type_rule != ANCE_GATHER_TYPES_LENGTH) return gather_refuse("unknown type code");
        if ((uintptr_t)h.d_records % 4) return gather_refuse("d_records not 4-byte aligned");
        if ((uintptr_t)h.d_index % 8) return gather_refuse("d_index not 8-byte aligned");
        if ((uintptr_t)h.d_ids % wide_align || (uintptr_t)h.d_mask % wide_align || (uintptr_t)h.d_types % 4)
            return gather_refuse(wide ? "an output not 4-byte (int64: 8-byte) aligned" : "an output not 4-byte aligned");
        if (B > (INT64_MAX / 8) / h.L) return gather_refuse("B * L too large");
        const int64_t per_block = (int64_t)GATHER_THREADS * GATHER_TOKENS;
        const int64_t nb = (B * (int64_t)h.L + per_block - 1) / per_block;
        if (nb > (int64_t)INT32_MAX) return gather_refuse("B * L too large");
        blocks = nb > blocks ? nb : blocks;
        GatherSeg &S = A.seg[s];
        S.rec = (const uint32_t *)h.d_records;
        S.index = h.d_index;
        S.ids = h.d_ids;
        S.mask = h.d_mask;
        S.types = (uint8_t *)h.d_types;
        S.n_records = h.n_records;
        S.L = h.L;
        S.mask_rule = h.mask_rule;
        S.type_rule = h.type_rule;
        S.vec = ((uintptr_t)h.d_ids | (uintptr_t)h.d_mask) % 16 == 0;
    }
    hipStream_t st = (hipStream_t)stream;
    if (wide)
        hipLaunchKernelGGL(gather_batch_kernel<true>, dim3((unsigned)blocks, (unsigned)n_segs), dim3(GATHER_THREADS), 0, st, A);
    else
        hipLaunchKernelGGL(gather_batch_kernel<false>, dim3((unsigned)blocks, (unsigned)n_segs), dim3(GATHER_THREADS), 0, st, A);
    return check_launch("ance_gather_batch");
}
