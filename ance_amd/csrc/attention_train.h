// What the fp32 and the 16-bit self-attention cores of the trainers share (attention_train.hip, attention_train_half.hip).
#pragma once
#include <stdint.h>

#include <hip/hip_runtime.h>

namespace ance {

// word c of the four words that lane E of this lane's quad holds (DPP quad broadcast, then a select on the lane's own c)
template <int E>
__device__ __forceinline__ uint32_t quad_word(const uint32_t w[4], int c) {
    const uint32_t t0 = (uint32_t)__builtin_amdgcn_update_dpp(0, (int)w[0], E * 0x55, 0xf, 0xf, false);
    const uint32_t t1 = (uint32_t)__builtin_amdgcn_update_dpp(0, (int)w[1], E * 0x55, 0xf, 0xf, false);
    const uint32_t t2 = (uint32_t)__builtin_amdgcn_update_dpp(0, (int)w[2], E * 0x55, 0xf, 0xf, false);
    const uint32_t t3 = (uint32_t)__builtin_amdgcn_update_dpp(0, (int)w[3], E * 0x55, 0xf, 0xf, false);
    return (c & 2) ? ((c & 1) ? t3 : t2) : ((c & 1) ? t1 : t0);
}

// first row and clamped length of sequence s: never a row outside [0, n_rows), whatever the descriptors say
template <class Params>
__device__ __forceinline__ int seq_bounds(const Params &P, int s, int *first) {
    const int f = P.seq_first[s];
    int len = P.seq_len[s];
    *first = f;
    if (f < 0 || f >= P.n_rows || len < 0) return 0;
    if (len > P.max_seq_len) len = P.max_seq_len;
    if (len > P.n_rows - f) len = P.n_rows - f;
    return len;
}

}  // namespace ance
