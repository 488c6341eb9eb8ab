// Philox4x32-10: the dropout stream of the trainers' kernels (include/ance_amd.h states the key and the counters).
#pragma once
#include <stdint.h>

#include <hip/hip_runtime.h>

namespace ance {

__device__ __forceinline__ void philox4(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3, uint32_t k0, uint32_t k1, uint32_t w[4]) {
#pragma unroll
    for (int r = 0; r < 10; ++r) {
        const uint64_t p0 = (uint64_t)0xD2511F53u * c0, p1 = (uint64_t)0xCD9E8D57u * c2;  // one 32 x 32 -> 64 multiply each
        const uint32_t hi0 = (uint32_t)(p0 >> 32), lo0 = (uint32_t)p0, hi1 = (uint32_t)(p1 >> 32), lo1 = (uint32_t)p1;
        c0 = hi1 ^ c1 ^ k0;
        c1 = lo1;
        c2 = hi0 ^ c3 ^ k1;
        c3 = lo0;
        k0 += 0x9E3779B9u;
        k1 += 0xBB67AE85u;
    }
    w[0] = c0; w[1] = c1; w[2] = c2; w[3] = c3;
}

// How a kernel instantiation draws its masks (the DROP template argument of every dropout kernel): not at all, under the host pair
// of its parameter block, or under the device stream.  The host instantiations are the code they were before the device stream
// existed; a device instantiation differs from its host twin by one uniform 16-byte read and a 64-bit add at kernel entry.
constexpr int DROP_NONE = 0, DROP_HOST = 1, DROP_DEVICE = 2;
inline int drop_mode(bool drops, const uint64_t *d_stream) { return !drops ? DROP_NONE : d_stream ? DROP_DEVICE : DROP_HOST; }

// The (seed, offset) a kernel draws under.  Params carries the host pair as (seed_lo, seed_hi, off_lo, off_hi) and d_stream, the
// device stream {uint64 seed, uint64 base} (include/ance_amd.h).  DROP_DEVICE: the seed is d_stream[0] and the offset d_stream[1]
// plus the host offset, a 64-bit add; read once, at kernel entry.
struct DropStream {
    uint32_t seed_lo, seed_hi, off_lo, off_hi;
};
template <int DROP, class Params>
__device__ __forceinline__ DropStream drop_stream(const Params &P) {
    DropStream D = {P.seed_lo, P.seed_hi, P.off_lo, P.off_hi};
    if (DROP == DROP_DEVICE) {
        const uint64_t seed = P.d_stream[0], off = P.d_stream[1] + ((uint64_t)P.off_hi << 32 | (uint64_t)P.off_lo);
        D.seed_lo = (uint32_t)seed;
        D.seed_hi = (uint32_t)(seed >> 32);
        D.off_lo = (uint32_t)off;
        D.off_hi = (uint32_t)(off >> 32);
    }
    return D;
}

// host side: a device stream must be 16-byte aligned (one 16-byte read)
inline bool stream_aligned(const uint64_t *d_stream) { return (uintptr_t)d_stream % 16 == 0; }

}  // namespace ance
