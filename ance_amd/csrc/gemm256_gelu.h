// The two GELUs of the 256 x 256 GEMM epilogues with their __constant__ coefficient tables: a header of ONE translation unit.
#pragma once
#include "common.h"

namespace ance {

// ---- fp16 mode: gelu_erf256 ----
// GELU(x) = x * Phi(x) = max(x, 0) - |x| * h(|x| / sqrt 2),  h(z) = erfc(z) / 2 = 2^q(z).
// q is a degree-5 least-squares fit of log2(erfc(z) / 2) on [0, 5] weighted by z h(z) (the factor
// the error is multiplied with); beyond 5 q keeps falling, so h underflows to 0 as it should.
// |GELU error| <= 8e-6 over [-9, 9] in fp32 (the stored result is fp16: 2^-11 relative), checked
// against scipy's erf when the coefficients were fitted.  One transcendental (v_exp_f32) and, on four
// adjacent columns at a time, packed bias add and final multiply-subtract -- the erfc rational form
// (Abramowitz-Stegun 7.1.26) this replaces needed v_rcp + v_exp + 17 scalar ops per element, and this epilogue runs on 3072 columns
// per token with no MFMA work to hide behind (one workgroup per CU).
typedef float f32x2 __attribute__((ext_vector_type(2)));
// coefficients live in constant memory (scalar loads) rather than as instruction literals: with literals hipcc
// emits one v_fmaak_f32 per element, with register operands the Horner steps become v_pk_fma_f32 (two elements
// per issue slot)
__constant__ float kGeluQ[6] = {-1.00054646f, -1.62252474f, -0.934321642f, -0.129834279f, 0.0201726463f, -0.00133047544f};

__device__ __forceinline__ f32x4 gelu_erf256(f32x4 x) {
    const f32x4 ax = __builtin_elementwise_abs(x);
    f32x4 out;
#pragma unroll
    for (int p = 0; p < 2; ++p) {
        const f32x2 a2 = {ax[2 * p], ax[2 * p + 1]};
        const f32x2 z = a2 * 0.70710678118654752440f;
        f32x2 q = z * kGeluQ[5] + kGeluQ[4];
        q = q * z + kGeluQ[3];
        q = q * z + kGeluQ[2];
        q = q * z + kGeluQ[1];
        q = q * z + kGeluQ[0];
        const f32x2 h = {__builtin_amdgcn_exp2f(q[0]), __builtin_amdgcn_exp2f(q[1])};
        const f32x2 x2 = {x[2 * p], x[2 * p + 1]};
        const f32x2 r = __builtin_elementwise_max(x2, f32x2{0.0f, 0.0f}) - a2 * h;
        out[2 * p] = r[0];
        out[2 * p + 1] = r[1];
    }
    return out;
}

// ---- split (fp32-grade) mode: gelu_exact / gelu_exact4 ----
// erf-form GELU (the reference's: transformers "gelu" = x Phi(x)) to fp32 grade WITHOUT the library erff.  ocml's erff is two
// branches (both executed in a 64-lane wave: ~38 VALU instructions per output) and the GELU epilogue of the split FFN1 GEMM was
// VALU-bound on it (20.6 us of a 67.6 us tile against 14.4 us for the plain fp32 store epilogue).  Here
//     Phi(x) = x >= 0 ? 1 - e : e,    e = erfc(|x| / sqrt 2) / 2 = 2^q(z),  z = min(|x| / sqrt 2, 6.6)
// with q a degree-9 polynomial fit of log2(erfc(z) / 2) on [0, 6.6] (weighted for the ABSOLUTE error of e: approximation error
// 1.1e-9; monomial in z, so that near z = 0 the sum is -1 plus small terms; beyond z = 6.6 e < 2^-66): 9 fma + v_exp_f32 + 6.
// Measured against the exact value in fp32 emulation (tests/test_gelu_poly.py, 8 M points): |error| / |x| <= 1.1e-7 everywhere
// -- torch's own fp32 erf-GELU, which is what the reference runs, is at 3.7e-7 -- mean |error| 1.7e-8 (torch 4.5e-8).
// (contraction off here and in the split epilogue: hipcc contracts a * b + c into an fma in SOME of the unrolled instances of
// a loop and not in others, so a row's last bit would depend on which pass / register slot of the tile it lands in -- and with
// it on the micro-batch split and the number of GPUs.  Every fused operation below is written out as fmaf.)
constexpr float GELU_Q[10] = {-1.0f, -1.627907395362854f, -0.918441653251648f, -0.14831341803073883f, 0.02773732878267765f,
                              6.778987153666094e-05f, -0.002261603018268943f, 0.0008423461113125086f, -0.00015156660811044276f,
                              1.1468856428109575e-05f};
__device__ __forceinline__ float gelu_exact(float x) {
#pragma clang fp contract(off)
    const float z = __builtin_fminf(__builtin_fabsf(x) * 0.70710678118654752440f, 6.6f);
    float q = GELU_Q[9];
#pragma unroll
    for (int k = 8; k >= 0; --k) q = __builtin_fmaf(q, z, GELU_Q[k]);
    const float e = __builtin_amdgcn_exp2f(q);
    return x * (x >= 0.0f ? 1.0f - e : e);
}

// Four at a time on the PACKED fp32 pipe (round 6): v_pk_fma_f32 runs two IEEE fmas per issue slot, and the GELU epilogue is bound by
// its vector instructions (9 of its ~21 per element are the Horner steps: they were v_fmaak_f32, one element each, because the
// coefficients were literals).  The coefficients come from constant memory here (scalar registers, as kGeluQ above), the steps are
// element-wise fmas on float2 -- the same operations in the same order: bit-identical to gelu_exact.
__constant__ float kGeluExactQ[10] = {GELU_Q[0], GELU_Q[1], GELU_Q[2], GELU_Q[3], GELU_Q[4], GELU_Q[5], GELU_Q[6], GELU_Q[7], GELU_Q[8], GELU_Q[9]};
__device__ __forceinline__ f32x4 gelu_exact4(const f32x4 x) {
#pragma clang fp contract(off)
    f32x4 out;
#pragma unroll
    for (int p = 0; p < 2; ++p) {
        const f32x2 x2 = {x[2 * p], x[2 * p + 1]};
        const f32x2 z = __builtin_elementwise_min(__builtin_elementwise_abs(x2) * 0.70710678118654752440f, f32x2{6.6f, 6.6f});
        f32x2 q = {kGeluExactQ[9], kGeluExactQ[9]};
#pragma unroll
        for (int k = 8; k >= 0; --k) q = __builtin_elementwise_fma(q, z, f32x2{kGeluExactQ[k], kGeluExactQ[k]});
        const float e0 = __builtin_amdgcn_exp2f(q[0]), e1 = __builtin_amdgcn_exp2f(q[1]);
        out[2 * p] = x2[0] * (x2[0] >= 0.0f ? 1.0f - e0 : e0);
        out[2 * p + 1] = x2[1] * (x2[1] >= 0.0f ? 1.0f - e1 : e1);
    }
    return out;
}

}  // namespace ance
