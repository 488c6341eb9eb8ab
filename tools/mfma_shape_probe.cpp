// Does the MFMA shape change the rate the board sustains at its power cap?  v_mfma_f32_32x32x16_f16 against
// v_mfma_f32_16x16x32_f16 at equal FLOPs per step and equal LDS bytes per FLOP, with the split GEMM's product pattern
// (hi x hi, lo x hi, hi x lo into one accumulator).  Measurement tool; not part of the library.
//   build: hipcc --offload-arch=gfx950 -O3 -o tools/mfma_shape_probe tools/mfma_shape_probe.cpp
//   run:   tools/mfma_shape_probe [seconds per case] [alternations]
// As tools/power_probe: 512 workgroups of 512 threads (one per CU, 8 waves with up to 256 registers each), launched in a loop for
// the given time while a host thread samples the amdgpu hwmon files; prints TF executed, mean power, mean clock per case and shape.
// One step is one K-tile of the split main loop of one wave, in its two phases:
//   32x32x16: P0 16 fragment reads, 24 MFMAs on acc[0..1][0..1] (2 k-steps x 3 products); P1 8 reads, 24 MFMAs on acc[0..1][2..3]
//             -- 8 f32x16 accumulators
//   16x16x32: P0 16 fragment reads, 48 MFMAs on acc[0..3][0..3] (3 products);             P1 8 reads, 48 MFMAs on acc[0..3][4..7]
//             -- 32 f32x4 accumulators
// Cases:
//   bare      operands in registers (the reads are skipped), random N(0, 1/3) halves
//   lds       + the 24 ds_read_b128 of a K-tile, feeding the MFMAs (lane-linear, conflict-free addresses)
//   lds_pair  as lds with the lo fragments small (|x| <= 2^-11: the lo halves of a pair)
// Before the rate cases it checks the arithmetic of both shapes on one wave against the exact (fp64) sums: f16 subnormal lo halves
// must be multiplied (not flushed), and the accumulation's signed error in fp32 ulps (RNE: mean ~ 0) for zero-mean and all-positive
// operands and a split-like chain (K = 3 x 768), as scripts/mfma_rounding_probe.py does for the GEMM.
#include <hip/hip_runtime.h>
#include <atomic>
#include <chrono>
#include <cctype>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <string>
#include <thread>
#include <vector>
#include <glob.h>

typedef _Float16 f16x8 __attribute__((ext_vector_type(8)));
typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef float f32x16 __attribute__((ext_vector_type(16)));

constexpr int IMG_HALVES = 32 * 1024;  // 64 KiB LDS image: hi fragments from the lower half, lo fragments from the upper

// fragment f (0..23) of a K-tile: its LDS offset (halves) for this lane; odd f are lo fragments
__device__ __forceinline__ int frag_off(int it, int w, int l, int f) {
    const int base = ((it * 97 + w * 13 + f * 5) & 15) * 1024 + l * 8;
    return (f & 1) * (IMG_HALVES / 2) + (base & (IMG_HALVES / 2 - 1));
}

template <bool LDS>
__global__ void __launch_bounds__(512, 1) probe32(const _Float16 *hi, const _Float16 *lo, float *sink, int iters) {
    extern __shared__ __attribute__((aligned(16))) _Float16 lds[];
    const int tid = threadIdx.x, l = tid & 63, w = tid >> 6;
    f16x8 fa[2][4], fb[2][4];  // A: [m block][hi k0 | hi k16 | lo k0 | lo k16], B: [n block][same]
    for (int y = 0; y < 2; ++y)
        for (int s = 0; s < 4; ++s) {
            const _Float16 *src = s < 2 ? hi : lo;
            fa[y][s] = *reinterpret_cast<const f16x8 *>(src + ((size_t)(blockIdx.x * 512 + tid) * 16 + y * 4 + s) * 8 % (IMG_HALVES * 16));
            fb[y][s] = *reinterpret_cast<const f16x8 *>(src + ((size_t)(blockIdx.x * 512 + tid) * 16 + 8 + y * 4 + s) * 8 % (IMG_HALVES * 16));
        }
    if (LDS) {
        for (int e = tid; e < IMG_HALVES / 8; e += 512) {
            const _Float16 *src = e * 8 < IMG_HALVES / 2 ? hi : lo;
            *reinterpret_cast<f16x8 *>(lds + e * 8) = *reinterpret_cast<const f16x8 *>(src + (size_t)e * 8);
        }
        __syncthreads();
    }
    f32x16 acc[2][4];
    for (int x = 0; x < 2; ++x)
        for (int y = 0; y < 4; ++y) acc[x][y] = f32x16{0};
    constexpr int pa[6] = {0, 2, 0, 1, 3, 1}, pb[6] = {0, 0, 2, 1, 1, 3};
    for (int it = 0; it < iters; ++it) {
#pragma unroll
        for (int ph = 0; ph < 2; ++ph) {
            if (LDS) {  // P0: A (8) + B (8), P1: A (8)
#pragma unroll
                for (int y = 0; y < 2; ++y)
#pragma unroll
                    for (int s = 0; s < 4; ++s) fa[y][s] = *reinterpret_cast<const f16x8 *>(lds + frag_off(it, w, l, ph * 8 + y * 4 + s));
                if (ph == 0)
#pragma unroll
                    for (int x = 0; x < 2; ++x)
#pragma unroll
                        for (int s = 0; s < 4; ++s) fb[x][s] = *reinterpret_cast<const f16x8 *>(lds + frag_off(it, w, l, 16 + x * 4 + s));
            }
#pragma unroll
            for (int x = 0; x < 2; ++x)
#pragma unroll
                for (int c = 0; c < 6; ++c)
#pragma unroll
                    for (int y = 0; y < 2; ++y)
                        acc[x][2 * ph + y] = __builtin_amdgcn_mfma_f32_32x32x16_f16(fb[x][pb[c]], fa[y][pa[c]], acc[x][2 * ph + y], 0, 0, 0);
        }
    }
    float s = 0.f;
    for (int x = 0; x < 2; ++x)
        for (int y = 0; y < 4; ++y)
            for (int e = 0; e < 16; ++e) s += acc[x][y][e];
    if (s == 12345.678f) sink[0] = s;
}

template <bool LDS>
__global__ void __launch_bounds__(512, 1) probe16(const _Float16 *hi, const _Float16 *lo, float *sink, int iters) {
    extern __shared__ __attribute__((aligned(16))) _Float16 lds[];
    const int tid = threadIdx.x, l = tid & 63, w = tid >> 6;
    f16x8 fa[4][2], fb[4][2];  // A: [m block of this phase][hi | lo], B: [n block][hi | lo]
    for (int y = 0; y < 4; ++y)
        for (int s = 0; s < 2; ++s) {
            const _Float16 *src = s == 0 ? hi : lo;
            fa[y][s] = *reinterpret_cast<const f16x8 *>(src + ((size_t)(blockIdx.x * 512 + tid) * 16 + y * 2 + s) * 8 % (IMG_HALVES * 16));
            fb[y][s] = *reinterpret_cast<const f16x8 *>(src + ((size_t)(blockIdx.x * 512 + tid) * 16 + 8 + y * 2 + s) * 8 % (IMG_HALVES * 16));
        }
    if (LDS) {
        for (int e = tid; e < IMG_HALVES / 8; e += 512) {
            const _Float16 *src = e * 8 < IMG_HALVES / 2 ? hi : lo;
            *reinterpret_cast<f16x8 *>(lds + e * 8) = *reinterpret_cast<const f16x8 *>(src + (size_t)e * 8);
        }
        __syncthreads();
    }
    f32x4 acc[4][8];
    for (int x = 0; x < 4; ++x)
        for (int y = 0; y < 8; ++y) acc[x][y] = f32x4{0};
    for (int it = 0; it < iters; ++it) {
#pragma unroll
        for (int ph = 0; ph < 2; ++ph) {
            if (LDS) {
#pragma unroll
                for (int y = 0; y < 4; ++y)
#pragma unroll
                    for (int s = 0; s < 2; ++s) fa[y][s] = *reinterpret_cast<const f16x8 *>(lds + frag_off(it, w, l, ph * 8 + y * 2 + s));
                if (ph == 0)
#pragma unroll
                    for (int x = 0; x < 4; ++x)
#pragma unroll
                        for (int s = 0; s < 2; ++s) fb[x][s] = *reinterpret_cast<const f16x8 *>(lds + frag_off(it, w, l, 16 + x * 2 + s));
            }
#pragma unroll
            for (int x = 0; x < 4; ++x)
#pragma unroll
                for (int p = 0; p < 3; ++p)
#pragma unroll
                    for (int y = 0; y < 4; ++y)
                        acc[x][4 * ph + y] = __builtin_amdgcn_mfma_f32_16x16x32_f16(fb[x][p == 2], fa[y][p == 1], acc[x][4 * ph + y], 0, 0, 0);
        }
    }
    float s = 0.f;
    for (int x = 0; x < 4; ++x)
        for (int y = 0; y < 8; ++y)
            for (int e = 0; e < 4; ++e) s += acc[x][y][e];
    if (s == 12345.678f) sink[0] = s;
}

// ---- arithmetic check: one wave, C[m][n] = sum_k A[m][k] B[n][k] over K (row-major A: M x K, B: N x K, fp16), out fp32 row-major
// 32x32x16: lane l holds row l & 31, k 8 (l >> 5) .. + 7 of a 16-deep step; C register i: row 8 (i >> 2) + 4 (l >> 5) + (i & 3),
//           column l & 31 (first operand = B -> columns... see below)
// Both kernels use the product orientation of the GEMM, mfma(B fragment, A fragment): the first operand indexes C's rows, so the
// output is C^T; we store C^T[n][m] accordingly.
__global__ void check32(const _Float16 *A, const _Float16 *B, float *out, int K) {
    const int l = threadIdx.x;
    f32x16 acc = f32x16{0};
    for (int k0 = 0; k0 < K; k0 += 16) {
        const f16x8 a = *reinterpret_cast<const f16x8 *>(A + (size_t)(l & 31) * K + k0 + 8 * (l >> 5));
        const f16x8 b = *reinterpret_cast<const f16x8 *>(B + (size_t)(l & 31) * K + k0 + 8 * (l >> 5));
        acc = __builtin_amdgcn_mfma_f32_32x32x16_f16(b, a, acc, 0, 0, 0);
    }
    for (int i = 0; i < 16; ++i) out[(size_t)(l & 31) * 32 + 8 * (i >> 2) + 4 * (l >> 5) + (i & 3)] = acc[i];  // out[m][n]
}
__global__ void check16(const _Float16 *A, const _Float16 *B, float *out, int K) {
    const int l = threadIdx.x;
    f32x4 acc = f32x4{0};
    for (int k0 = 0; k0 < K; k0 += 32) {
        const f16x8 a = *reinterpret_cast<const f16x8 *>(A + (size_t)(l & 15) * K + k0 + 8 * (l >> 4));
        const f16x8 b = *reinterpret_cast<const f16x8 *>(B + (size_t)(l & 15) * K + k0 + 8 * (l >> 4));
        acc = __builtin_amdgcn_mfma_f32_16x16x32_f16(b, a, acc, 0, 0, 0);
    }
    for (int i = 0; i < 4; ++i) out[(size_t)(l & 15) * 16 + 4 * (l >> 4) + i] = acc[i];  // out[m][n]
}

static std::string g_pci;
static std::string hwmon_file(const char *name) {
    glob_t g;
    std::string pat = (g_pci.empty() ? std::string("/sys/class/drm/card*/device/hwmon/hwmon*/") : "/sys/bus/pci/devices/" + g_pci + "/hwmon/hwmon*/") + name;
    std::string r;
    if (glob(pat.c_str(), 0, nullptr, &g) == 0 && g.gl_pathc > 0) r = g.gl_pathv[0];
    globfree(&g);
    return r;
}
static double read_num(const std::string &p) {
    FILE *f = fopen(p.c_str(), "r");
    if (!f) return -1;
    double v = -1;
    if (fscanf(f, "%lf", &v) != 1) v = -1;
    fclose(f);
    return v;
}

static unsigned long long g_st = 88172645463325252ull;
static double rnd() { g_st ^= g_st << 13; g_st ^= g_st >> 7; g_st ^= g_st << 17; return (double)((g_st >> 11) & 0xFFFFFFFFFFull) / (double)0x10000000000ull; }
static double ulp32(double x) { int e; std::frexp(std::fabs(x) > 1e-30 ? x : 1e-30, &e); return std::ldexp(1.0, e - 24); }

// returns false on a HIP error
static bool arith_check(bool &ok) {
    const int Kmax = 3072;
    _Float16 *dA, *dB;
    float *dO;
    if (hipMalloc(&dA, 32 * Kmax * 2) != hipSuccess || hipMalloc(&dB, 32 * Kmax * 2) != hipSuccess || hipMalloc(&dO, 32 * 32 * 4) != hipSuccess) return false;
    std::vector<_Float16> A(32 * Kmax), B(32 * Kmax);
    std::vector<float> O(32 * 32);
    ok = true;
    for (int shape = 0; shape < 2; ++shape) {
        const int T = shape == 0 ? 32 : 16;
        const char *nm = shape == 0 ? "32x32x16" : "16x16x32";
        // subnormals: A = j 2^-24 (j = 1..1023, all subnormal), B = 1 -> exact row sums
        {
            const int K = 128;
            for (int m = 0; m < 32; ++m)
                for (int k = 0; k < K; ++k) {
                    A[m * K + k] = (_Float16)(((m * K + k) % 1023 + 1) * std::ldexp(1.0, -24));
                    B[m * K + k] = (_Float16)1.0;
                }
            (void)hipMemcpy(dA, A.data(), 32 * K * 2, hipMemcpyHostToDevice);
            (void)hipMemcpy(dB, B.data(), 32 * K * 2, hipMemcpyHostToDevice);
            if (shape == 0) hipLaunchKernelGGL(check32, dim3(1), dim3(64), 0, 0, dA, dB, dO, K);
            else hipLaunchKernelGGL(check16, dim3(1), dim3(64), 0, 0, dA, dB, dO, K);
            if (hipMemcpy(O.data(), dO, T * T * 4, hipMemcpyDeviceToHost) != hipSuccess) return false;
            int bad = 0;
            for (int m = 0; m < T; ++m) {
                double want = 0;
                for (int k = 0; k < K; ++k) want += (double)(float)A[m * K + k];
                for (int n = 0; n < T; ++n) bad += (double)O[m * T + n] != want;
            }
            printf("arith %s subnormals: %d of %d outputs differ from the exact sum%s\n", nm, bad, T * T, bad ? "  FAIL" : "");
            ok = ok && bad == 0;
        }
        // rounding of the accumulation
        struct RC { const char *name; int K; bool pos; };
        const RC rcs[] = {{"zero_mean_K768", 768, false}, {"positive_K768", 768, true}, {"positive_K2304", 2304, true}, {"zero_mean_K2304", 2304, false}};
        for (const RC &rc : rcs) {
            double se = 0, sa = 0, mx = 0;
            long cnt = 0;
            for (int rep = 0; rep < 16; ++rep) {
                for (int i = 0; i < 32 * rc.K; ++i) {
                    double a = (rnd() + rnd() + rnd() - 1.5) * 2.0, b = (rnd() + rnd() + rnd() - 1.5) * 0.04;
                    if (rc.pos) { a = std::fabs(a) + 1.0; b = std::fabs(b) + 0.01; }
                    A[i] = (_Float16)a;
                    B[i] = (_Float16)b;
                }
                (void)hipMemcpy(dA, A.data(), 32 * rc.K * 2, hipMemcpyHostToDevice);
                (void)hipMemcpy(dB, B.data(), 32 * rc.K * 2, hipMemcpyHostToDevice);
                if (shape == 0) hipLaunchKernelGGL(check32, dim3(1), dim3(64), 0, 0, dA, dB, dO, rc.K);
                else hipLaunchKernelGGL(check16, dim3(1), dim3(64), 0, 0, dA, dB, dO, rc.K);
                if (hipMemcpy(O.data(), dO, T * T * 4, hipMemcpyDeviceToHost) != hipSuccess) return false;
                for (int m = 0; m < T; ++m)
                    for (int n = 0; n < T; ++n) {
                        double ex = 0;
                        for (int k = 0; k < rc.K; ++k) ex += (double)(float)A[m * rc.K + k] * (double)(float)B[n * rc.K + k];
                        const double e = ((double)O[m * T + n] - ex) / ulp32(ex);
                        se += e * (ex < 0 ? -1.0 : 1.0);
                        sa += std::fabs(e);
                        mx = std::fmax(mx, std::fabs(e));
                        ++cnt;
                    }
            }
            const double ms = se / cnt;
            // RNE: |mean signed error| stays well below truncation's ~ -0.5 x steps x (partial / result) on positive chains
            const bool rne = std::fabs(ms) < 0.5;
            printf("arith %s %-16s mean signed err %+8.4f ulp  mean |err| %7.3f ulp  max |err| %7.2f ulp%s\n", nm, rc.name, ms, sa / cnt, mx,
                   rne ? "" : "  NOT RNE-LIKE");
            ok = ok && rne;
        }
    }
    hipFree(dA); hipFree(dB); hipFree(dO);
    return true;
}

int main(int argc, char **argv) {
    const double seconds = argc > 1 ? atof(argv[1]) : 4.0;
    const int alternations = argc > 2 ? atoi(argv[2]) : 2;
    bool ok = false;
    if (!arith_check(ok)) { printf("HIP error in the arithmetic check: %s\n", hipGetErrorString(hipGetLastError())); return 2; }
    printf("arith %s\n", ok ? "OK" : "FAILED");
    fflush(stdout);

    const int n_src = IMG_HALVES * 16;  // 1 MiB per source
    std::vector<_Float16> h(n_src);
    _Float16 *d_hi, *d_lo, *d_small;
    float *sink;
    if (hipMalloc(&d_hi, (size_t)n_src * 2) != hipSuccess || hipMalloc(&d_lo, (size_t)n_src * 2) != hipSuccess ||
        hipMalloc(&d_small, (size_t)n_src * 2) != hipSuccess || hipMalloc(&sink, 64) != hipSuccess) return 2;
    for (int kind = 0; kind < 3; ++kind) {
        for (int i = 0; i < n_src; ++i) {
            const double u = rnd() + rnd() + rnd() + rnd() - 2.0;  // ~N(0, 1/3)
            h[i] = (_Float16)(kind == 2 ? u * 0.00048828125 : u);
        }
        (void)hipMemcpy(kind == 0 ? d_hi : kind == 1 ? d_lo : d_small, h.data(), (size_t)n_src * 2, hipMemcpyHostToDevice);
    }
    {
        char bdf[64] = {0};
        if (hipDeviceGetPCIBusId(bdf, sizeof(bdf), 0) == hipSuccess) {
            g_pci = bdf;
            for (char &ch : g_pci) ch = (char)tolower(ch);
            if (hwmon_file("freq1_input").empty()) g_pci.clear();
        }
    }
    const std::string fp = hwmon_file("power1_input").empty() ? hwmon_file("power1_average") : hwmon_file("power1_input");
    const std::string fc = hwmon_file("freq1_input"), fcap = hwmon_file("power1_cap");
    printf("power cap %.0f W; sampling %s\n", read_num(fcap) / 1e6, fp.c_str());
    const size_t lds_bytes = IMG_HALVES * 2;
    (void)hipFuncSetAttribute(reinterpret_cast<const void *>(probe32<true>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_bytes);
    (void)hipFuncSetAttribute(reinterpret_cast<const void *>(probe16<true>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_bytes);
    struct Case { const char *name; bool lds; const _Float16 *lo; };
    const Case cases[] = {{"bare", false, d_lo}, {"lds", true, d_lo}, {"lds_pair", true, d_small}};
    const int iters = 2048, grid = 512;
    for (int alt = 0; alt < alternations; ++alt)
        for (const Case &c : cases)
            for (int shape = 0; shape < 2; ++shape) {
                std::atomic<bool> stop{false};
                std::vector<double> pw, ck;
                std::thread sampler([&]() {
                    while (!stop.load()) {
                        const double p = read_num(fp), f = read_num(fc);
                        if (p > 0) pw.push_back(p / 1e6);
                        if (f > 0) ck.push_back(f / 1e6);
                        std::this_thread::sleep_for(std::chrono::milliseconds(100));
                    }
                });
                auto launch = [&]() {
                    const size_t sh = c.lds ? lds_bytes : 0;
                    if (shape == 0) {
                        if (c.lds) hipLaunchKernelGGL(probe32<true>, dim3(grid), dim3(512), sh, 0, d_hi, c.lo, sink, iters);
                        else hipLaunchKernelGGL(probe32<false>, dim3(grid), dim3(512), sh, 0, d_hi, c.lo, sink, iters);
                    } else {
                        if (c.lds) hipLaunchKernelGGL(probe16<true>, dim3(grid), dim3(512), sh, 0, d_hi, c.lo, sink, iters);
                        else hipLaunchKernelGGL(probe16<false>, dim3(grid), dim3(512), sh, 0, d_hi, c.lo, sink, iters);
                    }
                };
                launch();
                (void)hipDeviceSynchronize();
                const auto t0 = std::chrono::steady_clock::now();
                long launches = 0;
                double el = 0;
                while (el < seconds) {
                    for (int r = 0; r < 4; ++r) launch();
                    if (hipDeviceSynchronize() != hipSuccess) { stop.store(true); sampler.join(); printf("HIP error\n"); return 3; }
                    launches += 4;
                    el = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
                }
                stop.store(true);
                sampler.join();
                auto mean_tail = [](const std::vector<double> &v) { size_t s0 = v.size() > 14 ? 10 : 0; double s = 0; for (size_t i = s0; i < v.size(); ++i) s += v[i]; return v.size() > s0 ? s / (v.size() - s0) : -1.0; };
                // 48 32x32x16 (or 96 16x16x32) per step per wave: 48 x 2 x 32 x 32 x 16 FLOP
                const double flops = (double)launches * grid * 8.0 * iters * 48.0 * 2.0 * 32 * 32 * 16;
                printf("alt %d  %-9s %-9s %8.1f TF  power %7.1f W  sclk %7.1f MHz  err=%s\n", alt, c.name, shape == 0 ? "32x32x16" : "16x16x32",
                       flops / el / 1e12, mean_tail(pw), mean_tail(ck), hipGetErrorString(hipGetLastError()));
                fflush(stdout);
            }
    return ok ? 0 : 1;
}
