// Back-to-back launch period of the 16x16 register-staged kernel (gemm_splitk_reg16_kernel) at the shapes the joint step
// sends to it, through the library's own launchers (gemm_forward / gemm_dgrad choose the 16x16 geometry below 128 tiles
// of 32x32), on RANDOM operands, timed in C++ with HIP events: tools/gemm_bench.py launches from Python, whose ~8 us per
// call hides a 5-7 us kernel.  Rows: 256.  P_ROW (forward, bias + ReLU): 64 and 208 outputs, K = 1024 (the action and
// state output layers); P_COL (input gradient with mask): 64 outputs, contraction 1024 (the EpiActionSeed launch's shape).
//   hipcc --offload-arch=gfx950 -O3 -std=c++17 -mllvm -amdgpu-kernarg-preload-count=16 tools/reg16_lab.hip -o ab_libs/reg16_lab
#include <hip/hip_runtime.h>
#include <cstdio>
#include "../physicsvae_amd/csrc/pvae_gemm.h"
using namespace pvae;
#define CK(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) { printf("%s: %s\n", #x, hipGetErrorString(e_)); return 1; } } while (0)

__global__ void fill_kernel(float* p, size_t n, unsigned seed) {
    for (size_t i = blockIdx.x * 256ull + threadIdx.x; i < n; i += gridDim.x * 256ull) {
        unsigned x = (unsigned)i * 2654435761u + seed;
        x ^= x >> 15; x *= 2246822519u; x ^= x >> 13;
        p[i] = ((int)(x & 0xffff) - 32768) * (1.0f / 32768.0f);
    }
}
__global__ void empty_kernel(int) {}

template <class F>
static float period_us(hipStream_t st, hipEvent_t a, hipEvent_t b, F launch) {
    const int iters = 400;
    for (int i = 0; i < 40; ++i) launch();
    (void)hipStreamSynchronize(st);
    (void)hipEventRecord(a, st);
    for (int i = 0; i < iters; ++i) launch();
    (void)hipEventRecord(b, st);
    (void)hipEventSynchronize(b);
    float ms = 0;
    (void)hipEventElapsedTime(&ms, a, b);
    return ms * 1e3f / iters;
}

int main() {
    const int M = 256, K = 1024, NMAX = 256;
    hipStream_t st; CK(hipStreamCreate(&st));
    float *X, *W, *bias, *out, *dZ, *Wd, *act, *dX;
    CK(hipMalloc(&X, (size_t)M * K * 4)); CK(hipMalloc(&W, (size_t)NMAX * K * 4)); CK(hipMalloc(&bias, NMAX * 4));
    CK(hipMalloc(&out, (size_t)M * NMAX * 4)); CK(hipMalloc(&dZ, (size_t)M * K * 4)); CK(hipMalloc(&Wd, (size_t)K * NMAX * 4));
    CK(hipMalloc(&act, (size_t)M * NMAX * 4)); CK(hipMalloc(&dX, (size_t)M * NMAX * 4));
    float* bufs[] = {X, W, bias, dZ, Wd, act};
    const size_t lens[] = {(size_t)M * K, (size_t)NMAX * K, NMAX, (size_t)M * K, (size_t)K * NMAX, (size_t)M * NMAX};
    for (int i = 0; i < 6; ++i) hipLaunchKernelGGL(fill_kernel, dim3(256), dim3(256), 0, st, bufs[i], lens[i], 23u * (i + 1));
    CK(hipStreamSynchronize(st));
    hipEvent_t a, b; CK(hipEventCreate(&a)); CK(hipEventCreate(&b));
    printf("empty 256-workgroup kernel, back to back:                 %6.2f us\n",
           period_us(st, a, b, [&]() { hipLaunchKernelGGL(empty_kernel, dim3(256), dim3(256), 0, st, 0); }));
    for (int rep = 0; rep < 3; ++rep) {
        for (int n : {64, 208})
            printf("P_ROW 256 x %3d x 1024 (forward, bias + ReLU), %3d workgroups: %6.2f us\n", n, (M / 16) * (n / 16),
                   period_us(st, a, b, [&]() { (void)gemm_forward(X, K, W, K, bias, out, n, M, n, K, 1, st); }));
        printf("P_COL 256 x  64 x 1024 (input gradient, mask), %3d workgroups: %6.2f us\n", (M / 16) * (64 / 16),
               period_us(st, a, b, [&]() { (void)gemm_dgrad(dZ, K, Wd, 64, act, 64, dX, 64, M, 64, K, st); }));
    }
    CK(hipGetLastError());
    CK(hipStreamSynchronize(st));
    return 0;
}
