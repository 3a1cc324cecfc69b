// What does the SHAPE of a wave's 16-byte stores cost?  256 workgroups x 256 threads, one per CU (96 KB of LDS each keeps
// a second one off the CU), each writes one 64x64 fp32 tile of a 1024x1024 matrix with global_store_dwordx4 ... sc1 (the
// library's store_stream), four instructions per lane, in one of four shapes per wave-instruction:
//   a  the weight-gradient epilogue of rounds 1-9, straight out of the MFMA layout: 16 rows x four 16-byte pieces 32
//      bytes apart, the holes filled by a second instruction
//   b  16 rows x 64 contiguous bytes          c  8 rows x 128 contiguous bytes          d  4 rows x 256 contiguous bytes
// The tile -> workgroup mapping is wgrad_reg_body's (an XCD owns two tile columns).  Timed as the period of back-to-back
// launches above that of an empty kernel of the same grid and LDS; `reps` such sessions give the run-to-run spread.
// `tiles` > 1 writes that many matrices per launch (the same tile of each) to lift the stores above the launch floor.
//   hipcc --offload-arch=gfx950 -O3 -std=c++17 tools/store_shape_probe.hip -o ab_libs/store_shape_probe
//   ab_libs/store_shape_probe [reps = 7] [iters = 300]          timing table
//   rocprofv3 --pmc WRITE_SIZE ... -- ab_libs/store_shape_probe 1 4      (few launches per arm: bytes per launch by kernel name)
#include <hip/hip_runtime.h>
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <vector>
#include "../physicsvae_amd/csrc/pvae_gemm_common.h"
using namespace pvae;
#define CK(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) { printf("%s: %s\n", #x, hipGetErrorString(e_)); return 1; } } while (0)

constexpr int kN = 1024, kLds = 96 * 1024;

// ARM: 0 = a, 1 = b, 2 = c, 3 = d, -1 = no stores
template <int ARM>
__global__ void __launch_bounds__(256) store_shape_kernel(float* __restrict__ G, int tiles) {
    extern __shared__ float lds[];
    const int bid = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int xcd = bid & 7, loc = bid >> 3;
    const int q0 = (loc % 16) * 64, p0 = (xcd * 2 + loc / 16) * 64;
    v4f v = v4f{1.f, 2.f, 3.f, 4.f} * (float)(tid + 1);
    asm volatile("" : "+v"(v));
    if (ARM < 0) {
        if (tiles < 0) lds[tid] = v[0];          // (never: the kernel keeps its LDS allocation and its operands)
        return;
    }
    for (int m = 0; m < tiles; ++m) {
        float* g = G + (size_t)m * kN * kN + (size_t)q0 * kN + p0;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            int r, c;
            if (ARM == 0) {
                const int li = lane & 15, lh = lane >> 4;
                r = (wave >> 1) * 32 + 2 * li + (j >> 1);
                c = (wave & 1) * 32 + 8 * lh + 4 * (j & 1);
            } else if (ARM == 1) {
                r = 16 * wave + (lane >> 2);
                c = 16 * j + 4 * (lane & 3);
            } else if (ARM == 2) {
                r = 16 * wave + 8 * (j >> 1) + (lane >> 3);
                c = 32 * (j & 1) + 4 * (lane & 7);
            } else {
                r = 16 * wave + 4 * j + (lane >> 4);
                c = 4 * (lane & 15);
            }
            store_stream(g + (size_t)r * kN + c, v);
        }
    }
}

template <int ARM>
static float period_us(hipStream_t st, float* G, int tiles, int iters, hipEvent_t a, hipEvent_t b) {
    auto launch = [&]() { hipLaunchKernelGGL((store_shape_kernel<ARM>), dim3(256), dim3(256), kLds, st, G, tiles); };
    for (int i = 0; i < 20; ++i) launch();
    hipStreamSynchronize(st);
    hipEventRecord(a, st);
    for (int i = 0; i < iters; ++i) launch();
    hipEventRecord(b, st);
    hipEventSynchronize(b);
    float ms = 0;
    hipEventElapsedTime(&ms, a, b);
    return ms * 1e3f / iters;
}

template <int ARM>
static int check(hipStream_t st, float* G, std::vector<float>& h) {
    // every element of the matrix written exactly as thread (tid + 1) x {1, 2, 3, 4} says: the shapes cover the tile
    CK(hipMemsetAsync(G, 0xff, (size_t)kN * kN * 4, st));
    hipLaunchKernelGGL((store_shape_kernel<ARM>), dim3(256), dim3(256), kLds, st, G, 1);
    CK(hipMemcpyAsync(h.data(), G, (size_t)kN * kN * 4, hipMemcpyDeviceToHost, st));
    CK(hipStreamSynchronize(st));
    size_t bad = 0;
    for (size_t i = 0; i < h.size(); ++i) {
        const float x = h[i] / (float)((i & 3) + 1);
        bad += !(x >= 1.f && x <= 256.f && x == (float)(int)x);
    }
    if (bad) { printf("arm %d leaves %zu elements unwritten or wrong\n", ARM, bad); return 1; }
    return 0;
}

int main(int argc, char** argv) {
    const int reps = argc > 1 ? std::max(1, atoi(argv[1])) : 7, iters = argc > 2 ? std::max(1, atoi(argv[2])) : 300;
    constexpr int kTilesMax = 8;
    hipStream_t st; CK(hipStreamCreate(&st));
    float* G; CK(hipMalloc(&G, (size_t)kTilesMax * kN * kN * 4));
    CK(hipFuncSetAttribute((const void*)store_shape_kernel<-1>, hipFuncAttributeMaxDynamicSharedMemorySize, kLds));
    CK(hipFuncSetAttribute((const void*)store_shape_kernel<0>, hipFuncAttributeMaxDynamicSharedMemorySize, kLds));
    CK(hipFuncSetAttribute((const void*)store_shape_kernel<1>, hipFuncAttributeMaxDynamicSharedMemorySize, kLds));
    CK(hipFuncSetAttribute((const void*)store_shape_kernel<2>, hipFuncAttributeMaxDynamicSharedMemorySize, kLds));
    CK(hipFuncSetAttribute((const void*)store_shape_kernel<3>, hipFuncAttributeMaxDynamicSharedMemorySize, kLds));
    hipEvent_t a, b; CK(hipEventCreate(&a)); CK(hipEventCreate(&b));
    std::vector<float> h((size_t)kN * kN);
    if (check<0>(st, G, h) || check<1>(st, G, h) || check<2>(st, G, h) || check<3>(st, G, h)) return 1;
    CK(hipGetLastError());

    const char* names[5] = {"empty (no stores)", "a: 16 rows x 4 x 16 B, 32 B apart (epilogue of rounds 1-9)", "b: 16 rows x 64 B",
                            "c: 8 rows x 128 B", "d: 4 rows x 256 B"};
    for (int tiles : {1, kTilesMax}) {
        std::vector<float> t[5];
        for (int r = 0; r < reps; ++r) {                       // arms interleaved inside a session
            t[0].push_back(period_us<-1>(st, G, tiles, iters, a, b));
            t[1].push_back(period_us<0>(st, G, tiles, iters, a, b));
            t[2].push_back(period_us<1>(st, G, tiles, iters, a, b));
            t[3].push_back(period_us<2>(st, G, tiles, iters, a, b));
            t[4].push_back(period_us<3>(st, G, tiles, iters, a, b));
        }
        CK(hipGetLastError());
        printf("%d x 64x64 fp32 tile(s) per workgroup = %d MB per launch; period of back-to-back launches, us (%d sessions of %d launches)\n",
               tiles, tiles * 4, reps, iters);
        printf("  %-60s %7s %7s %7s %7s   %s\n", "arm", "min", "median", "max", "spread", "median above empty");
        float med0 = 0;
        for (int k = 0; k < 5; ++k) {
            std::sort(t[k].begin(), t[k].end());
            const float med = t[k][t[k].size() / 2];
            if (k == 0) med0 = med;
            printf("  %-60s %7.2f %7.2f %7.2f %7.2f   %6.2f", names[k], t[k].front(), med, t[k].back(), t[k].back() - t[k].front(), med - med0);
            if (k) printf("  (%.2f TB/s)", tiles * 4.194304f / (med - med0) );
            printf("\n");
        }
    }
    return 0;
}
