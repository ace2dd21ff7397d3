// What do nine v_mfma_f64_4x4x4_4b_f64 cost against three v_mfma_f64_16x16x4_f64 on gfx950, and which lane holds what?
//   hipcc -O3 --offload-arch=gfx950 -o /tmp/ubench_mfma4 tools/dev/ubench_mfma4.hip && /tmp/ubench_mfma4
// Same layout as ubench_overlap.hip: one workgroup of 8 waves per CU (two per SIMD: waves w and w + 4 share SIMD w % 4).
// A loop trip is what one k-step of the (32, .) Gram product issues: three 16x16x4 (the lower block triangle) or nine 4x4x4
// (the 36 lower 4x4 tiles, four per instruction), on nine accumulators round-robin (a dependent 4x4x4 accumulate needs 4 wait
// states).  Modes: 0 all waves 16x16x4; 1 all waves 4x4x4; 2 waves 0-3 16x16x4, waves 4-7 f64 FMAs; 3 waves 0-3 4x4x4, waves
// 4-7 f64 FMAs; 4 all waves f64 FMAs; 5/6: modes 0/1 with ONE wave per SIMD (256 threads).
// Times are device events over the whole grid and, per kind of wave, s_memtime ticks of block 0 (clock independent ratio).
// Then the lane map of the 4x4x4 form: A one-hot in lane la, B = lane + 1 in every lane; the lanes of D that come back non-zero
// share la's (block, row), and their value names the B lane of the same (block, k).
#include <hip/hip_runtime.h>
#include <cstdio>
#include <cstdlib>
typedef double double4_t __attribute__((ext_vector_type(4)));

__device__ __forceinline__ double run_mfma16(int n, double s) {
    double4_t a0 = {s, s, s, s}, a1 = a0, a2 = a0;
    double x = s, y = s + 1.0;
    for (int i = 0; i < n; i++) {
        a0 = __builtin_amdgcn_mfma_f64_16x16x4f64(x, y, a0, 0, 0, 0);
        a1 = __builtin_amdgcn_mfma_f64_16x16x4f64(x, y, a1, 0, 0, 0);
        a2 = __builtin_amdgcn_mfma_f64_16x16x4f64(x, y, a2, 0, 0, 0);
    }
    return a0[0] + a1[1] + a2[2];
}
__device__ __forceinline__ double run_mfma4(int n, double s) {
    double c[9];
    for (int k = 0; k < 9; k++) c[k] = s + k;
    double x = s, y = s + 1.0;
    for (int i = 0; i < n; i++) {
#pragma unroll
        for (int k = 0; k < 9; k++) c[k] = __builtin_amdgcn_mfma_f64_4x4x4f64(x, y, c[k], 0, 0, 0);
    }
    double r = 0; for (int k = 0; k < 9; k++) r += c[k];
    return r;
}
__device__ __forceinline__ double run_fma(int n, double s) {
    double c[8];
    for (int k = 0; k < 8; k++) c[k] = s + k;
    double x = s * 0.5, y = s + 1.0;
    for (int i = 0; i < n; i++) {
#pragma unroll
        for (int k = 0; k < 8; k++) asm volatile("v_fmac_f64 %0, %1, %2" : "+v"(c[k]) : "v"(x), "v"(y));
    }
    double r = 0; for (int k = 0; k < 8; k++) r += c[k];
    return r;
}

__global__ void __launch_bounds__(512) bench(int mode, int n, double* out, long long* ticks, double s) {
    const int wave = threadIdx.x >> 6;
    const bool first = wave < 4;
    const long long t0 = __builtin_readcyclecounter();
    double r = 0;
    switch (mode) {
        case 0: case 5: r = run_mfma16(n, s); break;                        // 3 n MFMAs per wave
        case 1: case 6: r = run_mfma4(n, s); break;                         // 9 n MFMAs per wave
        case 2: r = first ? run_mfma16(n, s) : run_fma(n, s); break;        // FMA waves: 8 n FMAs
        case 3: r = first ? run_mfma4(n, s) : run_fma(n, s); break;
        case 4: r = run_fma(n, s); break;
    }
    const long long t1 = __builtin_readcyclecounter();
    if (blockIdx.x == 0 && (threadIdx.x & 63) == 0) ticks[wave] = t1 - t0;
    if (r == 12345.678) out[threadIdx.x] = r;
}

__global__ void __launch_bounds__(64) lanemap(double* out) {
    const int lane = threadIdx.x;
    for (int la = 0; la < 64; la++) {
        const double a = (lane == la) ? 1.0 : 0.0, b = (double)(lane + 1);
        out[la * 64 + lane] = __builtin_amdgcn_mfma_f64_4x4x4f64(a, b, 0.0, 0, 0, 0);
    }
}

#define CK(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) { printf("HIP error %s at line %d\n", hipGetErrorString(e_), __LINE__); return 1; } } while (0)

int main() {
    double* out; CK(hipMalloc(&out, 64 * 64 * sizeof(double)));
    long long* ticks; CK(hipMalloc(&ticks, 8 * sizeof(long long)));
    hipEvent_t e0, e1; CK(hipEventCreate(&e0)); CK(hipEventCreate(&e1));
    const int n = 20000, grid = 256;
    const char* names[] = {"all 3x 16x16x4", "all 9x 4x4x4", "3x 16x16x4 | 8 f64 FMA", "9x 4x4x4 | 8 f64 FMA", "all 8 f64 FMA",
                           "3x 16x16x4, 1 wave/SIMD", "9x 4x4x4, 1 wave/SIMD"};
    printf("# a loop trip per wave = three 16x16x4, nine 4x4x4 or eight f64 FMAs; %d trips; %d workgroups\n", n, grid);
    printf("# ticks: s_memtime of block 0, waves 0 and 4 (the two kinds in the mixed modes), per loop trip\n");
    for (int rep = 0; rep < 2; rep++)
        for (int mode = 0; mode < 7; mode++) {
            const int threads = mode >= 5 ? 256 : 512;
            CK(hipMemset(ticks, 0, 8 * sizeof(long long)));
            bench<<<grid, threads>>>(mode, 100, out, ticks, 1.0);
            CK(hipDeviceSynchronize());
            CK(hipEventRecord(e0));
            bench<<<grid, threads>>>(mode, n, out, ticks, 1.0);
            CK(hipEventRecord(e1)); CK(hipEventSynchronize(e1));
            float ms; CK(hipEventElapsedTime(&ms, e0, e1));
            long long t[8]; CK(hipMemcpy(t, ticks, sizeof(t), hipMemcpyDeviceToHost));
            printf("mode %d %-26s %8.3f ms  %7.1f ns per trip   ticks per trip: wave0 %.1f  wave4 %.1f\n", mode, names[mode], ms,
                   ms * 1e6 / n, (double)t[0] / n, threads == 512 ? (double)t[4] / n : 0.0);
        }

    // lane map
    lanemap<<<1, 64>>>(out);
    CK(hipDeviceSynchronize());
    static double h[64 * 64];
    CK(hipMemcpy(h, out, sizeof(h), hipMemcpyDeviceToHost));
    printf("# lane map of v_mfma_f64_4x4x4_4b_f64: A one-hot in lane la, B[lane] = lane + 1\n");
    printf("# la : D lane <- B lane (the four non-zero results)\n");
    bool hyp = true;
    for (int la = 0; la < 64; la++) {
        printf("%2d :", la);
        int cnt = 0;
        for (int l = 0; l < 64; l++) {
            const double v = h[la * 64 + l];
            if (v == 0.0) continue;
            const int lb = (int)v - 1;
            printf("  D%-2d<-B%-2d", l, lb);
            cnt++;
            // hypothesis: A/B lane = 16 k + 4 block + i (or j); D lane = 16 i + 4 block + j
            const int i = la & 3, blk = (la >> 2) & 3, k = la >> 4, j = l & 3;
            if (l != 16 * i + 4 * blk + j || lb != 16 * k + 4 * blk + j) hyp = false;
        }
        if (cnt != 4) hyp = false;
        printf("\n");
    }
    printf("# A[i][k] in lane 16 k + 4 block + i, B[k][j] in lane 16 k + 4 block + j, D[i][j] in lane 16 i + 4 block + j: %s\n",
           hyp ? "CONFIRMED" : "NOT what the hardware does");
    return 0;
}
