// What does a 64-bit register copy cost on gfx950: one v_mov_b64 or two v_mov_b32?  The self-swap helpers of
// csrc/wave_common.h copy a double once per swap operand; this is the issue cost of those copies.
//   hipcc -O3 --offload-arch=gfx950 -o /tmp/ubench_mov64 tools/dev/ubench_mov64.hip && /tmp/ubench_mov64
// Independent copies (eight sources, eight destinations, no chain), 32 copies of 64 bits per trip.  Settings as in
// ubench_xchg.hip: one wave per SIMD; two per SIMD, the second doing the same; two per SIMD, the second running independent f64
// FMAs until the first is done (a counter in LDS, polled once per 32 of its instructions; the loop is bounded all the same).
#include <hip/hip_runtime.h>
#include <cstdio>

enum { MOV64 = 0, MOV32X2 = 1 };
enum { ALONE = 0, SAME = 1, VS_FMA = 2 };

template <int KIND>
__device__ __forceinline__ double run_mov(int n, double s) {
    double src[8], dst[8];
#pragma unroll
    for (int k = 0; k < 8; k++) { src[k] = s + k; dst[k] = 0.0; }
    for (int i = 0; i < n; i++) {
#pragma unroll
        for (int r = 0; r < 4; r++)
#pragma unroll
            for (int k = 0; k < 8; k++) {
                if constexpr (KIND == MOV64) {
                    asm volatile("v_mov_b64 %0, %1" : "=v"(dst[k]) : "v"(src[k]));
                } else {
                    int lo, hi;
                    asm volatile("v_mov_b32 %0, %2\n\tv_mov_b32 %1, %3" : "=&v"(lo), "=v"(hi) : "v"(__double2loint(src[k])), "v"(__double2hiint(src[k])));
                    dst[k] = __hiloint2double(hi, lo);
                }
            }
#pragma unroll
        for (int k = 0; k < 8; k++) asm volatile("" : "+v"(dst[k]));
    }
    double r = 0;
#pragma unroll
    for (int k = 0; k < 8; k++) r += dst[k];
    return r;
}
// the competitor: 32 instructions per trip, then a look at the counter
__device__ __forceinline__ double compete_fma(int nmax, double s, volatile int* done) {
    double c[8];
    for (int k = 0; k < 8; k++) c[k] = s + k;
    const double x = s * 0.5, y = s + 1.0;
    for (int i = 0; i < nmax && *done < 4; i++) {
#pragma unroll
        for (int k = 0; k < 32; k++) asm volatile("v_fmac_f64 %0, %1, %2" : "+v"(c[k & 7]) : "v"(x), "v"(y));
    }
    double r = 0;
    for (int k = 0; k < 8; k++) r += c[k];
    return r;
}

template <int KIND>
__global__ void __launch_bounds__(512) bench(int setting, int n, double* out, double s) {
    __shared__ int done;
    if (threadIdx.x == 0) done = 0;
    __syncthreads();
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    double r;
    if (wave < 4 || setting == SAME) {
        r = run_mov<KIND>(n, s);
        if (lane == 0) atomicAdd(&done, 1);
    } else {
        r = compete_fma(64 * n, s, &done);
    }
    if (r == 12345.678) out[threadIdx.x] = r;      // (threadIdx.x < 512: inside the 512 doubles of `out`)
}

template <int KIND>
static void run(const char* kind, double* out, hipEvent_t e0, hipEvent_t e1) {
    const int n = 20000, grid = 256;
    const char* settings[] = {"1 wave/SIMD", "2 waves/SIMD, same", "2 waves/SIMD, vs f64 FMA"};
    for (int setting = 0; setting < 3; setting++) {
        const int block = setting == ALONE ? 256 : 512;
        bench<KIND><<<grid, block>>>(setting, 100, out, 1.0);
        hipDeviceSynchronize();
        hipEventRecord(e0);
        bench<KIND><<<grid, block>>>(setting, n, out, 1.0);
        hipEventRecord(e1);
        hipEventSynchronize(e1);
        float ms;
        hipEventElapsedTime(&ms, e0, e1);
        // a trip is 32 copies of 64 bits per wave; with `same`, two waves share the SIMD: 64 per SIMD
        const double per = ms * 1e-3 * 2.4e9 / n / 32.0;
        printf("%-16s %-26s %8.3f ms  %6.2f cycles per 64-bit copy of one wave (2.4 GHz nominal)\n", kind, settings[setting], ms, per);
    }
}

int main() {
    double* out;
    if (hipMalloc(&out, 4096) != hipSuccess) { printf("no device\n"); return 1; }
    hipEvent_t e0, e1;
    hipEventCreate(&e0);
    hipEventCreate(&e1);
    run<MOV64>("v_mov_b64", out, e0, e1);
    run<MOV32X2>("v_mov_b32 x 2", out, e0, e1);
    printf("# 32 independent copies of 64 bits per trip (eight registers in turn), 20 000 trips, 256 workgroups of 4 or 8 waves\n");
    const hipError_t e = hipDeviceSynchronize();
    if (e != hipSuccess) { printf("error: %s\n", hipGetErrorString(e)); return 1; }
    return 0;
}
