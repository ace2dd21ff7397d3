// What does handing a double to the other 16-lane row of a 32-lane group cost on gfx950: v_permlane16_swap_b32 x 2 (VALU, no
// LDS), ds_swizzle_b32 x 2 or ds_bpermute_b32 x 2 (both through the LDS pipe, waited for with lgkmcnt)?
//   hipcc -O3 --offload-arch=gfx950 -o /tmp/ubench_xchg tools/dev/ubench_xchg.hip && /tmp/ubench_xchg
// Every exchange is followed by the add and the multiply of a reduction's last stage, v = (v + other row's v) / 2, the same in all
// kinds.  Two figures per kind: ISSUE, eight independent chains per wave (what an exchange costs when other work hides its
// latency), and LATENCY, one chain (what it costs on a dependent path).  Three settings: one wave per SIMD; two per SIMD, the
// second doing the same; two per SIMD, the second running independent f64 FMAs or LDS reads until the first is done (a counter in
// LDS, polled once per 32 of its instructions; the loop is bounded all the same).
#include <hip/hip_runtime.h>
#include <cstdio>

enum { SWAP = 0, SWIZZLE = 1, BPERMUTE = 2 };
enum { ALONE = 0, SAME = 1, VS_FMA = 2, VS_LDS = 3 };
constexpr int LDS_DOUBLES = 4096;

// v + the other row's v: for the swap that is [0] + [1] of the self-swap
template <int KIND>
__device__ __forceinline__ double pair_sum(double v, int baddr) {
    const int lo = __double2loint(v), hi = __double2hiint(v);
    if constexpr (KIND == SWAP) {
        auto a = __builtin_amdgcn_permlane16_swap(lo, lo, false, false);
        auto b = __builtin_amdgcn_permlane16_swap(hi, hi, false, false);
        return __hiloint2double(b[0], a[0]) + __hiloint2double(b[1], a[1]);
    } else if constexpr (KIND == SWIZZLE) {
        return v + __hiloint2double(__builtin_amdgcn_ds_swizzle(hi, 0x401F), __builtin_amdgcn_ds_swizzle(lo, 0x401F));
    } else {
        return v + __hiloint2double(__builtin_amdgcn_ds_bpermute(baddr, hi), __builtin_amdgcn_ds_bpermute(baddr, lo));
    }
}
template <int KIND, int CHAINS>
__device__ __forceinline__ double run_xchg(int n, double s, int baddr) {
    double c[CHAINS];
#pragma unroll
    for (int k = 0; k < CHAINS; k++) c[k] = s + k;
    for (int i = 0; i < n; i++) {
#pragma unroll
        for (int r = 0; r < 8 / CHAINS; r++)
#pragma unroll
            for (int k = 0; k < CHAINS; k++) {
                c[k] = pair_sum<KIND>(c[k], baddr) * 0.5;
                asm volatile("" : "+v"(c[k]));
            }
    }
    double r = 0;
#pragma unroll
    for (int k = 0; k < CHAINS; k++) r += c[k];
    return r;
}
// the competitors: 32 instructions per trip, then a look at the counter
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
__device__ __forceinline__ double compete_lds(int nmax, const double* buf, int lane, volatile int* done) {
    double c[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    for (int i = 0; i < nmax && *done < 4; i++) {
#pragma unroll
        for (int k = 0; k < 32; k++) c[k & 7] += buf[(lane + 64 * k + i) & (LDS_DOUBLES - 1)];   // (masked: inside buf)
    }
    double r = 0;
    for (int k = 0; k < 8; k++) r += c[k];
    return r;
}

template <int KIND, int CHAINS>
__global__ void __launch_bounds__(512) bench(int setting, int n, double* out, double s) {
    __shared__ double buf[LDS_DOUBLES];
    __shared__ int done;
    for (int i = threadIdx.x; i < LDS_DOUBLES; i += blockDim.x) buf[i] = s;
    if (threadIdx.x == 0) done = 0;
    __syncthreads();
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int baddr = 4 * (lane ^ 16);
    double r;
    if (wave < 4 || setting == SAME) {
        r = run_xchg<KIND, CHAINS>(n, s, baddr);
        if (lane == 0) atomicAdd(&done, 1);
    } else if (setting == VS_FMA) {
        r = compete_fma(64 * n, s, &done);
    } else {
        r = compete_lds(64 * n, buf, lane, &done);
    }
    if (r == 12345.678) out[threadIdx.x] = r;
}

template <int KIND, int CHAINS>
static void run(const char* kind, double* out, hipEvent_t e0, hipEvent_t e1) {
    const int n = 20000, grid = 256;
    const char* settings[] = {"1 wave/SIMD", "2 waves/SIMD, same", "2 waves/SIMD, vs f64 FMA", "2 waves/SIMD, vs LDS reads"};
    for (int setting = 0; setting < 4; setting++) {
        const int block = setting == ALONE ? 256 : 512;
        bench<KIND, CHAINS><<<grid, block>>>(setting, 100, out, 1.0);
        hipDeviceSynchronize();
        hipEventRecord(e0);
        bench<KIND, CHAINS><<<grid, block>>>(setting, n, out, 1.0);
        hipEventRecord(e1);
        hipEventSynchronize(e1);
        float ms;
        hipEventElapsedTime(&ms, e0, e1);
        // a trip is 8 exchanges per wave; with `same`, two waves share the SIMD: 16 per SIMD
        const double per = ms * 1e-3 * 2.4e9 / n / 8.0;
        printf("%-22s %-8s %-28s %8.3f ms  %6.1f cycles per exchange of one wave (2.4 GHz nominal)\n", kind,
               CHAINS == 8 ? "issue" : "latency", settings[setting], ms, per);
    }
}

int main() {
    double* out;
    if (hipMalloc(&out, 4096) != hipSuccess) { printf("no device\n"); return 1; }
    hipEvent_t e0, e1;
    hipEventCreate(&e0);
    hipEventCreate(&e1);
    run<SWAP, 8>("v_permlane16_swap x2", out, e0, e1);
    run<SWIZZLE, 8>("ds_swizzle x2", out, e0, e1);
    run<BPERMUTE, 8>("ds_bpermute x2", out, e0, e1);
    run<SWAP, 1>("v_permlane16_swap x2", out, e0, e1);
    run<SWIZZLE, 1>("ds_swizzle x2", out, e0, e1);
    run<BPERMUTE, 1>("ds_bpermute x2", out, e0, e1);
    printf("# an exchange = both halves of a double to the other 16-lane row, + v_add_f64 + v_mul_f64; issue: 8 independent chains, "
           "latency: 1 chain\n");
    const hipError_t e = hipDeviceSynchronize();
    if (e != hipSuccess) { printf("error: %s\n", hipGetErrorString(e)); return 1; }
    return 0;
}
