// general_form.hip -- a batch of GeneralLPs (a <= A x <= b, l <= x <= u, shared A) to and from the bounded equality form
// ([+-A | I] x^ = b^, 0 <= x^ <= u^) on the device: pycllp_hip_general_to_bounded and pycllp_hip_general_from_bounded
// (include/pycllp_hip.h).  The arithmetic is GeneralLP.to_bounded_equality_form's and BoundedMap.general's
// (pycllp_amd/lp.py) operation for operation -- separately rounded products and sums, no contraction -- so b^, c^, u^ and
// x, y, z, s carry the host's bits.
//
// Both kernels are memory bound and work on TILES of G consecutive LPs per workgroup: the arrays of a tile are contiguous in
// the caller's memory ([G n] of c, l, u; [G m] of a, b; [G N] of c^, u^ ...), so every element-wise pass runs coalesced over a
// flat 32-bit index and a short row (7 ... 1 280 doubles) never leaves lanes idle.  A caller's array is touched through
// 8-byte (double) and 4-byte (int) accesses only, from element 0 to the last element of its shape.
#include <hip/hip_runtime.h>
#include <math.h>
#include "../../include/pycllp_hip.h"
#include "host_error.h"

// The host rounds every product and every sum on its own.  hipcc's default (-ffp-contract=fast) fuses a product into the sum
// that takes it, also through __dmul_rn / __dadd_rn (inline * and + of the HIP headers, which a pragma here does not reach): the
// Makefile compiles this unit with -ffp-contract=off, and the pragma says the same for the code of this file.
#pragma clang fp contract(off)

namespace {

constexpr int kThreads = 256;
constexpr int kMaxRows = 256, kMaxCols = 1280;       // the bounded forms the solve kernels take: m <= 256, n + mk <= 1280
constexpr int kValid = 99;                           // "no check failed" in the per-LP minimum over the codes 1 .. 5
constexpr size_t kTileBytes = 24 * 1024;             // LDS of to_bounded's tile: six workgroups per CU (the A l sums wait on loads)
constexpr long kMaxGrid = 1L << 20;

struct ToBounded {
    int m, n, mk, G;
    long B;
    const int* rowmap;
    const double* Adata;
    const int* Aindptr;
    const int* Aindices;
    const double *a, *b, *c, *l, *u, *f;
    double *bh, *ch, *uh, *fh;
    int* invalid;
};

struct FromBounded {
    int m, n, mk, G;
    long B;
    const int* rowmap;
    const double *l, *fh;
    const int* invalid;
    const double *xh, *yh, *zh, *sh;
    double *x, *y, *z, *s, *pobj, *dobj;
    int *status, *iters;
};

__device__ __forceinline__ bool finite64(double v) { return fabs(v) < INFINITY; }      // false for NaN

// The tile in LDS: lt [G][n|1] the lower bounds l (0 where l_dev is NULL); at, bt [G][m|1] the row bounds a, b on the way in
// and b^ (by ORIGINAL row) and the slack's u^ on the way out -- the odd strides keep the lanes of a wavefront, which walk one
// row of A for consecutive LPs, on different banks; rs [m] the row sums of A^ (only where a tile holds an invalid LP);
// keep [mk] the original row of each kept row, rm [m] the row map, bad [G] the smallest failing check of each LP.
__global__ __launch_bounds__(kThreads) void general_to_bounded_kernel(const ToBounded p) {
    extern __shared__ __attribute__((aligned(16))) double tile[];
    const int m = p.m, n = p.n, mk = p.mk, N = n + mk, G = p.G, ls = n | 1, ms = m | 1, tid = threadIdx.x;
    double* lt = tile;
    double* at = lt + (size_t)G * ls;
    double* bt = at + (size_t)G * ms;
    double* rs = bt + (size_t)G * ms;
    int* keep = (int*)(rs + m);
    int* rm = keep + m;
    int* bad = rm + m;
    int* anybad = bad + G;
    for (int i = tid; i < m; i += kThreads) {
        const int r = p.rowmap[i];
        rm[i] = r;
        if (r != 0) keep[(r > 0 ? r : -r) - 1] = i;
    }
    const long tiles = (p.B + G - 1) / G;
    for (long t = blockIdx.x; t < tiles; t += gridDim.x) {
        const long lp0 = t * G;
        const int ga = (int)(p.B - lp0 < G ? p.B - lp0 : G);            // LPs of this tile
        if (tid < ga) bad[tid] = kValid;
        if (tid == 0) *anybad = 0;
        __syncthreads();
        // -- in: c, l, u checked (codes 1, 2, 5) and l kept; a, b kept; f checked (5)
        {
            const double* c = p.c + lp0 * n;
            const double* u = p.u + lp0 * n;
            const double* l = p.l ? p.l + lp0 * n : nullptr;
            for (unsigned e = tid; e < (unsigned)(ga * n); e += kThreads) {
                const unsigned g = e / (unsigned)n, j = e - g * n;
                const double lv = l ? l[e] : 0.0, uv = u[e], cv = c[e];
                int code = kValid;
                if (!finite64(cv)) code = 5;
                if (uv < lv) code = 2;
                if (!finite64(lv)) code = 1;
                if (code != kValid) { atomicMin(&bad[g], code); *anybad = 1; }
                lt[g * ls + j] = lv;
            }
            const double* a = p.a + lp0 * m;
            const double* b = p.b + lp0 * m;
            for (unsigned e = tid; e < (unsigned)(ga * m); e += kThreads) {
                const unsigned g = e / (unsigned)m, i = e - g * m;
                at[g * ms + i] = a[e];
                bt[g * ms + i] = b[e];
            }
            if (tid < ga && p.f && !finite64(p.f[lp0 + tid])) { atomicMin(&bad[tid], 5); *anybad = 1; }
        }
        __syncthreads();
        // -- one (LP, row) per thread, the LP index fastest: the lanes of a wavefront share the row's terms
        for (unsigned w = tid; w < (unsigned)(ga * m); w += kThreads) {
            const unsigned i = w / (unsigned)ga, g = w - i * ga;
            const int r = rm[i];
            const double av = at[g * ms + i], bv = bt[g * ms + i];
            const bool af = finite64(av), bf = finite64(bv);
            int code = kValid;
            if (r > 0 ? !bf : r < 0 ? !(bv == INFINITY && af) : (af || bf)) code = 4;
            if (af && av > bv) code = 3;
            if (code != kValid) { atomicMin(&bad[g], code); *anybad = 1; }
            if (r == 0) continue;
            double al = 0.0;
            const double* lg = lt + g * ls;
#pragma unroll 4                                                        // (the loads of four terms in flight; the sum stays in order)
            for (int q = p.Aindptr[i], q1 = p.Aindptr[i + 1]; q < q1; q++)
                al = __dadd_rn(al, __dmul_rn(p.Adata[q], lg[p.Aindices[q]]));
            const double bh = __dsub_rn(bv, al), ah = __dsub_rn(av, al);
            at[g * ms + i] = r > 0 ? bh : -ah;
            bt[g * ms + i] = (r > 0 && finite64(ah)) ? __dsub_rn(bh, ah) : INFINITY;
        }
        __syncthreads();
        if (*anybad) {                                                  // (one answer for the whole workgroup)
            for (int i = tid; i < m; i += kThreads) {
                const int r = rm[i];
                if (r == 0) continue;
                double sum = 0.0;
                for (int q = p.Aindptr[i], q1 = p.Aindptr[i + 1]; q < q1; q++) sum = __dadd_rn(sum, r > 0 ? p.Adata[q] : -p.Adata[q]);
                rs[i] = __dadd_rn(sum, 1.0);
            }
            __syncthreads();
        }
        // -- out: b^ [ga mk], c^ and u^ [ga N], f^ and invalid [ga]
        {
            double* bh = p.bh + lp0 * mk;
            for (unsigned e = tid; e < (unsigned)(ga * mk); e += kThreads) {
                const unsigned g = e / (unsigned)mk, k = e - g * mk;
                const int i = keep[k];
                bh[e] = bad[g] == kValid ? at[g * ms + i] : rs[i];
            }
            double* ch = p.ch + lp0 * N;
            double* uh = p.uh + lp0 * N;
            const double* c = p.c + lp0 * n;
            const double* u = p.u + lp0 * n;
            for (unsigned e = tid; e < (unsigned)(ga * N); e += kThreads) {
                const unsigned g = e / (unsigned)N, q = e - g * N;
                double cv = 0.0, uv = INFINITY;
                if (bad[g] == kValid) {
                    if (q < (unsigned)n) {
                        cv = c[g * n + q];
                        const double u0 = u[g * n + q];
                        if (finite64(u0)) uv = __dsub_rn(u0, lt[g * ls + q]);
                    } else {
                        uv = bt[g * ms + keep[q - n]];
                    }
                }
                ch[e] = cv;
                uh[e] = uv;
            }
            // f^ = f + c'l: one wavefront per LP, lane partial sums then a butterfly (any order will do: the host's is pairwise)
            const int lane = tid & 63;
            for (int g = tid >> 6; g < ga; g += kThreads >> 6) {
                double sum = 0.0;
                if (bad[g] == kValid) {
                    for (int j = lane; j < n; j += 64) sum = __dadd_rn(sum, __dmul_rn(c[(size_t)g * n + j], lt[g * ls + j]));
                    for (int d = 32; d > 0; d >>= 1) sum = __dadd_rn(sum, __shfl_xor(sum, d, 64));
                }
                if (lane == 0) {
                    const bool ok = bad[g] == kValid;
                    p.fh[lp0 + g] = ok ? __dadd_rn(p.f ? p.f[lp0 + g] : 0.0, sum) : 0.0;
                    p.invalid[lp0 + g] = ok ? 0 : bad[g];
                }
            }
        }
        __syncthreads();                                                // (the next tile overwrites lt, at, bt and bad)
    }
}

// Element-wise over a tile of G LPs: x = l + x^ [G n], z, s; y by the row map [G m]; the objectives, and what an invalid LP gets.
__global__ __launch_bounds__(kThreads) void general_from_bounded_kernel(const FromBounded p) {
    const int m = p.m, n = p.n, mk = p.mk, N = n + mk, G = p.G, tid = threadIdx.x;
    const double qnan = __longlong_as_double(0x7FF8000000000000LL);
    const long tiles = (p.B + G - 1) / G;
    for (long t = blockIdx.x; t < tiles; t += gridDim.x) {
        const long lp0 = t * G;
        const int ga = (int)(p.B - lp0 < G ? p.B - lp0 : G);
        const int* inv = p.invalid + lp0;
        {
            const double* l = p.l ? p.l + lp0 * n : nullptr;
            const double* xh = p.xh + lp0 * N;
            const double* zh = p.zh ? p.zh + lp0 * N : nullptr;
            const double* sh = p.sh ? p.sh + lp0 * N : nullptr;
            double* x = p.x + lp0 * n;
            double* z = p.z ? p.z + lp0 * n : nullptr;
            double* s = p.s ? p.s + lp0 * n : nullptr;
            for (unsigned e = tid; e < (unsigned)(ga * n); e += kThreads) {
                const unsigned g = e / (unsigned)n, j = e - g * n;
                const bool ok = inv[g] == 0;
                const size_t src = (size_t)g * N + j;
                x[e] = ok ? __dadd_rn(l ? l[e] : 0.0, xh[src]) : qnan;
                if (z) z[e] = ok ? zh[src] : qnan;
                if (s) s[e] = ok ? sh[src] : qnan;
            }
        }
        {
            const double* yh = p.yh + lp0 * mk;
            double* y = p.y + lp0 * m;
            for (unsigned e = tid; e < (unsigned)(ga * m); e += kThreads) {
                const unsigned g = e / (unsigned)m, i = e - g * m;
                const int r = p.rowmap[i];
                double v = 0.0;
                if (inv[g] != 0) v = qnan;
                else if (r > 0) v = yh[(size_t)g * mk + (r - 1)];
                else if (r < 0) v = -yh[(size_t)g * mk + (-r - 1)];
                y[e] = v;
            }
        }
        for (int g = tid; g < ga; g += kThreads) {
            const long lp = lp0 + g;
            const bool ok = inv[g] == 0;
            const double f = p.fh[lp];
            if (p.pobj) p.pobj[lp] = ok ? __dadd_rn(p.pobj[lp], f) : qnan;
            if (p.dobj) p.dobj[lp] = ok ? __dadd_rn(p.dobj[lp], f) : qnan;
            if (!ok) {
                p.status[lp] = PYCLLP_STATUS_NUMERICAL;
                if (p.iters) p.iters[lp] = 0;
            }
        }
    }
}

// PYCLLP_E_BADARG / PYCLLP_E_UNSUPPORTED for the sizes both entries take, 0 where they pass
int check_sizes(const char* entry, int m, int n, int mk, long B) {
    if (m < 1 || n < 1 || mk < 1 || mk > m || B < 0) return pycllp_entry_error(PYCLLP_E_BADARG, entry, "bad argument");
    if (m > kMaxRows || (long)n + mk > kMaxCols)
        return pycllp_entry_error(PYCLLP_E_UNSUPPORTED, entry, "beyond the bounded forms the solve kernels take (m <= 256, n + mk <= 1280)");
    return 0;
}

int launched(const char* what) {
    const hipError_t e = hipGetLastError();
    return e == hipSuccess ? 0 : pycllp_runtime_error((int)e, what);
}

}   // namespace

extern "C" {

int pycllp_hip_general_to_bounded(int m, int n, int mk, long B, const int* rowmap_dev, int nnz, const double* Adata_dev,
                                  const int* Aindptr_dev, const int* Aindices_dev, const double* a_dev, const double* b_dev,
                                  const double* c_dev, const double* l_dev, const double* u_dev, const double* f_dev,
                                  double* bh_dev, double* ch_dev, double* uh_dev, double* fh_dev, int* invalid_dev, void* stream) {
    static const char* entry = "pycllp_hip_general_to_bounded";
    // (order: everything PYCLLP_E_BADARG covers, then the sizes beyond the kernels; the pointers of per-LP arrays count when B > 0)
    if (nnz < 0 || !rowmap_dev || !Aindptr_dev || (nnz > 0 && (!Adata_dev || !Aindices_dev)))
        return pycllp_entry_error(PYCLLP_E_BADARG, entry, "bad argument");
    if (B > 0 && (!a_dev || !b_dev || !c_dev || !u_dev || !bh_dev || !ch_dev || !uh_dev || !fh_dev || !invalid_dev))
        return pycllp_entry_error(PYCLLP_E_BADARG, entry, "bad argument");
    if (const int rc = check_sizes(entry, m, n, mk, B)) return rc;
    if (B == 0) return 0;
    const size_t per_lp = sizeof(double) * ((size_t)(n | 1) + 2 * (size_t)(m | 1));
    long G = (long)(kTileBytes / per_lp);                               // >= 1: per_lp <= 14 360 bytes
    G = G > 64 ? 64 : G;
    G = G > B ? B : G;
    const size_t lds = (size_t)G * per_lp + sizeof(double) * m + sizeof(int) * (2 * (size_t)m + G + 1);
    const long tiles = (B + G - 1) / G;
    const ToBounded p = { m, n, mk, (int)G, B, rowmap_dev, Adata_dev, Aindptr_dev, Aindices_dev, a_dev, b_dev, c_dev, l_dev, u_dev,
                          f_dev, bh_dev, ch_dev, uh_dev, fh_dev, invalid_dev };
    hipLaunchKernelGGL(general_to_bounded_kernel, dim3((unsigned)(tiles < kMaxGrid ? tiles : kMaxGrid)), dim3(kThreads), lds,
                       (hipStream_t)stream, p);
    return launched("general_to_bounded_kernel");
}

int pycllp_hip_general_from_bounded(int m, int n, int mk, long B, const int* rowmap_dev, const double* l_dev, const double* fh_dev,
                                    const int* invalid_dev, const double* xh_dev, const double* yh_dev, const double* zh_dev,
                                    const double* sh_dev, double* x_dev, double* y_dev, double* z_dev, double* s_dev,
                                    double* pobj_dev, double* dobj_dev, int* status_dev, int* iters_dev, void* stream) {
    static const char* entry = "pycllp_hip_general_from_bounded";
    if (!rowmap_dev || (!zh_dev && z_dev) || (!sh_dev && s_dev)) return pycllp_entry_error(PYCLLP_E_BADARG, entry, "bad argument");
    if (B > 0 && (!fh_dev || !invalid_dev || !xh_dev || !yh_dev || !x_dev || !y_dev || !status_dev))
        return pycllp_entry_error(PYCLLP_E_BADARG, entry, "bad argument");
    if (const int rc = check_sizes(entry, m, n, mk, B)) return rc;
    if (B == 0) return 0;
    long G = 8192 / (m > n ? m : n);                                    // about 32 elements of the longest pass per thread
    G = G > B ? B : G;
    const long tiles = (B + G - 1) / G;
    const FromBounded p = { m, n, mk, (int)G, B, rowmap_dev, l_dev, fh_dev, invalid_dev, xh_dev, yh_dev, zh_dev, sh_dev,
                            x_dev, y_dev, z_dev, s_dev, pobj_dev, dobj_dev, status_dev, iters_dev };
    hipLaunchKernelGGL(general_from_bounded_kernel, dim3((unsigned)(tiles < kMaxGrid ? tiles : kMaxGrid)), dim3(kThreads), 0,
                       (hipStream_t)stream, p);
    return launched("general_from_bounded_kernel");
}

}   // extern "C"
