// general_form_pa.hip -- a batch of GeneralLPs in which every LP has its OWN values of A on one shared structure, to the bounded
// equality form on the device: pycllp_hip_general_to_bounded_batch (include/pycllp_hip.h).  It is
// general_form.hip's to_bounded with the matrix per LP: b^, c^, u^, f^ and the checks are that kernel's, operation for
// operation, and the matrix A^_k comes out in the layout the caller's gather plan states -- [m', n] row-major for
// pycllp_hip_dense_solve_batch_bounded, the values of [+-A_k | I] in CSR order for pycllp_hip_sparse_solve_batch_bounded.
// pycllp_hip_general_from_bounded needs no matrix and serves these batches as it is.
//
// The traffic is the matrix (nnz doubles in, out_len out, against 3 n + 2 m + 2 N for everything else), so it moves through
// flat passes over a tile of G consecutive LPs: the lanes of a wavefront walk ONE LP's values, never the same term of 64 LPs,
// whose addresses lie nnz doubles apart.  A caller's array is touched through 8-byte (double) and 4-byte (int) accesses only,
// and an LP's slice of Avals and of Ah is addressed with 64-bit offsets (B nnz passes 2^31 at 65 536 LPs of 256 x 128).
#include <hip/hip_runtime.h>
#include <math.h>
#include <limits.h>
#include "../../include/pycllp_hip.h"
#include "host_error.h"

// as general_form.hip: every product and every sum is rounded on its own (the Makefile adds -ffp-contract=off)
#pragma clang fp contract(off)

namespace {

constexpr int kThreads = 256;
constexpr int kMaxRows = 256, kMaxCols = 1280;       // the bounded forms the solve kernels take: m <= 256, n + mk <= 1280
constexpr int kValid = 99;                           // "no check failed" in the per-LP minimum over the codes 1 .. 5
constexpr int kChunk = 256;                          // terms of one LP whose products are staged in LDS at a time
constexpr size_t kTileBytes = 32 * 1024;             // LDS of a tile: four or five workgroups per CU
constexpr long kMaxGrid = 1L << 20;

struct ToBoundedBatch {
    int m, n, mk, G, nnz;
    long B, out_len;
    const int* rowmap;
    const int* Aorder;
    const int* Aindptr;
    const int* Aindices;
    const double* Avals;
    const int* gather;
    const double *a, *b, *c, *l, *u, *f;
    double *Ah, *bh, *ch, *uh, *fh;
    int* invalid;
};

__device__ __forceinline__ bool finite64(double v) { return fabs(v) < INFINITY; }      // false for NaN

// A flat index e = g * len + p that advances by the workgroup's width without a division per element.
struct Flat {
    unsigned g, p, len, dg, dp;
    __device__ Flat(unsigned len_, unsigned tid) : g(tid / len_), p(tid % len_), len(len_), dg(kThreads / len_), dp(kThreads % len_) {}
    __device__ void next() {
        g += dg;
        p += dp;
        if (p >= len) { p -= len; g++; }
    }
};

// The tile in LDS: lt [G][n|1] the lower bounds l (0 where l_dev is NULL); at, bt [G][m|1] the row bounds a, b on the way in
// and b^ (by ORIGINAL row) and the slack's u^ on the way out; st [G][m|1] the sums (A_k l_k)_i, carried from chunk to chunk so
// that a row's terms are added in their order, and for an invalid LP afterwards the row sums of A^_k; pt [G][chunk|1] the
// products of one chunk of terms.  The odd strides keep the lanes of a wavefront, which in the sum pass hold consecutive LPs
// of one row, on different banks.  keep [mk], rm [m], bad [G] as in general_form.hip.
__global__ __launch_bounds__(kThreads) void general_to_bounded_batch_kernel(const ToBoundedBatch p) {
    extern __shared__ __attribute__((aligned(16))) double tile[];
    const int m = p.m, n = p.n, mk = p.mk, N = n + mk, G = p.G, nnz = p.nnz, tid = threadIdx.x;
    const int ls = n | 1, ms = m | 1, ps = (nnz < kChunk ? nnz : kChunk) | 1;
    double* lt = tile;
    double* at = lt + (size_t)G * ls;
    double* bt = at + (size_t)G * ms;
    double* st = bt + (size_t)G * ms;
    double* pt = st + (size_t)G * ms;
    int* keep = (int*)(pt + (size_t)G * ps);
    int* rm = keep + m;
    int* bad = rm + m;
    for (int i = tid; i < m; i += kThreads) {
        const int r = p.rowmap[i];
        rm[i] = r;
        if (r != 0) keep[(r > 0 ? r : -r) - 1] = i;
    }
    const long tiles = (p.B + G - 1) / G;
    for (long t = blockIdx.x; t < tiles; t += gridDim.x) {
        const long lp0 = t * G;
        const int ga = (int)(p.B - lp0 < G ? p.B - lp0 : G);            // LPs of this tile
        const double* Av = p.Avals + lp0 * nnz;
        if (tid < ga) bad[tid] = kValid;
        __syncthreads();
        // -- in: c, l, u checked (codes 1, 2, 5) and l kept; a, b checked (3, 4) and kept; f checked (5)
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
                if (code != kValid) atomicMin(&bad[g], code);
                lt[g * ls + j] = lv;
            }
            const double* a = p.a + lp0 * m;
            const double* b = p.b + lp0 * m;
            for (unsigned e = tid; e < (unsigned)(ga * m); e += kThreads) {
                const unsigned g = e / (unsigned)m, i = e - g * m;
                const double av = a[e], bv = b[e];
                const int r = rm[i];
                const bool af = finite64(av), bf = finite64(bv);
                int code = kValid;
                if (r > 0 ? !bf : r < 0 ? !(bv == INFINITY && af) : (af || bf)) code = 4;
                if (af && av > bv) code = 3;
                if (code != kValid) atomicMin(&bad[g], code);
                at[g * ms + i] = av;
                bt[g * ms + i] = bv;
                st[g * ms + i] = 0.0;
            }
            if (tid < ga && p.f && !finite64(p.f[lp0 + tid])) atomicMin(&bad[tid], 5);
        }
        __syncthreads();
        // -- A_k l_k: the products of a chunk of terms, read flat in CSR term order (one LP's values under the lanes of a
        //    wavefront), then one (LP, row) per thread adds the terms of its row that lie in the chunk, in their order
        for (int q0 = 0; q0 < nnz; q0 += kChunk) {
            const int cl = nnz - q0 < kChunk ? nnz - q0 : kChunk;
            Flat f(cl, tid);
            for (unsigned e = tid; e < (unsigned)(ga * cl); e += kThreads, f.next()) {
                const unsigned tq = (unsigned)p.Aorder[q0 + f.p], col = (unsigned)p.Aindices[q0 + f.p];
                double v = 0.0;                                         // (a plan that points outside the LP reads nothing)
                if (tq < (unsigned)nnz && col < (unsigned)n) v = __dmul_rn(Av[(size_t)f.g * nnz + tq], lt[f.g * ls + col]);
                pt[f.g * ps + f.p] = v;
            }
            __syncthreads();
            for (unsigned w = tid; w < (unsigned)(ga * m); w += kThreads) {
                const unsigned i = w / (unsigned)ga, g = w - i * ga;
                if (rm[i] == 0) continue;
                int q = p.Aindptr[i], q1 = p.Aindptr[i + 1];
                q = q < q0 ? q0 : q;
                q1 = q1 > q0 + cl ? q0 + cl : q1;
                if (q >= q1) continue;
                double al = st[g * ms + i];
                const double* pg = pt + g * ps;
                for (; q < q1; q++) al = __dadd_rn(al, pg[q - q0]);
                st[g * ms + i] = al;
            }
            __syncthreads();
        }
        // -- b^ by original row and the slack's u^; for an LP with a code the row sums of its OWN A^_k instead (its values
        //    straight from memory: the rare case)
        for (unsigned w = tid; w < (unsigned)(ga * m); w += kThreads) {
            const unsigned i = w / (unsigned)ga, g = w - i * ga;
            const int r = rm[i];
            if (r == 0) continue;
            if (bad[g] != kValid) {
                double sum = 0.0;
                for (int q = p.Aindptr[i], q1 = p.Aindptr[i + 1]; q < q1; q++) {
                    const unsigned tq = (unsigned)p.Aorder[q];
                    const double v = tq < (unsigned)nnz ? Av[(size_t)g * nnz + tq] : 0.0;
                    sum = __dadd_rn(sum, r > 0 ? v : -v);
                }
                st[g * ms + i] = __dadd_rn(sum, 1.0);
                continue;
            }
            const double al = st[g * ms + i], av = at[g * ms + i], bv = bt[g * ms + i];
            const double bh = __dsub_rn(bv, al), ah = __dsub_rn(av, al);
            at[g * ms + i] = r > 0 ? bh : -ah;
            bt[g * ms + i] = (r > 0 && finite64(ah)) ? __dsub_rn(bh, ah) : INFINITY;
        }
        __syncthreads();
        // -- out: A^ [ga out_len] by the gather plan (stores flat, loads from the lines this tile has just read)
        {
            double* Ah = p.Ah + lp0 * p.out_len;
            const unsigned ol = (unsigned)p.out_len;
            Flat f(ol, tid);
            for (unsigned e = tid; e < (unsigned)ga * ol; e += kThreads, f.next()) {
                const int gv = p.gather[f.p];
                double v = 0.0;
                if (gv == INT_MAX) {
                    v = 1.0;
                } else if (gv != 0) {
                    const unsigned tq = (unsigned)(gv > 0 ? gv : -gv) - 1u;
                    if (tq < (unsigned)nnz) {
                        const double w = Av[(size_t)f.g * nnz + tq];
                        v = gv > 0 ? w : -w;
                    }
                }
                Ah[(size_t)f.g * ol + f.p] = v;
            }
        }
        // -- out: b^ [ga mk], c^ and u^ [ga N], f^ and invalid [ga]
        {
            double* bh = p.bh + lp0 * mk;
            for (unsigned e = tid; e < (unsigned)(ga * mk); e += kThreads) {
                const unsigned g = e / (unsigned)mk, k = e - g * mk;
                const int i = keep[k];
                bh[e] = bad[g] == kValid ? at[g * ms + i] : st[g * ms + i];
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
        __syncthreads();                                                // (the next tile overwrites the tile's arrays and bad)
    }
}

}   // namespace

extern "C" int pycllp_hip_general_to_bounded_batch(int m, int n, int mk, long B, const int* rowmap_dev, int nnz, const int* Aorder_dev,
                                                   const int* Aindptr_dev, const int* Aindices_dev, const double* Avals_dev,
                                                   long out_len, const int* gather_dev, const double* a_dev, const double* b_dev,
                                                   const double* c_dev, const double* l_dev, const double* u_dev, const double* f_dev,
                                                   double* Ah_dev, double* bh_dev, double* ch_dev, double* uh_dev, double* fh_dev,
                                                   int* invalid_dev, void* stream) {
    static const char* entry = "pycllp_hip_general_to_bounded_batch";
    // (order: everything PYCLLP_E_BADARG covers, then the sizes beyond the kernels; the pointers of per-LP arrays count when B > 0)
    if (nnz < 0 || out_len < 1 || !rowmap_dev || !Aindptr_dev || !gather_dev || (nnz > 0 && (!Aorder_dev || !Aindices_dev)))
        return pycllp_entry_error(PYCLLP_E_BADARG, entry, "bad argument");
    if (B > 0 && ((nnz > 0 && !Avals_dev) || !a_dev || !b_dev || !c_dev || !u_dev || !Ah_dev || !bh_dev || !ch_dev || !uh_dev
                  || !fh_dev || !invalid_dev))
        return pycllp_entry_error(PYCLLP_E_BADARG, entry, "bad argument");
    if (m < 1 || n < 1 || mk < 1 || mk > m || B < 0) return pycllp_entry_error(PYCLLP_E_BADARG, entry, "bad argument");
    // (out_len: at most the dense [m', N]; also what keeps a tile's flat index within 32 bits)
    if (m > kMaxRows || (long)n + mk > kMaxCols || out_len > (long)kMaxRows * kMaxCols)
        return pycllp_entry_error(PYCLLP_E_UNSUPPORTED, entry, "beyond the bounded forms the solve kernels take (m <= 256, n + mk <= 1280)");
    if (B == 0) return 0;
    const size_t per_lp = sizeof(double) * ((size_t)(n | 1) + 3 * (size_t)(m | 1) + (size_t)((nnz < kChunk ? nnz : kChunk) | 1));
    long G = (long)(kTileBytes / per_lp);                               // >= 1: per_lp <= 18 456 bytes
    G = G > 64 ? 64 : G;
    G = G > B ? B : G;
    const size_t lds = (size_t)G * per_lp + sizeof(int) * (2 * (size_t)m + G);
    const long tiles = (B + G - 1) / G;
    const ToBoundedBatch p = { m, n, mk, (int)G, nnz, B, out_len, rowmap_dev, Aorder_dev, Aindptr_dev, Aindices_dev, Avals_dev,
                               gather_dev, a_dev, b_dev, c_dev, l_dev, u_dev, f_dev, Ah_dev, bh_dev, ch_dev, uh_dev, fh_dev,
                               invalid_dev };
    hipLaunchKernelGGL(general_to_bounded_batch_kernel, dim3((unsigned)(tiles < kMaxGrid ? tiles : kMaxGrid)), dim3(kThreads), lds,
                       (hipStream_t)stream, p);
    const hipError_t e = hipGetLastError();
    return e == hipSuccess ? 0 : pycllp_runtime_error((int)e, "general_to_bounded_batch_kernel");
}
