// general_form.hip -- a batch of GeneralLPs (a <= A x <= b, l <= x <= u) to and from the bounded equality form
// ([+-A | I] x^ = b^, 0 <= x^ <= u^) on the device: pycllp_hip_general_to_bounded (shared A),
// pycllp_hip_general_to_bounded_batch (every LP its OWN values of A on one shared structure; section 22) and
// pycllp_hip_general_from_bounded, which needs no matrix and serves both (include/pycllp_hip.h).  The arithmetic is
// GeneralLP.to_bounded_equality_form's and BoundedMap.general's (pycllp_amd/lp.py) operation for operation -- separately rounded
// products and sums, no contraction -- so b^, c^, u^ and x, y, z, s carry the host's bits.
//
// All kernels are memory bound and work on TILES of G consecutive LPs per workgroup: the arrays of a tile are contiguous in
// the caller's memory ([G n] of c, l, u; [G m] of a, b; [G N] of c^, u^ ...), so every element-wise pass runs coalesced over a
// flat 32-bit index and a short row (7 ... 1 280 doubles) never leaves lanes idle.  A caller's array is touched through
// 8-byte (double) and 4-byte (int) accesses only, from element 0 to the last element of its shape.
//
// The two to_bounded kernels are ONE text wherever they do the same: the row map, the checks, the column pass, b^ and u^ of a
// row, and the whole output pass are the __device__ functions below.  Each kernel owns how A l is summed: the shared-A kernel
// gives a thread one (LP, row) whose terms the lanes of a wavefront share; with per-problem values that would put the lanes
// nnz doubles apart, so the batch kernel moves the matrix through flat passes -- the lanes of a wavefront walk ONE LP's values
// -- and also writes every LP's A^ in the layout the caller's gather plan states ([m', n] row-major for
// pycllp_hip_dense_solve_batch_bounded, the values of [+-A_k | I] in CSR order for pycllp_hip_sparse_solve_batch_bounded).
// There an LP's slice of Avals and of Ah is addressed with 64-bit offsets (B nnz passes 2^31 at 65 536 LPs of 256 x 128).
#include <hip/hip_runtime.h>
#include <math.h>
#include <limits.h>
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
constexpr int kChunk = 256;                          // batch kernel: terms of one LP whose products are staged in LDS at a time
constexpr size_t kSharedTileBytes = 24 * 1024;       // LDS of the shared-A tile: six workgroups per CU (the A l sums wait on loads)
constexpr size_t kBatchTileBytes = 32 * 1024;        // LDS of the per-problem tile: four or five workgroups per CU
constexpr long kMaxGrid = 1L << 20;

// what both to_bounded entries take of a batch besides its matrix
struct Vectors {
    int m, n, mk, G;
    long B;
    const int* rowmap;
    const double *a, *b, *c, *l, *u, *f;
    double *bh, *ch, *uh, *fh;
    int* invalid;
};

struct ToBounded {
    Vectors v;
    const double* Adata;
    const int* Aindptr;
    const int* Aindices;
};

struct ToBoundedBatch {
    Vectors v;
    int nnz;
    long out_len;
    const int* Aorder;
    const int* Aindptr;
    const int* Aindices;
    const double* Avals;
    const int* gather;
    double* Ah;
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

// The part of a tile in LDS that both to_bounded kernels hold: lt [G][n|1] the lower bounds l (0 where l_dev is NULL); at, bt
// [G][m|1] the row bounds a, b on the way in and b^ (by ORIGINAL row) and the slack's u^ on the way out -- the odd strides ls,
// ms keep the lanes of a wavefront, which hold consecutive LPs of one row, on different banks; keep [mk] the original row of
// each kept row, rm [m] the row map, bad [G] the smallest failing check of each LP.
struct Tile {
    int ls, ms;
    double *lt, *at, *bt;
    int *keep, *rm, *bad;
};

__device__ __forceinline__ void load_rowmap(const Vectors& p, const Tile& t, int tid) {
    for (int i = tid; i < p.m; i += kThreads) {
        const int r = p.rowmap[i];
        t.rm[i] = r;
        if (r != 0) t.keep[(r > 0 ? r : -r) - 1] = i;
    }
}

// LP g of the tile failed check `code` (kValid: none).  anybad: the shared-A kernel's "this tile holds an invalid LP", or NULL.
__device__ __forceinline__ void flag(const Tile& t, unsigned g, int code, int* anybad) {
    if (code != kValid) {
        atomicMin(&t.bad[g], code);
        if (anybad) *anybad = 1;
    }
}

// the checks of one row of kind r (> 0 a '+' row, < 0 a '-' row, 0 dropped) with the bounds a, b: codes 3 and 4
__device__ __forceinline__ int row_code(int r, double av, double bv) {
    const bool af = finite64(av), bf = finite64(bv);
    int code = kValid;
    if (r > 0 ? !bf : r < 0 ? !(bv == INFINITY && af) : (af || bf)) code = 4;
    if (af && av > bv) code = 3;
    return code;
}

// -- in: c, l, u checked (codes 1, 2, 5) and l kept; f checked (5)
__device__ __forceinline__ void column_pass(const Vectors& p, const Tile& t, long lp0, int ga, int* anybad, int tid) {
    const int n = p.n;
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
        flag(t, g, code, anybad);
        t.lt[g * t.ls + j] = lv;
    }
    if (tid < ga && p.f && !finite64(p.f[lp0 + tid])) flag(t, tid, 5, anybad);
}

// b^ of a kept row of kind r and its slack's u^ from the bounds a, b and al = (A l)_i, over a and b in LDS
__device__ __forceinline__ void bounded_row(int r, double av, double bv, double al, double* at, double* bt) {
    const double bh = __dsub_rn(bv, al), ah = __dsub_rn(av, al);
    *at = r > 0 ? bh : -ah;
    *bt = (r > 0 && finite64(ah)) ? __dsub_rn(bh, ah) : INFINITY;
}

// -- out: b^ [ga mk], c^ and u^ [ga N], f^ and invalid [ga].  An LP with a code gets b^ = A^ 1 from sums[g * stride + i]
//    (stride 0: one matrix for all), c^ = 0, u^ = +inf, f^ = 0.
__device__ __forceinline__ void output_pass(const Vectors& p, const Tile& t, long lp0, int ga, const double* sums, int stride, int tid) {
    const int n = p.n, mk = p.mk, N = n + mk, ls = t.ls, ms = t.ms;
    const double *lt = t.lt, *at = t.at, *bt = t.bt;
    const int *keep = t.keep, *bad = t.bad;
    double* bh = p.bh + lp0 * mk;
    for (unsigned e = tid; e < (unsigned)(ga * mk); e += kThreads) {
        const unsigned g = e / (unsigned)mk, k = e - g * mk;
        const int i = keep[k];
        bh[e] = bad[g] == kValid ? at[g * ms + i] : sums[g * stride + i];
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

// Shared A.  Beside the Tile: rs [m] the row sums of A^ (only where a tile holds an invalid LP: anybad).
__global__ __launch_bounds__(kThreads) void general_to_bounded_kernel(const ToBounded q) {
    extern __shared__ __attribute__((aligned(16))) double tile[];
    const Vectors& p = q.v;
    const int m = p.m, n = p.n, G = p.G, ls = n | 1, ms = m | 1, tid = threadIdx.x;
    double* lt = tile;
    double* at = lt + (size_t)G * ls;
    double* bt = at + (size_t)G * ms;
    double* rs = bt + (size_t)G * ms;
    int* keep = (int*)(rs + m);
    int* rm = keep + m;
    int* bad = rm + m;
    int* anybad = bad + G;
    const Tile t = { ls, ms, lt, at, bt, keep, rm, bad };
    load_rowmap(p, t, tid);
    const long tiles = (p.B + G - 1) / G;
    for (long ti = blockIdx.x; ti < tiles; ti += gridDim.x) {
        const long lp0 = ti * G;
        const int ga = (int)(p.B - lp0 < G ? p.B - lp0 : G);            // LPs of this tile
        if (tid < ga) bad[tid] = kValid;
        if (tid == 0) *anybad = 0;
        __syncthreads();
        column_pass(p, t, lp0, ga, anybad, tid);
        {                                                               // a, b kept
            const double* a = p.a + lp0 * m;
            const double* b = p.b + lp0 * m;
            for (unsigned e = tid; e < (unsigned)(ga * m); e += kThreads) {
                const unsigned g = e / (unsigned)m, i = e - g * m;
                at[g * ms + i] = a[e];
                bt[g * ms + i] = b[e];
            }
        }
        __syncthreads();
        // -- one (LP, row) per thread, the LP index fastest: the lanes of a wavefront share the row's terms
        for (unsigned w = tid; w < (unsigned)(ga * m); w += kThreads) {
            const unsigned i = w / (unsigned)ga, g = w - i * ga;
            const int r = rm[i];
            const double av = at[g * ms + i], bv = bt[g * ms + i];
            flag(t, g, row_code(r, av, bv), anybad);
            if (r == 0) continue;
            double al = 0.0;
            const double* lg = lt + g * ls;
#pragma unroll 4                                                        // (the loads of four terms in flight; the sum stays in order)
            for (int k = q.Aindptr[i], k1 = q.Aindptr[i + 1]; k < k1; k++)
                al = __dadd_rn(al, __dmul_rn(q.Adata[k], lg[q.Aindices[k]]));
            bounded_row(r, av, bv, al, &at[g * ms + i], &bt[g * ms + i]);
        }
        __syncthreads();
        if (*anybad) {                                                  // (one answer for the whole workgroup)
            for (int i = tid; i < m; i += kThreads) {
                const int r = rm[i];
                if (r == 0) continue;
                double sum = 0.0;
                for (int k = q.Aindptr[i], k1 = q.Aindptr[i + 1]; k < k1; k++) sum = __dadd_rn(sum, r > 0 ? q.Adata[k] : -q.Adata[k]);
                rs[i] = __dadd_rn(sum, 1.0);
            }
            __syncthreads();
        }
        output_pass(p, t, lp0, ga, rs, 0, tid);
        __syncthreads();                                                // (the next tile overwrites lt, at, bt and bad)
    }
}

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

// Per-problem values of A.  Beside the Tile: st [G][m|1] the sums (A_k l_k)_i, carried from chunk to chunk so that a row's
// terms are added in their order, and for an invalid LP afterwards the row sums of A^_k; pt [G][chunk|1] the products of one
// chunk of terms.
__global__ __launch_bounds__(kThreads) void general_to_bounded_batch_kernel(const ToBoundedBatch q) {
    extern __shared__ __attribute__((aligned(16))) double tile[];
    const Vectors& p = q.v;
    const int m = p.m, n = p.n, G = p.G, nnz = q.nnz, tid = threadIdx.x;
    const int ls = n | 1, ms = m | 1, ps = (nnz < kChunk ? nnz : kChunk) | 1;
    double* lt = tile;
    double* at = lt + (size_t)G * ls;
    double* bt = at + (size_t)G * ms;
    double* st = bt + (size_t)G * ms;
    double* pt = st + (size_t)G * ms;
    int* keep = (int*)(pt + (size_t)G * ps);
    int* rm = keep + m;
    int* bad = rm + m;
    const Tile t = { ls, ms, lt, at, bt, keep, rm, bad };
    load_rowmap(p, t, tid);
    const long tiles = (p.B + G - 1) / G;
    for (long ti = blockIdx.x; ti < tiles; ti += gridDim.x) {
        const long lp0 = ti * G;
        const int ga = (int)(p.B - lp0 < G ? p.B - lp0 : G);            // LPs of this tile
        const double* Av = q.Avals + lp0 * nnz;
        if (tid < ga) bad[tid] = kValid;
        __syncthreads();
        column_pass(p, t, lp0, ga, nullptr, tid);
        {                                                               // a, b checked (3, 4) and kept
            const double* a = p.a + lp0 * m;
            const double* b = p.b + lp0 * m;
            for (unsigned e = tid; e < (unsigned)(ga * m); e += kThreads) {
                const unsigned g = e / (unsigned)m, i = e - g * m;
                const double av = a[e], bv = b[e];
                flag(t, g, row_code(rm[i], av, bv), nullptr);
                at[g * ms + i] = av;
                bt[g * ms + i] = bv;
                st[g * ms + i] = 0.0;
            }
        }
        __syncthreads();
        // -- A_k l_k: the products of a chunk of terms, read flat in CSR term order (one LP's values under the lanes of a
        //    wavefront), then one (LP, row) per thread adds the terms of its row that lie in the chunk, in their order
        for (int q0 = 0; q0 < nnz; q0 += kChunk) {
            const int cl = nnz - q0 < kChunk ? nnz - q0 : kChunk;
            Flat f(cl, tid);
            for (unsigned e = tid; e < (unsigned)(ga * cl); e += kThreads, f.next()) {
                const unsigned tq = (unsigned)q.Aorder[q0 + f.p], col = (unsigned)q.Aindices[q0 + f.p];
                double v = 0.0;                                         // (a plan that points outside the LP reads nothing)
                if (tq < (unsigned)nnz && col < (unsigned)n) v = __dmul_rn(Av[(size_t)f.g * nnz + tq], lt[f.g * ls + col]);
                pt[f.g * ps + f.p] = v;
            }
            __syncthreads();
            for (unsigned w = tid; w < (unsigned)(ga * m); w += kThreads) {
                const unsigned i = w / (unsigned)ga, g = w - i * ga;
                if (rm[i] == 0) continue;
                int k = q.Aindptr[i], k1 = q.Aindptr[i + 1];
                k = k < q0 ? q0 : k;
                k1 = k1 > q0 + cl ? q0 + cl : k1;
                if (k >= k1) continue;
                double al = st[g * ms + i];
                const double* pg = pt + g * ps;
                for (; k < k1; k++) al = __dadd_rn(al, pg[k - q0]);
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
                for (int k = q.Aindptr[i], k1 = q.Aindptr[i + 1]; k < k1; k++) {
                    const unsigned tq = (unsigned)q.Aorder[k];
                    const double v = tq < (unsigned)nnz ? Av[(size_t)g * nnz + tq] : 0.0;
                    sum = __dadd_rn(sum, r > 0 ? v : -v);
                }
                st[g * ms + i] = __dadd_rn(sum, 1.0);
                continue;
            }
            bounded_row(r, at[g * ms + i], bt[g * ms + i], st[g * ms + i], &at[g * ms + i], &bt[g * ms + i]);
        }
        __syncthreads();
        // -- out: A^ [ga out_len] by the gather plan (stores flat, loads from the lines this tile has just read)
        {
            double* Ah = q.Ah + lp0 * q.out_len;
            const unsigned ol = (unsigned)q.out_len;
            Flat f(ol, tid);
            for (unsigned e = tid; e < (unsigned)ga * ol; e += kThreads, f.next()) {
                const int gv = q.gather[f.p];
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
        output_pass(p, t, lp0, ga, st, ms, tid);
        __syncthreads();                                                // (the next tile overwrites the tile's arrays and bad)
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

// PYCLLP_E_BADARG / PYCLLP_E_UNSUPPORTED for the sizes all entries take, 0 where they pass (out_len: at most the dense [m', N];
// also what keeps a tile's flat index within 32 bits)
int check_sizes(const char* entry, int m, int n, int mk, long B, long out_len = 1) {
    if (m < 1 || n < 1 || mk < 1 || mk > m || B < 0) return pycllp_entry_error(PYCLLP_E_BADARG, entry, "bad argument");
    if (m > kMaxRows || (long)n + mk > kMaxCols || out_len > (long)kMaxRows * kMaxCols)
        return pycllp_entry_error(PYCLLP_E_UNSUPPORTED, entry, "beyond the bounded forms the solve kernels take (m <= 256, n + mk <= 1280)");
    return 0;
}

// LPs of a to_bounded tile: as many as tile_bytes of LDS hold at per_lp bytes each (>= 1: per_lp <= 18 456 bytes), at most 64
long tile_lps(size_t tile_bytes, size_t per_lp, long B) {
    long G = (long)(tile_bytes / per_lp);
    G = G > 64 ? 64 : G;
    return G > B ? B : G;
}

dim3 grid_of(long B, long G) {
    const long tiles = (B + G - 1) / G;
    return dim3((unsigned)(tiles < kMaxGrid ? tiles : kMaxGrid));
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
    const long G = tile_lps(kSharedTileBytes, per_lp, B);
    const size_t lds = (size_t)G * per_lp + sizeof(double) * m + sizeof(int) * (2 * (size_t)m + G + 1);
    const ToBounded p = { { m, n, mk, (int)G, B, rowmap_dev, a_dev, b_dev, c_dev, l_dev, u_dev, f_dev, bh_dev, ch_dev, uh_dev, fh_dev,
                            invalid_dev }, Adata_dev, Aindptr_dev, Aindices_dev };
    hipLaunchKernelGGL(general_to_bounded_kernel, grid_of(B, G), dim3(kThreads), lds, (hipStream_t)stream, p);
    return launched("general_to_bounded_kernel");
}

int pycllp_hip_general_to_bounded_batch(int m, int n, int mk, long B, const int* rowmap_dev, int nnz, const int* Aorder_dev,
                                        const int* Aindptr_dev, const int* Aindices_dev, const double* Avals_dev, long out_len,
                                        const int* gather_dev, const double* a_dev, const double* b_dev, const double* c_dev,
                                        const double* l_dev, const double* u_dev, const double* f_dev, double* Ah_dev, double* bh_dev,
                                        double* ch_dev, double* uh_dev, double* fh_dev, int* invalid_dev, void* stream) {
    static const char* entry = "pycllp_hip_general_to_bounded_batch";
    // (the same order)
    if (nnz < 0 || out_len < 1 || !rowmap_dev || !Aindptr_dev || !gather_dev || (nnz > 0 && (!Aorder_dev || !Aindices_dev)))
        return pycllp_entry_error(PYCLLP_E_BADARG, entry, "bad argument");
    if (B > 0 && ((nnz > 0 && !Avals_dev) || !a_dev || !b_dev || !c_dev || !u_dev || !Ah_dev || !bh_dev || !ch_dev || !uh_dev
                  || !fh_dev || !invalid_dev))
        return pycllp_entry_error(PYCLLP_E_BADARG, entry, "bad argument");
    if (const int rc = check_sizes(entry, m, n, mk, B, out_len)) return rc;
    if (B == 0) return 0;
    const size_t per_lp = sizeof(double) * ((size_t)(n | 1) + 3 * (size_t)(m | 1) + (size_t)((nnz < kChunk ? nnz : kChunk) | 1));
    const long G = tile_lps(kBatchTileBytes, per_lp, B);
    const size_t lds = (size_t)G * per_lp + sizeof(int) * (2 * (size_t)m + G);
    const ToBoundedBatch p = { { m, n, mk, (int)G, B, rowmap_dev, a_dev, b_dev, c_dev, l_dev, u_dev, f_dev, bh_dev, ch_dev, uh_dev,
                                 fh_dev, invalid_dev }, nnz, out_len, Aorder_dev, Aindptr_dev, Aindices_dev, Avals_dev, gather_dev,
                               Ah_dev };
    hipLaunchKernelGGL(general_to_bounded_batch_kernel, grid_of(B, G), dim3(kThreads), lds, (hipStream_t)stream, p);
    return launched("general_to_bounded_batch_kernel");
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
    const FromBounded p = { m, n, mk, (int)G, B, rowmap_dev, l_dev, fh_dev, invalid_dev, xh_dev, yh_dev, zh_dev, sh_dev,
                            x_dev, y_dev, z_dev, s_dev, pobj_dev, dobj_dev, status_dev, iters_dev };
    hipLaunchKernelGGL(general_from_bounded_kernel, grid_of(B, G), dim3(kThreads), 0, (hipStream_t)stream, p);
    return launched("general_from_bounded_kernel");
}

}   // extern "C"
