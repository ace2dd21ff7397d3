// ipm_dense.hip -- batched dense primal-normal-equations interior-point LP solver for MI355X (gfx950).
//
// What it replaces in the reference (jetuk/pycllp): the OpenCL kernels pycllp/cl/primal_normal.cl
// (standard_primal_normal :201-284, primal_normal_step :122-156, initialize_xzyw :14-28) and
// pycllp/cl/ldl.cl (factor_primal_normal :314-378, forward_backward_primal_normal :505-537,
// residual_primal_normal :577-599, solve_primal_normal :602-653), hosted by pycllp/solvers/cl.py.
//
// Design (CDNA4-first, not a translation): the reference maps one LP to one work-item and re-reads
// x, z from global memory for every matrix entry.  Here ONE LP IS OWNED BY ONE 64-LANE WAVEFRONT for
// its whole solve; its state never leaves the CU:
//   * N-vectors (x, z, c, A'y, ...) live in registers, lane = column (columns lane and lane+64);
//   * m-vectors (y, b, rho, dy, ...) live in registers, lane = row (lane mod MP);
//   * the shared constraint matrix A sits in LDS once per workgroup, in two images: the operand order
//     of v_mfma_f64_16x16x4_f64 (for the Gram product and the A*v products) and row-major (for A'u);
//   * the Gram matrix M = A diag(x/z) A' is a true dense contraction and runs on the matrix cores
//     (MFMA f64 16x16x4, symmetric: only the lower 16x16 blocks), fused with A*x and A*(d.t);
//   * M goes through LDS once to turn the MFMA accumulator layout into "lane = row"; the modified
//     LDL' factorisation then runs out of registers (row i of the trailing matrix in lane i), the
//     transposed factor is staged in the wave's private LDS slab for the triangular solves;
//   * HBM traffic is the compulsory b, c in and x, y, z, objectives, status out: 16(m+N)+8N+24 B/LP.
// Workgroups are persistent: each wave strides over the batch.
//
// Numerical semantics follow oracle/ipm_dense_ref.c (the CPU restatement used by the tests), i.e. the
// reference algorithm with the SURVEY section 8(a) picks: relative stopping tolerance, DELTA/R of the
// OpenCL kernel, Nocedal-Wright diagonal guard, |r|-driven iterative refinement, NaN guard.
#include "dense_tab.h"

// ------------------------------------------------------------------------------------------------
// compile-time geometry
// ------------------------------------------------------------------------------------------------
template <int MP, int NP>
struct Geo {
    static_assert(MP == 16 || MP == 32, "row padding must be 16 or 32");
    static_assert(NP % 8 == 0 && NP >= 8 && NP <= 128, "column padding must be a multiple of 8, <= 128");
    static constexpr int JB = MP / 16;           // 16-row blocks of A
    static constexpr int KS = NP / 4;            // k-steps of the 16x16x4 MFMA
    static constexpr int NC = (NP > 64) ? 2 : 1; // columns per lane
    static constexpr int NL = 64 * NC;           // row-major image row length
    static constexpr int MS = MP + 2;            // row stride of the wave's matrix slab (16-B aligned rows,
                                                 // conflict-free b128 row reads)
    static constexpr int AMF = JB * KS * 64;     // doubles in the MFMA-order image
    static constexpr int ARM = MP * NL;          // doubles in the row-major image
    static constexpr int APACK = AMF + ARM;
    static constexpr int WSLAB = MP * MS + 3 * NP; // per-wave doubles: matrix slab + 3 k-layout vectors
    static constexpr size_t lds_bytes(int wpb) { return sizeof(double) * (size_t)(APACK + wpb * WSLAB); }
    // position of column j in a k-layout vector: lane group g = j&3 reads KS consecutive values
    __host__ __device__ static constexpr int kpos(int j) { return (j & 3) * KS + (j >> 2); }
};

// ------------------------------------------------------------------------------------------------
// pack kernel: A [m,n] row-major  ->  [ MFMA-operand image | row-major padded image ]
//   Amf[J][s][l] = A[16J + (l&15)][4s + (l>>4)]   (A/B operand lane map of v_mfma_f64_16x16x4_f64)
//   Arm[i][j]    = A[i][j]   (zero padded to MP x NL)
// ------------------------------------------------------------------------------------------------
template <int MP, int NP>
__global__ void pack_A_kernel(int m, int n, const double* __restrict__ A, double* __restrict__ pack) {
    using G = Geo<MP, NP>;
    int idx = blockIdx.x * blockDim.x + threadIdx.x;
    if (idx < G::AMF) {
        int l = idx & 63, s = (idx >> 6) % G::KS, J = (idx >> 6) / G::KS;
        int row = 16 * J + (l & 15), col = 4 * s + (l >> 4);
        pack[idx] = (row < m && col < n) ? A[(size_t)row * n + col] : 0.0;
    } else if (idx < G::APACK) {
        int k = idx - G::AMF;
        int row = k / G::NL, col = k % G::NL;
        pack[idx] = (row < m && col < n) ? A[(size_t)row * n + col] : 0.0;
    }
}

// ------------------------------------------------------------------------------------------------
// Per-wave Newton machinery
// ------------------------------------------------------------------------------------------------
template <int MP, int NP>
struct Wave {
    using G = Geo<MP, NP>;
    static constexpr int JB = G::JB, KS = G::KS, NC = G::NC, MS = G::MS;

    const double* Amf;  // LDS, MFMA-order image
    const double* Arm;  // LDS, row-major image
    double* slab;       // LDS, wave-private MP x MS matrix slab
    double* kx;         // LDS, wave-private k-layout vectors
    double* kd;
    double* kdt;
    int lane, ri, m, n;

    // v_q = sum_i A[i][col_q] * u[i]   (u in lane=row layout)  -- A'u, reference primal_normal.cl:138-141
    __device__ __forceinline__ void At_times(double u, double out[NC]) const {
#pragma unroll
        for (int q = 0; q < NC; q++) out[q] = 0.0;
        // chunks of 8 rows: bounded unrolling keeps the LDS loads the scheduler hoists (and the broadcast SGPRs) few
#pragma unroll 1
        for (int i0 = 0; i0 < MP; i0 += 8) {
#pragma unroll
            for (int ii = 0; ii < 8; ii++) {
                const int i = i0 + ii;
                const double ui = readlane_d(u, i);
#pragma unroll
                for (int q = 0; q < NC; q++) out[q] = fma(Arm[i * G::NL + lane + 64 * q], ui, out[q]);
            }
        }
    }

    // Gram product on the matrix cores, fused with A*x and A*(d.t).
    // In: kx, kd, kdt hold x, d = x/z and d*t in k-layout.  Out: M written to the slab (full symmetric),
    // Ax / Adt in lane=row layout.
    __device__ __forceinline__ void gram_fused(double& Ax, double& Adt) const {
        const int g = lane >> 4;
        double4_t acc[JB][JB];
        double axp[JB], adp[JB];
#pragma unroll
        for (int I = 0; I < JB; I++) {
            axp[I] = 0.0; adp[I] = 0.0;
#pragma unroll
            for (int J = 0; J < JB; J++) acc[I][J] = (double4_t){0.0, 0.0, 0.0, 0.0};
        }
        const double* px = kx + g * KS;
        const double* pd = kd + g * KS;
        const double* pt = kdt + g * KS;
        static_assert(KS % 2 == 0, "k-steps are processed in pairs");
        constexpr int SC = (KS % 4 == 0) ? 4 : 2;   // k-steps per chunk (bounded unrolling: see At_times)
#pragma unroll 1
        for (int s0 = 0; s0 < KS; s0 += SC) {
#pragma unroll
            for (int ss = 0; ss < SC; ss++) {
                const int s = s0 + ss;
                const double xk = px[s], dk = pd[s], tk = pt[s];
                double a[JB], ad[JB];
#pragma unroll
                for (int J = 0; J < JB; J++) {
                    a[J] = Amf[(J * KS + s) * 64 + lane];
                    axp[J] = fma(a[J], xk, axp[J]);
                    adp[J] = fma(a[J], tk, adp[J]);
                    ad[J] = a[J] * dk;
                }
#pragma unroll
                for (int I = 0; I < JB; I++)
#pragma unroll
                    for (int J = 0; J <= I; J++)
                        acc[I][J] = __builtin_amdgcn_mfma_f64_16x16x4f64(ad[I], a[J], acc[I][J], 0, 0, 0);
            }
        }
        // accumulator (I,J), register r4: row 16I + (lane>>4) + 4*r4, col 16J + (lane&15)
        const int cc = lane & 15;
#pragma unroll
        for (int I = 0; I < JB; I++)
#pragma unroll
            for (int J = 0; J <= I; J++)
#pragma unroll
                for (int r4 = 0; r4 < 4; r4++) {
                    int row = 16 * I + g + 4 * r4, col = 16 * J + cc;
                    double v = acc[I][J][r4];
                    slab[row * MS + col] = v;
                    if (I != J) slab[col * MS + row] = v;
                }
        // reduce the A*v partials over the 4 lane groups; pick this lane's row block
#pragma unroll
        for (int J = 0; J < JB; J++) {
            axp[J] += __shfl_xor(axp[J], 16, WAVE);
            axp[J] += __shfl_xor(axp[J], 32, WAVE);
            adp[J] += __shfl_xor(adp[J], 16, WAVE);
            adp[J] += __shfl_xor(adp[J], 32, WAVE);
        }
        if (JB == 1) { Ax = axp[0]; Adt = adp[0]; }
        else {
            const bool hiblk = (ri >> 4) & 1;
            Ax = hiblk ? axp[JB - 1] : axp[0];
            Adt = hiblk ? adp[JB - 1] : adp[0];
        }
    }

    // Modified LDL' (Nocedal-Wright 3.4 guard, ldl.cl:314-378) of the matrix whose row `ri` is in W.
    // On exit: slab[j*MS + i] = L[i][j] for i>j (0 elsewhere), rdiag = 1/D[ri].
    __device__ __forceinline__ void factor(double (&W)[MP], double beta2, double floor_, double& rdiag) const {
        rdiag = 1.0;
#pragma unroll
        for (int j = 0; j < MP; j++) {
            const double u = W[j];
            const double piv = readlane_d(u, j);
            double aD = fmax(fabs(piv), floor_);
            const bool below = ri > j;
            // guard: D_j = max(|D_j|, (theta/beta)^2, floor) with theta = max_{i>j} |u_i|; it only bites when
            // some u_i^2 > beta^2 * max(|D_j|, floor), which one ballot detects
            if (__any(below && (u * u > beta2 * aD))) {
                double theta = wave_max(below ? fabs(u) : 0.0);
                aD = fmax(aD, theta * theta / beta2);
            }
            const double rD = fast_rcp(aD);
            const double l = below ? u * rD : 0.0;
            if (ri == j) rdiag = rD;
            slab[j * MS + ri] = l;  // lanes >= MP write the same value as their twin: benign
            if (j + 1 < MP) {
                wave_lds_sync();
                const double* Lj = slab + j * MS;
                double lk[MP];
#pragma unroll
                for (int k = j + 1; k < MP; k++) lk[k] = Lj[k];          // broadcast reads, batched
#pragma unroll
                for (int k = j + 1; k < MP; k++) W[k] = fma(-u, lk[k], W[k]);
                // pin the update to column j: otherwise LLVM sinks the FMA chains to the column that consumes
                // them (a left-looking sweep), keeps every broadcast L value alive and spills ~2 KB per lane
#pragma unroll
                for (int k = j + 1; k < MP; k++) asm volatile("" : "+v"(W[k]));
            }
        }
        wave_lds_sync();
    }

    // s <- (L D L')^-1 s  (ldl.cl:505-537), s in lane=row layout
    __device__ __forceinline__ double fwd_back(double s, double rdiag) const {
        // forward, column oriented: t_i -= L[i][k] t_k
#pragma unroll 1
        for (int k0 = 0; k0 < MP; k0 += 8) {
#pragma unroll
            for (int kk = 0; kk < 8; kk++) {
                const int k = k0 + kk;
                const double tk = readlane_d(s, k);
                s = fma(-slab[k * MS + ri], tk, s);   // row MP-1 of the slab is all zero: harmless last step
            }
        }
        s *= rdiag;
        // backward, column oriented: s_j -= L[i][j] s_i for j < i; lane j owns row j of the slab
        const double* row = slab + ri * MS;
#pragma unroll 1
        for (int i0 = MP - 8; i0 >= 0; i0 -= 8) {
#pragma unroll
            for (int ii = 7; ii >= 0; ii--) {
                const int i = i0 + ii;
                const double si = readlane_d(s, i);
                s = fma(-row[i], si, s);              // row[i] = L[i][ri] for i > ri, 0 otherwise
            }
        }
        return s;
    }

    // u = A * vq  (vq per column -> lane=row layout) through the MFMA-order image: the k-layout copy of vq is
    // staged in the wave's kx slot, every lane accumulates its 4-column slice, two shuffles fold the 4 lane groups
    __device__ __forceinline__ double A_times(const double (&vq)[NC]) const {
#pragma unroll
        for (int q = 0; q < NC; q++) {
            const int j = lane + 64 * q;
            if (j < NP) kx[G::kpos(j)] = (j < n) ? vq[q] : 0.0;
        }
        wave_lds_sync();
        const double* px = kx + (lane >> 4) * KS;
        double acc[JB];
#pragma unroll
        for (int J = 0; J < JB; J++) acc[J] = 0.0;
        constexpr int SC = (KS % 4 == 0) ? 4 : 2;
#pragma unroll 1
        for (int s0 = 0; s0 < KS; s0 += SC) {
#pragma unroll
            for (int ss = 0; ss < SC; ss++) {
                const double xk = px[s0 + ss];
#pragma unroll
                for (int J = 0; J < JB; J++) acc[J] = fma(Amf[(J * KS + s0 + ss) * 64 + lane], xk, acc[J]);
            }
        }
#pragma unroll
        for (int J = 0; J < JB; J++) {
            acc[J] += __shfl_xor(acc[J], 16, WAVE);
            acc[J] += __shfl_xor(acc[J], 32, WAVE);
        }
        wave_lds_sync();
        if (JB == 1) return acc[0];
        return ((ri >> 4) & 1) ? acc[JB - 1] : acc[0];
    }

    // Newton step of the primal normal equations (ldl.cl:602-653) given x, z, c, v=A'y, b, mu:
    //   M dy = A d t - rho,  dx = d (t - A'dy),  then <= max_refine passes of x-space refinement
    //   e = rho - A dx ; M eta = e ; dx += d A'eta ; dy -= eta      (see oracle/ipm_dense_ref.c newton_dy)
    // Returns dy (lane=row); outputs dx, wv = A'dy (per column), rho and the refinement count.
    __device__ __forceinline__ double newton(const double (&x)[NC], const double (&z)[NC], const double (&c)[NC],
                                             const double (&v)[NC], double b, double mu, double etol, const DevOpts& o,
                                             double (&dx)[NC], double (&wv)[NC], double& rho, int& nref STAMP_ARGS) const {
        double d[NC], t[NC];
#pragma unroll
        for (int q = 0; q < NC; q++) {
            const int j = lane + 64 * q;
            const bool ok = j < n;
            d[q] = ok ? x[q] / z[q] : 0.0;
            t[q] = ok ? c[q] - v[q] + mu / x[q] : 0.0;
            if (j < NP) {
                const int p = G::kpos(j);
                kx[p] = ok ? x[q] : 0.0;
                kd[p] = d[q];
                kdt[p] = d[q] * t[q];
            }
        }
        wave_lds_sync();
        STAMP(1)
        double Ax, Adt;
        gram_fused(Ax, Adt);
        STAMP(2)
        rho = b - Ax;                       // primal_normal.cl:30-48
        const double rhs = Adt - rho;       // -(b - Ax - A d t), ldl.cl:198-219
        wave_lds_sync();
        double rdiag;
        {
            // pull row ri of M out of the slab; padded rows become identity rows
            double W[MP];
            const double* row = slab + ri * MS;
#pragma unroll
            for (int k = 0; k < MP; k++) W[k] = row[k];
            double diag = slab[ri * MS + ri];
            if (ri >= m) {
#pragma unroll
                for (int k = 0; k < MP; k++) W[k] = (k == ri) ? 1.0 : W[k];
                diag = 0.0;
            }
            const double beta2 = wave_max(fabs(diag));  // beta^2 = max |M_ii|, ldl.cl:280-294
            wave_lds_sync();
            STAMP(3)
            factor(W, beta2, o.pivot_floor, rdiag);
            STAMP(4)
        }
        double dy = fwd_back(rhs, rdiag);
        STAMP(5)
        At_times(dy, wv);
        STAMP(6)
#pragma unroll
        for (int q = 0; q < NC; q++) dx[q] = (t[q] - wv[q]) * d[q];   // primal_normal.cl:142
        nref = 0;
        for (;;) {
            const double e = rho - A_times(dx);
            const double maxe = wave_max(fabs(e));
            STAMP(7)
            if (!(maxe > etol) || nref >= o.max_refine) break;
            const double eta = fwd_back(e, rdiag);
            double w2[NC];
            At_times(eta, w2);
#pragma unroll
            for (int q = 0; q < NC; q++) {
                dx[q] = fma(d[q], w2[q], dx[q]);
                wv[q] -= w2[q];
            }
            dy -= eta;
            nref++;
        }
        return dy;
    }
};

// ------------------------------------------------------------------------------------------------
// stand-alone Newton step kernel: solve_primal_normal (ldl.cl:602-653) as launched by the reference's
// tests/test_ldl.py:219-273
// ------------------------------------------------------------------------------------------------
template <int MP, int NP>
__global__ void __launch_bounds__(512)
newton_kernel(int m, int n, long B, const double* __restrict__ pack, const double* __restrict__ xg,
              const double* __restrict__ zg, const double* __restrict__ yg, const double* __restrict__ bg,
              const double* __restrict__ cg, double mu, double* __restrict__ dyg, int* __restrict__ nrefg,
              DevOpts o) {
    using G = Geo<MP, NP>;
    constexpr int NC = G::NC;
    extern __shared__ __attribute__((aligned(16))) double lds[];
    const int tid = threadIdx.x;
    const int wpb = blockDim.x / WAVE;
    for (int i = tid; i < G::APACK; i += blockDim.x) lds[i] = pack[i];
    __syncthreads();
    Wave<MP, NP> w;
    const int wave = tid / WAVE;
    w.lane = tid & 63;
    w.ri = w.lane & (MP - 1);
    w.m = m; w.n = n;
    w.Amf = lds;
    w.Arm = lds + G::AMF;
    w.slab = lds + G::APACK + wave * G::WSLAB;
    w.kx = w.slab + MP * G::MS;
    w.kd = w.kx + NP;
    w.kdt = w.kd + NP;
    const int lane = w.lane, ri = w.ri;
    for (long lp = (long)blockIdx.x * wpb + wave; lp < B; lp += (long)gridDim.x * wpb) {
        double x[NC], z[NC], c[NC], v[NC], dx[NC], wv[NC];
#pragma unroll
        for (int q = 0; q < NC; q++) {
            const int j = lane + 64 * q;
            const bool ok = j < n;
            x[q] = ok ? xg[lp * n + j] : 1.0;
            z[q] = ok ? zg[lp * n + j] : 1.0;
            c[q] = ok ? cg[lp * n + j] : 0.0;
        }
        const double b = (ri < m) ? bg[lp * m + ri] : 0.0;
        const double y = (ri < m) ? yg[lp * m + ri] : 0.0;
        w.At_times(y, v);
        const double etol = o.refine_tol * (1.0 + sqrt(wave_sum((lane < MP) ? b * b : 0.0)));
        double rho;
        int nref;
#ifdef PYCLLP_PROFILE
        unsigned long long t_prev_ = 0, t_acc_[NPHASE] = {0};
#endif
        const double dy = w.newton(x, z, c, v, b, mu, etol, o, dx, wv, rho, nref STAMP_PASS);
        if (lane < MP && ri < m) dyg[lp * m + ri] = dy;
        if (nrefg && lane == 0) nrefg[lp] = nref;
    }
}

#include "ipm_group.inc"

// ------------------------------------------------------------------------------------------------
// setup kernel of a handle: the Gram matrix and A x of an LP's first iteration (x = z = 1), which depend on A, m and n alone.
// One workgroup of one wave runs gram_one<true> -- the very device function ipm_group_kernel would run on that pass -- on a
// zeroed slab with x and d staged as that kernel stages them, and writes the image GWave::gram_first reads: the slab, then A x by
// row.  (The slack columns' diagonal term is not in it: the solve kernel adds d_slack behind either route, as it did.)
// ------------------------------------------------------------------------------------------------
template <int MP, int NP, bool SL>
__global__ void __launch_bounds__(64)
first_gram_kernel(int m, int n, const double* __restrict__ Ag, double* __restrict__ img) {
    using G_ = GeoG<MP, NP, SL>;
    using W_ = GWave<MP, NP, SL>;
    constexpr int NCD = G_::NCD, ND = G_::ND, AS = G_::AS;
    const int nd = SL ? n - m : n;
    extern __shared__ __attribute__((aligned(16))) double lds[];
    const int lane = threadIdx.x, gl = lane & (MP - 1), grp = lane / MP;
    for (int i = lane; i < G_::AIMG; i += WAVE) {
        const int r = i / AS, cidx = i % AS;
        lds[i] = (r < m && cidx < nd) ? Ag[(size_t)r * n + cidx] : 0.0;
    }
    G_::fill_gram_table(lds, lane, WAVE);
    W_ w;
    w.lane = lane; w.gl = gl; w.grp = grp; w.m = m; w.n = n;
    w.Aimg = lds;
    w.slab0 = lds + G_::SHARED;
    w.slab = w.slab0 + grp * G_::SLAB;
    w.stage = w.slab0 + G_::G * G_::SLAB;
    for (int i = lane; i < G_::G * G_::SLAB; i += WAVE) w.slab0[i] = 0.0;
    // x = 1 and d = x * fast_rcp(z) of the start, formed as the solve kernel forms them (from values the compiler cannot fold)
    double one = 1.0;
    asm volatile("" : "+v"(one));
    const double d1 = one * fast_rcp(one);
    if (grp == 0) {
#pragma unroll
        for (int q = 0; q < NCD; q++) {
            const bool okq = gl + MP * q < nd;
            const int p = G_::kpos(gl + MP * q);
            w.stage[p] = okq ? one : 0.0;
            w.stage[ND + p] = okq ? d1 : 0.0;
            w.stage[2 * ND + p] = 0.0;
        }
    }
    __syncthreads();
    double ax = 0.0, ad;
    w.template gram_one<true>(0, ax, ad);
    wave_lds_sync();
    for (int i = lane; i < G_::SLAB; i += WAVE) img[i] = w.slab0[i];
    if (W_::FIRST_SLAB > G_::SLAB && lane == 0) img[G_::SLAB] = 0.0;
    if (lane < MP) img[W_::FIRST_SLAB + lane] = ax;
}

#include "ipm_group_hsd.inc"
#include "ipm_group_slot.inc"
#include "group_pa.h"
#include "ipm_block.inc"

// ------------------------------------------------------------------------------------------------
// host side: launch plans, launchers and their tables (dense_tab.h); the handle and the C ABI are abi_dense.hip's
// ------------------------------------------------------------------------------------------------
// newton_kernel: up to eight waves per workgroup, two workgroups per CU where the LDS takes them
template <int MP, int NP>
static LaunchPlan plan_newton(const DeviceLimits& d, long B, const DevOpts&) {
    using G = Geo<MP, NP>;
    int wpb = 8;
    while (wpb > 1 && G::lds_bytes(wpb) > (size_t)d.max_lds) wpb >>= 1;
    const long resident = (long)d.num_cu * ((size_t)d.max_lds / G::lds_bytes(wpb) >= 2 ? 2 : 1);
    return LaunchPlan{resident_blocks(B, wpb, resident), wpb * WAVE, (int)G::lds_bytes(wpb), MP, NP, 0};
}

template <int MP, int NP>
static hipError_t launch_pack(int m, int n, const double* A, double* pack, hipStream_t st) {
    using G = Geo<MP, NP>;
    const int threads = 256, blocks = (G::APACK + threads - 1) / threads;
    hipLaunchKernelGGL((pack_A_kernel<MP, NP>), dim3(blocks), dim3(threads), 0, st, m, n, A, pack);
    return hipGetLastError();
}

// Launch plan of a lane-group kernel on GeoG<MP, NP, SL>, starting from WPB waves per workgroup (as many as its launch bounds
// allow) and stepping down until the LDS takes them; then the small-batch rule (host.h)
template <int MP, int NP, bool SL, int WPB>
static LaunchPlan plan_group(const DeviceLimits& d, long B, const DevOpts& o) {
    using G = GeoG<MP, NP, SL>;
    int wpb = WPB;
    while (wpb > 1 && G::lds_bytes(wpb) > (size_t)d.max_lds) wpb--;
    const long resident = resident_cus(d, o);
    wpb = small_batch_wpb(B, resident, G::G, wpb);
    return LaunchPlan{resident_blocks(B, wpb, resident), wpb * WAVE, (int)G::lds_bytes(wpb), MP, NP, SL ? 1 : 0};
}

// Launch plan of the lane-group kernel for per-problem dense A (ipm_group_slot.inc, compiled in ipm_group_pa.hip): nothing is
// shared between waves there, every wave needs GeoPA::PW doubles (its G matrix areas + GeoG::WSZ), and one workgroup per CU
// holds as many waves as the LDS takes -- at most GeoPA::WPB_MAX, what the kernel's launch bounds allow.  The small-batch rule
// is plan_group's.  CAP: the most waves per workgroup; ipm_bounded_pa_kernel (bounds on per-problem A) has fewer than WPB_MAX.
template <int MP, int NP, bool SL, int CAP = GeoPA<GeoG<MP, NP, SL>>::WPB_MAX>
static LaunchPlan plan_group_pa(const DeviceLimits& d, long B, const DevOpts& o) {
    using P = GeoPA<GeoG<MP, NP, SL>>;
    static_assert(CAP >= 1 && CAP <= P::WPB_MAX, "the cap lies within what the LDS takes");
    int wpb = CAP;
    while (wpb > 1 && P::lds_bytes(wpb) > (size_t)d.max_lds) wpb--;
    const long resident = resident_cus(d, o);
    wpb = small_batch_wpb(B, resident, P::G, wpb);
    return LaunchPlan{resident_blocks(B, wpb, resident), wpb * WAVE, (int)P::lds_bytes(wpb), MP, NP, SL ? 1 : 0};
}

template <int MP, int NP, bool SL, bool HSD = false, bool PC = false, bool FULL = false>
static hipError_t launch_solve_group(const GroupPaArgs& a, const LaunchPlan& p, DevOpts o, hipStream_t st) {
    if constexpr (HSD) {
        auto kernel = hsd_group_kernel<MP, NP, SL>;
        const hipError_t e = set_dyn_lds((const void*)kernel, p.lds);
        if (e != hipSuccess) return e;
        hipLaunchKernelGGL(kernel, dim3(p.grid), dim3(p.block), p.lds, st, a.m, a.n, a.B, a.A, a.b, a.c, a.x, a.y, a.z, a.pobj,
                           a.dobj, a.status, a.iters, a.queue, o);
    } else {
        auto kernel = ipm_group_kernel<MP, NP, SL, PC, FULL>;
        const hipError_t e = set_dyn_lds((const void*)kernel, p.lds);
        if (e != hipSuccess) return e;
        hipLaunchKernelGGL(kernel, dim3(p.grid), dim3(p.block), p.lds, st, a.m, a.n, a.B, a.A, a.b, a.c, a.x, a.y, a.z, a.pobj,
                           a.dobj, a.status, a.iters, a.queue, o, a.first);
    }
    return hipGetLastError();
}

// first_gram_kernel on GeoG<MP, NP, SL>: the image (first_len doubles) of a handle's A for ipm_group_kernel<MP, NP, SL, ...>
template <int MP, int NP, bool SL>
static hipError_t launch_first_gram(int m, int n, const double* A, double* img, hipStream_t st) {
    using G = GeoG<MP, NP, SL>;
    auto kernel = first_gram_kernel<MP, NP, SL>;
    const int lds = (int)(sizeof(double) * (size_t)(G::SHARED + G::WSZ));
    const hipError_t e = set_dyn_lds((const void*)kernel, lds);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(kernel, dim3(1), dim3(WAVE), lds, st, m, n, A, img);
    return hipGetLastError();
}
// ... or { 0, null } for a shape whose kernels do not read one (GWave::FIRST_IMAGE)
template <int MP, int NP, bool SL>
constexpr FirstGram first_gram_of() {
    if constexpr (GWave<MP, NP, SL>::FIRST_IMAGE) return FirstGram{GWave<MP, NP, SL>::FIRST_LEN, launch_first_gram<MP, NP, SL>};
    else return FirstGram{0, nullptr};
}
#define FIRST_GRAM(MP, NP, SL) first_gram_of<MP, NP, SL>()

// The full-shape instantiation of the plain slack-aware kernel (ipm_group_kernel's FULL, for an LP with m = MP and n = NP: no
// padded column), launched on the generic instantiation's plan (same geometry).  A shape whose full-shape kernel had scratch
// or a spilt VGPR, or was slower than the generic one, would get a null launcher, which abi_dense.hip skips, and be named
// here: none (tools/kernel_resources.py, profiles/full_shape).
template <int MP, int NP>
constexpr dense_launch_fn full_group_kernel() { return launch_solve_group<MP, NP, true, false, false, true>; }

// the bounded slack-aware kernel (ipm_group_slot.inc): planned with PYCLLP_WPB_BOUNDED waves per workgroup
template <int MP, int NP>
static hipError_t launch_solve_bounded(const GroupPaArgs& a, const LaunchPlan& p, DevOpts o, hipStream_t st) {
    auto kernel = ipm_bounded_kernel<MP, NP>;
    const hipError_t e = set_dyn_lds((const void*)kernel, p.lds);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(kernel, dim3(p.grid), dim3(p.block), p.lds, st, a.m, a.n, a.B, a.A, a.b, a.c, a.u, a.x, a.y, a.z, a.s,
                       a.pobj, a.dobj, a.status, a.iters, a.queue, o);
    return hipGetLastError();
}

template <int MP, int NP>
static hipError_t launch_newton(const NewtonArgs& a, const LaunchPlan& p, DevOpts o, hipStream_t st) {
    const hipError_t e = set_dyn_lds((const void*)newton_kernel<MP, NP>, p.lds);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL((newton_kernel<MP, NP>), dim3(p.grid), dim3(p.block), p.lds, st, a.m, a.n, a.B, a.pack, a.x, a.z, a.y,
                       a.b, a.c, a.mu, a.dy, a.nref, o);
    return hipGetLastError();
}

#define GROUP_KERNEL(MP, NP, SL, HSD, PC) \
    { plan_group<MP, NP, SL, (HSD) ? hsd_wpb<MP>() : PYCLLP_WPB>, launch_solve_group<MP, NP, SL, HSD, PC> }
#define VARIANT(MP, NP) \
    { MP, NP, Geo<MP, NP>::APACK, launch_pack<MP, NP>, GROUP_KERNEL(MP, NP, false, false, false), \
      GROUP_KERNEL(MP, NP, false, true, false), GROUP_KERNEL(MP, NP, false, false, true), plan_newton<MP, NP>, launch_newton<MP, NP>, \
      FIRST_GRAM(MP, NP, false) },
#define SLACK_VARIANT(MP, NP) \
    { MP, NP, GROUP_KERNEL(MP, NP, true, false, false), GROUP_KERNEL(MP, NP, true, true, false), \
      GROUP_KERNEL(MP, NP, true, false, true), { plan_group<MP, NP, true, PYCLLP_WPB_BOUNDED>, launch_solve_bounded<MP, NP> }, \
      full_group_kernel<MP, NP>(), FIRST_GRAM(MP, NP, true), \
      { plan_group<MP, NP, true, PYCLLP_WPB_BOUNDED>, bounded_hsd_launcher<MP, NP>() } },
#define PA_PLAN(MP, NP) { MP, NP, 0, plan_group_pa<MP, NP, false> }, { MP, NP, 1, plan_group_pa<MP, NP, true> },
// ... with upper bounds: the same rule, at most PYCLLP_WPB_BOUNDED waves per workgroup
#define PABD_PLAN(MP, NP) { MP, NP, 1, plan_group_pa<MP, NP, true, GeoPA<GeoG<MP, NP, true>>::wpb_capped(PYCLLP_WPB_BOUNDED)> },

// The tables of dense_tab.h.  The device pass gets file-local copies: they are never emitted, but referencing the launchers is
// what makes the kernels get instantiated (as in ipm_group_pa.hip).
#ifdef __HIP_DEVICE_COMPILE__
namespace {
#endif
[[maybe_unused]] const Variant kVariants[] = { GROUP_SHAPES(VARIANT) };
[[maybe_unused]] const SlackVariant kSlackVariants[] = { GROUP_SHAPES(SLACK_VARIANT) };
[[maybe_unused]] const PaPlan kPaPlans_v[] = { GROUP_SHAPES(PA_PLAN) };
[[maybe_unused]] const PaPlan kPaBdPlans_v[] = { GROUP_SHAPES(PABD_PLAN) };
#ifdef __HIP_DEVICE_COMPILE__
}
#else
const int kNumVariants = sizeof(kVariants) / sizeof(kVariants[0]);
const int kNumSlackVariants = sizeof(kSlackVariants) / sizeof(kSlackVariants[0]);
const PaPlans kPaPlans = { kPaPlans_v, (int)(sizeof(kPaPlans_v) / sizeof(kPaPlans_v[0])) };
const PaPlans kPaBdPlans = { kPaBdPlans_v, (int)(sizeof(kPaBdPlans_v) / sizeof(kPaBdPlans_v[0])) };
#endif

// ------------------------------------------------------------------------------------------------
// the block kernel of the sparse path (ipm_block.inc) behind the launch functions of block.h.  It is compiled here and not in
// ipm_block.hip because the backend turns the same optimised IR into other machine code depending on the unit around it:
// 11 208 instructions here, with deferred_to_numerical_kernel behind it as in every earlier build (without it: 11 161), but
// 11 144 in a unit with the LDL' kernels alone.  abi_sparse.hip owns the handle and the launch plan.
// ------------------------------------------------------------------------------------------------
hipError_t block_set_lds(int lds) { return set_dyn_lds((const void*)ipm_block_kernel, lds); }

hipError_t block_launch_solve(const BlockA& A, long blocks, int lds, long B, const double* b, const double* c, double* x, double* y,
                              double* z, double* pobj, double* dobj, int* status, int* iters, int* qhead, const int* worklist,
                              const double* a_batch, DevOpts o, hipStream_t st) {
    hipLaunchKernelGGL(ipm_block_kernel, dim3((unsigned)blocks), dim3(BLK_T), lds, st, A, B, b, c, x, y, z, pobj, dobj, status,
                       iters, qhead, worklist, 0.0, nullptr, nullptr, a_batch, o);
    return hipGetLastError();
}

hipError_t block_launch_newton(const BlockA& A, long blocks, int lds, long B, const double* x, const double* z, const double* y,
                               const double* b, const double* c, double mu, double* dy, int* nref, int* qhead, DevOpts o,
                               hipStream_t st) {
    hipLaunchKernelGGL(ipm_block_kernel, dim3((unsigned)blocks), dim3(BLK_T), lds, st, A, B, b, c, (double*)x, (double*)y,
                       (double*)z, (double*)nullptr, (double*)nullptr, (int*)nullptr, (int*)nullptr, qhead, (const int*)nullptr, mu,
                       dy, nref, (const double*)nullptr, o);
    return hipGetLastError();
}

// LPs the wave kernel deferred (status -1) when no guarded kernel can take them: PYCLLP_STATUS_NUMERICAL
__global__ void deferred_to_numerical_kernel(const int* __restrict__ worklist, int* __restrict__ status) {
    const int n = worklist[0];
    for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) status[worklist[1 + i]] = PYCLLP_STATUS_NUMERICAL;
}

hipError_t block_launch_deferred_to_numerical(const int* worklist, int* status, hipStream_t st) {
    hipLaunchKernelGGL(deferred_to_numerical_kernel, dim3(64), dim3(256), 0, st, worklist, status);
    return hipGetLastError();
}
