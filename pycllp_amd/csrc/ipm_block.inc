// ipm_block.inc -- sparse shared-A path: one LP per WORKGROUP (256 threads), for LPs too large for a lane group.
//
// Replaces the reference's sparse twins: host ClSparsePrimalNormalSolver (pycllp/solvers/cl.py:127-278) and the
// kernels sparse_standard_primal_normal (pycllp/cl/primal_normal.cl:287-375), sparse_primal_normal_step (:158-198),
// sparse_*_infeasibility (:50-74, :96-120), sparse_AXZAt_ij/_ii (pycllp/cl/ldl.cl:140-196), sparse_primal_normal_rhs_i
// (:221-257), sparse_factor_primal_normal (:381-502), sparse_forward_backward_primal_normal (:540-574),
// sparse_solve_primal_normal (:656-712); BASELINE config 5 (m=128, N=384, density 0.025).
//
// Design: A is held in CSR and CSC form (in LDS when it fits, else read through L2); the Gram matrix
// M = A diag(x/z) A' is assembled from a term list prepared once at init (for every structurally non-zero entry
// (i,k) of M the products a_ij a_kj and their column j: deterministic, no atomics, nnz-proportional work); M and
// its factor live in LDS as a PACKED lower triangle (m(m+1)/2 f64, 66 KB at m=128) and are treated as dense --
// where the reference keeps L on a fixed CSR pattern derived from a numeric Cholesky of A A' (cl.py:186-196), which
// can drop structurally non-zero entries, this path takes whatever fill occurs.  N-vectors live in registers
// (thread = column), m-vectors in LDS.  The triangular solves run inside one wavefront (readlane broadcasts, no
// workgroup barriers).  Semantics = oracle/ipm_dense_ref.c, including the x-space refinement (the reference's
// sparse solve has its refinement commented out, ldl.cl:698-711).
// (BLK_T, BLK_MAX_M, BLK_MAX_N and BlockA, the device-side description of the shared constraint matrix: block.h)
#define BLK_NC (BLK_MAX_N / BLK_T)

__device__ __forceinline__ int tri_idx(int i, int k) { return i * (i + 1) / 2 + k; }

// block-wide reductions (4 waves) through a small LDS scratch; every thread gets the result
__device__ __forceinline__ double blk_sum(double v, double* red, int tid) {
    v = wave_sum(v);
    __syncthreads();
    if ((tid & 63) == 0) red[tid >> 6] = v;
    __syncthreads();
    return (red[0] + red[1]) + (red[2] + red[3]);
}
__device__ __forceinline__ double blk_max(double v, double* red, int tid) {
    v = wave_max(v);
    __syncthreads();
    if ((tid & 63) == 0) red[tid >> 6] = v;
    __syncthreads();
    return fmax(fmax(red[0], red[1]), fmax(red[2], red[3]));
}

__global__ void __launch_bounds__(BLK_T, 2)
ipm_block_kernel(BlockA A, long B, const double* __restrict__ bg, const double* __restrict__ cg,
                 double* __restrict__ xg, double* __restrict__ yg, double* __restrict__ zg, double* __restrict__ pobj,
                 double* __restrict__ dobj, int* __restrict__ status, int* __restrict__ iters, int* __restrict__ queue,
                 const int* __restrict__ worklist, double nwt_mu, double* __restrict__ nwt_dy, int* __restrict__ nwt_nref,
                 const double* __restrict__ a_batch, DevOpts o) {
    // nwt_dy != nullptr: stand-alone Newton step (sparse_solve_primal_normal, ldl.cl:656-712): x, z, y are INPUTS, mu is
    // nwt_mu, one pass of the Newton machinery below runs and dy (+ refinement passes used) is all that is stored
    // worklist != nullptr: solve only the LPs worklist[1 .. worklist[0]] (those the register-resident wave kernel deferred
    // because the Nocedal-Wright guard would have bitten); an empty list ends the workgroup before it stages anything
    if (worklist && worklist[0] <= 0) return;
    extern __shared__ __attribute__((aligned(16))) double lds[];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int m = A.m, n = A.n;
    const int ntri = m * (m + 1) / 2;
    const int mp = (m + 7) & ~7;           // m-vectors are padded to whole 8-row tiles (and stay 16-byte aligned)
    // ---- LDS carve-up (the host sizes it by block_lds_bytes, block.h: an upper bound of what follows) ----
    double* M = lds;                       // packed lower triangle, then L (unit diagonal implicit) in place
    double* vx = M + ((ntri + 1) & ~1);    // [n] staging of an N-vector (x, d*t, dx) for the CSR products
    double* vd = vx + ((n + 1) & ~1);      // [n] d = x/z for the Gram assembly
    double* ys = vd + ((n + 1) & ~1);      // [mp] y
    double* bs = ys + mp;                  // [mp] b
    double* rho = bs + mp;                 // [mp] b - A x
    double* sv = rho + mp;                 // [mp] solve vector
    double* dy = sv + mp;                  // [mp]
    double* ucol = dy + mp;                // [mp] raw pivot column
    double* rdg = ucol + mp;               // [mp] 1/D
    double* red = rdg + mp;                // [8] reduction scratch + broadcast slots
    double* tail = red + 8;
    const double* csr_val = A.csr_val; const int* csr_ptr = A.csr_ptr; const int* csr_col = A.csr_col;
    const double* csc_val = A.csc_val; const int* csc_ptr = A.csc_ptr; const int* csc_row = A.csc_row;
    double* lv = tail;                          // csr_val[nnz], csc_val[nnz] when A.a_in_lds
    const bool pa = a_batch != nullptr;         // per-problem values of A: reloaded into lv for every LP (host ensures a_in_lds)
    if (A.a_in_lds) {
        int* li = (int*)(lv + 2 * A.nnz);       // csr_col[nnz], csc_row[nnz], csr_ptr[m+1], csc_ptr[n+1]
        for (int e = tid; e < A.nnz; e += BLK_T) {
            lv[e] = A.csr_val[e]; lv[A.nnz + e] = A.csc_val[e];
            li[e] = A.csr_col[e]; li[A.nnz + e] = A.csc_row[e];
        }
        for (int e = tid; e <= m; e += BLK_T) li[2 * A.nnz + e] = A.csr_ptr[e];
        for (int e = tid; e <= n; e += BLK_T) li[2 * A.nnz + m + 1 + e] = A.csc_ptr[e];
        csr_val = lv; csc_val = lv + A.nnz; csr_col = li; csc_row = li + A.nnz;
        csr_ptr = li + 2 * A.nnz; csc_ptr = li + 2 * A.nnz + m + 1;
    }
    __syncthreads();

    const bool nwt = nwt_dy != nullptr;
    const bool warm = nwt || (o.flags & PYCLLP_FLAG_WARM_START) != 0;
    const bool autoscale = !nwt && (o.flags & PYCLLP_FLAG_AUTOSCALE) != 0;
    // PYCLLP_FLAG_HSD: the homogeneous self-dual embedding of oracle hsd_one_raw() / csrc/ipm_group_hsd.inc on this kernel's
    // machinery (two solves with one factor, tau and kappa as workgroup-uniform scalars)
    const bool hsd = !nwt && (o.flags & PYCLLP_FLAG_HSD) != 0;
    const double eta = 1.0 - o.delta, einf = 100.0 * o.eps;
    const double nm = (double)(n + m);
    STAMP_DECL

    // A'u for this thread's columns, u in LDS
    auto At_cols = [&](const double* u, double (&out)[BLK_NC]) {
#pragma unroll
        for (int q = 0; q < BLK_NC; q++) {
            const int j = tid + BLK_T * q;
            double acc = 0.0;
            if (j < n) for (int p = csc_ptr[j]; p < csc_ptr[j + 1]; p++) acc = fma(csc_val[p], u[csc_row[p]], acc);
            out[q] = acc;
        }
    };
    // (A v)_i for row i = tid (< m), v in LDS
    auto A_row = [&](const double* v) {
        double acc = 0.0;
        if (tid < m) for (int p = csr_ptr[tid]; p < csr_ptr[tid + 1]; p++) acc = fma(csr_val[p], v[csr_col[p]], acc);
        return acc;
    };
    // sv <- (L D L')^-1 sv, inside wave 0: lane owns rows lane and lane+64; column-oriented substitution with
    // readlane broadcasts (no workgroup barrier inside)
    auto solve_in_wave0 = [&]() {
        if (wave == 0) {
            const int i0 = lane, i1 = lane + 64;
            double s0 = (i0 < m) ? sv[i0] : 0.0, s1 = (i1 < m) ? sv[i1] : 0.0;
            // The factor entries of 8 steps are fetched together, then the 8 dependent steps run out of registers.
            // Columns < 64 broadcast from the first register of each lane, columns >= 64 from the second.
            const int mlo = m < 64 ? m : 64;
            for (int k0 = 0; k0 < mlo; k0 += 8) {             // forward, columns 0..63: t_i -= L[i][k] t_k
                double l0[8], l1[8];
#pragma unroll
                for (int kk = 0; kk < 8; kk++) {
                    const int k = k0 + kk;
                    l0[kk] = (i0 > k && i0 < m) ? M[tri_idx(i0, k)] : 0.0;
                    l1[kk] = (k < m && i1 < m) ? M[tri_idx(i1, k)] : 0.0;
                }
#pragma unroll
                for (int kk = 0; kk < 8; kk++) {
                    const double tk = readlane_d(s0, k0 + kk);
                    s0 = fma(-l0[kk], tk, s0);
                    s1 = fma(-l1[kk], tk, s1);
                }
            }
            for (int k0 = 64; k0 < m; k0 += 8) {              // forward, columns 64..m-1 (rows >= 64 only)
                double l1[8];
#pragma unroll
                for (int kk = 0; kk < 8; kk++) {
                    const int k = k0 + kk;
                    l1[kk] = (i1 > k && i1 < m) ? M[tri_idx(i1, k)] : 0.0;
                }
#pragma unroll
                for (int kk = 0; kk < 8; kk++) s1 = fma(-l1[kk], readlane_d(s1, k0 + kk - 64), s1);
            }
            if (i0 < m) s0 *= rdg[i0];
            if (i1 < m) s1 *= rdg[i1];
            for (int c0 = ((m - 1) & ~7); c0 >= 64; c0 -= 8) {   // backward, rows i >= 64: s_j -= L[i][j] s_i, j < i
                double l0[8], l1[8];
#pragma unroll
                for (int kk = 0; kk < 8; kk++) {
                    const int i = c0 + kk;
                    l0[kk] = (i < m && i0 < m) ? M[tri_idx(i, i0)] : 0.0;
                    l1[kk] = (i < m && i1 < i) ? M[tri_idx(i, i1)] : 0.0;
                }
#pragma unroll
                for (int kk = 7; kk >= 0; kk--) {
                    const double si = readlane_d(s1, c0 + kk - 64);
                    s0 = fma(-l0[kk], si, s0);
                    s1 = fma(-l1[kk], si, s1);
                }
            }
            for (int c0 = ((mlo - 1) & ~7); c0 >= 0; c0 -= 8) {  // backward, rows i < 64 (columns < 64 only)
                double l0[8];
#pragma unroll
                for (int kk = 0; kk < 8; kk++) {
                    const int i = c0 + kk;
                    l0[kk] = (i < mlo && i0 < i) ? M[tri_idx(i, i0)] : 0.0;
                }
#pragma unroll
                for (int kk = 7; kk >= 0; kk--) s0 = fma(-l0[kk], readlane_d(s0, c0 + kk), s0);
            }
            if (i0 < m) sv[i0] = s0;
            if (i1 < m) sv[i1] = s1;
        }
        __syncthreads();
    };
    // the same for TWO right-hand sides at once (HSD: p in `pa`, q in `sv`): one pass over the factor, two independent
    // dependency chains that fill each other's latency gaps
    auto solve2_in_wave0 = [&](double* pa) {
        if (wave == 0) {
            const int i0 = lane, i1 = lane + 64;
            double s0 = (i0 < m) ? sv[i0] : 0.0, s1 = (i1 < m) ? sv[i1] : 0.0;
            double t0 = (i0 < m) ? pa[i0] : 0.0, t1 = (i1 < m) ? pa[i1] : 0.0;
            const int mlo = m < 64 ? m : 64;
            for (int k0 = 0; k0 < mlo; k0 += 8) {
                double l0[8], l1[8];
#pragma unroll
                for (int kk = 0; kk < 8; kk++) {
                    const int k = k0 + kk;
                    l0[kk] = (i0 > k && i0 < m) ? M[tri_idx(i0, k)] : 0.0;
                    l1[kk] = (k < m && i1 < m) ? M[tri_idx(i1, k)] : 0.0;
                }
#pragma unroll
                for (int kk = 0; kk < 8; kk++) {
                    const double sk = readlane_d(s0, k0 + kk), tk = readlane_d(t0, k0 + kk);
                    s0 = fma(-l0[kk], sk, s0); t0 = fma(-l0[kk], tk, t0);
                    s1 = fma(-l1[kk], sk, s1); t1 = fma(-l1[kk], tk, t1);
                }
            }
            for (int k0 = 64; k0 < m; k0 += 8) {
                double l1[8];
#pragma unroll
                for (int kk = 0; kk < 8; kk++) {
                    const int k = k0 + kk;
                    l1[kk] = (i1 > k && i1 < m) ? M[tri_idx(i1, k)] : 0.0;
                }
#pragma unroll
                for (int kk = 0; kk < 8; kk++) {
                    const double sk = readlane_d(s1, k0 + kk - 64), tk = readlane_d(t1, k0 + kk - 64);
                    s1 = fma(-l1[kk], sk, s1); t1 = fma(-l1[kk], tk, t1);
                }
            }
            if (i0 < m) { s0 *= rdg[i0]; t0 *= rdg[i0]; }
            if (i1 < m) { s1 *= rdg[i1]; t1 *= rdg[i1]; }
            for (int c0 = ((m - 1) & ~7); c0 >= 64; c0 -= 8) {
                double l0[8], l1[8];
#pragma unroll
                for (int kk = 0; kk < 8; kk++) {
                    const int i = c0 + kk;
                    l0[kk] = (i < m && i0 < m) ? M[tri_idx(i, i0)] : 0.0;
                    l1[kk] = (i < m && i1 < i) ? M[tri_idx(i, i1)] : 0.0;
                }
#pragma unroll
                for (int kk = 7; kk >= 0; kk--) {
                    const double si = readlane_d(s1, c0 + kk - 64), ti = readlane_d(t1, c0 + kk - 64);
                    s0 = fma(-l0[kk], si, s0); t0 = fma(-l0[kk], ti, t0);
                    s1 = fma(-l1[kk], si, s1); t1 = fma(-l1[kk], ti, t1);
                }
            }
            for (int c0 = ((mlo - 1) & ~7); c0 >= 0; c0 -= 8) {
                double l0[8];
#pragma unroll
                for (int kk = 0; kk < 8; kk++) {
                    const int i = c0 + kk;
                    l0[kk] = (i < mlo && i0 < i) ? M[tri_idx(i, i0)] : 0.0;
                }
#pragma unroll
                for (int kk = 7; kk >= 0; kk--) {
                    const double si = readlane_d(s0, c0 + kk), ti = readlane_d(t0, c0 + kk);
                    s0 = fma(-l0[kk], si, s0); t0 = fma(-l0[kk], ti, t0);
                }
            }
            if (i0 < m) { sv[i0] = s0; pa[i0] = t0; }
            if (i1 < m) { sv[i1] = s1; pa[i1] = t1; }
        }
        __syncthreads();
    };

    for (;;) {
        // ---- next LP from the device-wide queue ----
        __syncthreads();
        if (tid == 0) {
            int nx = atomicAdd(queue, 1);
            if (worklist) nx = (nx < worklist[0]) ? worklist[1 + nx] : 0x7fffffff;
            ((int*)red)[14] = nx;
        }
        __syncthreads();
        const long lp = ((int*)red)[14];
        if (lp >= B) break;
        if (pa) {   // this LP's values of A: HBM -> LDS, by rows and (through csc_src) by columns
            for (int e = tid; e < A.nnz; e += BLK_T) {
                lv[e] = a_batch[lp * A.nnz + e];
                lv[A.nnz + e] = a_batch[lp * A.nnz + A.csc_src[e]];
            }
            __syncthreads();
        }

        double x[BLK_NC], z[BLK_NC], c[BLK_NC];
        bool ok[BLK_NC];
#pragma unroll
        for (int q = 0; q < BLK_NC; q++) {
            const int j = tid + BLK_T * q;
            ok[q] = j < n;
            c[q] = ok[q] ? cg[lp * n + j] : 0.0;
            x[q] = (warm && ok[q]) ? xg[lp * n + j] : 1.0;
            z[q] = (warm && ok[q]) ? zg[lp * n + j] : 1.0;
        }
        if (tid < m) {
            bs[tid] = bg[lp * m + tid];
            ys[tid] = (warm && yg) ? yg[lp * m + tid] : (hsd ? 0.0 : 1.0);
        }
        __syncthreads();
        double sb = 1.0, sc = 1.0;
        if (autoscale) {   // solve with b/max|b| and c/max|c| (PYCLLP_FLAG_AUTOSCALE); undone when storing
            double cm = 0.0;
#pragma unroll
            for (int q = 0; q < BLK_NC; q++) cm = fmax(cm, fabs(c[q]));
            sb = blk_max((tid < m) ? fabs(bs[tid]) : 0.0, red, tid);
            sc = blk_max(cm, red, tid);
            const bool scaled = autoscale_lp(o.flags, sb, sc, 0.0);   // (an LP the wave kernel deferred: the verdict it had there)
            sb = (scaled && sb > 0.0) ? sb : 1.0; sc = (scaled && sc > 0.0) ? sc : 1.0;
            if (tid < m) { bs[tid] = bs[tid] / sb; if (warm) ys[tid] = ys[tid] / sc; }
#pragma unroll
            for (int q = 0; q < BLK_NC; q++) {
                c[q] = c[q] / sc;
                if (warm) { x[q] = x[q] / sb; z[q] = z[q] / sc; }
            }
            __syncthreads();
        }
        double c2 = 0.0;
#pragma unroll
        for (int q = 0; q < BLK_NC; q++) c2 = fma(c[q], c[q], c2);
        const double nb2 = blk_sum((tid < m) ? bs[tid] * bs[tid] : 0.0, red, tid);
        const double nc2 = blk_sum(c2, red, tid);
        const double tol_r = o.eps * (1.0 + sqrt(nb2)), tol_s = o.eps * (1.0 + sqrt(nc2));
        const double etol = o.refine_tol * (1.0 + sqrt(nb2));
        const double nbn = sqrt(nb2), ncn = sqrt(nc2);
        double tau = 1.0, kap = 1.0;
        if (hsd && warm) {
            double g0 = 0.0;
#pragma unroll
            for (int q = 0; q < BLK_NC; q++) g0 += ok[q] ? x[q] * z[q] : 0.0;
            kap = blk_sum(g0, red, tid) / (double)n;
        }
        double normr0 = 1e300, norms0 = 1e300, po = 0.0, du = 0.0;
        int stat = PYCLLP_STATUS_ITERATION_LIMIT, it = 0;

        for (it = 0; it < o.max_iter; it++) {
            // ---- sigma, gamma, objectives ----
            double v[BLK_NC];
            At_cols(ys, v);
            double s2 = 0.0, gam = 0.0, pp = 0.0;
#pragma unroll
            for (int q = 0; q < BLK_NC; q++) {
                const double sg = ok[q] ? c[q] * tau - v[q] + z[q] : 0.0;   // tau = 1 on the plain path
                s2 = fma(sg, sg, s2);
                gam += ok[q] ? x[q] * z[q] : 0.0;
                pp += c[q] * (ok[q] ? x[q] : 0.0);
            }
            s2 = blk_sum(s2, red, tid); gam = blk_sum(gam, red, tid); po = blk_sum(pp, red, tid);
            du = blk_sum((tid < m) ? bs[tid] * ys[tid] : 0.0, red, tid);
            const double norms = sqrt(s2);
            // centering target: delta gamma/(n+m) (primal_normal.cl:272); HSD: delta (x'z + tau kappa)/(N+1)
            const double mu = nwt ? nwt_mu : (hsd ? o.delta * (gam + tau * kap) / (double)(n + 1) : o.delta * gam / nm);
            const double phi = du - po + kap;
            STAMP(0)
            // ---- d, t, staging ----
            double d[BLK_NC], t[BLK_NC];
#pragma unroll
            for (int q = 0; q < BLK_NC; q++) {
                const int j = tid + BLK_T * q;
                d[q] = ok[q] ? x[q] / z[q] : 0.0;
                // plain: t = c - A'y + mu/x;  HSD: t = r1 = mu/x - z + eta sigma
                t[q] = ok[q] ? (hsd ? fma(eta, c[q] * tau - v[q] + z[q], mu / x[q] - z[q]) : c[q] - v[q] + mu / x[q]) : 0.0;
                if (ok[q]) { vx[j] = x[q]; vd[j] = d[q]; }
            }
            for (int e = tid; e < ntri; e += BLK_T) M[e] = 0.0;
            __syncthreads();
            // ---- rho = b - A x ; Gram assembly from the term list (ldl.cl:140-196) ----
            const double Ax = A_row(vx);
            for (int e = tid; e < A.n_entries; e += BLK_T) {
                double acc = 0.0;
                for (int p = A.ent_ptr[e]; p < A.ent_ptr[e + 1]; p++)
                    acc = fma(pa ? lv[A.term_ia[p]] * lv[A.term_ib[p]] : A.term_w[p], vd[A.term_col[p]], acc);
                M[A.ent_tri[e]] = acc;
            }
            __syncthreads();
#pragma unroll
            for (int q = 0; q < BLK_NC; q++) if (ok[q]) vx[tid + BLK_T * q] = d[q] * t[q];
            __syncthreads();
            const double Adt = A_row(vx);
            STAMP(1)
            const double rho_i = (tid < m) ? bs[tid] * tau - Ax : 0.0;   // tau = 1 on the plain path
            double rp = 0.0, rq = 0.0;                                  // HSD: the two right-hand sides (M p = ., M q = .)
            if (hsd) {
                // stop tests of this point (oracle hsd_one_raw), before the factorisation
                const double normr_h = sqrt(blk_sum(rho_i * rho_i, red, tid));
                if (!(isfinite(normr_h) && isfinite(norms) && isfinite(gam) && isfinite(tau) && isfinite(kap))) { stat = PYCLLP_STATUS_NUMERICAL; break; }
                if (normr_h <= tol_r * tau && norms <= tol_s * tau && gam <= o.eps * tau * (tau + fabs(po))) { stat = PYCLLP_STATUS_OPTIMAL; break; }
                const bool p_ray = po > 0.0 && fma(nbn, tau, normr_h) <= einf * po;
                const bool d_ray = du < 0.0 && fma(ncn, tau, norms) <= einf * -du;
                if (p_ray || d_ray) {
                    stat = (p_ray && d_ray) ? ((-du > po) ? PYCLLP_STATUS_PRIMAL_INFEASIBLE : PYCLLP_STATUS_DUAL_INFEASIBLE)
                                            : (p_ray ? PYCLLP_STATUS_DUAL_INFEASIBLE : PYCLLP_STATUS_PRIMAL_INFEASIBLE);
                    break;
                }
                // M p = A(d c) - b  and  M q = A(d r1) - eta rho
                __syncthreads();
#pragma unroll
                for (int q = 0; q < BLK_NC; q++) if (ok[q]) vx[tid + BLK_T * q] = d[q] * c[q];
                __syncthreads();
                const double Adc = A_row(vx);
                if (tid < m) rho[tid] = rho_i;
                rp = (tid < m) ? Adc - bs[tid] : 0.0;
                rq = fma(-eta, rho_i, Adt);
            } else {
                if (tid < m) { rho[tid] = rho_i; sv[tid] = Adt - rho_i; }
            }
            const double beta2 = blk_max((tid < m) ? fabs(M[tri_idx(tid, tid)]) : 0.0, red, tid);   // ldl.cl:296-311
            // pivot floor of column j (primal_normal.cl:275): the reference's absolute constant, or on the HSD path
            // pivot_floor^2 |M_jj| -- relative to the pivot's own original diagonal entry (see the oracle).  The vector
            // lives in `dy`, which is idle until the solves.
            double* flr = dy;
            if (hsd) {
                if (tid < m) flr[tid] = o.pivot_floor * o.pivot_floor * fabs(M[tri_idx(tid, tid)]);
                __syncthreads();
            }
            STAMP(2)
            // ---- modified LDL' in place on the packed triangle (ldl.cl:381-502, dense fill) ----
            // Rows are dealt in balanced pairs: threads (p, q), p = tid & 63, q = tid >> 6, share rows p and m-1-p and
            // take every 4th column of their trailing updates.  guard = false: the Nocedal-Wright term is left out and
            // the sweep only records whether it would have bitten (then M is re-assembled and the sweep repeated with
            // the guard: exactly ldl.cl:487); this removes a workgroup reduction from every column.
            // Cold path (guard = true after a re-assembly of M): LDS read-modify-write sweep with the guard applied.
            auto factor = [&](bool guard) -> bool {
                const int p = tid & 63, q = tid >> 6;
                const int half = (m + 1) / 2;
                const int ra = p, rb = m - 1 - p;            // pair p < ceil(m/2): rows p and m-1-p (the middle row once)
                const bool va = p < half, vb = p < half && rb > ra;
                bool viol = false;
                for (int j = 0; j < m; j++) {
                    const double piv = M[tri_idx(j, j)];
                    const double ua = (va && ra > j) ? M[tri_idx(ra, j)] : 0.0;
                    const double ub = (vb && rb > j) ? M[tri_idx(rb, j)] : 0.0;
                    double aD = fmax(fabs(piv), hsd ? flr[j] : o.pivot_floor);
                    if (guard) {
                        const double theta = blk_max((q == 0) ? fmax(fabs(ua), fabs(ub)) : 0.0, red, tid);
                        aD = fmax(aD, theta * theta / beta2);                      // ldl.cl:487
                    } else {
                        viol = viol || (ua * ua > beta2 * aD) || (ub * ub > beta2 * aD);
                        __syncthreads();                                          // column j has been read by everyone
                    }
                    const double rD = 1.0 / aD;
                    const double la = ua * rD, lb = ub * rD;
                    if (q == 0) {
                        if (va && ra > j) { ucol[ra] = ua; M[tri_idx(ra, j)] = la; }
                        if (vb && rb > j) { ucol[rb] = ub; M[tri_idx(rb, j)] = lb; }
                    }
                    if (tid == j) rdg[j] = rD;
                    __syncthreads();
                    // rows ra < rb share the pivot-column values u_k; their loads are issued together so that one LDS
                    // round trip serves 8 FMAs
                    if (vb && rb > j) {
                        double* Ma = M + tri_idx(ra, 0);
                        double* Mb = M + tri_idx(rb, 0);
                        const int enda = (va && ra > j) ? ra : j;     // last column of row a's update (none if <= j)
                        int k = j + 1 + q;
                        for (; k + 12 <= enda; k += 16) {
                            const double u0 = ucol[k], u1 = ucol[k + 4], u2 = ucol[k + 8], u3 = ucol[k + 12];
                            const double a0 = Ma[k], a1 = Ma[k + 4], a2 = Ma[k + 8], a3 = Ma[k + 12];
                            const double b0 = Mb[k], b1 = Mb[k + 4], b2 = Mb[k + 8], b3 = Mb[k + 12];
                            Ma[k] = fma(-la, u0, a0); Ma[k + 4] = fma(-la, u1, a1); Ma[k + 8] = fma(-la, u2, a2); Ma[k + 12] = fma(-la, u3, a3);
                            Mb[k] = fma(-lb, u0, b0); Mb[k + 4] = fma(-lb, u1, b1); Mb[k + 8] = fma(-lb, u2, b2); Mb[k + 12] = fma(-lb, u3, b3);
                        }
                        for (; k <= enda; k += 4) {
                            const double u0 = ucol[k];
                            Ma[k] = fma(-la, u0, Ma[k]);
                            Mb[k] = fma(-lb, u0, Mb[k]);
                        }
                        for (; k + 28 <= rb; k += 32) {
                            double uu[8], bb[8];
#pragma unroll
                            for (int e = 0; e < 8; e++) { uu[e] = ucol[k + 4 * e]; bb[e] = Mb[k + 4 * e]; }
#pragma unroll
                            for (int e = 0; e < 8; e++) Mb[k + 4 * e] = fma(-lb, uu[e], bb[e]);
                        }
                        for (; k <= rb; k += 4) Mb[k] = fma(-lb, ucol[k], Mb[k]);
                    } else if (va && ra > j) {   // the middle row of an odd m
                        double* Ma = M + tri_idx(ra, 0);
                        for (int k = j + 1 + q; k <= ra; k += 4) Ma[k] = fma(-la, ucol[k], Ma[k]);
                    }
                    __syncthreads();
                }
                return blk_max(viol ? 1.0 : 0.0, red, tid) > 0.0;
            };
            // Hot path: BLOCKED right-looking LDL' with NB-column panels; the trailing update -- almost all of
            // the m^3/3 flops -- runs on the matrix cores (v_mfma_f64_16x16x4_f64), and there are 2 workgroup barriers per
            // PANEL instead of one per column.  Per panel kb:
            //   * every wave that owns panel rows factors the NB x NB diagonal block redundantly in registers (lane = row,
            //     broadcasts by DPP row_newbcast, as the dense group kernel does), so the panel needs no barrier;
            //   * thread = panel row: forward substitution u_c -= u_l L_kk[c][l] (right-looking order: the updates of one
            //     step are independent, the dependency chain is NB long), L_kk read from the lanes that hold it
            //     (v_readlane), then l_c = u_c / D_c goes back to the packed triangle;
            //   * 16 x 16 block pairs (I, J), J <= I, of everything below/right of the panel are dealt round-robin to the
            //     4 waves: C_IJ -= (L_I D) L_J' as NB/4 MFMAs into independent accumulators.
            // No guard; it records whether the guard would have bitten (then: re-assembly + `factor(true)`, as before).
            auto factor_blocked = [&]() -> bool {
                constexpr int NB = 16;                       // panel width = block size of the trailing update
                const int nbk = (m + 15) >> 4;               // number of panels = number of 16 x 16 block rows
                const int r16 = lane & 15, kq = lane >> 4;
                double* dgv = ucol;                          // D_j (the solves want 1/D_j: rdg)
                bool viol = false;
                double W[NB], aDv[NB], rDv[NB];              // the diagonal block of the panel in flight (lane = row)
                // ---- panel kb: diagonal block (redundantly in every wave that owns panel rows) + panel rows ----
                auto panel = [&](int kb) {
                    const int c0 = NB * kb, prow0 = c0 + NB, nprow = m - prow0;
                    const int ir = c0 + r16;
                    const bool rv = ir < m;                  // lane holds a real row of the diagonal block
                    {
                        const double* Mr = M + tri_idx(rv ? ir : 0, c0);
#pragma unroll
                        for (int c = 0; c < NB; c++)
                            W[c] = rv ? ((c <= r16) ? Mr[c] : 0.0) : ((c == r16) ? 1.0 : 0.0);
                    }
                    // floor of this lane's row: one LDS read per panel, handed to the column loop by DPP
                    const double myf = hsd ? flr[rv ? ir : m - 1] : o.pivot_floor;
                    static_for<0, NB>([&](auto jc) {
                        constexpr int j = decltype(jc)::value;
                        const double u = W[j];
                        const double piv = row_bcast<j>(u);
                        const double aD = fmax(fabs(piv), row_bcast<j>(myf));
                        const double rD = fast_rcp(aD);
                        const bool below = r16 > j;
                        viol = viol | (below & (u * u > beta2 * aD));
                        const double li = below ? u * rD : 0.0;
                        static_for<j + 1, NB>([&](auto kc) {
                            constexpr int k = decltype(kc)::value;
                            W[k] = fma(-li, row_bcast<k>(u), W[k]);
                        });
                        W[j] = li; aDv[j] = aD; rDv[j] = rD;
                    });
                    if (wave == 0 && lane < NB && rv) {
#pragma unroll
                        for (int c = 0; c < NB; c++)
                            if (c == r16) { rdg[ir] = rDv[c]; dgv[ir] = aDv[c]; }
                    }
                    // panel rows: thread = row
                    const bool prow_ok = tid < nprow;
                    double* Mp = M + tri_idx(prow_ok ? prow0 + tid : 0, c0);
                    double ur[NB];
#pragma unroll
                    for (int c = 0; c < NB; c++) ur[c] = prow_ok ? Mp[c] : 0.0;
                    static_for<0, NB>([&](auto lc) {
                        constexpr int l = decltype(lc)::value;
                        const double ul = ur[l];
                        viol = viol | (prow_ok & (ul * ul > beta2 * aDv[l]));
                        static_for<l + 1, NB>([&](auto cc) {
                            constexpr int c = decltype(cc)::value;
                            ur[c] = fma(-ul, row_bcast<c>(W[l]), ur[c]);   // every 16-lane row holds its own copy of L_kk
                        });
                    });
                    if (prow_ok) {
#pragma unroll
                        for (int c = 0; c < NB; c++) Mp[c] = ur[c] * rDv[c];
                    }
                };
                // the diagonal block's rows of L go back to M only after a barrier: before it another wave may still be
                // reading the raw block for its own (redundant) factorisation
                auto store_diag = [&](int kb) {
                    const int c0 = NB * kb, ir = c0 + r16;
                    if (wave == 0 && lane < NB && ir < m) {
                        double* Mr = M + tri_idx(ir, c0);
#pragma unroll
                        for (int c = 0; c < NB; c++)
                            if (c < r16) Mr[c] = W[c];
                    }
                };
                // C_IJ -= (L_I D) L_J' for the panel with first column c0 (blocks I >= J > panel)
                auto pair_update = [&](int I, int J, int c0) {
                    const int col = 16 * J + r16;
                    double cin[4];
                    bool cv[4]; int ci[4];
#pragma unroll
                    for (int r4 = 0; r4 < 4; r4++) {
                        const int row = 16 * I + kq + 4 * r4;
                        cv[r4] = row < m && col <= row;
                        ci[r4] = tri_idx(cv[r4] ? row : 0, cv[r4] ? col : 0);
                        cin[r4] = cv[r4] ? M[ci[r4]] : 0.0;
                    }
                    const int ia = 16 * I + r16, ib = 16 * J + r16;
                    const bool av = ia < m, bv = ib < m;
                    const double* Ma = M + tri_idx(av ? ia : 0, c0 + kq);
                    const double* Mb = M + tri_idx(bv ? ib : 0, c0 + kq);
                    double a[NB / 4], bq[NB / 4];
#pragma unroll
                    for (int s4 = 0; s4 < NB / 4; s4++) {
                        a[s4] = av ? -Ma[4 * s4] * dgv[c0 + kq + 4 * s4] : 0.0;
                        bq[s4] = bv ? Mb[4 * s4] : 0.0;
                    }
                    double4_t acc[NB / 4];
#pragma unroll
                    for (int s4 = 0; s4 < NB / 4; s4++) {
                        acc[s4] = (s4 == 0) ? (double4_t){cin[0], cin[1], cin[2], cin[3]} : (double4_t){0.0, 0.0, 0.0, 0.0};
                        acc[s4] = __builtin_amdgcn_mfma_f64_16x16x4f64(a[s4], bq[s4], acc[s4], 0, 0, 0);
                    }
#pragma unroll
                    for (int r4 = 0; r4 < 4; r4++) {
                        double v = acc[0][r4];
#pragma unroll
                        for (int s4 = 1; s4 < NB / 4; s4++) v += acc[s4][r4];
                        if (cv[r4]) M[ci[r4]] = v;
                    }
                };
                // waves that work on panel kb: wave 0, plus wave w while w * 64 panel rows are not enough
                auto panel_waves = [&](int kb) { const int np = m - NB * (kb + 1); return np > 64 ? 2 : 1; };

                // LOOK-AHEAD schedule: once the first block column of trailing update kb is done, panel kb+1 can be
                // factored (waves 0..) WHILE the remaining block columns of trailing update kb are processed by the
                // other waves -- the serial pivot chain no longer sits between two trailing updates with 2-3 waves idle.
                if (wave < panel_waves(0)) panel(0);
                STAMP(8)
                __syncthreads();
                store_diag(0);
                for (int kb = 0; kb + 1 < nbk; kb++) {
                    const int c0 = NB * kb, I0 = kb + 1, nrem = nbk - I0;
                    // phase A: block column I0 (what panel kb+1 needs), all four waves
                    for (int i = wave; i < nrem; i += 4) pair_update(I0 + i, I0, c0);
                    __syncthreads();
                    // phase B: panel kb+1 on its waves, the rest of trailing update kb on the others
                    const int npw = panel_waves(kb + 1);
                    if (wave < npw) {
                        panel(kb + 1);
                        STAMP(8)
                    } else {
                        const int nh = 4 - npw, hidx = wave - npw, n2 = nrem - 1;
                        int Ip = 0, base = 0;
                        for (int pr = hidx; pr < n2 * (n2 + 1) / 2; pr += nh) {
                            while (base + Ip + 1 <= pr) { base += Ip + 1; Ip++; }
                            pair_update(I0 + 1 + Ip, I0 + 1 + (pr - base), c0);
                        }
                    }
                    __syncthreads();
                    store_diag(kb + 1);
                    STAMP(3)
                }
                __syncthreads();
                return blk_max(viol ? 1.0 : 0.0, red, tid) > 0.0;
            };
            const bool redo = factor_blocked();
            if (redo || (o.flags & PYCLLP_FLAG_FORCE_GUARD_PATH)) {
                // re-assemble M and factor with the guard applied
                for (int e = tid; e < ntri; e += BLK_T) M[e] = 0.0;
                __syncthreads();
                for (int e = tid; e < A.n_entries; e += BLK_T) {
                    double acc = 0.0;
                    for (int pp2 = A.ent_ptr[e]; pp2 < A.ent_ptr[e + 1]; pp2++)
                        acc = fma(pa ? lv[A.term_ia[pp2]] * lv[A.term_ib[pp2]] : A.term_w[pp2], vd[A.term_col[pp2]], acc);
                    M[A.ent_tri[e]] = acc;
                }
                __syncthreads();
                (void)factor(true);
            }
            STAMP(3)
            // ---- solve, A'dy, dx ----
            double wv[BLK_NC], dx[BLK_NC];
            double dtau = 0.0;
            if (hsd) {
                double* pv = ucol;                 // free again after the factorisation
                if (tid < m) { pv[tid] = rp; sv[tid] = rq; }
                __syncthreads();
                solve2_in_wave0(pv);               // p (in pv) and q (in sv) in one pass over the factor
                STAMP(4)
                double ap[BLK_NC], aq[BLK_NC];
                At_cols(pv, ap);
                At_cols(sv, aq);
                double dsum = 0.0, nsum = 0.0;
#pragma unroll
                for (int q = 0; q < BLK_NC; q++) {
                    const double cp = c[q] - ap[q];
                    const double u = d[q] * cp;
                    dx[q] = d[q] * (t[q] - aq[q]);     // v
                    ap[q] = u;
                    wv[q] = 0.0;
                    dsum = fma(u, cp, dsum);
                    nsum = fma(c[q], dx[q], nsum);
                }
                const double den = blk_sum(dsum, red, tid) + kap / tau;
                const double num = fma(eta, phi, mu / tau - kap) + blk_sum((tid < m) ? bs[tid] * sv[tid] : 0.0, red, tid)
                                   - blk_sum(nsum, red, tid);
                dtau = num / den;
                if (tid < m) {
                    dy[tid] = fma(pv[tid], dtau, sv[tid]);
                    rho[tid] = fma(bs[tid], dtau, eta * rho_i);   // target of the refinement: A dx - b dtau = eta rho
                }
#pragma unroll
                for (int q = 0; q < BLK_NC; q++) dx[q] = fma(ap[q], dtau, dx[q]);
                __syncthreads();
            } else {
                solve_in_wave0();
                if (tid < m) dy[tid] = sv[tid];
                __syncthreads();
                STAMP(4)
                At_cols(dy, wv);
#pragma unroll
                for (int q = 0; q < BLK_NC; q++) dx[q] = (t[q] - wv[q]) * d[q];
            }
            const double etol_it = hsd ? o.refine_tol * (1.0 + nbn) * fmax(tau, kap) : etol;
            STAMP(5)
            // ---- x-space refinement (oracle newton_dy) ----
            int nref = 0;
            for (;;) {
                __syncthreads();
#pragma unroll
                for (int q = 0; q < BLK_NC; q++) if (ok[q]) vx[tid + BLK_T * q] = dx[q];
                __syncthreads();
                const double e = (tid < m) ? rho[tid] - A_row(vx) : 0.0;
                const double maxe = blk_max(fabs(e), red, tid);
                if (!(maxe > etol_it) || nref >= o.max_refine) break;
                if (tid < m) sv[tid] = e;
                __syncthreads();
                solve_in_wave0();
                double w2[BLK_NC];
                At_cols(sv, w2);
#pragma unroll
                for (int q = 0; q < BLK_NC; q++) { dx[q] = fma(d[q], w2[q], dx[q]); wv[q] -= w2[q]; }
                if (tid < m) dy[tid] -= sv[tid];
                nref++;
            }
            if (nwt) {
                if (tid < m) nwt_dy[lp * m + tid] = dy[tid];
                if (tid == 0 && nwt_nref) nwt_nref[lp] = nref;
                break;
            }
            const double normr = sqrt(blk_sum(rho_i * rho_i, red, tid));
            const double dybad = blk_max((tid < m && !isfinite(dy[tid])) ? 1.0 : 0.0, red, tid);
            STAMP(6)

            if (!hsd) {
                if (!(isfinite(normr) && isfinite(norms) && isfinite(gam))) { stat = PYCLLP_STATUS_NUMERICAL; break; }
                if (normr <= tol_r && norms <= tol_s && gam <= o.eps * (1.0 + fabs(po))) { stat = PYCLLP_STATUS_OPTIMAL; break; }
                if (normr > 10.0 * normr0 && normr > PYCLLP_GROWTH_FLOOR * tol_r) { stat = PYCLLP_STATUS_PRIMAL_INFEASIBLE; break; }
                if (norms > 10.0 * norms0 && norms > PYCLLP_GROWTH_FLOOR * tol_s) { stat = PYCLLP_STATUS_DUAL_INFEASIBLE; break; }
            }
            if (dybad > 0.0 || !isfinite(dtau)) { stat = PYCLLP_STATUS_NUMERICAL; break; }

            // ---- step (primal_normal.cl:158-198) ----
            const double dkap = hsd ? mu / tau - kap - kap / tau * dtau : 0.0;
            double dz[BLK_NC], th = hsd ? fmax(fmax(-dtau / tau, -dkap / kap), 0.0) : 0.0;
#pragma unroll
            for (int q = 0; q < BLK_NC; q++) {
                dz[q] = ok[q] ? (mu - z[q] * dx[q]) / x[q] - z[q] : 0.0;
                if (ok[q]) th = fmax(th, fmax(-dz[q] / z[q], -dx[q] / x[q]));
            }
            th = blk_max(th, red, tid);
            const double theta = fmin(o.r / th, 1.0);
            if (tid < m) ys[tid] = fma(theta, dy[tid], ys[tid]);
#pragma unroll
            for (int q = 0; q < BLK_NC; q++) { x[q] = fma(theta, dx[q], x[q]); z[q] = fma(theta, dz[q], z[q]); }
            if (hsd) { tau = fma(theta, dtau, tau); kap = fma(theta, dkap, kap); }
            normr0 = normr; norms0 = norms;
            __syncthreads();
            STAMP(7)
        }
        __syncthreads();
        if (nwt) continue;
        // HSD: optimal (and iteration-limit) points leave the homogeneous scaling (hsd.c:266-273); certificates stay
        const double rt = (hsd && (stat == PYCLLP_STATUS_OPTIMAL || stat == PYCLLP_STATUS_ITERATION_LIMIT)) ? 1.0 / tau : 1.0;
#pragma unroll
        for (int q = 0; q < BLK_NC; q++) {
            const int j = tid + BLK_T * q;
            if (ok[q]) { xg[lp * n + j] = x[q] * rt * sb; if (zg) zg[lp * n + j] = z[q] * rt * sc; }
        }
        if (yg && tid < m) yg[lp * m + tid] = ys[tid] * rt * sc;
        if (tid == 0) {
            if (pobj) pobj[lp] = po * rt * (sb * sc);
            if (dobj) dobj[lp] = du * rt * (sb * sc);
            status[lp] = stat;
            if (iters) iters[lp] = it;
        }
        STAMP(9)
    }
    if (o.prof && tid == 0) { STAMP_FLUSH_BLOCK(o, blockIdx.x) }
}
