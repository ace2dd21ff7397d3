// ipm_wreg_hsd.inc -- the solve kernel of the wavefront-per-LP family on the homogeneous self-dual embedding, on wreg_wave.h
namespace {

// ------------------------------------------------------------------------------------------------------------------
// the same solve on the homogeneous self-dual embedding (PYCLLP_FLAG_HSD; oracle hsd_one_raw, ipm_block_kernel's run-time
// branch, csrc/ipm_group_hsd.inc): tau and kappa are wave-uniform scalars, one factorisation serves the two right-hand
// sides  M p = A(d c) - b  and  M q = A(d r1) - eta rho, the pivot floor of column j is pivot_floor^2 |M_jj|
// Written once in wreg_wave.h, for this kernel and ipm_wreg_bounded_hsd_kernel (ipm_wreg_bdhsd.inc): the stop verdict
// (WREG_HSD_RAYS, WREG_HSD_VERDICT), pass 0's hand-over (hsd_hand_over_p), dy and the refinement's right-hand side behind dtau
// (WREG_HSD_DY), the tail of a refinement pass (WREG_HSD_REFINE_TAIL), dkappa and the start of the ratio test (hsd_dkappa,
// hsd_ratio0); the LP's load and store (load_lp, store_lp) are shared with ipm_wreg_kernel.
// ------------------------------------------------------------------------------------------------------------------
template <int MB, int NQ, bool DA, bool PA>
__global__ void __launch_bounds__(256, 1)
hsd_wreg_kernel(WregTab T, long B, const double* __restrict__ ag, const double* __restrict__ bg, const double* __restrict__ cg,
                double* __restrict__ xg, double* __restrict__ yg, double* __restrict__ zg, double* __restrict__ pobj,
                double* __restrict__ dobj, int* __restrict__ status, int* __restrict__ iters, int* __restrict__ queue,
                int* __restrict__ defer, DevOpts o) {
    using G = WGeo<MB>;
    constexpr int MR = G::MR, MP = G::MP;
    extern __shared__ __attribute__((aligned(16))) unsigned char lraw[];
    WReg<MB, NQ, DA, PA> w;
    USE_AGPR_FORM();
    wreg_setup(w, T, lraw, threadIdx.x);
    const int& lane = w.lane;
    const int n = w.n;
    const bool warm = (o.flags & PYCLLP_FLAG_WARM_START) != 0;
    const bool autoscale = (o.flags & PYCLLP_FLAG_AUTOSCALE) != 0;
    const double eta = 1.0 - o.delta, einf = 100.0 * o.eps;
    double* vx = w.stage_();
    double* pv = w.flr_();          // p = M^-1 (A(d c) - b): the floor vector is dead once the factor exists
    bool okc[NQ], okr[MR];
    w.masks(okc, okr);

    long lp = next_item(queue, lane);
    STAMP_DECL
    while (lp < B) {
        if constexpr (PA) load_lp_values(w, ag, lp, T.nnz);
        const __amdgpu_buffer_rsrc_t rc = row_rsrc(cg + lp * n, n), rx = row_rsrc(xg + lp * n, n), rz = row_rsrc(zg ? zg + lp * n : nullptr, n);
        // x and z cross the loop's back edge in LDS (where load_lp parks them and where they wait during factor and solves), as in ipm_wreg_kernel
        const LpStart s0 = load_lp<true>(w, okc, okr, lp, bg, yg, rc, rx, rz, warm, o.flags);
        const double sc = s0.sc;
        const double nbn = uni(sqrt(s0.nb2)), ncn = uni(sqrt(s0.nc2));
        const double tol_r = uni(o.eps * (1.0 + nbn)), tol_s = uni(o.eps * (1.0 + ncn));
        double tau = 1.0, kap = 1.0;
        if (warm) kap = uni(s0.g0 / (double)n);
        double po = 0.0, du = 0.0;
        int stat = PYCLLP_STATUS_ITERATION_LIMIT, it = 0;
        bool running = true;

        while (running) {
            double x[NQ], z[NQ];
#pragma unroll
            for (int qq = 0; qq < NQ; qq++) {
                x[qq] = w.px(qq);
                z[qq] = w.pz(qq);
            }
            wave_lds_sync();
            // ---- sigma = c tau - A'y + z, gamma, objectives ----
            double v[NQ], cq[NQ], sg[NQ];
#pragma unroll
            for (int qq = 0; qq < NQ; qq++) cq[qq] = buf_ld(rc, w.coff(qq));   // in flight (vmcnt) while A'y runs on LDS; 0 in the padded positions
            w.At(w.ys_(), v);
            if (autoscale) {
#pragma unroll
                for (int qq = 0; qq < NQ; qq++) cq[qq] = cq[qq] / sc;
            }
            double s2 = 0.0, gam = 0.0, pp = 0.0;
#pragma unroll
            for (int qq = 0; qq < NQ; qq++) {
                sg[qq] = okc[qq] ? cq[qq] * tau - v[qq] + z[qq] : 0.0;
                s2 = fma(sg[qq], sg[qq], s2);
                gam += okc[qq] ? x[qq] * z[qq] : 0.0;
                pp += cq[qq] * (okc[qq] ? x[qq] : 0.0);
            }
            double dd = 0.0;
#pragma unroll
            for (int r2 = 0; r2 < MR; r2++) {
                const int i = lane + 64 * r2;
                dd += (i < MP) ? w.bs_()[i] * w.ys_()[i] : 0.0;
            }
            s2 = wsum(s2); gam = wsum(gam); po = wsum(pp); du = wsum(dd);
            const double norms = uni(sqrt(s2));
            const double mu = uni(o.delta * (gam + tau * kap) / (double)(n + 1));
            const double phi = uni(du - po + kap);
            // ---- d, t = r1 = mu/x - z + eta sigma; rho = b tau - A x ----
            double t[NQ];
#pragma unroll
            for (int qq = 0; qq < NQ; qq++) {
                const int j = lane + 64 * qq;
                const double dq = okc[qq] ? x[qq] * fast_rcp(z[qq]) : 0.0;
                t[qq] = okc[qq] ? fma(eta, sg[qq], mu * fast_rcp(x[qq]) - z[qq]) : 0.0;
                vx[j] = okc[qq] ? x[qq] : 0.0;
                w.vd_()[j] = dq;
            }
            wave_lds_sync();
            double rho[MR], Ax[MR], Md[MR];
            w.template Arow<false>(vx, Ax, Md);
            double r2s = 0.0;
#pragma unroll
            for (int r2 = 0; r2 < MR; r2++) {
                const int i = lane + 64 * r2;
                rho[r2] = okr[r2] ? w.bs_()[i] * tau - Ax[r2] : 0.0;
                r2s = fma(rho[r2], rho[r2], r2s);
            }
            const double normr = uni(sqrt(wsum(r2s)));
            // ---- stop tests (oracle hsd_one_raw): optimal, or a primal / dual ray ----
            WREG_HSD_RAYS(einf)
            WREG_HSD_VERDICT(tol_r, tol_s)
            if (running) {
                // ---- A(d r1), diag(M), A(d c) ----
                wave_lds_sync();
#pragma unroll
                for (int qq = 0; qq < NQ; qq++) vx[lane + 64 * qq] = w.vd_()[lane + 64 * qq] * t[qq];
                wave_lds_sync();
                double Adt[MR], Adc[MR], dummy[MR];
                w.template Arow<true>(vx, Adt, Md);
                wave_lds_sync();
#pragma unroll
                for (int qq = 0; qq < NQ; qq++) vx[lane + 64 * qq] = w.vd_()[lane + 64 * qq] * cq[qq];
                wave_lds_sync();
                w.template Arow<false>(vx, Adc, dummy);
                double rq[MR], bmax = 0.0;
#pragma unroll
                for (int r2 = 0; r2 < MR; r2++) {
                    const int i = lane + 64 * r2;
                    rq[r2] = okr[r2] ? fma(-eta, rho[r2], Adt[r2]) : 0.0;
                    if (i < MP) {
                        w.um_()[i] = okr[r2] ? Adc[r2] - w.bs_()[i] : 0.0;                   // right-hand side of p
                        w.flr_()[i] = o.pivot_floor * o.pivot_floor * fabs(Md[r2]);         // floor of column i
                    }
                    bmax = fmax(bmax, okr[r2] ? fabs(Md[r2]) : 0.0);
                }
                const double beta2 = uni(wmax(bmax));
                wave_lds_sync();
                STAMP(0)
                w.gram(Md);
                STAMP(1)
                // t = r1, x and z wait in the stage while factor and the solves have the registers
#pragma unroll
                for (int qq = 0; qq < NQ; qq++) {
                    w.stage_()[lane + 64 * qq] = t[qq];
                    w.px(qq) = x[qq];
                    w.pz(qq) = z[qq];
                }
                const bool viol = w.template factor<true>(beta2, 0.0 STAMP_PASS);
                if (viol || (o.flags & PYCLLP_FLAG_FORCE_GUARD_PATH)) { stat = -1; running = false; }
                else {
                    // ---- one loop around the ONE copy of the block substitution: pass 0 solves for p, pass 1 for q and
                    //      combines them through dtau, the following passes are the x-space refinement ----
                    // (u = c - A'p waits in d's place between the two solves: d = x / z is formed again from the parked x, z
                    // where a pass needs it; c comes back from memory, in flight while the substitution runs)
                    double dx[NQ], dy[MR], rhot[MR];
                    double dtau = 0.0, etol_it = 0.0;
                    bool bad = false;
                    int pass = 0;
                    for (;;) {
                        double c2q[NQ];
                        if (pass < 2) {
#pragma unroll
                            for (int qq = 0; qq < NQ; qq++) c2q[qq] = buf_ld(rc, w.coff(qq));
                        }
                        w.solve();
                        STAMP(7)
                        double w2[NQ], d[NQ];
                        w.At(w.um_(), w2);
                        if (autoscale && pass < 2) {
#pragma unroll
                            for (int qq = 0; qq < NQ; qq++) c2q[qq] = c2q[qq] / sc;
                        }
#pragma unroll
                        for (int qq = 0; qq < NQ; qq++)
                            d[qq] = okc[qq] ? w.px(qq) * fast_rcp(w.pz(qq)) : 0.0;
                        bool more = true;
                        if (pass == 0) {
                            // c - A'p is kept (in d's place); p moves to pv, q's right-hand side into um
#pragma unroll
                            for (int qq = 0; qq < NQ; qq++) w.vd_()[lane + 64 * qq] = c2q[qq] - w2[qq];
                            wave_lds_sync();
                            hsd_hand_over_p(w, rq);
                        } else {
                            if (pass == 1) {
                                double dsum = 0.0, nsum = 0.0, bq = 0.0;
                                double u[NQ];
#pragma unroll
                                for (int qq = 0; qq < NQ; qq++) {
                                    const double tq = w.stage_()[lane + 64 * qq];
                                    u[qq] = w.vd_()[lane + 64 * qq];
                                    dx[qq] = d[qq] * (tq - w2[qq]);                       // v = d (r1 - A'q)
                                    dsum = fma(d[qq] * u[qq], u[qq], dsum);               // |sqrt(d)(c - A'p)|^2
                                    nsum = fma(c2q[qq], dx[qq], nsum);                    // c'v
                                }
#pragma unroll
                                for (int r2 = 0; r2 < MR; r2++) {
                                    const int i = lane + 64 * r2;
                                    bq += (i < MP) ? w.bs_()[i] * w.um_()[i] : 0.0;       // b'q
                                }
                                const double den = wsum(dsum) + kap / tau;
                                const double num = fma(eta, phi, mu / tau - kap) + wsum(bq) - wsum(nsum);
                                dtau = uni(num / den);
                                WREG_HSD_DY(eta)
#pragma unroll
                                for (int qq = 0; qq < NQ; qq++) dx[qq] = fma(d[qq] * u[qq], dtau, dx[qq]);   // dx = u dtau + v, u = d (c - A'p)
                                etol_it = uni(o.refine_tol * (1.0 + nbn) * fmax(tau, kap));
                            } else {
#pragma unroll
                                for (int qq = 0; qq < NQ; qq++) dx[qq] = fma(d[qq], w2[qq], dx[qq]);
#pragma unroll
                                for (int r2 = 0; r2 < MR; r2++) dy[r2] -= (lane + 64 * r2 < MP) ? w.um_()[lane + 64 * r2] : 0.0;
                            }
                            WREG_HSD_REFINE_TAIL(okc[qq])
                        }
                        if (!more) break;
                        pass++;
                    }
                    if (__any(bad) || !isfinite(dtau)) { stat = PYCLLP_STATUS_NUMERICAL; running = false; }
                    else {
                        // ---- step: ratio test over x, z, tau, kappa ----
                        const double dkap = hsd_dkappa(mu, tau, kap, dtau);
                        double dz[NQ], xs[NQ], zs[NQ], th = hsd_ratio0(tau, kap, dtau, dkap);
#pragma unroll
                        for (int qq = 0; qq < NQ; qq++) {
                            xs[qq] = w.px(qq);
                            zs[qq] = w.pz(qq);
                        }
#pragma unroll
                        for (int qq = 0; qq < NQ; qq++) {
                            const double rx = fast_rcp(xs[qq]), rz = fast_rcp(zs[qq]);
                            dz[qq] = okc[qq] ? (mu - zs[qq] * dx[qq]) * rx - zs[qq] : 0.0;
                            if (okc[qq]) th = fmax(th, fmax(-dz[qq] * rz, -dx[qq] * rx));
                        }
                        th = wmax(th);
                        const double theta = uni(fmin(o.r / th, 1.0));
                        wave_lds_sync();
#pragma unroll
                        for (int r2 = 0; r2 < MR; r2++) {
                            const int i = lane + 64 * r2;
                            if (i < MP) w.ys_()[i] = fma(theta, dy[r2], w.ys_()[i]);
                        }
#pragma unroll
                        for (int qq = 0; qq < NQ; qq++) {
                            w.px(qq) = fma(theta, dx[qq], xs[qq]);
                            w.pz(qq) = fma(theta, dz[qq], zs[qq]);
                        }
                        tau = uni(fma(theta, dtau, tau)); kap = uni(fma(theta, dkap, kap));
                        wave_lds_sync();
                        it++;
                        if (it >= o.max_iter) running = false;
                        STAMP(9)
                    }
                }
            }
        }
        wave_lds_sync();
        // optimal (and iteration-limit) points leave the homogeneous scaling (hsd.c:266-273); certificates stay
        const double rt = (stat == PYCLLP_STATUS_OPTIMAL || stat == PYCLLP_STATUS_ITERATION_LIMIT) ? 1.0 / tau : 1.0;
        store_lp(w, okr, lp, stat, it, rt, s0.sb, sc, po, du, rx, rz, yg, pobj, dobj, status, iters, defer);
        lp = next_item(queue, lane);
        STAMP(9)
    }
    STAMP_FLUSH(o, blockIdx.x * 4 + (threadIdx.x >> 6))
}

}  // namespace
