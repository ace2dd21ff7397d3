// ipm_wreg_solve.inc -- the solve kernel of the wavefront-per-LP family (plain path and predictor-corrector) on wreg_wave.h
namespace {

// ------------------------------------------------------------------------------------------------------------------
// solve kernel: sparse_standard_primal_normal (primal_normal.cl:287-375), one LP per wavefront
// ------------------------------------------------------------------------------------------------------------------
// PC (PYCLLP_FLAG_PREDCORR): Mehrotra's predictor-corrector, oracle ipm_one_pc -- after the iteration's one factorisation a
// predictor solve with mu = 0, the centering parameter from how far it gets, then the corrector solve (newton_solve with the
// per-column target cor = mu - dx_a dz_a): one more block substitution, A'u and A v per iteration, about half the iterations
// on config 5's structure (52.7 -> 25.5)
template <int MB, int NQ, bool DA, bool PA, bool PC = false>
__global__ void __launch_bounds__(256, 1)
ipm_wreg_kernel(WregTab T, long B, const double* __restrict__ ag, const double* __restrict__ bg, const double* __restrict__ cg,
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
    const int m = w.m, n = w.n;
    const bool warm = (o.flags & PYCLLP_FLAG_WARM_START) != 0;
    const bool autoscale = (o.flags & PYCLLP_FLAG_AUTOSCALE) != 0;
    const double nm = (double)(n + m);
    double* vx = w.stage_();
    bool okc[NQ], okr[MR];
    w.masks(okc, okr);

    long lp = next_item(queue, lane);
    STAMP_DECL
    while (lp < B) {
        if constexpr (PA) load_lp_values(w, ag, lp, T.nnz);
        const __amdgpu_buffer_rsrc_t rc = row_rsrc(cg + lp * n, n), rx = row_rsrc(xg + lp * n, n), rz = row_rsrc(zg ? zg + lp * n : nullptr, n);
        const LpStart s0 = load_lp<false>(w, okc, okr, lp, bg, yg, rc, rx, rz, warm, o.flags);
        const double sc = s0.sc, nb2 = s0.nb2, nc2 = s0.nc2;
        const double tol_r = uni(o.eps * (1.0 + sqrt(nb2))), tol_s = uni(o.eps * (1.0 + sqrt(nc2)));
        const double etol = uni(o.refine_tol * (1.0 + sqrt(nb2)));
        double normr0 = 1e300, norms0 = 1e300, po = 0.0, du = 0.0;
        int stat = PYCLLP_STATUS_ITERATION_LIMIT, it = 0;
        bool running = true;
        // The residuals cv = c - A'y and rho = b - A x are CARRIED from iteration to iteration (cv -= theta A'dy,
        // rho -= theta A dx: both products exist anyway, from the Newton step and its refinement test) and recomputed from
        // the point itself only at the start and when the carried values pass the optimality test -- the verdict is then
        // taken again on the exact ones (as the dense group kernel does for rho), and the iteration goes on if it fails.
        // x, z (parked by load_lp) and cv cross the loop's back edge IN LDS (the slots where they wait during factor and solve anyway), not in
        // registers: 36 loop-carried registers through this loop's control flow end up in scratch
        // (rho lives in the floor vector's place, which this kernel does not use)
        bool refresh = true, fresh = false;

        while (running) {
            double x[NQ], z[NQ], cv[NQ], rho[MR];
#pragma unroll
            for (int r2 = 0; r2 < MR; r2++) rho[r2] = (lane + 64 * r2 < MP) ? w.flr_()[lane + 64 * r2] : 0.0;
#pragma unroll
            for (int qq = 0; qq < NQ; qq++) {
                x[qq] = w.px(qq);
                z[qq] = w.pz(qq);
                cv[qq] = w.vd_()[lane + 64 * qq];       // (not yet there in the first pass: refresh sets it)
            }
            wave_lds_sync();
            if (refresh) {
                double v[NQ], cq[NQ], Ax[MR], dm[MR];
#pragma unroll
                for (int qq = 0; qq < NQ; qq++) cq[qq] = buf_ld(rc, w.coff(qq));   // in flight (vmcnt) while A'y runs on LDS; 0 in the padded positions
                w.At(w.ys_(), v);
                if (autoscale) {
#pragma unroll
                    for (int qq = 0; qq < NQ; qq++) cq[qq] = cq[qq] / sc;
                }
#pragma unroll
                for (int qq = 0; qq < NQ; qq++) {
                    cv[qq] = okc[qq] ? cq[qq] - v[qq] : 0.0;
                    vx[lane + 64 * qq] = okc[qq] ? x[qq] : 0.0;
                }
                wave_lds_sync();
                w.template Arow<false>(vx, Ax, dm);
#pragma unroll
                for (int r2 = 0; r2 < MR; r2++) {
                    const int i = lane + 64 * r2;
                    rho[r2] = okr[r2] ? w.bs_()[i] - Ax[r2] : 0.0;
                    if (i < MP) w.flr_()[i] = rho[r2];
                }
                wave_lds_sync();
                refresh = false; fresh = true;
            }
            // ---- sigma, gamma, objectives (primal_normal.cl:96-120, 245-248); c'x = cv'x + y'(b - rho) ----
            double s2 = 0.0, gam = 0.0, pp = 0.0;
#pragma unroll
            for (int qq = 0; qq < NQ; qq++) {
                const double sg = okc[qq] ? cv[qq] + z[qq] : 0.0;
                s2 = fma(sg, sg, s2);
                gam += okc[qq] ? x[qq] * z[qq] : 0.0;
                pp += okc[qq] ? cv[qq] * x[qq] : 0.0;
            }
            double dd = 0.0, r2s = 0.0;
#pragma unroll
            for (int r2 = 0; r2 < MR; r2++) {
                const int i = lane + 64 * r2;
                const double bi = (i < MP) ? w.bs_()[i] : 0.0, yi = (i < MP) ? w.ys_()[i] : 0.0;
                dd = fma(bi, yi, dd);
                pp = fma(yi, bi - rho[r2], pp);
                r2s = fma(rho[r2], rho[r2], r2s);
            }
            s2 = wsum(s2); gam = wsum(gam); po = wsum(pp); du = wsum(dd);
            const double norms = uni(sqrt(s2));
            const double normr = uni(sqrt(wsum(r2s)));
            double mu = PC ? 0.0 : uni(o.delta * gam / nm);      // PC: 0 for the predictor, set from its outcome below
            STAMP(10)
            // ---- stop tests (primal_normal.cl:256-269; oracle ipm_one_path) ----
            if (!(isfinite(normr) && isfinite(norms) && isfinite(gam))) { stat = PYCLLP_STATUS_NUMERICAL; running = false; }
            else if (normr <= tol_r && norms <= tol_s && gam <= o.eps * (1.0 + fabs(po))) {
                if (fresh) { stat = PYCLLP_STATUS_OPTIMAL; running = false; } else refresh = true;
            }
            else if (normr > 10.0 * normr0 && normr > PYCLLP_GROWTH_FLOOR * tol_r) { stat = PYCLLP_STATUS_PRIMAL_INFEASIBLE; running = false; }
            else if (norms > 10.0 * norms0 && norms > PYCLLP_GROWTH_FLOOR * tol_s) { stat = PYCLLP_STATUS_DUAL_INFEASIBLE; running = false; }
            STAMP(11)
            if (running && !refresh) {
                // ---- d, t (primal_normal.cl:50-74); rhs = A (d t) - rho, diag(M) ----
#pragma unroll
                for (int qq = 0; qq < NQ; qq++) {
                    const int j = lane + 64 * qq;
                    const double dq = okc[qq] ? x[qq] * fast_rcp(z[qq]) : 0.0;      // v_rcp_f64 + 2 Newton steps (<= 2 ulp), as
                    const double tq = okc[qq] ? cv[qq] + mu * fast_rcp(x[qq]) : 0.0;   // the dense group kernel
                    vx[j] = dq * tq;
                    w.vd_()[j] = dq;
                }
                wave_lds_sync();
                double Adt[MR], Md[MR];
                w.template Arow<true>(vx, Adt, Md);
                double bmax = 0.0;
#pragma unroll
                for (int r2 = 0; r2 < MR; r2++) {
                    const int i = lane + 64 * r2;
                    if (i < MP) w.um_()[i] = okr[r2] ? Adt[r2] - rho[r2] : 0.0;
                    bmax = fmax(bmax, okr[r2] ? fabs(Md[r2]) : 0.0);
                }
                const double beta2 = wmax(bmax);     // ldl.cl:296-311
                wave_lds_sync();
                STAMP(0)
                // ---- M = A diag(d) A' into registers; factor ----
                w.gram(Md);
                STAMP(1)
                // cv (in d's place, which is not needed any more: the Newton step forms it again), x and z wait in LDS while
                // factor and solve have the registers
#pragma unroll
                for (int qq = 0; qq < NQ; qq++) {
                    w.vd_()[lane + 64 * qq] = cv[qq];
                    w.px(qq) = x[qq];
                    w.pz(qq) = z[qq];
                }
                const bool viol = w.template factor<false>(beta2, o.pivot_floor STAMP_PASS);
                if (viol || (o.flags & PYCLLP_FLAG_FORCE_GUARD_PATH)) { stat = -1; running = false; }
                else {
                    double dy[MR], wv[NQ], dx[NQ], e[MR], rhn[MR];
                    double cor[NQ];
                    bool bad;
#pragma unroll
                    for (int r2 = 0; r2 < MR; r2++) rhn[r2] = (lane + 64 * r2 < MP) ? w.flr_()[lane + 64 * r2] : 0.0;
                    if constexpr (PC) {
                        // ---- predictor: um holds A(d t_a) - rho with t_a = cv (mu = 0) ----
                        w.solve();
                        double w2[NQ], dxa[NQ], dza[NQ], tha = 0.0, ga = 0.0;
                        w.At(w.um_(), w2);
#pragma unroll
                        for (int qq = 0; qq < NQ; qq++) {
                            const double xq = w.px(qq), zq = w.pz(qq);
                            const double rx = fast_rcp(xq), rz = fast_rcp(zq);
                            const double dq = okc[qq] ? xq * rz : 0.0;
                            const double ta = okc[qq] ? w.vd_()[lane + 64 * qq] : 0.0;
                            dxa[qq] = (ta - w2[qq]) * dq;
                            dza[qq] = okc[qq] ? (-zq * dxa[qq]) * rx - zq : 0.0;
                            if (okc[qq]) tha = fmax(tha, fmax(-dza[qq] * rz, -dxa[qq] * rx));
                        }
                        const double theta_a = uni(fmin(1.0 / wmax(tha), 1.0));
#pragma unroll
                        for (int qq = 0; qq < NQ; qq++) {
                            const double xq = w.px(qq), zq = w.pz(qq);
                            ga += okc[qq] ? fma(theta_a, dxa[qq], xq) * fma(theta_a, dza[qq], zq) : 0.0;
                        }
                        const double sgm = wsum(ga) / gam;
                        mu = uni(sgm * sgm * sgm * gam / (double)n);
                        // ---- corrector right-hand side: A(d t_c) - rho, t_c = cv + cor / x ----
                        wave_lds_sync();
#pragma unroll
                        for (int qq = 0; qq < NQ; qq++) {
                            const double xq = w.px(qq), zq = w.pz(qq);
                            cor[qq] = okc[qq] ? mu - dxa[qq] * dza[qq] : 0.0;
                            const double tq = okc[qq] ? w.vd_()[lane + 64 * qq] + cor[qq] * fast_rcp(xq) : 0.0;
                            vx[lane + 64 * qq] = (okc[qq] ? xq * fast_rcp(zq) : 0.0) * tq;
                        }
                        wave_lds_sync();
                        double Adt2[MR], dmy[MR];
                        w.template Arow<false>(vx, Adt2, dmy);
#pragma unroll
                        for (int r2 = 0; r2 < MR; r2++) if (lane + 64 * r2 < MP) w.um_()[lane + 64 * r2] = okr[r2] ? Adt2[r2] - rhn[r2] : 0.0;
                        wave_lds_sync();
                    }
                    (void)newton_solve<true, PC>(w, okc, okr, rhn, etol, o.max_refine, mu, dy, dx, wv, e, bad, cor STAMP_PASS);
#pragma unroll
                    for (int qq = 0; qq < NQ; qq++) {
                        cv[qq] = w.vd_()[lane + 64 * qq];
                        x[qq] = w.px(qq);
                        z[qq] = w.pz(qq);
                    }
                    if (bad) { stat = PYCLLP_STATUS_NUMERICAL; running = false; }
                    else {
                        // ---- step (primal_normal.cl:158-198) ----
                        double dz[NQ], th = 0.0;
#pragma unroll
                        for (int qq = 0; qq < NQ; qq++) {
                            const double rx = fast_rcp(x[qq]), rz = fast_rcp(z[qq]);
                            dz[qq] = okc[qq] ? ((PC ? cor[qq] : mu) - z[qq] * dx[qq]) * rx - z[qq] : 0.0;
                            if (okc[qq]) th = fmax(th, fmax(-dz[qq] * rz, -dx[qq] * rx));
                        }
                        th = wmax(th);
                        const double theta = uni(fmin(o.r / th, 1.0));
                        wave_lds_sync();
#pragma unroll
                        for (int r2 = 0; r2 < MR; r2++) {
                            const int i = lane + 64 * r2;
                            if (i < MP) {
                                w.ys_()[i] = fma(theta, dy[r2], w.ys_()[i]);
                                w.flr_()[i] = fma(-theta, rhn[r2] - e[r2], rhn[r2]);       // A dx = rho - e
                            }
                        }
#pragma unroll
                        for (int qq = 0; qq < NQ; qq++) {
                            w.px(qq) = fma(theta, dx[qq], x[qq]);
                            w.pz(qq) = fma(theta, dz[qq], z[qq]);
                            w.vd_()[lane + 64 * qq] = okc[qq] ? fma(-theta, wv[qq], cv[qq]) : 0.0;
                        }
                        normr0 = normr; norms0 = norms;
                        fresh = false;
                        wave_lds_sync();
                        it++;
                        if (it >= o.max_iter) running = false;   // status stays ITERATION_LIMIT
                        STAMP(9)
                    }
                }
            }
        }
        wave_lds_sync();
        store_lp(w, okr, lp, stat, it, 1.0, s0.sb, sc, po, du, rx, rz, yg, pobj, dobj, status, iters, defer);
        lp = next_item(queue, lane);
        STAMP(9)
    }
    STAMP_FLUSH(o, blockIdx.x * 4 + (threadIdx.x >> 6))
}

}  // namespace
