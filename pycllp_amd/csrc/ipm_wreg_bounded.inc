// ipm_wreg_bounded.inc -- the register-resident one-LP-per-wavefront kernel (ipm_wreg_kernel) for LPs with UPPER BOUNDS:
//   maximise c'x  subject to  A x = b,  0 <= x <= u        (u_j = +inf: no bound;  u_j = 0: the column is fixed at 0)
// the bounded equality form of a GeneralLP (pycllp_amd/lp.py, GeneralLP.to_bounded_equality_form), any shared A.  On
// wreg_wave.h; compiled by ipm_wreg_bd.hip and ipm_wreg_bdpa.hip.  The step is the one of ipm_group_slot.inc (DESIGN.md
// sections 14 and 15; tests/bounded_twin.py restates it):
//   d = 1 / (z/x + s/t),  t~ = c - A'y + mu/x - mu/t + (s/t) tau,  tau = u - x - t,  mu = delta gamma / (n + m + N_b)
//   M dy = A (d t~) - rho,  dx = d (t~ - A'dy),  dz = (mu - z dx)/x - z,  dt = tau - dx,  ds = (mu - s dt)/t - s
// A column without a bound carries no t, s: every formula is then the one of ipm_wreg_kernel.  A fixed column takes no part in
// the iteration: it ends at x = 0 with the duals z = max(A'y - c, 0), s = max(c - A'y, 0).
// Only the per-column phases are new: gram(), factor<false>(), newton_solve<false> (block substitution + x-space refinement),
// At() and Arow() are the WReg<MB, NQ, DA> members, unchanged.  Differences from ipm_wreg_kernel:
//   * no carried residuals: cv = c - A'y and rho = b - A x are recomputed from the point at the top of every iteration (one
//     A'y and one A x more per iteration), so every verdict is taken on fresh residuals and the path is the twin's;
//   * t and s cross the factorisation and the loop's back edge in 2 NP more doubles per wave BEHIND the wave area
//     (G::WAVE_D(NQ)): the stage, the tile and every other offset of the wave area are those of ipm_wreg_kernel; the bounded
//     plan (wreg_plan_create_bounded) reserves the extra doubles.  x and z wait where ipm_wreg_kernel parks them, t~ where the
//     Newton kernel parks its t (stage_()[0, NP)), d in vd_(), rho in flr_().  u and c are read from global memory;
//   * an LP whose LDL' the Nocedal-Wright guard would have changed has no guarded kernel to go to: it ends NUMERICAL;
//   * a verdict reached inside an iteration (NUMERICAL, ITERATION_LIMIT) is stored at the top of the next pass, where the
//     point's A'y is at hand for the duals of the fixed columns; the point itself is the one the verdict was reached on.
// No warm start, no predictor-corrector, no HSD.
// Written once in wreg_wave.h, for this text and ipm_wreg_bdhsd.inc: the class of a column (col_class), the places of t and s
// (WReg::pt, ps), the per-LP scale factors (bounded_scales), the store of a finished LP (WREG_BOUNDED_STORE) and the tail of the
// step (WREG_BOUNDED_ADVANCE).
// The text serves three units: ipm_wreg_bd.hip (ipm_wreg_bounded_kernel, a shared A), ipm_wreg_bdpa.hip
// (ipm_wreg_bounded_pa_kernel, per-problem values of A on structure tables; DESIGN.md section 18) and ipm_wreg_bddapa.hip
// (ipm_wreg_bounded_dapa_kernel, per-problem dense matrices, an image per wave; DESIGN.md section 25).

namespace {

// PYCLLP_WREG_BOUNDED_PA (defined by ipm_wreg_bdpa.hip in front of this text): per-problem values of A on structure-only
// tables, WReg<MB, NQ, false, true>; the kernel is then ipm_wreg_bounded_pa_kernel<MB, NQ> and takes ag [B, nnz] in the plan's
// CSR order.  The wave's copy of its LP's values sits where t and s sit otherwise (cvl_() = W0 + WAVE_D), so t and s go BEHIND
// it, at the wave-uniform run-time offset WAVE_D + nnzp (nnzp is even: 16-byte alignment stays).  A preprocessor switch, not a
// template argument: the kernel's signature differs, and the shared-A kernels stay instruction for instruction what they were.
// PYCLLP_WREG_BOUNDED_DAPA (defined by ipm_wreg_bddapa.hip): per-problem DENSE matrices, WReg<MB, NQ, true, true>; the kernel is
// then ipm_wreg_bounded_dapa_kernel<MB, NQ> and takes ag [B, m, nd] row-major (nd = n - m: the bounded form ends in the
// identity, which the image leaves out).  The wave's image starts where t and s sit otherwise (wimg_() = W0 + WAVE_D), so t
// and s go BEHIND it, at the wave-uniform run-time offset WAVE_D + img_rows x AS (img_rows is a multiple of 8: the offset stays
// even, 16-byte aligned).  A wave's area: [wave area | image img_rows x AS | t NP | s NP].  The image's pad rows and columns are
// zeroed once per wave by wreg_setup; this text writes behind the wave area only at TS and above, never into the image.
#if defined(PYCLLP_WREG_BOUNDED_DAPA)
template <int MB, int NQ>
__global__ void __launch_bounds__(256, 1)
ipm_wreg_bounded_dapa_kernel(WregTab T, long B, const double* __restrict__ ag, const double* __restrict__ bg,
                             const double* __restrict__ cg, const double* __restrict__ ug, double* __restrict__ xg,
                             double* __restrict__ yg, double* __restrict__ zg, double* __restrict__ sg, double* __restrict__ pobj,
                             double* __restrict__ dobj, int* __restrict__ status, int* __restrict__ iters, int* __restrict__ queue,
                             DevOpts o) {
    using G = WGeo<MB>;
    constexpr int MR = G::MR, MP = G::MP;
    const int TS = G::WAVE_D(NQ) + T.img_rows * T.as;                         // t at W0[TS, TS + NP), s behind it
    extern __shared__ __attribute__((aligned(16))) unsigned char lraw[];
    WReg<MB, NQ, true, true> w;
#elif defined(PYCLLP_WREG_BOUNDED_PA)
template <int MB, int NQ>
__global__ void __launch_bounds__(256, 1)
ipm_wreg_bounded_pa_kernel(WregTab T, long B, const double* __restrict__ ag, const double* __restrict__ bg,
                           const double* __restrict__ cg, const double* __restrict__ ug, double* __restrict__ xg,
                           double* __restrict__ yg, double* __restrict__ zg, double* __restrict__ sg, double* __restrict__ pobj,
                           double* __restrict__ dobj, int* __restrict__ status, int* __restrict__ iters, int* __restrict__ queue,
                           DevOpts o) {
    using G = WGeo<MB>;
    constexpr int MR = G::MR, MP = G::MP;
    const int TS = G::WAVE_D(NQ) + T.nnzp;                                    // t at W0[TS, TS + NP), s behind it
    extern __shared__ __attribute__((aligned(16))) unsigned char lraw[];
    WReg<MB, NQ, false, true> w;
#else
template <int MB, int NQ, bool DA>
__global__ void __launch_bounds__(256, 1)
ipm_wreg_bounded_kernel(WregTab T, long B, const double* __restrict__ bg, const double* __restrict__ cg,
                        const double* __restrict__ ug, double* __restrict__ xg, double* __restrict__ yg, double* __restrict__ zg,
                        double* __restrict__ sg, double* __restrict__ pobj, double* __restrict__ dobj, int* __restrict__ status,
                        int* __restrict__ iters, int* __restrict__ queue, DevOpts o) {
    using G = WGeo<MB>;
    constexpr int MR = G::MR, MP = G::MP, TS = G::WAVE_D(NQ);   // t at W0[TS, TS + NP), s behind it
    extern __shared__ __attribute__((aligned(16))) unsigned char lraw[];
    WReg<MB, NQ, DA> w;
#endif
    USE_AGPR_FORM();
    wreg_setup(w, T, lraw, threadIdx.x);
    const int& lane = w.lane;
    const int m = w.m, n = w.n;
    const bool autoscale = (o.flags & PYCLLP_FLAG_AUTOSCALE) != 0;
    double* vx = w.stage_();
    bool okc[NQ], okr[MR];
    w.masks(okc, okr);

    long lp = next_item(queue, lane);
    STAMP_DECL
    while (lp < B) {
#if defined(PYCLLP_WREG_BOUNDED_PA) || defined(PYCLLP_WREG_BOUNDED_DAPA)
        load_lp_values(w, ag, lp, T.nnz);      // before anything reads A
#endif
        // padded positions read u = 0 (buffer offset past the row): they take no part, like a fixed column
        const __amdgpu_buffer_rsrc_t rc = row_rsrc(cg + lp * n, n), ru = row_rsrc(ug + lp * n, n);
        // PYCLLP_FLAG_AUTOSCALE: b, u / sb and c / sc (else both are 1)
        const LpScales sf = bounded_scales(w, okr, lp, bg, rc, ru, o.flags);
        const double sb = sf.sb, sc = sf.sc;
        // ---- start: z = s = y = 1, x = min(1, u/2), t = u - x (tau = 0); norms for the tolerances ----
        double c2 = 0.0, u2 = 0.0, nbc = 0.0;
#pragma unroll
        for (int qq = 0; qq < NQ; qq++) {
            const unsigned jo = w.coff(qq);
            double cj = buf_ld(rc, jo), uj = buf_ld(ru, jo);
            if (autoscale) { cj = cj / sc; uj = uj / sb; }
            const auto [a, bq] = col_class(uj);
            c2 += a ? cj * cj : 0.0;
            u2 += bq ? uj * uj : 0.0;
            nbc += bq ? 1.0 : 0.0;
            const double xq = bq ? fmin(1.0, 0.5 * uj) : 1.0;
            w.px(qq) = xq;
            w.pz(qq) = 1.0;
            w.pt(TS, qq) = bq ? uj - xq : 1.0;
            w.ps(TS, qq) = 1.0;
        }
        double b2 = 0.0;
#pragma unroll
        for (int r2 = 0; r2 < MR; r2++) {
            const int i = lane + 64 * r2;
            double bi = okr[r2] ? bg[lp * m + i] : 0.0;
            if (autoscale) bi = bi / sb;
            b2 = fma(bi, bi, b2);
            if (i < MP) { w.bs_()[i] = bi; w.ys_()[i] = okr[r2] ? 1.0 : 0.0; }
        }
        wave_lds_sync();
        const double nb2 = wsum(b2), nc2 = wsum(c2), nu2 = wsum(u2);
        const double tol_r = uni(o.eps * (1.0 + sqrt(nb2))), tol_s = uni(o.eps * (1.0 + sqrt(nc2)));
        const double tol_u = uni(o.eps * (1.0 + sqrt(nu2))), etol = uni(o.refine_tol * (1.0 + sqrt(nb2)));
        const double ncomp = uni((double)(n + m) + wsum(nbc));
        double normr0 = 1e300, norms0 = 1e300;
        int it = 0, forced = -1;      // forced >= 0: the verdict reached inside the last pass, stored by this one
        bool running = true;

        while (running) {
            double x[NQ], z[NQ], cq[NQ], uq[NQ], v[NQ], rho[MR];
#pragma unroll
            for (int qq = 0; qq < NQ; qq++) { const unsigned jo = w.coff(qq); cq[qq] = buf_ld(rc, jo); uq[qq] = buf_ld(ru, jo); }
            w.At(w.ys_(), v);          // (c and u in flight meanwhile)
#pragma unroll
            for (int qq = 0; qq < NQ; qq++) {
                if (autoscale) { cq[qq] = cq[qq] / sc; uq[qq] = uq[qq] / sb; }
                x[qq] = w.px(qq);
                z[qq] = w.pz(qq);
                vx[lane + 64 * qq] = col_class(uq[qq]).a ? x[qq] : 0.0;
            }
            wave_lds_sync();
            {
                double Ax[MR], dm[MR];
                w.template Arow<false>(vx, Ax, dm);
#pragma unroll
                for (int r2 = 0; r2 < MR; r2++) rho[r2] = okr[r2] ? w.bs_()[lane + 64 * r2] - Ax[r2] : 0.0;
            }
            // ---- dual infeasibility, complementarity, bound residual, objectives of THIS point ----
            double s2 = 0.0, gam = 0.0, tau2 = 0.0, pp = 0.0, dd = 0.0, r2s = 0.0;
#pragma unroll
            for (int qq = 0; qq < NQ; qq++) {
                const auto [a, bq] = col_class(uq[qq]);
                const double tq = w.pt(TS, qq), sq = w.ps(TS, qq);
                const double sgq = a ? (cq[qq] - v[qq]) + z[qq] - (bq ? sq : 0.0) : 0.0;
                const double tau = bq ? (uq[qq] - x[qq]) - tq : 0.0;
                s2 = fma(sgq, sgq, s2);
                tau2 = fma(tau, tau, tau2);
                gam += a ? x[qq] * z[qq] : 0.0;
                gam += bq ? sq * tq : 0.0;
                pp += a ? cq[qq] * x[qq] : 0.0;
                dd += bq ? uq[qq] * sq : 0.0;
            }
#pragma unroll
            for (int r2 = 0; r2 < MR; r2++) {
                const int i = lane + 64 * r2;
                dd = fma((i < MP) ? w.bs_()[i] : 0.0, (i < MP) ? w.ys_()[i] : 0.0, dd);
                r2s = fma(rho[r2], rho[r2], r2s);
            }
            s2 = wsum(s2); gam = wsum(gam); tau2 = wsum(tau2);
            const double po = wsum(pp), du = wsum(dd);
            const double norms = uni(sqrt(s2)), normr = uni(sqrt(wsum(r2s))), ntau = uni(sqrt(tau2));
            const double mu = uni(o.delta * gam / ncomp);
            // ---- stop tests ----
            int stat = PYCLLP_STATUS_ITERATION_LIMIT;
            if (forced >= 0) { stat = forced; running = false; }
            else if (!(isfinite(normr) && isfinite(norms) && isfinite(gam) && isfinite(ntau))) { stat = PYCLLP_STATUS_NUMERICAL; running = false; }
            else if (normr <= tol_r && norms <= tol_s && gam <= o.eps * (1.0 + fabs(po)) && ntau <= tol_u) { stat = PYCLLP_STATUS_OPTIMAL; running = false; }
            else if (normr > 10.0 * normr0 && normr > PYCLLP_GROWTH_FLOOR * tol_r) { stat = PYCLLP_STATUS_PRIMAL_INFEASIBLE; running = false; }
            else if (norms > 10.0 * norms0 && norms > PYCLLP_GROWTH_FLOOR * tol_s) { stat = PYCLLP_STATUS_DUAL_INFEASIBLE; running = false; }
            if (!running) {
                // ---- store the LP; the reduced cost of a fixed column is c - A'y ----
                WREG_BOUNDED_STORE(1.0, cq[qq] - v[qq])
                break;
            }
            // ---- d = 1 / (z/x + s/t), t~ = c - A'y + mu/x - mu/t + (s/t) tau; rhs = A (d t~) - rho, diag(M) ----
            double tt[NQ];
#pragma unroll
            for (int qq = 0; qq < NQ; qq++) {
                const auto [a, bq] = col_class(uq[qq]);
                const double tq = w.pt(TS, qq), sq = w.ps(TS, qq);
                const double rx = fast_rcp(x[qq]), rt = fast_rcp(tq);
                const double tau = (uq[qq] - x[qq]) - tq;
                double dq, tn;
                if (bq) {
                    dq = fast_rcp(fma(z[qq], rx, sq * rt));
                    tn = (cq[qq] - v[qq]) + mu * rx - mu * rt + (sq * rt) * tau;
                } else {
                    dq = x[qq] * fast_rcp(z[qq]);
                    tn = (cq[qq] - v[qq]) + mu * rx;
                }
                dq = a ? dq : 0.0;
                tt[qq] = a ? tn : 0.0;
                vx[lane + 64 * qq] = dq * tt[qq];
                w.vd_()[lane + 64 * qq] = dq;
            }
            wave_lds_sync();
            double beta2;
            {
                double Adt[MR], Md[MR], bmax = 0.0;
                w.template Arow<true>(vx, Adt, Md);
#pragma unroll
                for (int r2 = 0; r2 < MR; r2++) {
                    const int i = lane + 64 * r2;
                    if (i < MP) { w.um_()[i] = okr[r2] ? Adt[r2] - rho[r2] : 0.0; w.flr_()[i] = rho[r2]; }
                    bmax = fmax(bmax, okr[r2] ? fabs(Md[r2]) : 0.0);
                }
                beta2 = wmax(bmax);
                wave_lds_sync();
                // ---- M = A diag(d) A' into registers; factor ----
                w.gram(Md);
            }
            // t~, x and z wait in the stage while factor and solve have the registers
#pragma unroll
            for (int qq = 0; qq < NQ; qq++) {
                w.stage_()[lane + 64 * qq] = tt[qq];
                w.px(qq) = x[qq];
                w.pz(qq) = z[qq];
            }
            const bool viol = w.template factor<false>(beta2, o.pivot_floor STAMP_PASS);
            if (viol) { forced = PYCLLP_STATUS_NUMERICAL; continue; }   // the guard would have bitten: no guarded kernel here
            double dy[MR], wv[NQ], dx[NQ], e[MR], rhn[MR];
            bool bad;
#pragma unroll
            for (int r2 = 0; r2 < MR; r2++) rhn[r2] = (lane + 64 * r2 < MP) ? w.flr_()[lane + 64 * r2] : 0.0;
            (void)newton_solve<false>(w, okc, okr, rhn, etol, o.max_refine, mu, dy, dx, wv, e, bad, nullptr STAMP_PASS);
            if (bad) { forced = PYCLLP_STATUS_NUMERICAL; continue; }
            // ---- step: theta = min(r / max(0, -dx/x, -dz/z, -dt/t, -ds/s), 1) ----
            double th = 0.0;
            double dz[NQ], dt[NQ], ds[NQ];
#pragma unroll
            for (int qq = 0; qq < NQ; qq++) {
                const unsigned jo = w.coff(qq);
                double uj = buf_ld(ru, jo);
                if (autoscale) uj = uj / sb;
                const auto [a, bq] = col_class(uj);
                const double xq = w.px(qq), zq = w.pz(qq);
                const double tq = w.pt(TS, qq), sq = w.ps(TS, qq);
                const double rx = fast_rcp(xq), rz = fast_rcp(zq), rt = fast_rcp(tq);
                const double tau = (uj - xq) - tq;
                dz[qq] = a ? (mu - zq * dx[qq]) * rx - zq : 0.0;
                dt[qq] = bq ? tau - dx[qq] : 0.0;
                ds[qq] = bq ? (mu - sq * dt[qq]) * rt - sq : 0.0;
                if (a) th = fmax(th, fmax(-dz[qq] * rz, -dx[qq] * rx));
                if (bq) th = fmax(th, fmax(-dt[qq] * rt, -ds[qq] * fast_rcp(sq)));
            }
            th = wmax(th);
            const double theta = uni(fmin(o.r / th, 1.0));
            wave_lds_sync();
            WREG_BOUNDED_ADVANCE()
            normr0 = normr; norms0 = norms;
            wave_lds_sync();
            it++;
            if (it >= o.max_iter) forced = PYCLLP_STATUS_ITERATION_LIMIT;
        }
        wave_lds_sync();
        lp = next_item(queue, lane);
    }
}

}  // namespace
