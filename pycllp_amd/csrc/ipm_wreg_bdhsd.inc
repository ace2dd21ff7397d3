// ipm_wreg_bdhsd.inc -- ipm_wreg_bounded_hsd_kernel<MB, NQ, DA>: the wavefront-per-LP kernel for LPs with UPPER BOUNDS on one
// shared A, on the homogeneous self-dual embedding (DESIGN.md section 27).
//   maximise c'x  subject to  A x = b,  0 <= x <= u        (u_j = +inf: no bound;  u_j = 0: the column is fixed at 0)
// The system is section 26's, formula for formula (csrc/ipm_group_bdhsd.inc; tests/bounded_hsd_twin.py restates it):
//     rho = b tau - A x,   omega = u tau - x - t (bnd),   sigma = c tau - A'y + z - s,   phi = b'y + u's - c'x + kappa
//     mu = (x'z + s't + tau kappa) / (N_act + N_bnd + 1),   dmu = delta mu,   eta = 1 - delta
//     zx = z/x,  st = s/t,  d = 1/(zx + st),  w = d st,  h = t - dmu/s + eta omega,  r0 = eta sigma + dmu/x - z
//     dr = d r0 + w h,  dc = d c + w u
//     M = A d A',  M p = A dc - b,  M q = A dr - eta rho                      (ONE factorisation, two right-hand sides)
//     e = c - A'p,  uu = d e + w u,  v = d (r0 - A'q) + w h
//     dtau = (eta phi + b'q + dmu/tau - kappa - c'v + sum_bnd u w (r0 - A'q - zx h)) / (sum d e^2 + sum_bnd zx w u^2 + kappa/tau)
//     dy = p dtau + q,  dx = uu dtau + v,  dz = (dmu - z dx)/x - z,  dkappa = dmu/tau - kappa - (kappa/tau) dtau
//     t >= s:  dt = eta omega + u dtau - dx,  ds = (dmu - s dt)/t - s
//     t <  s:  ds = dz + eta sigma + c dtau - A'dy,  dt = dmu/s - t - (t/s) ds
// The wave mechanics are hsd_wreg_kernel's (ipm_wreg_hsd.inc): one loop around the ONE copy of the block substitution (pass 0
// solves for p, pass 1 for q and combines them through dtau, later passes refine A dx - b dtau = eta rho in x-space),
// factor<true> with the floor vector pivot_floor^2 |M_jj|, tau and kappa wave-uniform through uni(); the LDS plan is
// ipm_wreg_bounded_kernel's (wreg_plan_create_bounded: t at W0[TS, TS + NP), s behind it).  What this text has in common with
// either of the two is written once, in wreg_wave.h:
//   with ipm_wreg_bounded.inc   col_class, WReg::pt / ps, bounded_scales, WREG_BOUNDED_STORE, WREG_BOUNDED_ADVANCE
//   with ipm_wreg_hsd.inc       WREG_HSD_RAYS / WREG_HSD_VERDICT (the stop verdict; forced and the loop bound go in front of it),
//                               hsd_hand_over_p, WREG_HSD_DY, WREG_HSD_REFINE_TAIL, hsd_dkappa, hsd_ratio0
// The per-column arithmetic (d, r0, h, w, the two dt / ds branches), the start point and the control flow are this kernel's own.
// What waits where, per wave:
//   x, z      px(), pz() across the factorisation, the passes and the loop's back edge (registers across gram(), which stages
//             through the whole stage on term tables)
//   t, s      pt(), ps() (W0[TS ..), W0[TS + NP ..)): written by the start and by the step only
//   sigma     stage_()[0, NP) from the factorisation to pass 1, which forms r0 again from it and the parked x, z (the same
//             expression as in front of the factorisation: the same bits); behind pass 1 the place is vx, the staging of A dx
//   vd_()     d for Arow<true> and gram(); A'p from pass 0 to pass 1; from pass 1 on g = eta sigma + c dtau - A'dy, which every
//             refinement pass corrects by its A'eta: the second branch is then ds = dz + g, and sigma need not outlive pass 1
//   flr_()    the floor vector until factor<true> returns; p from pass 0 to pass 1 (hsd_wreg_kernel's pv).  rho is NOT parked
//             there (as ipm_wreg_bounded_kernel does): it stays in registers, as in hsd_wreg_kernel
//   h, omega, w, d are formed again from x, z, t, s and u where a pass needs them; c and u come back through the buffer descriptors.
// So two N-vectors behind the wave area suffice and the kernel runs on the handle's bounded plan, at its waves per workgroup.
// Every verdict is taken at the top of a pass, on the residuals and objectives of the point it returns (the loop bound first, as
// in the oracle); a verdict reached inside a pass (the guard would have bitten, a non-finite step: NUMERICAL) is stored by the
// next one, as in ipm_wreg_bounded_kernel.  Statuses 2 and 4 leave the certificate as it stands; 0 and 5 divide x, y, z, s and the
// objectives by tau.  A fixed column ends at x = 0 with z = max(-r, 0), s = max(r, 0), r = c tau - A'y, on the same scaling.
// No warm start, no predictor-corrector, no guarded kernel to defer to.
namespace {

template <int MB, int NQ, bool DA>
__global__ void __launch_bounds__(256, 1)
ipm_wreg_bounded_hsd_kernel(WregTab T, long B, const double* __restrict__ bg, const double* __restrict__ cg,
                            const double* __restrict__ ug, double* __restrict__ xg, double* __restrict__ yg,
                            double* __restrict__ zg, double* __restrict__ sg, double* __restrict__ pobj,
                            double* __restrict__ dobj, int* __restrict__ status, int* __restrict__ iters,
                            int* __restrict__ queue, DevOpts o) {
    using G = WGeo<MB>;
    constexpr int MR = G::MR, MP = G::MP, TS = G::WAVE_D(NQ);   // t at W0[TS, TS + NP), s behind it
    extern __shared__ __attribute__((aligned(16))) unsigned char lraw[];
    WReg<MB, NQ, DA> w;
    USE_AGPR_FORM();
    wreg_setup(w, T, lraw, threadIdx.x);
    const int& lane = w.lane;
    const int m = w.m, n = w.n;
    const bool autoscale = (o.flags & PYCLLP_FLAG_AUTOSCALE) != 0;
    double* vx = w.stage_();
    double* pv = w.flr_();          // p = M^-1 (A dc - b): the floor vector is dead once the factor exists
    bool okc[NQ], okr[MR];
    w.masks(okc, okr);
    // option-derived doubles stay out of loop-invariant VGPRs (DESIGN.md section 26): formed from the SGPR where they are used
#define BH_ETA (1.0 - sopaque(o.delta))
#define BH_EINF (100.0 * sopaque(o.eps))

    long lp = next_item(queue, lane);
    STAMP_DECL
    while (lp < B) {
        // padded positions read u = 0 (buffer offset past the row): they take no part, like a fixed column
        const __amdgpu_buffer_rsrc_t rc = row_rsrc(cg + lp * n, n), ru = row_rsrc(ug + lp * n, n);
        // PYCLLP_FLAG_AUTOSCALE: b, u / sb and c / sc (else both are 1)
        const LpScales sf = bounded_scales(w, okr, lp, bg, rc, ru, o.flags);
        const double sb = sf.sb, sc = sf.sc;
        // ---- start: x = z = 1 (act), t = s = 1 (bnd), y = 0, tau = kappa = 1; norms for the tolerances ----
        double c2 = 0.0, bu2 = 0.0, cnt = 0.0;
#pragma unroll
        for (int qq = 0; qq < NQ; qq++) {
            const unsigned jo = w.coff(qq);
            double cj = buf_ld(rc, jo), uj = buf_ld(ru, jo);
            if (autoscale) { cj = cj / sc; uj = uj / sb; }
            const auto [a, bq] = col_class(uj);
            c2 += a ? cj * cj : 0.0;
            bu2 += bq ? uj * uj : 0.0;
            cnt += (a ? 1.0 : 0.0) + (bq ? 1.0 : 0.0);
            w.px(qq) = 1.0;
            w.pz(qq) = 1.0;
            w.pt(TS, qq) = 1.0;
            w.ps(TS, qq) = 1.0;
        }
#pragma unroll
        for (int r2 = 0; r2 < MR; r2++) {
            const int i = lane + 64 * r2;
            double bi = okr[r2] ? bg[lp * m + i] : 0.0;
            if (autoscale) bi = bi / sb;
            bu2 = fma(bi, bi, bu2);
            if (i < MP) { w.bs_()[i] = bi; w.ys_()[i] = 0.0; }
        }
        wave_lds_sync();
        const double nbn = uni(sqrt(wsum(bu2))), ncn = uni(sqrt(wsum(c2)));      // nb = sqrt(|b|^2 + |u_bnd|^2), nc = |c_act|
        const double ncomp = uni(wsum(cnt) + 1.0);                                // N_act + N_bnd + 1
        double tau = 1.0, kap = 1.0;
        int it = 0, forced = -1;      // forced >= 0: the verdict reached inside the last pass, stored by this one
        bool running = true;

        while (running) {
            double x[NQ], z[NQ], cq[NQ], uq[NQ], v[NQ], sgm[NQ], rho[MR];
#pragma unroll
            for (int qq = 0; qq < NQ; qq++) { const unsigned jo = w.coff(qq); cq[qq] = buf_ld(rc, jo); uq[qq] = buf_ld(ru, jo); }
            w.At(w.ys_(), v);          // (c and u in flight meanwhile)
            // ---- sigma, omega, complementarity, objectives of THIS point; d and the acting part of x for rho ----
            double s2 = 0.0, om2 = 0.0, gam = 0.0, pp = 0.0, dd = 0.0;
#pragma unroll
            for (int qq = 0; qq < NQ; qq++) {
                const int j = lane + 64 * qq;
                if (autoscale) { cq[qq] = cq[qq] / sc; uq[qq] = uq[qq] / sb; }
                x[qq] = w.px(qq);
                z[qq] = w.pz(qq);
                const auto [a, bq] = col_class(uq[qq]);
                const double tq = w.pt(TS, qq), sq = w.ps(TS, qq);
                const double sgq = a ? fma(cq[qq], tau, z[qq] - v[qq]) - (bq ? sq : 0.0) : 0.0;
                const double om = bq ? fma(uq[qq], tau, -x[qq]) - tq : 0.0;
                sgm[qq] = sgq;
                s2 = fma(sgq, sgq, s2);
                om2 = fma(om, om, om2);
                gam += a ? x[qq] * z[qq] : 0.0;
                gam += bq ? sq * tq : 0.0;
                pp += a ? cq[qq] * x[qq] : 0.0;
                dd += bq ? uq[qq] * sq : 0.0;
                const double stq = bq ? sq * fast_rcp(tq) : 0.0;
                vx[j] = a ? x[qq] : 0.0;
                w.vd_()[j] = a ? fast_rcp(fma(z[qq], fast_rcp(x[qq]), stq)) : 0.0;
            }
            wave_lds_sync();
            {
                double Ax[MR], dm[MR];
                w.template Arow<false>(vx, Ax, dm);
#pragma unroll
                for (int r2 = 0; r2 < MR; r2++) {
                    const int i = lane + 64 * r2;
                    rho[r2] = okr[r2] ? fma(w.bs_()[i], tau, -Ax[r2]) : 0.0;
                    om2 = fma(rho[r2], rho[r2], om2);
                    dd = fma((i < MP) ? w.bs_()[i] : 0.0, (i < MP) ? w.ys_()[i] : 0.0, dd);
                }
            }
            s2 = wsum(s2); gam = wsum(gam);
            const double po = wsum(pp), du = wsum(dd);
            const double norms = uni(sqrt(s2)), normr = uni(sqrt(wsum(om2)));      // normr = sqrt(|rho|^2 + |omega|^2)
            // ---- stop tests (oracle hsd_one_raw on the expansion): the loop bound, NUMERICAL, OPTIMAL, a primal / dual ray ----
            int stat = PYCLLP_STATUS_ITERATION_LIMIT;
            {
                WREG_HSD_RAYS(BH_EINF)
                if (forced >= 0) { stat = forced; running = false; }
                else if (it >= o.max_iter) running = false;
                else WREG_HSD_VERDICT(o.eps * (1.0 + nbn), o.eps * (1.0 + ncn))
            }
            if (!running) {
                // ---- store the LP; the reduced cost of a fixed column is c tau - A'y ----
                // optimal (and iteration-limit) points leave the homogeneous scaling; certificates stay
                const double rt = (stat == PYCLLP_STATUS_OPTIMAL || stat == PYCLLP_STATUS_ITERATION_LIMIT) ? 1.0 / tau : 1.0;
                WREG_BOUNDED_STORE(rt, fma(cq[qq], tau, -v[qq]))
                break;
            }
            const double dmu = uni(o.delta * ((gam + tau * kap) / ncomp));
            const double phi = uni(du - po + kap);
            // ---- dr = d r0 + w h, dc = d c + w u; A dr with diag(M), A dc ----
            wave_lds_sync();
            double dcv[NQ];
#pragma unroll
            for (int qq = 0; qq < NQ; qq++) {
                const int j = lane + 64 * qq;
                const auto [a, bq] = col_class(uq[qq]);
                const double tq = w.pt(TS, qq), sq = w.ps(TS, qq);
                const double dq = w.vd_()[j];
                const double wq = dq * (bq ? sq * fast_rcp(tq) : 0.0);
                const double om = bq ? fma(uq[qq], tau, -x[qq]) - tq : 0.0;
                const double hq = bq ? fma(BH_ETA, om, tq - dmu * fast_rcp(sq)) : 0.0;
                const double r0q = a ? fma(BH_ETA, sgm[qq], fma(dmu, fast_rcp(x[qq]), -z[qq])) : 0.0;
                dcv[qq] = a ? fma(dq, cq[qq], bq ? wq * uq[qq] : 0.0) : 0.0;
                vx[j] = fma(dq, r0q, wq * hq);
            }
            wave_lds_sync();
            double rq[MR], beta2;
            {
                double Adr[MR], Adc[MR], Md[MR], dummy[MR], bmax = 0.0;
                w.template Arow<true>(vx, Adr, Md);
                wave_lds_sync();
#pragma unroll
                for (int qq = 0; qq < NQ; qq++) vx[lane + 64 * qq] = dcv[qq];
                wave_lds_sync();
                w.template Arow<false>(vx, Adc, dummy);
                const double pf = sopaque(o.pivot_floor);
#pragma unroll
                for (int r2 = 0; r2 < MR; r2++) {
                    const int i = lane + 64 * r2;
                    rq[r2] = okr[r2] ? fma(-BH_ETA, rho[r2], Adr[r2]) : 0.0;
                    if (i < MP) {
                        w.um_()[i] = okr[r2] ? Adc[r2] - w.bs_()[i] : 0.0;        // right-hand side of p
                        w.flr_()[i] = pf * pf * fabs(Md[r2]);                     // floor of column i
                    }
                    bmax = fmax(bmax, okr[r2] ? fabs(Md[r2]) : 0.0);
                }
                beta2 = uni(wmax(bmax));
                wave_lds_sync();
                STAMP(0)
                // ---- M = A diag(d) A' into registers ----
                w.gram(Md);
                STAMP(1)
            }
            // sigma, x and z wait in the stage while factor and the solves have the registers
#pragma unroll
            for (int qq = 0; qq < NQ; qq++) {
                w.stage_()[lane + 64 * qq] = sgm[qq];
                w.px(qq) = x[qq];
                w.pz(qq) = z[qq];
            }
            const bool viol = w.template factor<true>(beta2, 0.0 STAMP_PASS);
            if (viol) { forced = PYCLLP_STATUS_NUMERICAL; continue; }   // the guard would have bitten: no guarded kernel here
            // ---- one loop around the ONE copy of the block substitution: pass 0 solves for p, pass 1 for q and combines them
            //      through dtau, the following passes are the x-space refinement ----
            double dx[NQ], dy[MR], rhot[MR];
            double dtau = 0.0, etol_it = 0.0;
            bool bad = false;
            int pass = 0;
            for (;;) {
                // (u and, for pass 1, c come back from memory, in flight while the substitution runs)
                double c2q[NQ], u2q[NQ];
                if (pass > 0) {
#pragma unroll
                    for (int qq = 0; qq < NQ; qq++) u2q[qq] = buf_ld(ru, w.coff(qq));
                }
                if (pass == 1) {
#pragma unroll
                    for (int qq = 0; qq < NQ; qq++) c2q[qq] = buf_ld(rc, w.coff(qq));
                }
                w.solve();
                STAMP(7)
                double w2[NQ];
                w.At(w.um_(), w2);
                bool more = true;
                if (pass == 0) {
                    // A'p is kept (in d's place); p moves to pv, q's right-hand side into um
#pragma unroll
                    for (int qq = 0; qq < NQ; qq++) w.vd_()[lane + 64 * qq] = w2[qq];
                    wave_lds_sync();
                    hsd_hand_over_p(w, rq);
                } else {
                    if (autoscale) {
#pragma unroll
                        for (int qq = 0; qq < NQ; qq++) u2q[qq] = u2q[qq] / sb;
                    }
                    if (pass == 1) {
                        if (autoscale) {
#pragma unroll
                            for (int qq = 0; qq < NQ; qq++) c2q[qq] = c2q[qq] / sc;
                        }
                        double dsum = 0.0, nsum = 0.0, bqs = 0.0;
                        double uu[NQ];
#pragma unroll
                        for (int qq = 0; qq < NQ; qq++) {
                            const int j = lane + 64 * qq;
                            const auto [a, bq] = col_class(u2q[qq]);
                            const double xq = w.px(qq), zq = w.pz(qq), tq = w.pt(TS, qq), sq = w.ps(TS, qq);
                            const double sgq = w.stage_()[j], ap = w.vd_()[j];
                            const double rx = fast_rcp(xq);
                            const double zxq = zq * rx;
                            const double stq = bq ? sq * fast_rcp(tq) : 0.0;
                            const double om = bq ? fma(u2q[qq], tau, -xq) - tq : 0.0;
                            const double dq = a ? fast_rcp(zxq + stq) : 0.0;
                            const double wq = dq * stq;
                            const double hq = bq ? fma(BH_ETA, om, tq - dmu * fast_rcp(sq)) : 0.0;
                            const double r0q = a ? fma(BH_ETA, sgq, fma(dmu, rx, -zq)) : 0.0;
                            const double wu = bq ? wq * u2q[qq] : 0.0;
                            const double cp = a ? c2q[qq] - ap : 0.0;                 // e = c - A'p
                            const double vq = fma(dq, r0q - w2[qq], wq * hq);         // v = d (r0 - A'q) + w h
                            uu[qq] = fma(dq, cp, wu);
                            dx[qq] = vq;
                            dsum = fma(dq * cp, cp, dsum);
                            dsum += bq ? zxq * wu * u2q[qq] : 0.0;
                            nsum += a ? c2q[qq] * vq : 0.0;
                            nsum -= bq ? wu * (r0q - w2[qq] - zxq * hq) : 0.0;
                        }
#pragma unroll
                        for (int r2 = 0; r2 < MR; r2++) {
                            const int i = lane + 64 * r2;
                            bqs += (i < MP) ? w.bs_()[i] * w.um_()[i] : 0.0;          // b'q
                        }
                        const double den = wsum(dsum) + kap / tau;
                        const double num = fma(BH_ETA, phi, dmu / tau - kap) + wsum(bqs) - wsum(nsum);
                        dtau = uni(num / den);
                        WREG_HSD_DY(BH_ETA)
#pragma unroll
                        for (int qq = 0; qq < NQ; qq++) {
                            const int j = lane + 64 * qq;
                            const bool a = col_class(u2q[qq]).a;
                            dx[qq] = fma(uu[qq], dtau, dx[qq]);                                   // dx = uu dtau + v
                            const double wv = fma(w.vd_()[j], dtau, w2[qq]);                      // A'dy = A'p dtau + A'q
                            w.vd_()[j] = a ? fma(BH_ETA, w.stage_()[j], fma(c2q[qq], dtau, -wv)) : 0.0;   // g = eta sigma + c dtau - A'dy
                        }
                        etol_it = uni(o.refine_tol * (1.0 + nbn) * fmax(tau, kap));
                    } else {
#pragma unroll
                        for (int qq = 0; qq < NQ; qq++) {
                            const int j = lane + 64 * qq;
                            const auto [a, bq] = col_class(u2q[qq]);
                            const double tq = w.pt(TS, qq), sq = w.ps(TS, qq);
                            const double stq = bq ? sq * fast_rcp(tq) : 0.0;
                            const double dq = a ? fast_rcp(fma(w.pz(qq), fast_rcp(w.px(qq)), stq)) : 0.0;
                            dx[qq] = fma(dq, w2[qq], dx[qq]);
                            w.vd_()[j] += a ? w2[qq] : 0.0;                                       // A'dy -= A'eta
                        }
#pragma unroll
                        for (int r2 = 0; r2 < MR; r2++) dy[r2] -= (lane + 64 * r2 < MP) ? w.um_()[lane + 64 * r2] : 0.0;
                    }
                    WREG_HSD_REFINE_TAIL(col_class(u2q[qq]).a)
                }
                if (!more) break;
                pass++;
            }
            if (__any(bad) || !isfinite(dtau)) { forced = PYCLLP_STATUS_NUMERICAL; continue; }
            // ---- step: ratio test over x, z, t, s, tau, kappa; the two branches for dt, ds switched at t < s ----
            const double dkap = hsd_dkappa(dmu, tau, kap, dtau);
            double dz[NQ], dt[NQ], ds[NQ], th = hsd_ratio0(tau, kap, dtau, dkap);
#pragma unroll
            for (int qq = 0; qq < NQ; qq++) {
                const int j = lane + 64 * qq;
                double uj = buf_ld(ru, w.coff(qq));
                if (autoscale) uj = uj / sb;
                const auto [a, bq] = col_class(uj);
                const double xq = w.px(qq), zq = w.pz(qq), tq = w.pt(TS, qq), sq = w.ps(TS, qq);
                const double rx = fast_rcp(xq), rz = fast_rcp(zq), rt = fast_rcp(tq), rs = fast_rcp(sq);
                const double om = bq ? fma(uj, tau, -xq) - tq : 0.0;
                dx[qq] = a ? dx[qq] : 0.0;
                dz[qq] = a ? (dmu - zq * dx[qq]) * rx - zq : 0.0;
                // (the multiplier of the other one's rounding error is min(s/t, t/s): DESIGN.md section 26)
                const double dt1 = fma(uj, dtau, BH_ETA * om) - dx[qq];
                const double ds1 = (dmu - sq * dt1) * rt - sq;
                const double ds2 = dz[qq] + w.vd_()[j];
                const double dt2 = fma(dmu, rs, -tq) - (tq * rs) * ds2;
                const bool first = tq >= sq;
                dt[qq] = bq ? (first ? dt1 : dt2) : 0.0;
                ds[qq] = bq ? (first ? ds1 : ds2) : 0.0;
                if (a) th = fmax(th, fmax(-dz[qq] * rz, -dx[qq] * rx));
                if (bq) th = fmax(th, fmax(-dt[qq] * rt, -ds[qq] * rs));
            }
            th = wmax(th);
            const double theta = uni(fmin(o.r / th, 1.0));
            wave_lds_sync();
            WREG_BOUNDED_ADVANCE()
            tau = uni(fma(theta, dtau, tau)); kap = uni(fma(theta, dkap, kap));
            wave_lds_sync();
            it++;
            STAMP(9)
        }
        wave_lds_sync();
        lp = next_item(queue, lane);
    }
    STAMP_FLUSH(o, blockIdx.x * 4 + (threadIdx.x >> 6))
#undef BH_ETA
#undef BH_EINF
}

}  // namespace
