// ipm_group_bdhsd.inc -- ipm_bounded_hsd_kernel<MP, NP>: the lane-group kernel for LPs with UPPER BOUNDS on one shared
// A = [A_dense | I], on the homogeneous self-dual embedding (DESIGN.md section 26).
//   maximise c'x  subject to  A x = b,  0 <= x <= u        (u_j = +inf: no bound;  u_j = 0: the column is fixed at 0)
// The machinery is hsd_group_kernel's (ipm_group_hsd.inc: GWaveH, one factorisation with two right-hand sides carried through the
// sweep, At_times2, backward2, the own-diagonal pivot floor) and the t, s, u phases are ipm_group_slot_body.inc's; what is new is
// the reduced Newton system with bounds -- the exact Schur complement of hsd_one_raw (oracle/ipm_dense_ref.c) on the explicit
// expansion Ae = [[A_act, 0], [E_bnd, I]], be = (b; u_bnd), ce = (c_act; 0), duals (y; .), dual slacks (z; s):
//     rho = b tau - A x,   omega = u tau - x - t (bnd),   sigma = c tau - A'y + z - s,   phi = b'y + u's - c'x + kappa
//     mu = (x'z + s't + tau kappa) / (N_act + N_bnd + 1),   dmu = delta mu,   eta = 1 - delta
//     zx = z/x,  st = s/t,  d = 1/(zx + st),  w = d st,  h = t - dmu/s + eta omega,  r0 = eta sigma + dmu/x - z
//     dr = d r0 + w h,  dc = d c + w u
//     M = A d A',  M p = A dc - b,  M q = A dr - eta rho                      (ONE factorisation, two right-hand sides)
//     e = c - A'p,  uu = d e + w u,  v = dr - d A'q
//     dtau = (eta phi + b'q + dmu/tau - kappa - c'v + sum_bnd u w (r0 - A'q - zx h)) / (sum d e^2 + sum_bnd zx w u^2 + kappa/tau)
//     dy = p dtau + q,  dx = uu dtau + v,  dz = (dmu - z dx)/x - z,  dkappa = dmu/tau - kappa - (kappa/tau) dtau
//     t >= s:  dt = eta omega + u dtau - dx,  ds = (dmu - s dt)/t - s
//     t <  s:  ds = dz + eta sigma + c dtau - A'dy,  dt = dmu/s - t - (t/s) ds
// (bnd(q): 0 < u < inf; everything indexed by bnd is absent elsewhere).  The two branches for dt, ds are not a refinement: with
// the first pair alone an active upper bound (t ~ 1e-11) multiplies dt's rounding error, ~eps u, by s/t into ds and the dual
// residual grows before the stop test is met; with the second alone a basic column (s ~ 1e-13) does the same to dt through
// t/s.  Switched at t < s neither multiplier exceeds 1.
// Statuses 2 and 4 leave the certificate as it stands; 0 and 5 divide x, y, z, s and the objectives by tau.  A fixed column ends
// at x = 0 with z = max(-r, 0), s = max(r, 0), r = c tau - A'y, on the same scaling.
// Registers: seven N-vectors per slot (x, z, t, s, u, c, A'y) plus tau, kappa; the kernel runs PYCLLP_WPB_BOUNDED waves per
// workgroup, one per SIMD, with the whole register file per lane, as ipm_bounded_kernel.

template <int MP, int NP>
__global__ void __launch_bounds__(PYCLLP_WPB_BOUNDED * 64)
ipm_bounded_hsd_kernel(int m, int n, long B, const double* __restrict__ Ag, const double* __restrict__ bg,
                       const double* __restrict__ cg, const double* __restrict__ ug, double* __restrict__ xg,
                       double* __restrict__ yg, double* __restrict__ zg, double* __restrict__ sg, double* __restrict__ pobj,
                       double* __restrict__ dobj, int* __restrict__ status, int* __restrict__ iters, int* __restrict__ queue,
                       DevOpts o) {
    constexpr bool SL = true;
    using G_ = GeoG<MP, NP, SL>;
    constexpr int G = G_::G, NCG = G_::NCG, NCD = G_::NCD, ND = G_::ND, AS = G_::AS;
    const int nd = n - m;
    extern __shared__ __attribute__((aligned(16))) double lds[];
    const int tid = threadIdx.x;
    const int wpb = blockDim.x / WAVE;
    double* Aimg = lds;
    for (int i = tid; i < G_::AIMG; i += blockDim.x) {
        const int r = i / AS, cidx = i % AS;
        Aimg[i] = (r < m && cidx < nd) ? Ag[(size_t)r * n + cidx] : 0.0;
    }
    G_::fill_gram_table(lds, tid, blockDim.x);
    __syncthreads();

    GWaveH<MP, NP, SL> w;
    const int wave = __builtin_amdgcn_readfirstlane(tid / WAVE);
    const int lane = tid & 63, gl = lane & (MP - 1), grp = lane / MP;
    w.lane = lane; w.gl = gl; w.grp = grp; w.m = m; w.n = n;
    w.Aimg = Aimg;
    w.slab0 = lds + G_::SHARED + wave * G_::WSZ;
    w.slab = w.slab0 + grp * G_::SLAB;
    w.stage = w.slab0 + G * G_::SLAB;
    if constexpr (GWave<MP, NP, SL>::COLB) {
#pragma unroll
        for (int cidx = 0; cidx < 16; cidx++) w.xb[cidx] = lds_addr(w.slab) + 8u * (unsigned)G_::sidx(cidx, gl);
    }
    if constexpr (GWave<MP, NP, SL>::ROWB) {
#pragma unroll
        for (int p2 = 0; p2 < 16; p2++) w.rb[p2] = lds_addr(w.slab + gl * G_::MS) + 16u * (unsigned)(p2 ^ (gl & 15));
    }
    for (int i = lane; i < G * G_::SLAB; i += WAVE) w.slab0[i] = 0.0;     // see ipm_group_kernel
    wave_lds_sync();
    const bool rowok = gl < m;
    const bool autoscale = (o.flags & PYCLLP_AUTOSCALE_ANY) != 0;
    const unsigned long long gmask = (MP == 32) ? 0xFFFFFFFFull : 0xFFFFull;
    // option-derived doubles stay out of loop-invariant VGPRs: see hsd_group_kernel
#define HSD_ETA (1.0 - sopaque(o.delta))
#define HSD_EINF (100.0 * sopaque(o.eps))

    const long nslots = (long)gridDim.x * wpb * G;
    long lp = (long)grp * ((long)gridDim.x * wpb) + (long)blockIdx.x * wpb + wave;      // group-major: see ipm_group_kernel
    bool live = lp < B, fresh = live;

    // per-slot state: u = 0 marks a column that takes no part (padding, or fixed); u = +inf one without an upper bound
    double x[NCG], z[NCG], t[NCG], s[NCG], u[NCG], c[NCG], v[NCG];   // v = A'y, carried incrementally
    bool ok[NCG];
#pragma unroll
    for (int q = 0; q < NCG; q++) {
        ok[q] = (q < NCD) ? (gl + MP * q < nd) : (gl < m);
        x[q] = 1.0; z[q] = 1.0; t[q] = 1.0; s[q] = 1.0; u[q] = 0.0; c[q] = 0.0; v[q] = 0.0;
    }
    auto act = [&](int q) { return u[q] > 0.0; };                        // takes part
    auto bnd = [&](int q) { return u[q] > 0.0 && u[q] < HUGE_VAL; };     // carries t, s
    auto gcol = [&](int q, int g_) { return (q < NCD) ? g_ + MP * q : nd + g_; };   // from an OPAQUE lane index: see hsd_group_kernel
    double b = 0.0, y = 0.0, tau = 1.0, kap = 1.0, nb = 0.0, nc = 0.0;
    double ncomp = 1.0;                     // N_act + N_bnd + 1, the complementarity pairs of the slot's LP
    int it = 0;

    while (__any(live)) {
        if (__any(fresh)) {
            if (fresh) {
                const int go = w.ogl();
#pragma unroll
                for (int q = 0; q < NCG; q++) {
                    const int j = gcol(q, go);
                    c[q] = ok[q] ? cg[lp * n + j] : 0.0;
                    u[q] = ok[q] ? ug[lp * n + j] : 0.0;
                }
                b = rowok ? bg[lp * m + go] : 0.0;
            }
            if (autoscale) {   // b, u / max|b| and c / max|c|, exactly as ipm_bounded_kernel; undone when storing
                double cm = 0.0, ca = 0.0, um = 0.0;
#pragma unroll
                for (int q = 0; q < NCG; q++) {
                    cm = fmax(cm, act(q) ? fabs(c[q]) : 0.0);
                    ca = fmax(ca, fabs(c[q])); um = fmax(um, bnd(q) ? u[q] : 0.0);
                }
                double sb = grp_max<MP>(fabs(b)), sc = grp_max<MP>(cm);
                const bool scaled = autoscale_lp(o.flags, sb, grp_max<MP>(ca), grp_max<MP>(um));
                sb = (scaled && sb > 0.0) ? sb : 1.0; sc = (scaled && sc > 0.0) ? sc : 1.0;
                sb = (sb < HUGE_VAL) ? sb : 1.0;     // (an Inf in b is no scale factor: see ipm_group_slot_body.inc)
                if (fresh) {
                    b = b / sb;
#pragma unroll
                    for (int q = 0; q < NCG; q++) { c[q] = c[q] / sc; u[q] = u[q] / sb; }
                }
            }
            double c2 = 0.0, u2 = 0.0, cnt = 0.0;
#pragma unroll
            for (int q = 0; q < NCG; q++) {
                c2 += act(q) ? c[q] * c[q] : 0.0;
                u2 += bnd(q) ? u[q] * u[q] : 0.0;
                cnt += (act(q) ? 1.0 : 0.0) + (bnd(q) ? 1.0 : 0.0);
            }
            const double nb2 = grp_sum<MP>(b * b + u2), nc2 = grp_sum<MP>(c2);
            const double cnts = grp_sum<MP>(cnt);
            if (fresh) {
                // start: x = z = 1 (act), t = s = 1 (bnd), y = 0, tau = kappa = 1
#pragma unroll
                for (int q = 0; q < NCG; q++) { x[q] = 1.0; z[q] = 1.0; t[q] = 1.0; s[q] = 1.0; v[q] = 0.0; }
                y = 0.0; tau = 1.0; kap = 1.0;
                nb = sqrt(nb2); nc = sqrt(nc2);
                ncomp = cnts + 1.0;
                it = 0;
            }
            fresh = false;
        }

        // ---- residuals of this point ----  (rho from x every pass, never carried: see hsd_group_kernel)
        double rho;
        {
            double xm[NCG];
#pragma unroll
            for (int q = 0; q < NCG; q++) xm[q] = act(q) ? x[q] : 0.0;
            rho = fma(b, tau, -w.A_times(xm));
        }
        double s2 = 0.0, om2 = 0.0, gam = 0.0, pp = 0.0, dd = b * y;
#pragma unroll
        for (int q = 0; q < NCG; q++) {
            const bool a = act(q), bq = bnd(q);
            const double sgq = a ? fma(c[q], tau, z[q] - v[q]) - (bq ? s[q] : 0.0) : 0.0;
            const double om = bq ? fma(u[q], tau, -x[q]) - t[q] : 0.0;
            s2 = fma(sgq, sgq, s2);
            om2 = fma(om, om, om2);
            gam += a ? x[q] * z[q] : 0.0;
            gam += bq ? s[q] * t[q] : 0.0;
            pp += a ? c[q] * x[q] : 0.0;
            dd += bq ? u[q] * s[q] : 0.0;
        }
        s2 = grp_sum<MP>(s2); gam = grp_sum<MP>(gam);
        const double po = grp_sum<MP>(pp);
        const double du = grp_sum<MP>(dd);
        const double norms = sqrt(s2);
        const double normr = sqrt(grp_sum<MP>(fma(rho, rho, om2)));

        // store a finished LP and hand the slot its next one from the device-wide queue
        auto finalize = [&](int stat_) {
            double sb = 1.0, sc = 1.0;
            const int go = w.ogl();
            int gro = grp;
            asm volatile("" : "+v"(gro));
            if (autoscale) {   // recover the scale factors from the inputs (cheaper than carrying them in registers)
                double cm = 0.0, ca = 0.0, um = 0.0;
#pragma unroll
                for (int q = 0; q < NCG; q++) {
                    const double cj = ok[q] ? fabs(cg[lp * n + gcol(q, go)]) : 0.0;
                    const double uj = ok[q] ? ug[lp * n + gcol(q, go)] : 0.0;
                    cm = fmax(cm, act(q) ? cj : 0.0);
                    ca = fmax(ca, cj); um = fmax(um, (uj > 0.0 && uj < HUGE_VAL) ? uj : 0.0);
                }
                sb = grp_max<MP>(rowok ? fabs(bg[lp * m + go]) : 0.0);
                sc = grp_max<MP>(cm);
                const bool scaled = autoscale_lp(o.flags, sb, grp_max<MP>(ca), grp_max<MP>(um));
                sb = (scaled && sb > 0.0) ? sb : 1.0; sc = (scaled && sc > 0.0) ? sc : 1.0;
                sb = (sb < HUGE_VAL) ? sb : 1.0;
            }
            // optimal (and iteration-limit) points leave the homogeneous scaling; certificates stay
            const double rt = (stat_ == PYCLLP_STATUS_OPTIMAL || stat_ == PYCLLP_STATUS_ITERATION_LIMIT) ? 1.0 / tau : 1.0;
#pragma unroll
            for (int q = 0; q < NCG; q++) {
                const int j = gcol(q, go);
                if (ok[q]) {
                    const bool a = act(q), bq = bnd(q);
                    const double r = fma(c[q], tau, -v[q]);      // reduced cost of a fixed column
                    xg[lp * n + j] = a ? x[q] * rt * sb : 0.0;
                    if (zg) zg[lp * n + j] = (a ? z[q] : fmax(-r, 0.0)) * rt * sc;
                    if (sg) sg[lp * n + j] = (bq ? s[q] : (a ? 0.0 : fmax(r, 0.0))) * rt * sc;
                }
            }
            if (yg && rowok) yg[lp * m + go] = y * rt * sc;
            // (po, du are those of the point stored: the iteration limit is met at the top of a pass)
            if (go == 0) {
                if (pobj) pobj[lp] = po * rt * (sb * sc);
                if (dobj) dobj[lp] = du * rt * (sb * sc);
                status[lp] = stat_;
                if (iters) iters[lp] = it;
            }
            int nxt = 0;
            if (go == 0) nxt = atomicAdd(queue, 1);
            nxt = __shfl(nxt, gro * MP, WAVE);
            lp = nslots + (long)nxt;
            live = lp < B;
            fresh = live;
            if (!live) {   // park the slot on harmless values
#pragma unroll
                for (int q = 0; q < NCG; q++) { x[q] = 1.0; z[q] = 1.0; t[q] = 1.0; s[q] = 1.0; u[q] = 0.0; c[q] = 0.0; v[q] = 0.0; }
                b = 0.0; y = 0.0; tau = 1.0; kap = 1.0;
            }
        };

        // ---- stop tests (oracle hsd_one_raw on the expansion) ----
        {
            int stat_e = PYCLLP_STATUS_ITERATION_LIMIT;
            bool fin_e = false;
            if (live) {
                fin_e = true;
                const bool p_ray = (int)(po > 0.0) & (int)(fma(nb, tau, normr) <= HSD_EINF * po);
                const bool d_ray = (int)(du < 0.0) & (int)(fma(nc, tau, norms) <= HSD_EINF * -du);
                if (it >= o.max_iter) stat_e = PYCLLP_STATUS_ITERATION_LIMIT;   // the oracle's loop bound comes first
                else if (!(isfinite(normr) && isfinite(norms) && isfinite(gam) && isfinite(tau) && isfinite(kap)))
                    stat_e = PYCLLP_STATUS_NUMERICAL;
                else if (normr <= o.eps * (1.0 + nb) * tau && norms <= o.eps * (1.0 + nc) * tau &&
                         gam <= o.eps * tau * (tau + fabs(po)))
                    stat_e = PYCLLP_STATUS_OPTIMAL;
                else if (p_ray || d_ray)
                    stat_e = (p_ray && d_ray) ? ((-du > po) ? PYCLLP_STATUS_PRIMAL_INFEASIBLE : PYCLLP_STATUS_DUAL_INFEASIBLE)
                                             : (p_ray ? PYCLLP_STATUS_DUAL_INFEASIBLE : PYCLLP_STATUS_PRIMAL_INFEASIBLE);
                else fin_e = false;
            }
            if (__any(fin_e)) {
                if (fin_e) finalize(stat_e);
                continue;
            }
        }

        const double mu = (gam + tau * kap) / ncomp, dmu = o.delta * mu;
        const double phi = du - po + kap;

        // ---- the step quantities of column q: d, w = d s/t, h, r0 (all zero where the column takes no part) ----
        auto column = [&](int q, double& dq, double& wq, double& hq, double& r0q, double& zxq) {
            const bool a = act(q), bq = bnd(q);
            const double rx = fast_rcp(x[q]);
            const double sgq = fma(c[q], tau, z[q] - v[q]) - (bq ? s[q] : 0.0);
            zxq = z[q] * rx;
            const double stq = bq ? s[q] * fast_rcp(t[q]) : 0.0;
            const double om = bq ? fma(u[q], tau, -x[q]) - t[q] : 0.0;
            dq = a ? fast_rcp(zxq + stq) : 0.0;
            wq = dq * stq;
            hq = bq ? fma(HSD_ETA, om, t[q] - dmu * fast_rcp(s[q])) : 0.0;
            r0q = a ? fma(HSD_ETA, sgq, fma(dmu, rx, -z[q])) : 0.0;
        };

        // ---- Gram product, fused with A dc and A dr ----
        double Adc = 0.0, Adr = 0.0;
        auto do_gram = [&](double& Adc_, double& Adr_) {
            double d[NCG], dc[NCG], dr[NCG];
#pragma unroll
            for (int q = 0; q < NCG; q++) {
                double wq, hq, r0q, zxq;
                column(q, d[q], wq, hq, r0q, zxq);
                dc[q] = act(q) ? fma(d[q], c[q], bnd(q) ? wq * u[q] : 0.0) : 0.0;
                dr[q] = fma(d[q], r0q, wq * hq);
            }
            const int go = w.ogl();
#pragma unroll 1
            for (int g = 0; g < G; g++) {
                if (__shfl((int)live, g * MP, WAVE) == 0) continue;      // an idle lane group
                if (grp == g) {
#pragma unroll
                    for (int q = 0; q < NCD; q++) {
                        const int p = G_::kpos(go + MP * q);
                        w.stage[p] = dc[q];                // gram_one's "x" operand
                        w.stage[ND + p] = d[q];
                        w.stage[2 * ND + p] = dr[q];
                    }
                }
                wave_lds_sync();
                double axg, adg;
                w.template gram_one<true, true>(g, axg, adg);
                wave_lds_sync();
                if (grp == g) { Adc_ = axg; Adr_ = adg; }
            }
            // identity columns: the slack's dc, dr go straight to row gl, d_slack onto the diagonal of M
            Adc_ += dc[NCG - 1];
            Adr_ += dr[NCG - 1];
            w.slab[G_::sidx(go, go)] += d[NCG - 1];
            wave_lds_sync();
        };
        do_gram(Adc, Adr);
        double pv = Adc - b;
        double qv = fma(-HSD_ETA, rho, Adr);
        double rdiag;
        constexpr bool CARRY = GWave<MP, NP, SL>::CARRY;
        double fr[2] = {pv, qv};   // both right-hand sides ride through the sweep (see ipm_group_kernel)
        bool fused = CARRY;
        constexpr bool SPLIT = GWave<MP, NP, SL>::SPLIT;
        {
            double W[MP];
            const int go = w.ogl();
            if (m < MP) {   // padded rows: identity rows, set in the slab before the rows are fetched (see ipm_group_kernel)
                if (!rowok) w.slab[G_::sidx(go, go)] = 1.0;
                wave_lds_sync();
            }
            w.template load_row_for_sweep<SPLIT>(W);
            double diag = rowok ? w.slab[G_::sidx(go, go)] : 0.0;
            const double beta2 = grp_max<MP>(fabs(diag));
            // pivot floor of column j: pivot_floor^2 |M_jj|, through the (idle) staging area of the group: see hsd_group_kernel
            int gro = grp;
            asm volatile("" : "+v"(gro));
            double* fl = w.stage + gro * MP;
            const double pf = sopaque(o.pivot_floor);
            const double myfloor = pf * pf * fabs(diag);
            fl[go] = myfloor;
            wave_lds_sync();
            bool redo;
            if constexpr (CARRY) redo = w.template factor_dpp_fwd<true, SPLIT>(W, beta2, 0.0, live, rdiag, fr, fl);
            else redo = w.template factor_dpp<true, SPLIT>(W, beta2, 0.0, live, rdiag, fl);
            if (redo || (o.flags & PYCLLP_FLAG_FORCE_GUARD_PATH)) {
                double t1, t2;
                do_gram(t1, t2);
                fl[go] = myfloor;          // do_gram used the staging area
                wave_lds_sync();
                rdiag = w.factor_guarded_inplace(rowok, beta2, 0.0, fl);
                fused = false;             // the carried forward halves belong to the dropped factor
            }
        }
        if (fused) { pv = fr[0]; qv = fr[1]; w.backward2(pv, qv, rdiag); }
        else w.fwd_back2(pv, qv, rdiag);
        double ap[NCG], aq[NCG], dx[NCG], d[NCG], wv[NCG];
        w.template At_times2<false>(pv, qv, ap, aq);
        double dsum = 0.0, nsum = 0.0;
#pragma unroll
        for (int q = 0; q < NCG; q++) {
            const bool a = act(q), bq = bnd(q);
            double wq, hq, r0q, zxq;
            column(q, d[q], wq, hq, r0q, zxq);
            const double wu = bq ? wq * u[q] : 0.0;
            const double cp = a ? c[q] - ap[q] : 0.0;        // e
            const double uu = fma(d[q], cp, wu);
            const double vq = fma(d[q], r0q - aq[q], wq * hq);   // v = dr - d A'q
            dx[q] = vq;
            dsum = fma(d[q] * cp, cp, dsum);
            dsum += bq ? zxq * wu * u[q] : 0.0;
            nsum += a ? c[q] * vq : 0.0;
            nsum -= bq ? wu * (r0q - aq[q] - zxq * hq) : 0.0;
            wv[q] = ap[q];                          // A'p, for A'dy below
            ap[q] = uu;                             // keep uu in its place
        }
        // (grp_sum pins its inputs: dtau is bit-uniform over the lane group)
        const double den = grp_sum<MP>(dsum) + kap / tau;
        const double num = fma(HSD_ETA, phi, dmu / tau - kap) + grp_sum<MP>(b * qv) - grp_sum<MP>(nsum);
        const double dtau = num / den;
        double dy = fma(pv, dtau, qv);
#pragma unroll
        for (int q = 0; q < NCG; q++) {
            dx[q] = fma(ap[q], dtau, dx[q]);
            wv[q] = fma(wv[q], dtau, aq[q]);        // A'dy = A'p dtau + A'q
        }
        // ---- x-space refinement of  A dx - b dtau = eta rho ----
        const double etol = o.refine_tol * (1.0 + nb) * fmax(tau, kap);
        const double rhs_e = fma(b, dtau, HSD_ETA * rho);
        int nref = 0;
        double e;
        for (;;) {
            e = rhs_e - w.A_times(dx);
            const double maxe = grp_max<MP>(fabs(e));
            const bool need = live && (maxe > etol) && (nref < o.max_refine);
            if (!__any(need)) break;
            const double ec = w.fwd_back(need ? e : 0.0, rdiag);
            double w2[NCG];
            w.At_times(ec, w2);
#pragma unroll
            for (int q = 0; q < NCG; q++) {
                dx[q] = fma(d[q], w2[q], dx[q]);
                wv[q] -= w2[q];
            }
            dy -= ec;
            nref += need ? 1 : 0;
        }
        const unsigned long long nf = __ballot(!isfinite(dy) || !isfinite(dtau));
        int grb = grp;
        asm volatile("" : "+v"(grb));
        const bool bad = ((nf >> (grb * MP)) & gmask) != 0ull;
        bool fin = bad;

        if (!fin) {
            const double dkap = dmu / tau - kap - kap / tau * dtau;
            double dz[NCG], dt[NCG], ds[NCG];
            double th = fmax(fmax(-dtau / tau, -dkap / kap), 0.0);
#pragma unroll
            for (int q = 0; q < NCG; q++) {
                const bool a = act(q), bq = bnd(q);
                const double rx = fast_rcp(x[q]), rz = fast_rcp(z[q]), rt_ = fast_rcp(t[q]), rs = fast_rcp(s[q]);
                const double sgq = fma(c[q], tau, z[q] - v[q]) - (bq ? s[q] : 0.0);
                const double om = bq ? fma(u[q], tau, -x[q]) - t[q] : 0.0;
                dz[q] = a ? (dmu - z[q] * dx[q]) * rx - z[q] : 0.0;
                // two branches for dt, ds (see the header): the multiplier of the other one's rounding error is min(s/t, t/s)
                const double dt1 = fma(u[q], dtau, HSD_ETA * om) - dx[q];
                const double ds1 = (dmu - s[q] * dt1) * rt_ - s[q];
                const double ds2 = dz[q] + fma(HSD_ETA, sgq, fma(c[q], dtau, -wv[q]));
                const double dt2 = fma(dmu, rs, -t[q]) - (t[q] * rs) * ds2;
                const bool first = t[q] >= s[q];
                dt[q] = bq ? (first ? dt1 : dt2) : 0.0;
                ds[q] = bq ? (first ? ds1 : ds2) : 0.0;
                if (a) th = fmax(th, fmax(-dz[q] * rz, -dx[q] * rx));
                if (bq) th = fmax(th, fmax(-dt[q] * rt_, -ds[q] * rs));
            }
            th = grp_max<MP>(th);
            const double theta = fmin(o.r / th, 1.0);
            y = fma(theta, dy, y);
#pragma unroll
            for (int q = 0; q < NCG; q++) {
                const bool a = act(q), bq = bnd(q);     // a fixed column stands still
                x[q] = a ? fma(theta, dx[q], x[q]) : x[q];
                z[q] = a ? fma(theta, dz[q], z[q]) : z[q];
                t[q] = bq ? fma(theta, dt[q], t[q]) : t[q];
                s[q] = bq ? fma(theta, ds[q], s[q]) : s[q];
                v[q] = fma(theta, wv[q], v[q]);
            }
            tau = fma(theta, dtau, tau);
            kap = fma(theta, dkap, kap);
            it++;
        }
        if (fin && live) finalize(PYCLLP_STATUS_NUMERICAL);
    }
#undef HSD_ETA
#undef HSD_EINF
}
