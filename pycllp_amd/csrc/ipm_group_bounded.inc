// ipm_group_bounded.inc -- the slack-aware lane-group kernel (ipm_group.inc, SL = true) for LPs with UPPER BOUNDS:
//   maximise c'x  subject to  A x = b,  0 <= x <= u        (u_j = +inf: no bound;  u_j = 0: the column is fixed at 0)
// the bounded equality form of a GeneralLP (pycllp_amd/lp.py, GeneralLP.to_bounded_equality_form), A = [A_dense | I].
// Primal-normal step with x + t = u, t >= 0 and the dual Aty - z + s = c, s >= 0 (DESIGN.md section 14):
//   d = 1 / (z/x + s/t),  t~ = c - A'y + mu/x - mu/t + (s/t) tau,  tau = u - x - t,  mu = delta gamma / (n + m + N_b)
//   M dy = A (d t~) - rho,  dx = d (t~ - A'dy),  dz = (mu - z dx)/x - z,  dt = tau - dx,  ds = (mu - s dt)/t - s
// A column without a bound carries no t, s: every formula is then the one of ipm_group_kernel.  A fixed column (u = 0) takes
// no part in the iteration: it ends at x = 0 with the duals z = max(A'y - c, 0), s = max(c - A'y, 0).
// Only the per-column phases differ from ipm_group_kernel; the Gram product, the LDL' (both paths), the substitution and
// the refinement are the GWave<MP, NP, true> members, unchanged.  Simplifications against the plain kernel: rho = b - A x comes
// from the Gram pass every iteration (no carried residual), so the stop test of a point runs after its Gram product and a slot
// that finishes idles through the rest of that pass; no warm start, no predictor-corrector.
// Registers: seven N-vectors per slot (x, z, t, s, u, c, A'y) and four kept reciprocals instead of four and two; at (32, 96)
// that does not fit 256 registers, so the kernel runs PYCLLP_WPB_BOUNDED = 4 waves per workgroup, one per SIMD, with the
// whole 512-register file per lane (DESIGN.md section 14 has the measured cost).

#ifndef PYCLLP_WPB_BOUNDED
#define PYCLLP_WPB_BOUNDED 4
#endif

template <int MP, int NP>
__global__ void __launch_bounds__(PYCLLP_WPB_BOUNDED * 64)
ipm_bounded_kernel(int m, int n, long B, const double* __restrict__ Ag, const double* __restrict__ bg,
                   const double* __restrict__ cg, const double* __restrict__ ug, double* __restrict__ xg,
                   double* __restrict__ yg, double* __restrict__ zg, double* __restrict__ sg, double* __restrict__ pobj,
                   double* __restrict__ dobj, int* __restrict__ status, int* __restrict__ iters, int* __restrict__ queue,
                   DevOpts o) {
    using G_ = GeoG<MP, NP, true>;
    constexpr int G = G_::G, NCG = G_::NCG, NCD = G_::NCD, ND = G_::ND, JB = G_::JB, AS = G_::AS;
    const int nd = n - m;                   // dense columns of A (the last m columns are the identity)
    extern __shared__ __attribute__((aligned(16))) double lds[];
    const int tid = threadIdx.x;
    const int wpb = blockDim.x / WAVE;
    double* Aimg = lds;
    double* colsum = lds + G_::AIMG;
    for (int i = tid; i < G_::AIMG; i += blockDim.x) {
        const int r = i / AS, cidx = i % AS;
        Aimg[i] = (r < m && cidx < nd) ? Ag[(size_t)r * n + cidx] : 0.0;
    }
    G_::fill_gram_table(lds, tid, blockDim.x);
    __syncthreads();
    for (int j = tid; j < ND; j += blockDim.x) {
        double sacc = 0.0;
        for (int i = 0; i < MP; i++) sacc += Aimg[i * AS + j];
        colsum[j] = sacc;
    }
    __syncthreads();

    GWave<MP, NP, true> w;
    const int wave = tid / WAVE;
    const int lane = tid & 63, gl = lane & (MP - 1), grp = lane / MP;
    w.lane = lane; w.gl = gl; w.grp = grp; w.m = m; w.n = n;
    w.Aimg = Aimg;
    w.slab0 = lds + G_::SHARED + wave * G_::WSZ;
    w.slab = w.slab0 + grp * G_::SLAB;
    w.stage = w.slab0 + G * G_::SLAB;
    if constexpr (GWave<MP, NP, true>::COLB) {
#pragma unroll
        for (int cidx = 0; cidx < 16; cidx++) w.xb[cidx] = lds_addr(w.slab) + 8u * (unsigned)G_::sidx(cidx, gl);
    }
    if constexpr (GWave<MP, NP, true>::ROWB) {
#pragma unroll
        for (int p2 = 0; p2 < 16; p2++) w.rb[p2] = lds_addr(w.slab + gl * G_::MS) + 16u * (unsigned)(p2 ^ (gl & 15));
    }
    for (int i = lane; i < G * G_::SLAB; i += WAVE) w.slab0[i] = 0.0;
    wave_lds_sync();
    const bool rowok = gl < m;
    const bool autoscale = (o.flags & PYCLLP_FLAG_AUTOSCALE) != 0;
    const unsigned long long gmask = (MP == 32) ? 0xFFFFFFFFull : 0xFFFFull;

    const long nslots = (long)gridDim.x * wpb * G;
    long lp = (long)grp * ((long)gridDim.x * wpb) + (long)blockIdx.x * wpb + wave;
    bool live = lp < B, fresh = live;

    // per-slot state.  u = 0 marks a column that takes no part (padding, or fixed); u = +inf one without an upper bound.
    double x[NCG], z[NCG], t[NCG], s[NCG], u[NCG], c[NCG], v[NCG];
    bool ok[NCG];
#pragma unroll
    for (int q = 0; q < NCG; q++) {
        ok[q] = (q < NCD) ? (gl + MP * q < nd) : (gl < m);
        x[q] = 1.0; z[q] = 1.0; t[q] = 1.0; s[q] = 1.0; u[q] = 0.0; c[q] = 0.0; v[q] = 0.0;
    }
    auto act = [&](int q) { return u[q] > 0.0; };
    auto bnd = [&](int q) { return u[q] > 0.0 && u[q] < HUGE_VAL; };
    auto gcol = [&](int q, int g_) { return (q < NCD) ? g_ + MP * q : nd + g_; };
    double b = 0.0, y = 0.0;
    double tol_r = 0.0, tol_s = 0.0, tol_u = 0.0, etol = 0.0, normr0 = 1e300, norms0 = 1e300, ncomp = 1.0;
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
                    v[q] = (q < NCD) ? colsum[go + MP * q] : (rowok ? 1.0 : 0.0);   // A'y for y = 1
                }
                b = rowok ? bg[lp * m + go] : 0.0;
                y = rowok ? 1.0 : 0.0;
            }
            if (autoscale) {   // b, u / max|b| and c / max|c| (PYCLLP_FLAG_AUTOSCALE); undone when storing
                double cm = 0.0;
#pragma unroll
                for (int q = 0; q < NCG; q++) cm = fmax(cm, act(q) ? fabs(c[q]) : 0.0);
                double sb = grp_max<MP>(fabs(b)), sc = grp_max<MP>(cm);
                sb = (sb > 0.0) ? sb : 1.0; sc = (sc > 0.0) ? sc : 1.0;
                if (fresh) {
                    b = b / sb;
#pragma unroll
                    for (int q = 0; q < NCG; q++) { c[q] = c[q] / sc; u[q] = u[q] / sb; }
                }
            }
            double c2 = 0.0, u2 = 0.0, nb = 0.0;
#pragma unroll
            for (int q = 0; q < NCG; q++) {
                c2 += act(q) ? c[q] * c[q] : 0.0;
                u2 += bnd(q) ? u[q] * u[q] : 0.0;
                nb += bnd(q) ? 1.0 : 0.0;
            }
            const double nb2 = grp_sum<MP>(b * b), nc2 = grp_sum<MP>(c2), nu2 = grp_sum<MP>(u2), nbs = grp_sum<MP>(nb);
            if (fresh) {
                // start: z = s = y = 1, x = min(1, u/2), t = u - x (tau = 0)
#pragma unroll
                for (int q = 0; q < NCG; q++) {
                    x[q] = bnd(q) ? fmin(1.0, 0.5 * u[q]) : 1.0;
                    t[q] = bnd(q) ? u[q] - x[q] : 1.0;
                    z[q] = 1.0; s[q] = 1.0;
                }
                tol_r = o.eps * (1.0 + sqrt(nb2));
                tol_s = o.eps * (1.0 + sqrt(nc2));
                tol_u = o.eps * (1.0 + sqrt(nu2));
                etol = o.refine_tol * (1.0 + sqrt(nb2));
                ncomp = (double)(n + m) + nbs;
                normr0 = 1e300; norms0 = 1e300; it = 0;
            }
            fresh = false;
        }

        // ---- dual infeasibility, complementarity, bound residual, objectives ----
        double s2 = 0.0, gam = 0.0, pp = 0.0, tau2 = 0.0, du = b * y;
#pragma unroll
        for (int q = 0; q < NCG; q++) {
            const bool a = act(q), bq = bnd(q);
            const double sgq = a ? c[q] - v[q] + z[q] - (bq ? s[q] : 0.0) : 0.0;
            const double tau = bq ? (u[q] - x[q]) - t[q] : 0.0;
            s2 = fma(sgq, sgq, s2);
            tau2 = fma(tau, tau, tau2);
            gam += a ? x[q] * z[q] : 0.0;
            gam += bq ? s[q] * t[q] : 0.0;
            pp += a ? c[q] * x[q] : 0.0;
            du += bq ? u[q] * s[q] : 0.0;
        }
        s2 = grp_sum<MP>(s2); gam = grp_sum<MP>(gam); tau2 = grp_sum<MP>(tau2);
        const double po = grp_sum<MP>(pp);
        du = grp_sum<MP>(du);
        const double norms = sqrt(s2), ntau = sqrt(tau2);
        const double mu = o.delta * gam / ncomp;

        // store a finished LP and hand the slot its next one from the device-wide queue
        auto finalize = [&](int stat_) {
            double sb = 1.0, sc = 1.0;
            const int go = w.ogl();
            int gro = grp;
            asm volatile("" : "+v"(gro));
            if (autoscale) {   // the scale factors from the inputs
                double cm = 0.0;
#pragma unroll
                for (int q = 0; q < NCG; q++) cm = fmax(cm, act(q) ? fabs(cg[lp * n + gcol(q, go)]) : 0.0);
                sb = grp_max<MP>(rowok ? fabs(bg[lp * m + go]) : 0.0);
                sc = grp_max<MP>(cm);
                sb = (sb > 0.0) ? sb : 1.0; sc = (sc > 0.0) ? sc : 1.0;
            }
#pragma unroll
            for (int q = 0; q < NCG; q++) {
                const int j = gcol(q, go);
                if (ok[q]) {
                    const bool a = act(q), bq = bnd(q);
                    const double r = c[q] - v[q];      // reduced cost of a fixed column
                    xg[lp * n + j] = a ? x[q] * sb : 0.0;
                    if (zg) zg[lp * n + j] = (a ? z[q] : fmax(-r, 0.0)) * sc;
                    if (sg) sg[lp * n + j] = (bq ? s[q] : (a ? 0.0 : fmax(r, 0.0))) * sc;
                }
            }
            if (yg && rowok) yg[lp * m + go] = y * sc;
            // the iteration limit is met after a step, and po, du above belong to the point before it: the objectives stored are
            // those of the point stored (as ipm_wreg_bounded_kernel and the twin store them)
            double pof = po, duf = du;
            if (stat_ == PYCLLP_STATUS_ITERATION_LIMIT) {
                double pp2 = 0.0, dd2 = b * y;
#pragma unroll
                for (int q = 0; q < NCG; q++) {
                    pp2 += act(q) ? c[q] * x[q] : 0.0;
                    dd2 += bnd(q) ? u[q] * s[q] : 0.0;
                }
                pof = grp_sum<MP>(pp2);
                duf = grp_sum<MP>(dd2);
            }
            if (go == 0) {
                if (pobj) pobj[lp] = pof * (sb * sc);
                if (dobj) dobj[lp] = duf * (sb * sc);
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
                b = 0.0; y = 0.0;
            }
        };

        // ---- d = 1 / (z/x + s/t), t~ = c - A'y + mu/x - mu/t + (s/t) tau ----
        double rxk[NCG], rzk[NCG], rtk[NCG];
#pragma unroll
        for (int q = 0; q < NCG; q++) { rxk[q] = fast_rcp(x[q]); rzk[q] = fast_rcp(z[q]); rtk[q] = fast_rcp(t[q]); }
        auto newton_dt = [&](int q, double& dq, double& tq) {
            const bool a = act(q), bq = bnd(q);
            const double tau = (u[q] - x[q]) - t[q];
            if (bq) {
                dq = fast_rcp(fma(z[q], rxk[q], s[q] * rtk[q]));
                tq = c[q] - v[q] + mu * rxk[q] - mu * rtk[q] + (s[q] * rtk[q]) * tau;
            } else {
                dq = x[q] * rzk[q];
                tq = c[q] - v[q] + mu * rxk[q];
            }
            dq = a ? dq : 0.0;
            tq = a ? tq : 0.0;
        };
        auto do_gram = [&](double& Ax_, double& Adt_) {
            double d[NCG], tt[NCG];
#pragma unroll
            for (int q = 0; q < NCG; q++) newton_dt(q, d[q], tt[q]);
#pragma unroll 1
            for (int g = 0; g < G; g++) {
                if (__shfl((int)live, g * MP, WAVE) == 0) continue;
                if (grp == g) {
#pragma unroll
                    for (int q = 0; q < NCD; q++) {
                        const int p = G_::kpos(gl + MP * q);
                        w.stage[p] = act(q) ? x[q] : 0.0;
                        w.stage[ND + p] = d[q];
                        w.stage[2 * ND + p] = d[q] * tt[q];
                    }
                }
                wave_lds_sync();
                double axp[JB], adp[JB];
                w.template gram_one<true, true>(g, axp, adp);
                wave_lds_sync();
                if (grp == g) {
                    Ax_ = (JB == 1) ? axp[0] : ((gl >> 4) ? axp[JB - 1] : axp[0]);
                    Adt_ = (JB == 1) ? adp[0] : ((gl >> 4) ? adp[JB - 1] : adp[0]);
                }
            }
            Ax_ += act(NCG - 1) ? x[NCG - 1] : 0.0;
            Adt_ += d[NCG - 1] * tt[NCG - 1];
            w.slab[G_::sidx(gl, gl)] += d[NCG - 1];
            wave_lds_sync();
        };
        double Ax = 0.0, Adt = 0.0;
        do_gram(Ax, Adt);
        const double rho = b - Ax;
        const double normr = sqrt(grp_sum<MP>(rho * rho));

        // ---- stop tests of THIS point ----
        int stat = PYCLLP_STATUS_ITERATION_LIMIT;
        bool fin = true;
        if (!(isfinite(normr) && isfinite(norms) && isfinite(gam) && isfinite(ntau))) stat = PYCLLP_STATUS_NUMERICAL;
        else if (normr <= tol_r && norms <= tol_s && gam <= o.eps * (1.0 + fabs(po)) && ntau <= tol_u) stat = PYCLLP_STATUS_OPTIMAL;
        else if (normr > 10.0 * normr0 && normr > PYCLLP_GROWTH_FLOOR * tol_r) stat = PYCLLP_STATUS_PRIMAL_INFEASIBLE;
        else if (norms > 10.0 * norms0 && norms > PYCLLP_GROWTH_FLOOR * tol_s) stat = PYCLLP_STATUS_DUAL_INFEASIBLE;
        else fin = false;
        const bool work = live && !fin;     // a finishing slot idles through the rest of the pass

        const double rhs = Adt - rho;
        double rdiag;
        {
            double W[MP];
            const int gd = w.ogl();
            if (m < MP) {
                if (!rowok) w.slab[G_::sidx(gd, gd)] = 1.0;
                wave_lds_sync();
            }
            w.load_own_row(W);
            double diag = rowok ? w.slab[G_::sidx(gd, gd)] : 0.0;
            const double beta2 = grp_max<MP>(fabs(diag));
            wave_lds_sync();
            const bool redo = w.factor_dpp(W, beta2, o.pivot_floor, work, rdiag);
            if (redo || (o.flags & PYCLLP_FLAG_FORCE_GUARD_PATH)) {
                double Ax2, Adt2;
                do_gram(Ax2, Adt2);
                rdiag = w.factor_guarded_inplace(rowok, beta2, o.pivot_floor);
            }
        }
        double dy = w.fwd_back(rhs, rdiag);
        double wv[NCG], dx[NCG], d[NCG];
        w.At_times(dy, wv);
#pragma unroll
        for (int q = 0; q < NCG; q++) {
            double tq;
            newton_dt(q, d[q], tq);
            dx[q] = (tq - wv[q]) * d[q];
        }
        // ---- x-space iterative refinement (as ipm_group_kernel) ----
        int nref = 0;
        for (;;) {
            const double e = rho - w.A_times(dx);
            const double maxe = grp_max<MP>(fabs(e));
            const bool need = work && (maxe > etol) && (nref < o.max_refine);
            if (!__any(need)) break;
            const double eta = w.fwd_back(need ? e : 0.0, rdiag);
            double w2[NCG];
            w.At_times(eta, w2);
#pragma unroll
            for (int q = 0; q < NCG; q++) {
                dx[q] = fma(d[q], w2[q], dx[q]);
                wv[q] -= w2[q];
            }
            dy -= eta;
            nref += need ? 1 : 0;
        }
        const unsigned long long nf = __ballot(!isfinite(dy));
        const bool dy_bad = ((nf >> (grp * MP)) & gmask) != 0ull;
        if (!fin && dy_bad) { fin = true; stat = PYCLLP_STATUS_NUMERICAL; }

        if (!fin) {
            // ---- step: theta = min(r / max(0, -dx/x, -dz/z, -dt/t, -ds/s), 1) ----
            double dz[NCG], dt[NCG], ds[NCG];
            double th = 0.0;
#pragma unroll
            for (int q = 0; q < NCG; q++) {
                const bool a = act(q), bq = bnd(q);
                const double tau = (u[q] - x[q]) - t[q];
                dz[q] = a ? (mu - z[q] * dx[q]) * rxk[q] - z[q] : 0.0;
                dt[q] = bq ? tau - dx[q] : 0.0;
                ds[q] = bq ? (mu - s[q] * dt[q]) * rtk[q] - s[q] : 0.0;
                if (a) th = fmax(th, fmax(-dz[q] * rzk[q], -dx[q] * rxk[q]));
                if (bq) th = fmax(th, fmax(-dt[q] * rtk[q], -ds[q] * fast_rcp(s[q])));
            }
            th = grp_max<MP>(th);
            const double theta = fmin(o.r / th, 1.0);
            y = fma(theta, dy, y);
#pragma unroll
            for (int q = 0; q < NCG; q++) {
                const bool a = act(q), bq = bnd(q);
                x[q] = a ? fma(theta, dx[q], x[q]) : x[q];
                z[q] = a ? fma(theta, dz[q], z[q]) : z[q];
                t[q] = bq ? fma(theta, dt[q], t[q]) : t[q];
                s[q] = bq ? fma(theta, ds[q], s[q]) : s[q];
                v[q] = fma(theta, wv[q], v[q]);
            }
            normr0 = normr; norms0 = norms;
            it++;
            if (it >= o.max_iter) fin = true;   // status stays ITERATION_LIMIT
        }
        if (fin && live) finalize(stat);
    }
}
