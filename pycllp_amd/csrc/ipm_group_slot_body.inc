// ipm_group_slot_body.inc -- the text of one slot iteration, included into the body of ipm_bounded_kernel, of
// ipm_group_pa_kernel and of ipm_bounded_pa_kernel (ipm_group_slot.inc, which has the algorithm notes).  It expects in scope: MP, NP and the constants SL,
// BD (upper bounds: t, s, u), PA (per-slot A areas); the kernel arguments m, n, B, Ag, bg, cg, ug, xg, yg, zg, sg, pobj, dobj,
// status, iters, queue, o (ug, sg: BD only).  Each phase is written once, in the form of the bounded algorithm (DESIGN.md
// section 14); strike the BD parts and the plain step of ipm_group_kernel is left.
    using G_ = GeoG<MP, NP, SL>;
    using P_ = GeoPA<G_>;
    constexpr int G = G_::G, NCG = G_::NCG, NCD = G_::NCD, ND = G_::ND, JB = G_::JB, AS = G_::AS;
    static_assert(SL || !BD, "the bounded equality form ends in the identity");
    const int nd = SL ? n - m : n;          // dense columns of A as stored (the last m columns of the LP are the identity when SL)
    extern __shared__ __attribute__((aligned(16))) double lds[];
    const int tid = threadIdx.x;
    const int wpb = blockDim.x / WAVE;
    if constexpr (!PA) {   // the one A of the batch: image, Gram table and column sums, once per workgroup
        for (int i = tid; i < G_::AIMG; i += blockDim.x) {
            const int r = i / AS, cidx = i % AS;
            lds[i] = (r < m && cidx < nd) ? Ag[(size_t)r * n + cidx] : 0.0;
        }
        G_::fill_gram_table(lds, tid, blockDim.x);
        __syncthreads();
        for (int j = tid; j < ND; j += blockDim.x) {
            double sacc = 0.0;
            for (int i = 0; i < MP; i++) sacc += lds[i * AS + j];
            lds[G_::AIMG + j] = sacc;
        }
        __syncthreads();
    }

    GWave<MP, NP, SL> w;
    const int wave = tid / WAVE;
    const int lane = tid & 63, gl = lane & (MP - 1), grp = lane / MP;
    double* const areas = PA ? lds + wave * P_::PW : nullptr;     // PA: G areas of this wave, then its slabs and staging region
    if constexpr (PA) {
        // pad rows and columns of every image (and the column sums behind it) are zero from here on; a refill writes rows < m,
        // columns < nd only
        for (int i = lane; i < G * P_::AREA; i += WAVE) areas[i] = 0.0;
        wave_lds_sync();
        for (int g = 0; g < G; g++) G_::fill_gram_table(areas + g * P_::AREA, lane, WAVE);
    }
    const double* const own_area = PA ? areas + grp * P_::AREA : lds;   // image, column sums and Gram table of the lane's own group
    w.lane = lane; w.gl = gl; w.grp = grp; w.m = m; w.n = n;
    w.Aimg = own_area;
    w.slab0 = PA ? areas + G * P_::AREA : lds + G_::SHARED + wave * G_::WSZ;
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
    for (int i = lane; i < G * G_::SLAB; i += WAVE) w.slab0[i] = 0.0;
    wave_lds_sync();
    const bool rowok = gl < m;
    const bool autoscale = (o.flags & PYCLLP_FLAG_AUTOSCALE) != 0;
    const unsigned long long gmask = (MP == 32) ? 0xFFFFFFFFull : 0xFFFFull;
    const int asz = PA ? m * nd : 0;        // PA: doubles of one A_k

    // slots in GROUP-major order (as ipm_group_kernel): a batch smaller than the launch's slots leaves whole lane groups idle
    const long nslots = (long)gridDim.x * wpb * G;
    long lp = (long)grp * ((long)gridDim.x * wpb) + (long)blockIdx.x * wpb + wave;
    bool live = lp < B, fresh = live;

    // per-slot state.  BD: u = 0 marks a column that takes no part (padding, or fixed); u = +inf one without an upper bound.
    // Without BD, t, s, u are never written, and every read of them is an operand that BD = false or bnd(q) = false leaves unevaluated.
    double x[NCG], z[NCG], t[NCG], s[NCG], u[NCG], c[NCG], v[NCG];
    bool ok[NCG];
#pragma unroll
    for (int q = 0; q < NCG; q++) {
        ok[q] = (q < NCD) ? (gl + MP * q < nd) : (gl < m);
        x[q] = 1.0; z[q] = 1.0; c[q] = 0.0; v[q] = 0.0;
        if constexpr (BD) { t[q] = 1.0; s[q] = 1.0; u[q] = 0.0; }
    }
    auto act = [&](int q) { if constexpr (BD) return u[q] > 0.0; else return ok[q]; };                      // takes part
    auto bnd = [&](int q) { if constexpr (BD) return u[q] > 0.0 && u[q] < HUGE_VAL; else return false; };   // carries t, s
    // global column of register q (dense registers first, then (SL) the slack column of row gl) from an OPAQUE lane index: the
    // cold paths that need it (loading / storing an LP) must not leave per-lane 64-bit addresses alive across the iterations
    // (hoisted out of the persistent loop they cost ~30 registers and, at 256, scratch)
    // acc + c_q x_q over the columns that take part.  Without BD c is zero where a column takes none (only a fixed column has a
    // cost), so masking x alone is enough and the product contracts into an FMA: the form of ipm_group_kernel
    auto add_cx = [&](int q, double acc) {
        if constexpr (BD) return acc + (act(q) ? c[q] * x[q] : 0.0); else return acc + c[q] * (ok[q] ? x[q] : 0.0);
    };
    auto gcol = [&](int q, int g_) { return (q < NCD) ? g_ + MP * q : nd + g_; };
    double b = 0.0, y = 0.0;
    double tol_r = 0.0, tol_s = 0.0, tol_u = 0.0, etol = 0.0, normr0 = 1e300, norms0 = 1e300;
    double ncomp = 1.0;                     // BD: n + m + N_b, the complementarity pairs of the slot's LP
    int it = 0;

    while (__any(live)) {
        if (__any(fresh)) {
            if constexpr (PA) {
                // ---- refill: the whole wave copies the matrix of every fresh slot into that slot's image, then its column sums ----
#pragma unroll 1
                for (int g = 0; g < G; g++) {
                    if (__shfl((int)fresh, g * MP, WAVE) == 0) continue;
                    const unsigned lo_ = (unsigned)__shfl((int)(unsigned)(lp & 0xFFFFFFFFl), g * MP, WAVE);
                    const int hi_ = __shfl((int)(lp >> 32), g * MP, WAVE);
                    const long lpg = ((long)hi_ << 32) | (long)lo_;
                    const double* src = Ag + (size_t)lpg * (size_t)asz;
                    double* img = areas + g * P_::AREA;
                    // flat, coalesced reads, eight in flight per lane; (row, column) of element i advance by WAVE per step without a
                    // division: WAVE = sr nd + sc
                    int r = lane / nd, cidx = lane - r * nd;
                    const int sr = WAVE / nd, sc = WAVE - sr * nd;
#pragma unroll 1
                    for (int i0 = lane; i0 < asz; i0 += 8 * WAVE) {
                        double av[8];
#pragma unroll
                        for (int k = 0; k < 8; k++) av[k] = (i0 + k * WAVE < asz) ? src[i0 + k * WAVE] : 0.0;
#pragma unroll
                        for (int k = 0; k < 8; k++) {
                            if (i0 + k * WAVE < asz) img[r * AS + cidx] = av[k];
                            cidx += sc; r += sr;
                            if (cidx >= nd) { cidx -= nd; r++; }
                        }
                    }
                    wave_lds_sync();
                    for (int j = lane; j < ND; j += WAVE) {
                        double sacc = 0.0;
                        for (int i = 0; i < MP; i++) sacc += img[i * AS + j];
                        img[G_::AIMG + j] = sacc;
                    }
                }
                wave_lds_sync();
            }
            if (fresh) {
                const int go = w.ogl();
                const double* colsum = own_area + G_::AIMG;
#pragma unroll
                for (int q = 0; q < NCG; q++) {
                    const int j = gcol(q, go);
                    c[q] = ok[q] ? cg[lp * n + j] : 0.0;
                    if constexpr (BD) u[q] = ok[q] ? ug[lp * n + j] : 0.0;
                    v[q] = (q < NCD) ? colsum[go + MP * q] : (rowok ? 1.0 : 0.0);   // A'y for y = 1
                }
                b = rowok ? bg[lp * m + go] : 0.0;
                y = rowok ? 1.0 : 0.0;
            }
            if (autoscale) {   // solve the LP with b, u / max|b| and c / max|c| (PYCLLP_FLAG_AUTOSCALE); undone when storing
                // the per-LP verdict (autoscale_lp) looks at max|c| over ALL columns and at the largest finite positive u
                double cm = 0.0, ca = 0.0, um = 0.0;
#pragma unroll
                for (int q = 0; q < NCG; q++) {
                    cm = fmax(cm, (!BD || act(q)) ? fabs(c[q]) : 0.0);   // (c = 0 where !ok)
                    if constexpr (BD) { ca = fmax(ca, fabs(c[q])); um = fmax(um, bnd(q) ? u[q] : 0.0); }
                }
                double sb = grp_max<MP>(fabs(b)), sc = grp_max<MP>(cm);
                bool scaled;
                if constexpr (BD) scaled = autoscale_lp(o.flags, sb, grp_max<MP>(ca), grp_max<MP>(um));
                else scaled = autoscale_lp(o.flags, sb, sc, 0.0);
                sb = (scaled && sb > 0.0) ? sb : 1.0; sc = (scaled && sc > 0.0) ? sc : 1.0;
                // BD: sb = inf -- an Inf in b: the LP ends NUMERICAL at iteration 0 either way -- is no scale factor: u / inf = 0
                // would turn every column into a fixed one, for finalize's scale factors and stores too
                if constexpr (BD) sb = (sb < HUGE_VAL) ? sb : 1.0;
                if (fresh) {
                    b = b / sb;
#pragma unroll
                    for (int q = 0; q < NCG; q++) {
                        c[q] = c[q] / sc;
                        if constexpr (BD) u[q] = u[q] / sb;
                    }
                }
            }
            double c2 = 0.0, u2 = 0.0, nb = 0.0;
#pragma unroll
            for (int q = 0; q < NCG; q++) {
                if constexpr (BD) c2 += act(q) ? c[q] * c[q] : 0.0; else c2 = fma(c[q], c[q], c2);
                u2 += bnd(q) ? u[q] * u[q] : 0.0;
                nb += bnd(q) ? 1.0 : 0.0;
            }
            const double nb2 = grp_sum<MP>(b * b), nc2 = grp_sum<MP>(c2);
            double nu2 = 0.0, nbs = 0.0;
            if constexpr (BD) { nu2 = grp_sum<MP>(u2); nbs = grp_sum<MP>(nb); }
            if (fresh) {
                // start: z = s = y = 1, x = min(1, u/2), t = u - x (tau = 0)
#pragma unroll
                for (int q = 0; q < NCG; q++) {
                    x[q] = bnd(q) ? fmin(1.0, 0.5 * u[q]) : 1.0;
                    if constexpr (BD) t[q] = bnd(q) ? u[q] - x[q] : 1.0;
                    z[q] = 1.0;
                    if constexpr (BD) s[q] = 1.0;
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
            if constexpr (BD) gam += bq ? s[q] * t[q] : 0.0;
            pp = add_cx(q, pp);
            if constexpr (BD) du += bq ? u[q] * s[q] : 0.0;
        }
        s2 = grp_sum<MP>(s2); gam = grp_sum<MP>(gam);
        if constexpr (BD) tau2 = grp_sum<MP>(tau2);
        const double po = grp_sum<MP>(pp);
        du = grp_sum<MP>(du);
        const double norms = sqrt(s2), ntau = sqrt(tau2);
        const double mu = o.delta * gam / (BD ? ncomp : (double)(n + m));

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
                    cm = fmax(cm, act(q) ? cj : 0.0);
                    if constexpr (BD) {   // (u[q] is the scaled bound: the verdict of the load came from the input)
                        const double uj = ok[q] ? ug[lp * n + gcol(q, go)] : 0.0;
                        ca = fmax(ca, cj); um = fmax(um, (uj > 0.0 && uj < HUGE_VAL) ? uj : 0.0);
                    }
                }
                sb = grp_max<MP>(rowok ? fabs(bg[lp * m + go]) : 0.0);
                sc = grp_max<MP>(cm);
                bool scaled;
                if constexpr (BD) scaled = autoscale_lp(o.flags, sb, grp_max<MP>(ca), grp_max<MP>(um));
                else scaled = autoscale_lp(o.flags, sb, sc, 0.0);
                sb = (scaled && sb > 0.0) ? sb : 1.0; sc = (scaled && sc > 0.0) ? sc : 1.0;
            }
#pragma unroll
            for (int q = 0; q < NCG; q++) {
                const int j = gcol(q, go);
                if (ok[q]) {
                    const bool a = act(q), bq = bnd(q);
                    const double r = c[q] - v[q];      // reduced cost of a fixed column
                    xg[lp * n + j] = a ? x[q] * sb : 0.0;
                    if (zg) zg[lp * n + j] = (a ? z[q] : fmax(-r, 0.0)) * sc;
                    if constexpr (BD) {
                        if (sg) sg[lp * n + j] = (bq ? s[q] : (a ? 0.0 : fmax(r, 0.0))) * sc;
                    }
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
                    pp2 = add_cx(q, pp2);
                    if constexpr (BD) dd2 += bnd(q) ? u[q] * s[q] : 0.0;
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
            if (!live) {   // park the slot on harmless values (PA: its image keeps the last LP's matrix: finite, never stored from)
#pragma unroll
                for (int q = 0; q < NCG; q++) {
                    x[q] = 1.0; z[q] = 1.0; c[q] = 0.0; v[q] = 0.0;
                    if constexpr (BD) { t[q] = 1.0; s[q] = 1.0; u[q] = 0.0; }
                }
                b = 0.0; y = 0.0;
            }
        };

        // ---- d = 1 / (z/x + s/t), t~ = c - A'y + mu/x - mu/t + (s/t) tau;  no bound: d = x/z, t~ = c - A'y + mu/x ----
        double rxk[NCG], rzk[NCG], rtk[NCG];
#pragma unroll
        for (int q = 0; q < NCG; q++) {
            rxk[q] = fast_rcp(x[q]); rzk[q] = fast_rcp(z[q]);
            if constexpr (BD) rtk[q] = fast_rcp(t[q]);
        }
        auto newton_dt = [&](int q, double& dq, double& tq) {
            const bool a = act(q), bq = bnd(q);
            const double tau = BD ? (u[q] - x[q]) - t[q] : 0.0;
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
                double axg, adg;
                if constexpr (PA) w.Aimg = areas + g * P_::AREA;       // group g's matrix (wave-uniform)
                w.template gram_one<true, true>(g, axg, adg);
                if constexpr (PA) w.Aimg = own_area;
                wave_lds_sync();
                if (grp == g) { Ax_ = axg; Adt_ = adg; }
            }
            if (SL) {   // identity columns: x_slack and (d t~)_slack go straight to row gl, d_slack onto the diagonal of M
                Ax_ += act(NCG - 1) ? x[NCG - 1] : 0.0;
                Adt_ += d[NCG - 1] * tt[NCG - 1];
                w.slab[G_::sidx(gl, gl)] += d[NCG - 1];
                wave_lds_sync();
            }
        };
        double Ax = 0.0, Adt = 0.0;
        do_gram(Ax, Adt);
        const double rho = b - Ax;
        const double normr = sqrt(grp_sum<MP>(rho * rho));

        // ---- stop tests of THIS point ----
        int stat = PYCLLP_STATUS_ITERATION_LIMIT;
        bool fin = true;
        if (!(isfinite(normr) && isfinite(norms) && isfinite(gam) && (!BD || isfinite(ntau)))) stat = PYCLLP_STATUS_NUMERICAL;
        else if (normr <= tol_r && norms <= tol_s && gam <= o.eps * (1.0 + fabs(po)) && (!BD || ntau <= tol_u)) stat = PYCLLP_STATUS_OPTIMAL;
        else if (normr > 10.0 * normr0 && normr > PYCLLP_GROWTH_FLOOR * tol_r) stat = PYCLLP_STATUS_PRIMAL_INFEASIBLE;
        else if (norms > 10.0 * norms0 && norms > PYCLLP_GROWTH_FLOOR * tol_s) stat = PYCLLP_STATUS_DUAL_INFEASIBLE;
        else fin = false;
        const bool work = live && !fin;     // a finishing slot idles through the rest of the pass

        const double rhs = Adt - rho;
        double rdiag;
        constexpr bool CARRY = GWave<MP, NP, SL>::CARRY;
        double fs[1] = {rhs};     // the first solve's right-hand side rides through the sweep (see ipm_group_kernel)
        bool fused = CARRY;
        // the split sweep (GWave::factor_sweep); the bounded per-problem-A kernel at (32, 96) alone keeps the plain one: 0 -> 4 spilt
        // VGPRs with it
        constexpr bool SPLIT = GWave<MP, NP, SL>::SPLIT && !(BD && PA && MP == 32 && NP == 96);
        {
            double W[MP];
            const int gd = w.ogl();
            if (m < MP) {
                if (!rowok) w.slab[G_::sidx(gd, gd)] = 1.0;
                wave_lds_sync();
            }
            w.template load_row_for_sweep<SPLIT>(W);
            double diag = rowok ? w.slab[G_::sidx(gd, gd)] : 0.0;
            const double beta2 = grp_max<MP>(fabs(diag));
            wave_lds_sync();
            bool redo;
            if constexpr (CARRY) redo = w.template factor_dpp_fwd<false, SPLIT>(W, beta2, o.pivot_floor, work, rdiag, fs);
            else redo = w.template factor_dpp<false, SPLIT>(W, beta2, o.pivot_floor, work, rdiag);
            if (redo || (o.flags & PYCLLP_FLAG_FORCE_GUARD_PATH)) {
                double Ax2, Adt2;
                do_gram(Ax2, Adt2);
                rdiag = w.factor_guarded_inplace(rowok, beta2, o.pivot_floor);
                fused = false;    // the carried forward half belongs to the dropped factor
            }
        }
        double dy = fused ? w.back_after_sweep(fs[0], rdiag) : w.fwd_back(rhs, rdiag);
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
                const double tau = BD ? (u[q] - x[q]) - t[q] : 0.0;
                dz[q] = a ? (mu - z[q] * dx[q]) * rxk[q] - z[q] : 0.0;
                dt[q] = bq ? tau - dx[q] : 0.0;
                ds[q] = bq ? (mu - s[q] * dt[q]) * rtk[q] - s[q] : 0.0;
                // (act(q) afresh: sharing dz's flag makes the BD = false kernels branch around dz instead of selecting it)
                if (act(q)) th = fmax(th, fmax(-dz[q] * rzk[q], -dx[q] * rxk[q]));
                if (bq) th = fmax(th, fmax(-dt[q] * rtk[q], -ds[q] * fast_rcp(s[q])));
            }
            th = grp_max<MP>(th);
            const double theta = fmin(o.r / th, 1.0);
            y = fma(theta, dy, y);
#pragma unroll
            for (int q = 0; q < NCG; q++) {
                // only a fixed column (BD) must stand still; elsewhere dx = dz = 0 where a column takes no part, and every register steps
                const bool a = !BD || act(q), bq = bnd(q);
                x[q] = a ? fma(theta, dx[q], x[q]) : x[q];
                z[q] = a ? fma(theta, dz[q], z[q]) : z[q];
                if constexpr (BD) {
                    t[q] = bq ? fma(theta, dt[q], t[q]) : t[q];
                    s[q] = bq ? fma(theta, ds[q], s[q]) : s[q];
                }
                v[q] = fma(theta, wv[q], v[q]);
            }
            normr0 = normr; norms0 = norms;
            it++;
            if (it >= o.max_iter) fin = true;   // status stays ITERATION_LIMIT
        }
        if (fin && live) finalize(stat);
    }
