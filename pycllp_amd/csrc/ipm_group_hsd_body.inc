// ipm_group_hsd_body.inc -- the text of one lane-group kernel on the homogeneous self-dual embedding, included into the body of
// hsd_group_kernel (ipm_group_hsd.inc, which has the model and GWaveH), of ipm_bounded_hsd_kernel (ipm_group_bdhsd.inc, which
// has the bounded system) and of ipm_bounded_pa_hsd_kernel (ipm_group_pabdhsd.inc: every LP has its own A).  It expects in
// scope: MP, NP and the constants SL, BD (upper bounds: t, s, u), PA (per-slot A areas, Ag [B, m, n - m]; with SL and BD only);
// the kernel arguments
// m, n, B, Ag, bg, cg, ug, xg, yg, zg, sg, pobj, dobj, status, iters, queue, o (ug, sg: BD only).  Each phase is written once, in
// the form of the bounded system (DESIGN.md section 26); strike the BD parts and the step of section 9 is left.  Where the two
// kernels form the same quantity in different instruction forms, each keeps its own under BD: both stay instruction for
// instruction what they were as texts of their own (profiles/group_hsd_body).  Included, not called: see ipm_group_slot.inc.
    using G_ = GeoG<MP, NP, SL>;
    using P_ = GeoPA<G_>;                   // PA only
    constexpr int G = G_::G, NCG = G_::NCG, NCD = G_::NCD, ND = G_::ND, AS = G_::AS;
    static_assert(SL || !BD, "the bounded equality form ends in the identity");
    static_assert(!PA || (SL && BD), "per-slot areas exist on the bounded embedding only");
    const int nd = SL ? n - m : n;          // dense columns of A as stored (the last m columns of the LP are the identity when SL)
    extern __shared__ __attribute__((aligned(16))) double lds[];
    const int tid = threadIdx.x;
    const int wpb = blockDim.x / WAVE;
    double* Aimg = lds;
    if constexpr (!PA) {   // the one A of the batch: image and Gram table, once per workgroup
        for (int i = tid; i < G_::AIMG; i += blockDim.x) {
            const int r = i / AS, cidx = i % AS;
            Aimg[i] = (r < m && cidx < nd) ? Ag[(size_t)r * n + cidx] : 0.0;
        }
        G_::fill_gram_table(lds, tid, blockDim.x);
        __syncthreads();
    }

    GWaveH<MP, NP, SL> w;
    const int wave = __builtin_amdgcn_readfirstlane(tid / WAVE);
    const int lane = tid & 63, gl = lane & (MP - 1), grp = lane / MP;
    // PA (as ipm_group_slot_body.inc): G areas of this wave -- image, the place of the column sums, Gram table --, then its slabs
    // and staging region; nothing is shared between the waves, so there is no workgroup barrier
    double* const areas = PA ? lds + wave * P_::PW : nullptr;
    if constexpr (PA) {
        // pad rows and columns of every image are zero from here on: a refill writes rows < m, columns < nd only.  The column
        // sums behind an image stay zero: the embedding starts at y = 0, A'y = 0 and never reads them.  (A slot that parks keeps
        // its last LP's matrix; a NaN in it turns the parked group's own values NaN, and the `live` masks keep them there)
        for (int i = lane; i < G * P_::AREA; i += WAVE) areas[i] = 0.0;
        wave_lds_sync();
        for (int g = 0; g < G; g++) G_::fill_gram_table(areas + g * P_::AREA, lane, WAVE);
        Aimg = areas + grp * P_::AREA;      // the lane's own group's area
    }
    w.lane = lane; w.gl = gl; w.grp = grp; w.m = m; w.n = n;
    w.Aimg = Aimg;
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
    for (int i = lane; i < G * G_::SLAB; i += WAVE) w.slab0[i] = 0.0;     // see ipm_group_kernel
    wave_lds_sync();
    const bool rowok = gl < m;
    const bool warm = !BD && (o.flags & PYCLLP_FLAG_WARM_START) != 0;     // warm start exists only without bounds
    const bool autoscale = (o.flags & (BD ? PYCLLP_AUTOSCALE_ANY : PYCLLP_FLAG_AUTOSCALE)) != 0;
    const unsigned long long gmask = (MP == 32) ? 0xFFFFFFFFull : 0xFFFFull;
    // Wave-uniform doubles derived from the options (1 - delta, 100 eps, pivot_floor^2, N + 1) are NOT named here: as invariants
    // of the persistent loop they would each sit in a VGPR pair for the whole solve (f64 has no scalar ALU) -- or, at 256
    // registers, in scratch.  They are re-derived where they are used from an opaque copy of the SGPR-resident option.
#define HSD_ETA (1.0 - sopaque(o.delta))
#define HSD_EINF (100.0 * sopaque(o.eps))

    const long nslots = (long)gridDim.x * wpb * G;
    long lp = (long)grp * ((long)gridDim.x * wpb) + (long)blockIdx.x * wpb + wave;      // group-major: see ipm_group_kernel
    bool live = lp < B, fresh = live;

    // per-slot state.  BD: u = 0 marks a column that takes no part (padding, or fixed); u = +inf one without an upper bound.
    // Without BD, t, s, u are never written, and every read of them is an operand that BD = false or bnd(q) = false leaves unevaluated.
    double x[NCG], z[NCG], t[NCG], s[NCG], u[NCG], c[NCG], v[NCG];   // v = A'y, carried incrementally
    bool ok[NCG];
#pragma unroll
    for (int q = 0; q < NCG; q++) {
        ok[q] = (q < NCD) ? (gl + MP * q < nd) : (gl < m);
        x[q] = 1.0; z[q] = 1.0;
        if constexpr (BD) { t[q] = 1.0; s[q] = 1.0; u[q] = 0.0; }
        c[q] = 0.0; v[q] = 0.0;
    }
    auto act = [&](int q) { if constexpr (BD) return u[q] > 0.0; else return ok[q]; };                      // takes part
    auto bnd = [&](int q) { if constexpr (BD) return u[q] > 0.0 && u[q] < HUGE_VAL; else return false; };   // carries t, s
    // acc + c_q x_q over the columns that take part.  Without BD c is zero where a column takes none (only a fixed column has a
    // cost), so masking x alone is enough and the product contracts into an FMA
    auto add_cx = [&](int q, double acc) {
        if constexpr (BD) return acc + (act(q) ? c[q] * x[q] : 0.0); else return acc + c[q] * (ok[q] ? x[q] : 0.0);
    };
    // global column of register q (dense registers first, then the slack column of row gl), from an opaque lane index: the cold
    // paths that need it (loading / storing an LP) must not leave per-lane addresses alive across the iterations
    auto gcol = [&](int q, int g_) { return (q < NCD) ? g_ + MP * q : nd + g_; };
    double b = 0.0, y = 0.0, tau = 1.0, kap = 1.0, nb = 0.0, nc = 0.0;
    double ncomp = 1.0;                       // BD: N_act + N_bnd + 1, the complementarity pairs of the slot's LP
    double po_prev = 0.0, du_prev = 0.0;      // !BD: c'x and b'y of the point the last step started from
    int it = 0;

    while (__any(live)) {
        if (__any(fresh)) {
            if constexpr (PA) {
                // ---- refill: the whole wave copies the matrix of every fresh slot into that slot's image (no column sums:
                // the start is y = 0) ----
                const int asz = m * nd;     // doubles of one A_k
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
                }
                wave_lds_sync();
            }
            if (fresh) {
                const int go = w.ogl();
#pragma unroll
                for (int q = 0; q < NCG; q++) {
                    const int j = gcol(q, go);
                    c[q] = ok[q] ? cg[lp * n + j] : 0.0;
                    if constexpr (BD) u[q] = ok[q] ? ug[lp * n + j] : 0.0;
                    else {
                        x[q] = (warm && ok[q]) ? xg[lp * n + j] : 1.0;
                        z[q] = (warm && ok[q]) ? zg[lp * n + j] : 1.0;
                        v[q] = 0.0;
                    }
                }
                b = rowok ? bg[lp * m + go] : 0.0;
                if constexpr (!BD) y = (rowok && warm && yg) ? yg[lp * m + go] : 0.0;
            }
            if (autoscale) {   // solve the LP with b, u / max|b| and c / max|c|; undone when storing
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
                if constexpr (BD) sb = (sb < HUGE_VAL) ? sb : 1.0;     // (an Inf in b is no scale factor: see ipm_group_slot_body.inc)
                if (fresh) {
                    b = b / sb;
#pragma unroll
                    for (int q = 0; q < NCG; q++) {
                        c[q] = c[q] / sc;
                        if constexpr (BD) u[q] = u[q] / sb;
                    }
                    if (warm) {
                        y = y / sc;
#pragma unroll
                        for (int q = 0; q < NCG; q++) { x[q] = x[q] / sb; z[q] = z[q] / sc; }
                    }
                }
            }
            double c2 = 0.0, u2 = 0.0, cnt = 0.0, g0 = 0.0;
#pragma unroll
            for (int q = 0; q < NCG; q++) {
                if constexpr (BD) c2 += act(q) ? c[q] * c[q] : 0.0; else c2 = fma(c[q], c[q], c2);
                u2 += bnd(q) ? u[q] * u[q] : 0.0;
                cnt += (act(q) ? 1.0 : 0.0) + (bnd(q) ? 1.0 : 0.0);
                if constexpr (!BD) g0 += ok[q] ? x[q] * z[q] : 0.0;      // x'z of a warm start
            }
            const double nb2 = grp_sum<MP>(BD ? b * b + u2 : b * b), nc2 = grp_sum<MP>(c2);     // |(b; u_bnd)|^2, |c_act|^2
            double cnts = 0.0;
            if constexpr (BD) cnts = grp_sum<MP>(cnt); else g0 = grp_sum<MP>(g0);
            double vw[NCG];
            if (warm) w.At_times(y, vw);
            if (fresh) {
                // start: x = z = 1 (act), t = s = 1 (bnd), y = 0, tau = kappa = 1; a warm start keeps x, y, z and A'y
                if constexpr (BD) {
#pragma unroll
                    for (int q = 0; q < NCG; q++) { x[q] = 1.0; z[q] = 1.0; t[q] = 1.0; s[q] = 1.0; v[q] = 0.0; }
                    y = 0.0; tau = 1.0; kap = 1.0;
                    nb = sqrt(nb2); nc = sqrt(nc2);
                    ncomp = cnts + 1.0;
                    it = 0;
                } else {
                    nb = sqrt(nb2); nc = sqrt(nc2);
                    tau = 1.0;
                    kap = warm ? g0 / (double)n : 1.0;
                    it = 0;
                    if (warm) {
#pragma unroll
                        for (int q = 0; q < NCG; q++) v[q] = vw[q];
                    }
                }
            }
            fresh = false;
        }

        // ---- residuals of this point ----
        // rho is recomputed from x every pass (one A v): carried from step to step instead (rho+ = rho + theta (e - eta rho))
        // its absolute rounding error stays ~1e-15 while x itself shrinks to 1e-13 on slowly collapsing infeasible LPs
        double rho;
        {
            double xm[NCG];
#pragma unroll
            for (int q = 0; q < NCG; q++) xm[q] = act(q) ? x[q] : 0.0;
            rho = fma(b, tau, -w.A_times(xm));
        }
        double s2 = 0.0, om2 = 0.0, gam = 0.0, pp = 0.0, dd = BD ? b * y : 0.0;   // dd: b'y + u's; without BD b'y is formed below
#pragma unroll
        for (int q = 0; q < NCG; q++) {
            const bool a = act(q), bq = bnd(q);
            const double sgq = a ? fma(c[q], tau, z[q] - v[q]) - (bq ? s[q] : 0.0) : 0.0;
            const double om = bq ? fma(u[q], tau, -x[q]) - t[q] : 0.0;
            s2 = fma(sgq, sgq, s2);
            om2 = fma(om, om, om2);
            gam += a ? x[q] * z[q] : 0.0;
            if constexpr (BD) gam += bq ? s[q] * t[q] : 0.0;
            pp = add_cx(q, pp);
            if constexpr (BD) dd += bq ? u[q] * s[q] : 0.0;
        }
        s2 = grp_sum<MP>(s2); gam = grp_sum<MP>(gam);
        const double po = grp_sum<MP>(pp);
        const double du = grp_sum<MP>(BD ? dd : b * y);
        const double norms = sqrt(s2);
        const double normr = sqrt(grp_sum<MP>(BD ? fma(rho, rho, om2) : rho * rho));

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
                    if constexpr (BD) {   // (u[q] is the scaled bound: the verdict of the load came from the input)
                        const double cj = ok[q] ? fabs(cg[lp * n + gcol(q, go)]) : 0.0;
                        const double uj = ok[q] ? ug[lp * n + gcol(q, go)] : 0.0;
                        cm = fmax(cm, act(q) ? cj : 0.0);
                        ca = fmax(ca, cj); um = fmax(um, (uj > 0.0 && uj < HUGE_VAL) ? uj : 0.0);
                    } else cm = fmax(cm, ok[q] ? fabs(cg[lp * n + gcol(q, go)]) : 0.0);
                }
                sb = grp_max<MP>(rowok ? fabs(bg[lp * m + go]) : 0.0);
                sc = grp_max<MP>(cm);
                bool scaled;      // (the verdict of the load: the same maxima)
                if constexpr (BD) scaled = autoscale_lp(o.flags, sb, grp_max<MP>(ca), grp_max<MP>(um));
                else scaled = autoscale_lp(o.flags, sb, sc, 0.0);
                sb = (scaled && sb > 0.0) ? sb : 1.0; sc = (scaled && sc > 0.0) ? sc : 1.0;
                if constexpr (BD) sb = (sb < HUGE_VAL) ? sb : 1.0;
            }
            // optimal (and iteration-limit) points leave the homogeneous scaling (hsd.c:266-273); certificates stay
            const double rt = (stat_ == PYCLLP_STATUS_OPTIMAL || stat_ == PYCLLP_STATUS_ITERATION_LIMIT) ? 1.0 / tau : 1.0;
#pragma unroll
            for (int q = 0; q < NCG; q++) {
                const int j = gcol(q, go);
                if (ok[q]) {
                    if constexpr (BD) {
                        const bool a = act(q), bq = bnd(q);
                        const double r = fma(c[q], tau, -v[q]);      // reduced cost of a fixed column
                        xg[lp * n + j] = a ? x[q] * rt * sb : 0.0;
                        if (zg) zg[lp * n + j] = (a ? z[q] : fmax(-r, 0.0)) * rt * sc;
                        if (sg) sg[lp * n + j] = (bq ? s[q] : (a ? 0.0 : fmax(r, 0.0))) * rt * sc;
                    } else {   // every column stored takes part
                        xg[lp * n + j] = x[q] * rt * sb;
                        if (zg) zg[lp * n + j] = z[q] * rt * sc;
                    }
                }
            }
            if (yg && rowok) yg[lp * m + go] = y * rt * sc;
            // The iteration limit is met at the top of a pass, so po, du are those of the point stored: what BD returns.  Without BD:
            // the objectives of the point the last step started from, over the tau it ended on -- what the oracle (hsd_one_raw) and
            // the other kernels of that variant return there
            const bool lim = !BD && stat_ == PYCLLP_STATUS_ITERATION_LIMIT && it > 0;
            if (go == 0) {
                if (pobj) pobj[lp] = (lim ? po_prev : po) * rt * (sb * sc);
                if (dobj) dobj[lp] = (lim ? du_prev : du) * rt * (sb * sc);
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
                for (int q = 0; q < NCG; q++) {
                    x[q] = 1.0; z[q] = 1.0;
                    if constexpr (BD) { t[q] = 1.0; s[q] = 1.0; u[q] = 0.0; }
                    c[q] = 0.0; v[q] = 0.0;
                }
                b = 0.0; y = 0.0; tau = 1.0; kap = 1.0;
            }
        };

        // ---- stop tests (oracle hsd_one_raw; BD: on the expansion) ----
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

        const double mu = (gam + tau * kap) / (BD ? ncomp : (double)(iopaque(n) + 1)), dmu = o.delta * mu;
        const double phi = du - po + kap;
        if constexpr (!BD) { po_prev = po; du_prev = du; }

        // ---- the step quantities of column q: d, r0 and (BD) w = d s/t, h, z/x (all zero where the column takes no part);
        // without a bound d = 1/(z/x) is formed as x/z ----
        auto column = [&](int q, double& dq, double& wq, double& hq, double& r0q, double& zxq) {
            const bool a = act(q), bq = bnd(q);
            const double rx = fast_rcp(x[q]), rz = BD ? 0.0 : fast_rcp(z[q]);
            const double sgq = fma(c[q], tau, z[q] - v[q]) - (bq ? s[q] : 0.0);
            if constexpr (BD) {
                zxq = z[q] * rx;
                const double stq = bq ? s[q] * fast_rcp(t[q]) : 0.0;
                const double om = bq ? fma(u[q], tau, -x[q]) - t[q] : 0.0;
                dq = a ? fast_rcp(zxq + stq) : 0.0;
                wq = dq * stq;
                hq = bq ? fma(HSD_ETA, om, t[q] - dmu * fast_rcp(s[q])) : 0.0;
            } else dq = a ? x[q] * rz : 0.0;
            r0q = a ? fma(HSD_ETA, sgq, fma(dmu, rx, -z[q])) : 0.0;
        };

        // ---- Gram product, fused with A dc and A dr ----
        double Adc = 0.0, Adr = 0.0;
        auto do_gram = [&](double& Adc_, double& Adr_) {
            double d[NCG], dc[NCG], dr[NCG];
#pragma unroll
            for (int q = 0; q < NCG; q++) {
                if constexpr (BD) {
                    double wq, hq, r0q, zxq;
                    column(q, d[q], wq, hq, r0q, zxq);
                    dc[q] = act(q) ? fma(d[q], c[q], bnd(q) ? wq * u[q] : 0.0) : 0.0;
                    dr[q] = fma(d[q], r0q, wq * hq);
                } else {
                    const double rx = fast_rcp(x[q]), rz = fast_rcp(z[q]);
                    const double sgq = fma(c[q], tau, z[q] - v[q]);
                    d[q] = ok[q] ? x[q] * rz : 0.0;
                    dr[q] = ok[q] ? fma(HSD_ETA, sgq, fma(dmu, rx, -z[q])) : 0.0;     // r0
                }
            }
            // without BD the products d c, d r0 are formed where they are used
            const int go = w.ogl();
#pragma unroll 1
            for (int g = 0; g < G; g++) {
                if (__shfl((int)live, g * MP, WAVE) == 0) continue;      // an idle lane group
                if (grp == g) {
#pragma unroll
                    for (int q = 0; q < NCD; q++) {
                        const int p = G_::kpos(go + MP * q);
                        w.stage[p] = BD ? dc[q] : d[q] * c[q];               // gram_one's "x" operand
                        w.stage[ND + p] = d[q];
                        w.stage[2 * ND + p] = BD ? dr[q] : d[q] * dr[q];
                    }
                }
                wave_lds_sync();
                double axg, adg;
                if constexpr (PA) w.Aimg = areas + g * P_::AREA;       // group g's matrix (wave-uniform)
                w.template gram_one<true, BD>(g, axg, adg);
                if constexpr (PA) w.Aimg = Aimg;
                wave_lds_sync();
                if (grp == g) { Adc_ = axg; Adr_ = adg; }
            }
            if (SL) {   // identity columns: the slack's dc, dr go straight to row gl, d_slack onto the diagonal of M
                Adc_ += BD ? dc[NCG - 1] : d[NCG - 1] * c[NCG - 1];
                Adr_ += BD ? dr[NCG - 1] : d[NCG - 1] * dr[NCG - 1];
                w.slab[G_::sidx(go, go)] += d[NCG - 1];
                wave_lds_sync();
            }
        };
        do_gram(Adc, Adr);
        double pv = Adc - b;
        double qv = fma(-HSD_ETA, rho, Adr);
        double rdiag;
        constexpr bool CARRY = GWave<MP, NP, SL>::CARRY;
        double fr[2] = {pv, qv};   // both right-hand sides ride through the sweep (see ipm_group_kernel)
        bool fused = CARRY;
        constexpr bool SPLIT = GWave<MP, NP, SL>::SPLIT;   // the split sweep (GWave::factor_sweep): no kernel here pays registers for it
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
            // pivot floor of column j: pivot_floor^2 |M_jj| -- relative to the pivot's own original diagonal entry (see the
            // oracle); the vector goes to the (idle) staging area of the group and is read back as a broadcast per column
            int gro = grp;
            asm volatile("" : "+v"(gro));
            double* fl = w.stage + gro * MP;
            const double pf = sopaque(o.pivot_floor);
            const double myfloor = pf * pf * fabs(diag);
            fl[go] = myfloor;
            wave_lds_sync();
            // (a software-pipelined sweep paid 1.7 % here only while hsd_group_kernel ran one wave per SIMD; see GWave::factor_dpp)
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
        // (the (32, 128) kernel without the identity tail alone keeps u1, u2 through the staging area: 0 -> 3 spilt registers otherwise)
        constexpr bool AT_STAGED = MP == 32 && NP == 128 && !SL;
        w.template At_times2<AT_STAGED>(pv, qv, ap, aq);
        // ---- e = c - A'p,  uu = d e + w u,  v = dr - d A'q, and the sums of dtau.  ap keeps uu in place of A'p; wv keeps what
        // A'dy = A'p dtau + A'q is formed from below: A'p with BD, e without ----
        double dsum = 0.0, nsum = 0.0;
#pragma unroll
        for (int q = 0; q < NCG; q++) {
            if constexpr (BD) {
                const bool a = act(q), bq = bnd(q);
                double wq, hq, r0q, zxq;
                column(q, d[q], wq, hq, r0q, zxq);
                const double wu = bq ? wq * u[q] : 0.0;
                const double cp = a ? c[q] - ap[q] : 0.0;
                const double uu = fma(d[q], cp, wu);
                const double vq = fma(d[q], r0q - aq[q], wq * hq);
                dx[q] = vq;
                dsum = fma(d[q] * cp, cp, dsum);
                dsum += bq ? zxq * wu * u[q] : 0.0;
                nsum += a ? c[q] * vq : 0.0;
                nsum -= bq ? wu * (r0q - aq[q] - zxq * hq) : 0.0;
                wv[q] = ap[q];
                ap[q] = uu;
            } else {
                const double rx = fast_rcp(x[q]), rz = fast_rcp(z[q]);
                const double sgq = fma(c[q], tau, z[q] - v[q]);
                d[q] = ok[q] ? x[q] * rz : 0.0;
                const double r0q = ok[q] ? fma(HSD_ETA, sgq, fma(dmu, rx, -z[q])) : 0.0;
                const double cp = c[q] - ap[q];
                const double uu = d[q] * cp;
                dx[q] = d[q] * (r0q - aq[q]);
                ap[q] = uu;
                wv[q] = cp;
                dsum = fma(uu, cp, dsum);
                nsum = fma(c[q], dx[q], nsum);
            }
        }
        // (grp_sum pins its inputs: dtau is bit-uniform over the lane group)
        const double den = grp_sum<MP>(dsum) + kap / tau;
        const double num = fma(HSD_ETA, phi, dmu / tau - kap) + grp_sum<MP>(b * qv) - grp_sum<MP>(nsum);
        const double dtau = num / den;
        double dy = fma(pv, dtau, qv);
#pragma unroll
        for (int q = 0; q < NCG; q++) {
            dx[q] = fma(ap[q], dtau, dx[q]);
            wv[q] = fma(BD ? wv[q] : c[q] - wv[q], dtau, aq[q]);   // A'dy = A'p dtau + A'q
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
            // ---- step: theta = min(r / max(0, -dtau/tau, -dkappa/kappa, -dx/x, -dz/z, -dt/t, -ds/s), 1) ----
            const double dkap = dmu / tau - kap - kap / tau * dtau;
            double dz[NCG], dt[NCG], ds[NCG];
            double th = fmax(fmax(-dtau / tau, -dkap / kap), 0.0);
#pragma unroll
            for (int q = 0; q < NCG; q++) {
                const bool a = act(q), bq = bnd(q);
                const double rx = fast_rcp(x[q]), rz = fast_rcp(z[q]), rt_ = BD ? fast_rcp(t[q]) : 0.0, rs = BD ? fast_rcp(s[q]) : 0.0;
                const double sgq = fma(c[q], tau, z[q] - v[q]) - (bq ? s[q] : 0.0);
                const double om = bq ? fma(u[q], tau, -x[q]) - t[q] : 0.0;
                dz[q] = a ? (dmu - z[q] * dx[q]) * rx - z[q] : 0.0;
                if constexpr (BD) {
                    // two branches for dt, ds (see ipm_group_bdhsd.inc): the multiplier of the other one's rounding error is min(s/t, t/s)
                    const double dt1 = fma(u[q], dtau, HSD_ETA * om) - dx[q];
                    const double ds1 = (dmu - s[q] * dt1) * rt_ - s[q];
                    const double ds2 = dz[q] + fma(HSD_ETA, sgq, fma(c[q], dtau, -wv[q]));
                    const double dt2 = fma(dmu, rs, -t[q]) - (t[q] * rs) * ds2;
                    const bool first = t[q] >= s[q];
                    dt[q] = bq ? (first ? dt1 : dt2) : 0.0;
                    ds[q] = bq ? (first ? ds1 : ds2) : 0.0;
                }
                if (a) th = fmax(th, fmax(-dz[q] * rz, -dx[q] * rx));
                if (bq) th = fmax(th, fmax(-dt[q] * rt_, -ds[q] * rs));
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
            tau = fma(theta, dtau, tau);
            kap = fma(theta, dkap, kap);
            it++;
        }
        if (fin && live) finalize(PYCLLP_STATUS_NUMERICAL);
    }
#undef HSD_ETA
#undef HSD_EINF
