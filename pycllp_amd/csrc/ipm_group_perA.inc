// ipm_group_perA.inc -- the lane-group kernel (ipm_group.inc) for batches in which EVERY LP HAS ITS OWN DENSE A:
//   maximise c_k'x  subject to  A_k x = b_k,  x >= 0,   A_k [m, n] (SL = false) or A_k = [A_k dense [m, n - m] | I] (SL = true)
// (DESIGN.md section 16).  ipm_group_kernel copies the one shared A into LDS once per workgroup; here every SLOT (lane group)
// owns an area of the shape GeoG::SHARED -- row-major image with the odd stride AS, the column sums A'1, the MP = 32 Gram
// store table -- and nothing is shared between the waves of a workgroup, so the kernel has no workgroup barrier at all.  A slot
// that takes an LP from the queue (and at its first LP) has the whole wave copy that LP's matrix, m x a_cols contiguous
// doubles, from HBM into its image and recompute the column sums; the pad rows and columns are zeroed once and never
// written again (every LP of a batch has the same m and a_cols).
// The Gram product, the LDL' (both paths), the substitution, A'u, A v and the refinement are the GWave<MP, NP, SL> members,
// unchanged: they address the matrix through w.Aimg, which is set to group g's area (wave-uniform) before gram_one(g, ..) and
// to the lane's own group's area (lane-varying; the members' addresses are per-lane values anyway) before everything else.
// The per-slot phases are those of ipm_group_kernel (DESIGN.md section 2) in the simplified order of ipm_bounded_kernel:
// rho = b - A x comes from the Gram pass every iteration (no carried residual, no predicted stop test), so the stop test of a
// point runs after its Gram product and a slot that finishes idles through the rest of that pass; no warm start, no
// predictor-corrector, no HSD.  At the iteration limit the objectives stored are those of the point stored.

// (GeoPA -- the per-wave LDS of this kernel and the waves its launch bounds allow -- is in group_pa.h, which the launch plan shares.)

template <int MP, int NP, bool SL>
__global__ void __launch_bounds__((GeoPA<GeoG<MP, NP, SL>>::WPB_MAX * 64))
ipm_group_pa_kernel(int m, int n, long B, const double* __restrict__ Ag, const double* __restrict__ bg,
                    const double* __restrict__ cg, double* __restrict__ xg, double* __restrict__ yg,
                    double* __restrict__ zg, double* __restrict__ pobj, double* __restrict__ dobj,
                    int* __restrict__ status, int* __restrict__ iters, int* __restrict__ queue, DevOpts o) {
    using G_ = GeoG<MP, NP, SL>;
    using P_ = GeoPA<G_>;
    constexpr int G = G_::G, NCG = G_::NCG, NCD = G_::NCD, ND = G_::ND, JB = G_::JB, AS = G_::AS;
    const int nd = SL ? n - m : n;          // columns of A_k as stored (the last m columns of the LP are the identity when SL)
    extern __shared__ __attribute__((aligned(16))) double lds[];
    const int tid = threadIdx.x;
    const int wpb = blockDim.x / WAVE;
    const int wave = tid / WAVE;
    const int lane = tid & 63, gl = lane & (MP - 1), grp = lane / MP;
    double* areas = lds + wave * P_::PW;            // G areas of this wave, then its slabs and staging region
    // pad rows and columns of every image (and the column sums behind it) are zero from here on; a refill writes rows < m,
    // columns < nd only
    for (int i = lane; i < G * P_::AREA; i += WAVE) areas[i] = 0.0;
    wave_lds_sync();
    for (int g = 0; g < G; g++) G_::fill_gram_table(areas + g * P_::AREA, lane, WAVE);

    GWave<MP, NP, SL> w;
    w.lane = lane; w.gl = gl; w.grp = grp; w.m = m; w.n = n;
    const double* own_area = areas + grp * P_::AREA;      // the image of the lane's own group
    w.Aimg = own_area;
    w.slab0 = areas + G * P_::AREA;
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
    const int asz = m * nd;                 // doubles of one A_k

    const long nslots = (long)gridDim.x * wpb * G;
    long lp = (long)grp * ((long)gridDim.x * wpb) + (long)blockIdx.x * wpb + wave;
    bool live = lp < B, fresh = live;

    double x[NCG], z[NCG], c[NCG], v[NCG];
    bool ok[NCG];
#pragma unroll
    for (int q = 0; q < NCG; q++) {
        ok[q] = (q < NCD) ? (gl + MP * q < nd) : (gl < m);
        x[q] = 1.0; z[q] = 1.0; c[q] = 0.0; v[q] = 0.0;
    }
    auto gcol = [&](int q, int g_) { return (q < NCD) ? g_ + MP * q : nd + g_; };
    double b = 0.0, y = 0.0;
    double tol_r = 0.0, tol_s = 0.0, etol = 0.0, normr0 = 1e300, norms0 = 1e300;
    int it = 0;

    while (__any(live)) {
        if (__any(fresh)) {
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
                    for (int u = 0; u < 8; u++) av[u] = (i0 + u * WAVE < asz) ? src[i0 + u * WAVE] : 0.0;
#pragma unroll
                    for (int u = 0; u < 8; u++) {
                        if (i0 + u * WAVE < asz) img[r * AS + cidx] = av[u];
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
            if (fresh) {
                const int go = w.ogl();
                const double* colsum = own_area + G_::AIMG;
#pragma unroll
                for (int q = 0; q < NCG; q++) {
                    const int j = gcol(q, go);
                    c[q] = ok[q] ? cg[lp * n + j] : 0.0;
                    x[q] = 1.0; z[q] = 1.0;
                    v[q] = (q < NCD) ? colsum[go + MP * q] : (rowok ? 1.0 : 0.0);   // A'y for y = 1
                }
                b = rowok ? bg[lp * m + go] : 0.0;
                y = rowok ? 1.0 : 0.0;
            }
            if (autoscale) {   // solve the LP with b/max|b| and c/max|c| (PYCLLP_FLAG_AUTOSCALE); undone when storing
                double cm = 0.0;
#pragma unroll
                for (int q = 0; q < NCG; q++) cm = fmax(cm, fabs(c[q]));
                double sb = grp_max<MP>(fabs(b)), sc = grp_max<MP>(cm);
                sb = (sb > 0.0) ? sb : 1.0; sc = (sc > 0.0) ? sc : 1.0;
                if (fresh) {
                    b = b / sb;
#pragma unroll
                    for (int q = 0; q < NCG; q++) c[q] = c[q] / sc;
                }
            }
            double c2 = 0.0;
#pragma unroll
            for (int q = 0; q < NCG; q++) c2 = fma(c[q], c[q], c2);
            const double nb2 = grp_sum<MP>(b * b), nc2 = grp_sum<MP>(c2);
            if (fresh) {
                tol_r = o.eps * (1.0 + sqrt(nb2));
                tol_s = o.eps * (1.0 + sqrt(nc2));
                etol = o.refine_tol * (1.0 + sqrt(nb2));
                normr0 = 1e300; norms0 = 1e300; it = 0;
            }
            fresh = false;
        }

        // ---- dual infeasibility, complementarity, objectives (as ipm_group_kernel) ----
        double s2 = 0.0, gam = 0.0, pp = 0.0;
#pragma unroll
        for (int q = 0; q < NCG; q++) {
            const double sg = ok[q] ? c[q] - v[q] + z[q] : 0.0;
            s2 = fma(sg, sg, s2);
            gam += ok[q] ? x[q] * z[q] : 0.0;
            pp += c[q] * (ok[q] ? x[q] : 0.0);
        }
        s2 = grp_sum<MP>(s2); gam = grp_sum<MP>(gam);
        const double po = grp_sum<MP>(pp);
        const double du = grp_sum<MP>(b * y);
        const double norms = sqrt(s2);
        const double mu = o.delta * gam / (double)(n + m);

        // store a finished LP and hand the slot its next one from the device-wide queue
        auto finalize = [&](int stat_) {
            double sb = 1.0, sc = 1.0;
            const int go = w.ogl();
            int gro = grp;
            asm volatile("" : "+v"(gro));
            if (autoscale) {   // the scale factors from the inputs
                double cm = 0.0;
#pragma unroll
                for (int q = 0; q < NCG; q++) cm = fmax(cm, ok[q] ? fabs(cg[lp * n + gcol(q, go)]) : 0.0);
                sb = grp_max<MP>(rowok ? fabs(bg[lp * m + go]) : 0.0);
                sc = grp_max<MP>(cm);
                sb = (sb > 0.0) ? sb : 1.0; sc = (sc > 0.0) ? sc : 1.0;
            }
#pragma unroll
            for (int q = 0; q < NCG; q++) {
                const int j = gcol(q, go);
                if (ok[q]) {
                    xg[lp * n + j] = x[q] * sb;
                    if (zg) zg[lp * n + j] = z[q] * sc;
                }
            }
            if (yg && rowok) yg[lp * m + go] = y * sc;
            // the iteration limit is met after a step, and po, du above belong to the point before it: the objectives stored are
            // those of the point stored (as ipm_bounded_kernel stores them)
            double pof = po, duf = du;
            if (stat_ == PYCLLP_STATUS_ITERATION_LIMIT) {
                double pp2 = 0.0;
#pragma unroll
                for (int q = 0; q < NCG; q++) pp2 += c[q] * (ok[q] ? x[q] : 0.0);
                pof = grp_sum<MP>(pp2);
                duf = grp_sum<MP>(b * y);
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
            if (!live) {   // park the slot on harmless values (its image keeps the last LP's matrix: finite, never stored from)
#pragma unroll
                for (int q = 0; q < NCG; q++) { x[q] = 1.0; z[q] = 1.0; c[q] = 0.0; v[q] = 0.0; }
                b = 0.0; y = 0.0;
            }
        };

        // ---- d = x/z, t = c - A'y + mu/x ----
        double rxk[NCG], rzk[NCG];
#pragma unroll
        for (int q = 0; q < NCG; q++) { rxk[q] = fast_rcp(x[q]); rzk[q] = fast_rcp(z[q]); }
        auto newton_dt = [&](int q, double& dq, double& tq) {
            dq = ok[q] ? x[q] * rzk[q] : 0.0;
            tq = ok[q] ? c[q] - v[q] + mu * rxk[q] : 0.0;
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
                        w.stage[p] = ok[q] ? x[q] : 0.0;
                        w.stage[ND + p] = d[q];
                        w.stage[2 * ND + p] = d[q] * tt[q];
                    }
                }
                wave_lds_sync();
                double axp[JB], adp[JB];
                w.Aimg = areas + g * P_::AREA;         // group g's matrix (wave-uniform)
                w.template gram_one<true, true>(g, axp, adp);
                w.Aimg = own_area;
                wave_lds_sync();
                if (grp == g) {
                    Ax_ = (JB == 1) ? axp[0] : ((gl >> 4) ? axp[JB - 1] : axp[0]);
                    Adt_ = (JB == 1) ? adp[0] : ((gl >> 4) ? adp[JB - 1] : adp[0]);
                }
            }
            if (SL) {   // identity columns: x_slack and (d t)_slack go straight to row gl, d_slack onto the diagonal of M
                Ax_ += ok[NCG - 1] ? x[NCG - 1] : 0.0;
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
        if (!(isfinite(normr) && isfinite(norms) && isfinite(gam))) stat = PYCLLP_STATUS_NUMERICAL;
        else if (normr <= tol_r && norms <= tol_s && gam <= o.eps * (1.0 + fabs(po))) stat = PYCLLP_STATUS_OPTIMAL;
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
            // ---- step: theta = min(r / max(0, -dx/x, -dz/z), 1) ----
            double dz[NCG];
            double th = 0.0;
#pragma unroll
            for (int q = 0; q < NCG; q++) {
                dz[q] = ok[q] ? (mu - z[q] * dx[q]) * rxk[q] - z[q] : 0.0;
                if (ok[q]) th = fmax(th, fmax(-dz[q] * rzk[q], -dx[q] * rxk[q]));
            }
            th = grp_max<MP>(th);
            const double theta = fmin(o.r / th, 1.0);
            y = fma(theta, dy, y);
#pragma unroll
            for (int q = 0; q < NCG; q++) {
                x[q] = fma(theta, dx[q], x[q]);
                z[q] = fma(theta, dz[q], z[q]);
                v[q] = fma(theta, wv[q], v[q]);
            }
            normr0 = normr; norms0 = norms;
            it++;
            if (it >= o.max_iter) fin = true;   // status stays ITERATION_LIMIT
        }
        if (fin && live) finalize(stat);
    }
}
