// ipm_group_hsd.inc -- the group-per-LP solve kernel on the homogeneous self-dual embedding (PYCLLP_FLAG_HSD).
//
// Same machinery as ipm_group.inc (one LP per lane group, MFMA Gram product, register-resident LDL', DPP solves,
// slot refill from the device queue); what changes is the Newton system.  The model is the one of the reference's CPU
// solver ipo/hsd.c:27-312 (x, z, y plus tau = `phi`, kappa = `psi`), re-derived on the normal equations -- see
// hsd_one_raw() in oracle/ipm_dense_ref.c, which this kernel follows statement by statement:
//     rho = b tau - A x,  sigma = c tau - A'y + z,  phi = b'y - c'x + kappa,  mu = (x'z + tau kappa)/(N + 1)
//     M p = A(d c) - b,   M q = A(d r1) - eta rho          (ONE factorisation, two right-hand sides)
//     dtau = (eta phi - c'v + b'q + delta mu/tau - kappa) / (|sqrt(d)(c - A'p)|^2 + kappa/tau)
//     dy = p dtau + q,  dx = u dtau + v,  u = d (c - A'p),  v = d (r1 - A'q)
// Infeasible and unbounded LPs end after ~12-15 iterations with a certificate (status 2: y, z with b'y < 0 and
// A'y - z ~ 0; status 4: x with c'x > 0 and A x ~ 0) instead of running into the heuristic 10x-growth exits or the
// iteration limit of the plain path.  Cost per iteration: one extra forward/back substitution (run interleaved with
// the first, same factor loads), one extra A'u (fused, same A loads) and a handful of group reductions; the Gram
// product is unchanged -- its two fused mat-vecs now carry A(d c) and A(d r1), so rho = b tau - A x costs one A v.

#ifndef PYCLLP_HSD_AT_RB
#define PYCLLP_HSD_AT_RB 4   // rows of A per batch of the pipelined two-vector A'u
#endif
template <int MP, int NP, bool SL>
struct GWaveH : GWave<MP, NP, SL> {
    using Base = GWave<MP, NP, SL>;
    using G_ = GeoG<MP, NP, SL>;
    static constexpr int G = G_::G, NCG = G_::NCG, NCD = G_::NCD, AS = G_::AS, MS = G_::MS;

    // A'u1 and A'u2 in one pass over the image of A (pipelined like GWave::At_times; u1 and u2 from registers like there, or
    // STAGED through the wave's staging area)
    template <bool STAGED = false>
    __device__ __forceinline__ void At_times2(double u1, double u2, double (&o1)[NCG], double (&o2)[NCG]) const {
        const int g = this->ogl();     // opaque: see GWave::ogl()
        double ur1[2] = {u1, u1}, ur2[2] = {u2, u2};
        const __attribute__((address_space(3))) double* ub = nullptr;
        if constexpr (STAGED) {
            this->stage[this->grp * MP + g] = u1;
            this->stage[G * MP + this->grp * MP + g] = u2;
            wave_lds_sync();
            unsigned uba = lds_addr(this->stage + this->grp * MP);      // opaque: see GWave::A_times
            asm volatile("" : "+v"(uba));
            ub = (const __attribute__((address_space(3))) double*)(size_t)uba;
        } else if constexpr (MP == 32) {   // (whole wave active)
            ur1[0] = top_row_d(u1); ur1[1] = bottom_row_d(u1);
            ur2[0] = top_row_d(u2); ur2[1] = bottom_row_d(u2);
        }
        const double* ac = this->Aimg + g;
        constexpr int RB = PYCLLP_HSD_AT_RB, NB = MP / RB;
        double a0[RB][NCD], a1[RB][NCD], u0[RB][2], u1_[RB][2];
#define AT_LOAD(A_, U_, I0)                                                                     \
    static_for<0, RB>([&](auto ic_) {                                                           \
        constexpr int ii = decltype(ic_)::value, i_ = (I0) + ii;                                \
        if constexpr (STAGED) {                                                                 \
            U_[ii][0] = ub[i_ + tok];                                                           \
            U_[ii][1] = ub[G * MP + i_ + tok];                                                  \
        } else {                                                                                \
            U_[ii][0] = row_bcast<(i_ & 15)>(ur1[i_ >> 4]);                                     \
            U_[ii][1] = row_bcast<(i_ & 15)>(ur2[i_ >> 4]);                                     \
        }                                                                                       \
        _Pragma("unroll") for (int q = 0; q < NCD; q++) A_[ii][q] = ac[i_ * AS + MP * q + tok]; \
    });
#define AT_USE(A_, U_)                                                                          \
    _Pragma("unroll") for (int ii = 0; ii < RB; ii++) {                                         \
        asm volatile("" : "+v"(U_[ii][0]));                                                     \
        asm volatile("" : "+v"(U_[ii][1]));                                                     \
        _Pragma("unroll") for (int q = 0; q < NCD; q++) asm volatile("" : "+v"(A_[ii][q]));     \
    }                                                                                           \
    asm volatile("" : "+v"(tok));                                                               \
    _Pragma("unroll") for (int ii = 0; ii < RB; ii++)                                           \
        _Pragma("unroll") for (int q = 0; q < NCD; q++) {                                       \
            o1[q] = fma(A_[ii][q], U_[ii][0], o1[q]);                                           \
            o2[q] = fma(A_[ii][q], U_[ii][1], o2[q]);                                           \
        }                                                                                       \
    /* the sums are pinned too: left free, the scheduler sinks every FMA below the last batch's loads and the whole   */ \
    /* image of A (128 registers at (32, 64)) is live at once -- 323 spilled registers at 8 waves per CU               */ \
    _Pragma("unroll") for (int q = 0; q < NCD; q++) { asm volatile("" : "+v"(o1[q])); asm volatile("" : "+v"(o2[q])); }
#pragma unroll
        for (int q = 0; q < NCG; q++) { o1[q] = 0.0; o2[q] = 0.0; }
        if (SL) { o1[NCG - 1] = u1; o2[NCG - 1] = u2; }
        int tok = 0;
        asm volatile("" : "+v"(tok));
        AT_LOAD(a0, u0, 0)
        static_for<0, NB / 2>([&](auto bc) {
            constexpr int b2 = 2 * decltype(bc)::value;
            AT_LOAD(a1, u1_, (b2 + 1) * RB)
            AT_USE(a0, u0)
            if constexpr (b2 + 2 < NB) { AT_LOAD(a0, u0, (b2 + 2) * RB) }
            AT_USE(a1, u1_)
        });
#undef AT_LOAD
#undef AT_USE
        if constexpr (STAGED) wave_lds_sync();
    }

    // (s, t) <- (L D L')^-1 (s, t): GWave::fwd_back for two right-hand sides, the two dependency chains interleaved
    // (forward2 / backward2 are its halves: behind factor_dpp_fwd, which carries both right-hand sides through the sweep, the
    // caller runs backward2 alone)
    __device__ __forceinline__ void fwd_back2(double& s, double& t, double rdiag) const {
        forward2(s, t);
        backward2(s, t, rdiag);
    }
    __device__ __forceinline__ void forward2(double& s, double& t) const {
        const int gl = this->gl;
        const int g = this->ogl();
        const double* slab = this->slab;
        double lf[MP];
        if constexpr (Base::COLB) {
#pragma unroll
            for (int k = 0; k < MP - 1; k++) lf[k] = *(const __attribute__((address_space(3))) double*)(size_t)(this->xb[k & 15] + 256u * (unsigned)(k & ~15));
        } else {
#pragma unroll
            for (int k = 0; k < MP - 1; k++) lf[k] = slab[G_::sidx(k, g)];
        }
#pragma unroll
        for (int k = 0; k < MP - 1; k++) asm volatile("" : "+v"(lf[k]));
        if constexpr (MP == 16) {
            subst15_up2(s, t, lf);
        } else {
            const bool top = gl < 16;
            if (top) subst15_up2(s, t, lf);
            const double so = top_row_d(s), to = top_row_d(t);          // (outside the branches: both rows active)
            if (!top) {
                s -= dot16_bcast(so, lf); t -= dot16_bcast(to, lf);
                subst15_up2(s, t, lf + 16);
            }
        }
    }
    __device__ __forceinline__ void backward2(double& s, double& t, double rdiag) const {
        const int gl = this->gl;
        s *= rdiag; t *= rdiag;
        double lb[MP];
        this->load_own_row(lb);
#pragma unroll
        for (int i = 1; i < MP; i++) asm volatile("" : "+v"(lb[i]));
        if constexpr (MP == 16) {
            subst15_down2(s, t, lb);
        } else {
            const bool top = gl < 16;
            if (!top) subst15_down2(s, t, lb + 16);
            const double so = bottom_row_d(s), to = bottom_row_d(t);    // (outside the branches: both rows active)
            if (top) {
                s -= dot16_bcast(so, lb + 16); t -= dot16_bcast(to, lb + 16);
                subst15_down2(s, t, lb);
            }
        }
    }
};

#ifndef PYCLLP_WPB_HSD
#define PYCLLP_WPB_HSD 8    // waves per workgroup for MP = 32 (4 = one per SIMD, 512 registers per lane: what rounds 1-2 needed)
#endif
// the 16-row variants fit into 256 registers without scratch: they run 8 waves per CU like the plain kernel
template <int MP> constexpr int hsd_wpb() { return MP == 16 ? PYCLLP_WPB : PYCLLP_WPB_HSD; }

template <int MP, int NP, bool SL>
__global__ void __launch_bounds__(hsd_wpb<MP>() * 64)
hsd_group_kernel(int m, int n, long B, const double* __restrict__ Ag, const double* __restrict__ bg,
                 const double* __restrict__ cg, double* __restrict__ xg, double* __restrict__ yg,
                 double* __restrict__ zg, double* __restrict__ pobj, double* __restrict__ dobj,
                 int* __restrict__ status, int* __restrict__ iters, int* __restrict__ queue, DevOpts o) {
    using G_ = GeoG<MP, NP, SL>;
    constexpr int G = G_::G, NCG = G_::NCG, NCD = G_::NCD, ND = G_::ND, JB = G_::JB, AS = G_::AS;
    const int nd = SL ? n - m : n;
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
    const bool warm = (o.flags & PYCLLP_FLAG_WARM_START) != 0;
    const bool autoscale = (o.flags & PYCLLP_FLAG_AUTOSCALE) != 0;
    const unsigned long long gmask = (MP == 32) ? 0xFFFFFFFFull : 0xFFFFull;
    // Wave-uniform doubles derived from the options (1 - delta, 100 eps, pivot_floor^2, N + 1) are NOT named here: as invariants
    // of the persistent loop they would each sit in a VGPR pair for the whole solve (f64 has no scalar ALU) -- or, at 256
    // registers, in scratch.  They are re-derived where they are used from an opaque copy of the SGPR-resident option.
#define HSD_ETA (1.0 - sopaque(o.delta))
#define HSD_EINF (100.0 * sopaque(o.eps))

    const long nslots = (long)gridDim.x * wpb * G;
    long lp = (long)grp * ((long)gridDim.x * wpb) + (long)blockIdx.x * wpb + wave;      // group-major: see ipm_group_kernel
    bool live = lp < B, fresh = live;

    double x[NCG], z[NCG], c[NCG], v[NCG];   // v = A'y, carried incrementally
    bool ok[NCG];
#pragma unroll
    for (int q = 0; q < NCG; q++) {
        ok[q] = (q < NCD) ? (gl + MP * q < nd) : (gl < m);
        x[q] = 1.0; z[q] = 1.0; c[q] = 0.0; v[q] = 0.0;
    }
    // global column of register q (dense registers first, then the slack column of row gl), from an opaque lane index: the cold
    // paths that need it (loading / storing an LP) must not leave per-lane addresses alive across the iterations
    auto gcol = [&](int q, int g_) { return (q < NCD) ? g_ + MP * q : nd + g_; };
    double b = 0.0, y = 0.0, tau = 1.0, kap = 1.0, nb = 0.0, nc = 0.0;
    double po_prev = 0.0, du_prev = 0.0;      // c'x and b'y of the point the last step started from
    int it = 0;

    while (__any(live)) {
        if (__any(fresh)) {
            if (fresh) {
                const int go = w.ogl();
#pragma unroll
                for (int q = 0; q < NCG; q++) {
                    const int j = gcol(q, go);
                    c[q] = ok[q] ? cg[lp * n + j] : 0.0;
                    x[q] = (warm && ok[q]) ? xg[lp * n + j] : 1.0;
                    z[q] = (warm && ok[q]) ? zg[lp * n + j] : 1.0;
                    v[q] = 0.0;
                }
                b = rowok ? bg[lp * m + go] : 0.0;
                y = (rowok && warm && yg) ? yg[lp * m + go] : 0.0;
            }
            if (autoscale) {
                double cm = 0.0;
#pragma unroll
                for (int q = 0; q < NCG; q++) cm = fmax(cm, fabs(c[q]));
                double sb = grp_max<MP>(fabs(b)), sc = grp_max<MP>(cm);
                const bool scaled = autoscale_lp(o.flags, sb, sc, 0.0);
                sb = (scaled && sb > 0.0) ? sb : 1.0; sc = (scaled && sc > 0.0) ? sc : 1.0;
                if (fresh) {
                    b = b / sb;
#pragma unroll
                    for (int q = 0; q < NCG; q++) c[q] = c[q] / sc;
                    if (warm) {
                        y = y / sc;
#pragma unroll
                        for (int q = 0; q < NCG; q++) { x[q] = x[q] / sb; z[q] = z[q] / sc; }
                    }
                }
            }
            double c2 = 0.0, g0 = 0.0;
#pragma unroll
            for (int q = 0; q < NCG; q++) {
                c2 = fma(c[q], c[q], c2);
                g0 += ok[q] ? x[q] * z[q] : 0.0;
            }
            const double nb2 = grp_sum<MP>(b * b), nc2 = grp_sum<MP>(c2);
            g0 = grp_sum<MP>(g0);
            double vw[NCG];
            if (warm) w.At_times(y, vw);
            if (fresh) {
                nb = sqrt(nb2); nc = sqrt(nc2);
                tau = 1.0;
                kap = warm ? g0 / (double)n : 1.0;
                it = 0;
                if (warm) {
#pragma unroll
                    for (int q = 0; q < NCG; q++) v[q] = vw[q];
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
            for (int q = 0; q < NCG; q++) xm[q] = ok[q] ? x[q] : 0.0;
            rho = fma(b, tau, -w.A_times(xm));
        }
        double s2 = 0.0, gam = 0.0, pp = 0.0;
#pragma unroll
        for (int q = 0; q < NCG; q++) {
            const double sg = ok[q] ? fma(c[q], tau, z[q] - v[q]) : 0.0;
            s2 = fma(sg, sg, s2);
            gam += ok[q] ? x[q] * z[q] : 0.0;
            pp += c[q] * (ok[q] ? x[q] : 0.0);
        }
        s2 = grp_sum<MP>(s2); gam = grp_sum<MP>(gam);
        const double po = grp_sum<MP>(pp);
        const double du = grp_sum<MP>(b * y);
        const double norms = sqrt(s2);
        const double normr = sqrt(grp_sum<MP>(rho * rho));

        auto finalize = [&](int stat_) {
            double sb = 1.0, sc = 1.0;
            const int go = w.ogl();
            int gro = grp;
            asm volatile("" : "+v"(gro));
            if (autoscale) {
                double cm = 0.0;
#pragma unroll
                for (int q = 0; q < NCG; q++) cm = fmax(cm, ok[q] ? fabs(cg[lp * n + gcol(q, go)]) : 0.0);
                sb = grp_max<MP>(rowok ? fabs(bg[lp * m + go]) : 0.0);
                sc = grp_max<MP>(cm);
                const bool scaled = autoscale_lp(o.flags, sb, sc, 0.0);      // (the verdict of the load: the same maxima)
                sb = (scaled && sb > 0.0) ? sb : 1.0; sc = (scaled && sc > 0.0) ? sc : 1.0;
            }
            // optimal (and iteration-limit) points leave the homogeneous scaling (hsd.c:266-273); certificates stay
            const double rt = (stat_ == PYCLLP_STATUS_OPTIMAL || stat_ == PYCLLP_STATUS_ITERATION_LIMIT) ? 1.0 / tau : 1.0;
#pragma unroll
            for (int q = 0; q < NCG; q++) {
                const int j = gcol(q, go);
                if (ok[q]) {
                    xg[lp * n + j] = x[q] * rt * sb;
                    if (zg) zg[lp * n + j] = z[q] * rt * sc;
                }
            }
            if (yg && rowok) yg[lp * m + go] = y * rt * sc;
            // at the iteration limit: the objectives of the point the last step started from, over the tau it ended on -- what the
            // oracle (hsd_one_raw) and the other kernels of this variant return there
            const bool lim = stat_ == PYCLLP_STATUS_ITERATION_LIMIT && it > 0;
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
            if (!live) {
#pragma unroll
                for (int q = 0; q < NCG; q++) { x[q] = 1.0; z[q] = 1.0; c[q] = 0.0; v[q] = 0.0; }
                b = 0.0; y = 0.0; tau = 1.0; kap = 1.0;
            }
        };

        // ---- stop tests (oracle hsd_one_raw) ----
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

        const double mu = (gam + tau * kap) / (double)(iopaque(n) + 1), dmu = o.delta * mu;
        const double phi = du - po + kap;
        po_prev = po; du_prev = du;

        // ---- Gram product, fused with A(d c) and A(d r1) ----
        double Adc = 0.0, Adr = 0.0;
        auto do_gram = [&](double& Adc_, double& Adr_) {
            double d[NCG], r1[NCG];
#pragma unroll
            for (int q = 0; q < NCG; q++) {
                const double rx = fast_rcp(x[q]), rz = fast_rcp(z[q]);
                const double sg = fma(c[q], tau, z[q] - v[q]);
                d[q] = ok[q] ? x[q] * rz : 0.0;
                r1[q] = ok[q] ? fma(HSD_ETA, sg, fma(dmu, rx, -z[q])) : 0.0;
            }
            const int go = w.ogl();
#pragma unroll 1
            for (int g = 0; g < G; g++) {
                if (__shfl((int)live, g * MP, WAVE) == 0) continue;      // an idle lane group
                if (grp == g) {
#pragma unroll
                    for (int q = 0; q < NCD; q++) {
                        const int p = G_::kpos(go + MP * q);
                        w.stage[p] = d[q] * c[q];          // gram_one's "x" operand
                        w.stage[ND + p] = d[q];
                        w.stage[2 * ND + p] = d[q] * r1[q];
                    }
                }
                wave_lds_sync();
                double axg, adg;
                w.gram_one(g, axg, adg);
                wave_lds_sync();
                if (grp == g) { Adc_ = axg; Adr_ = adg; }
            }
            if (SL) {
                Adc_ += d[NCG - 1] * c[NCG - 1];
                Adr_ += d[NCG - 1] * r1[NCG - 1];
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
        constexpr bool SPLIT = GWave<MP, NP, SL>::SPLIT;   // the split sweep (GWave::factor_sweep): no HSD kernel pays registers for it
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
            // (a software-pipelined sweep paid 1.7 % here only while this kernel ran one wave per SIMD; see GWave::factor_dpp)
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
        double dsum = 0.0, nsum = 0.0;
#pragma unroll
        for (int q = 0; q < NCG; q++) {
            const double rx = fast_rcp(x[q]), rz = fast_rcp(z[q]);
            const double sg = fma(c[q], tau, z[q] - v[q]);
            d[q] = ok[q] ? x[q] * rz : 0.0;
            const double r1 = ok[q] ? fma(HSD_ETA, sg, fma(dmu, rx, -z[q])) : 0.0;
            const double cp = c[q] - ap[q];
            const double u = d[q] * cp;
            dx[q] = d[q] * (r1 - aq[q]);        // v
            ap[q] = u;                          // keep u in place of A'p ...
            wv[q] = cp;                         // ... and c - A'p for the update of A'y below
            dsum = fma(u, cp, dsum);
            nsum = fma(c[q], dx[q], nsum);
        }
        const double den = grp_sum<MP>(dsum) + kap / tau;
        const double num = fma(HSD_ETA, phi, dmu / tau - kap) + grp_sum<MP>(b * qv) - grp_sum<MP>(nsum);
        const double dtau = num / den;
        double dy = fma(pv, dtau, qv);
#pragma unroll
        for (int q = 0; q < NCG; q++) {
            dx[q] = fma(ap[q], dtau, dx[q]);
            wv[q] = fma(c[q] - wv[q], dtau, aq[q]);   // A'dy = A'p dtau + A'q
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
            double dz[NCG];
            double th = fmax(fmax(-dtau / tau, -dkap / kap), 0.0);
#pragma unroll
            for (int q = 0; q < NCG; q++) {
                const double rx = fast_rcp(x[q]), rz = fast_rcp(z[q]);
                dz[q] = ok[q] ? (dmu - z[q] * dx[q]) * rx - z[q] : 0.0;
                if (ok[q]) th = fmax(th, fmax(-dz[q] * rz, -dx[q] * rx));
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
            tau = fma(theta, dtau, tau);
            kap = fma(theta, dkap, kap);
            it++;
        }
        if (fin && live) finalize(PYCLLP_STATUS_NUMERICAL);
    }
#undef HSD_ETA
#undef HSD_EINF
}
