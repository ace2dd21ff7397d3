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

// The kernel is the text of ipm_group_hsd_body.inc under BD = false; ipm_bounded_hsd_kernel (ipm_group_bdhsd.inc) is the same
// text with upper bounds, BD = true, and ipm_bounded_pa_hsd_kernel (ipm_group_pabdhsd.inc) with upper bounds and per-slot areas
// for per-problem matrices, PA = true (GeoPA: group_pa.h).

template <int MP, int NP, bool SL>
__global__ void __launch_bounds__(hsd_wpb<MP>() * 64)
hsd_group_kernel(int m, int n, long B, const double* __restrict__ Ag, const double* __restrict__ bg,
                 const double* __restrict__ cg, double* __restrict__ xg, double* __restrict__ yg,
                 double* __restrict__ zg, double* __restrict__ pobj, double* __restrict__ dobj,
                 int* __restrict__ status, int* __restrict__ iters, int* __restrict__ queue, DevOpts o) {
    constexpr bool BD = false, PA = false;
    const double* const ug = nullptr; double* const sg = nullptr;   // BD only
#include "ipm_group_hsd_body.inc"
}
