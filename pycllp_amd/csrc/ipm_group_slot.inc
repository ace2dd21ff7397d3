// ipm_group_slot.inc -- the three lane-group kernels (ipm_group.inc) that iterate in the simplified order.  They share ONE text
// of the slot iteration, ipm_group_slot_body.inc, compiled under the constants SL, BD, PA:
//   ipm_bounded_kernel<MP, NP>        SL = true, BD = true,  PA = false    LPs with UPPER BOUNDS on one shared A
//   ipm_group_pa_kernel<MP, NP, SL>            BD = false, PA = true     EVERY LP HAS ITS OWN DENSE A
//   ipm_bounded_pa_kernel<MP, NP>     SL = true, BD = true,  PA = true     both (DESIGN.md section 17; ipm_group_pabd.hip)
// The text is included into each
// __global__, not called: behind a force-inlined function template the same text compiles to other instruction streams
// (ipm_bounded_kernel<32, 96> then spills four VGPRs); included, the bounded kernels are what they were as a file of their own.
//
// BD (DESIGN.md section 14):
//   maximise c'x  subject to  A x = b,  0 <= x <= u        (u_j = +inf: no bound;  u_j = 0: the column is fixed at 0)
// the bounded equality form of a GeneralLP (pycllp_amd/lp.py, GeneralLP.to_bounded_equality_form), A = [A_dense | I].
// Primal-normal step with x + t = u, t >= 0 and the dual Aty - z + s = c, s >= 0:
//   d = 1 / (z/x + s/t),  t~ = c - A'y + mu/x - mu/t + (s/t) tau,  tau = u - x - t,  mu = delta gamma / (n + m + N_b)
//   M dy = A (d t~) - rho,  dx = d (t~ - A'dy),  dz = (mu - z dx)/x - z,  dt = tau - dx,  ds = (mu - s dt)/t - s
// A column without a bound carries no t, s: every formula is then the one of ipm_group_kernel.  A fixed column (u = 0) takes
// no part in the iteration: it ends at x = 0 with the duals z = max(A'y - c, 0), s = max(c - A'y, 0).
// Without BD no column has a bound: act(q) is ok[q], bnd(q) is false, and t, s, u, the bound residual and the s output do not
// exist.  Strike the BD parts below and what is left is the plain step, d = x/z, t~ = c - A'y + mu/x.
// Registers with BD: seven N-vectors per slot (x, z, t, s, u, c, A'y) and four kept reciprocals instead of four and two; at
// (32, 96) that does not fit 256 registers, so ipm_bounded_kernel runs PYCLLP_WPB_BOUNDED = 4 waves per workgroup, one per
// SIMD, with the whole 512-register file per lane (DESIGN.md section 14 has the measured cost).
//
// PA (DESIGN.md section 16):
//   maximise c_k'x  subject to  A_k x = b_k,  x >= 0,   A_k [m, n] (SL = false) or A_k = [A_k dense [m, n - m] | I] (SL = true)
// Without PA the one shared A is copied into LDS once per workgroup, as in ipm_group_kernel.  With PA every SLOT (lane group)
// owns an area of the shape GeoG::SHARED -- row-major image with the odd stride AS, the column sums A'1, the MP = 32 Gram
// store table -- and nothing is shared between the waves of a workgroup, so the kernel has no workgroup barrier at all.  A slot
// that takes an LP from the queue (and at its first LP) has the whole wave copy that LP's matrix, m x a_cols contiguous
// doubles, from HBM into its image and recompute the column sums; the pad rows and columns are zeroed once and never
// written again (every LP of a batch has the same m and a_cols).  The GWave members address the matrix through w.Aimg, which
// is set to group g's area (wave-uniform) before gram_one(g, ..) and to the lane's own group's area (lane-varying; the
// members' addresses are per-lane values anyway) before everything else.
// (GeoPA -- the per-wave LDS with PA and the waves its launch bounds allow -- is in group_pa.h, which the launch plan shares.)
//
// Only the per-column phases are written here; the Gram product, the LDL' (both paths), the substitution, A'u, A v and the
// refinement are the GWave<MP, NP, SL> members, unchanged.  Simplifications against ipm_group_kernel: rho = b - A x comes from
// the Gram pass every iteration (no carried residual, no predicted stop test), so the stop test of a point runs after its Gram
// product and a slot that finishes idles through the rest of that pass; no warm start, no predictor-corrector, no HSD.
#include "group_pa.h"

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
    constexpr bool SL = true, BD = true, PA = false;
#include "ipm_group_slot_body.inc"
}

template <int MP, int NP, bool SL>
__global__ void __launch_bounds__((GeoPA<GeoG<MP, NP, SL>>::WPB_MAX * 64))
ipm_group_pa_kernel(int m, int n, long B, const double* __restrict__ Ag, const double* __restrict__ bg,
                    const double* __restrict__ cg, double* __restrict__ xg, double* __restrict__ yg,
                    double* __restrict__ zg, double* __restrict__ pobj, double* __restrict__ dobj,
                    int* __restrict__ status, int* __restrict__ iters, int* __restrict__ queue, DevOpts o) {
    constexpr bool BD = false, PA = true;
    const double* const ug = nullptr; double* const sg = nullptr;   // BD only
#include "ipm_group_slot_body.inc"
}

// BD && PA: the union of the two above.  The bounded text needs the whole register file per lane, so never more than one wave
// per SIMD (PYCLLP_WPB_BOUNDED), and fewer where the per-wave LDS (GeoPA::PW, as ipm_group_pa_kernel's) does not take four:
// 4 / 4 / 4 / 4 / 3 / 2 waves per workgroup at the six shapes.  A refill needs neither u nor the other vectors of the LP (it
// runs before they are loaded); a parked slot has u = 0, so none of its columns takes part and its image -- the last LP's
// matrix, or zeros -- only ever meets d = 0.
template <int MP, int NP>
__global__ void __launch_bounds__((GeoPA<GeoG<MP, NP, true>>::wpb_capped(PYCLLP_WPB_BOUNDED) * 64))
ipm_bounded_pa_kernel(int m, int n, long B, const double* __restrict__ Ag, const double* __restrict__ bg,
                      const double* __restrict__ cg, const double* __restrict__ ug, double* __restrict__ xg,
                      double* __restrict__ yg, double* __restrict__ zg, double* __restrict__ sg, double* __restrict__ pobj,
                      double* __restrict__ dobj, int* __restrict__ status, int* __restrict__ iters, int* __restrict__ queue,
                      DevOpts o) {
    constexpr bool SL = true, BD = true, PA = true;
#include "ipm_group_slot_body.inc"
}
