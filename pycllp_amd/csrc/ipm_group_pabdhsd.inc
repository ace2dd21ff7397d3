// ipm_group_pabdhsd.inc -- ipm_bounded_pa_hsd_kernel<MP, NP>: the lane-group kernel for batches of LPs with UPPER BOUNDS and
// PER-PROBLEM dense A_k = [A_k dense [m, n - m] | I], on the homogeneous self-dual embedding (DESIGN.md section 28).
//   maximise c_k'x  subject to  A_k x = b_k,  0 <= x <= u_k        (u_j = +inf: no bound;  u_j = 0: the column is fixed at 0)
// The kernel is the text of ipm_group_hsd_body.inc under SL = true, BD = true, PA = true: the system of ipm_bounded_hsd_kernel
// (ipm_group_bdhsd.inc has the formulas), statement for statement, on the per-slot areas of ipm_bounded_pa_kernel
// (ipm_group_slot.inc, GeoPA of group_pa.h).  What PA adds to the text:
//   - no workgroup-shared image and no workgroup barrier: per wave G areas of GeoG::SHARED doubles, zeroed once, their Gram
//     tables filled once; the wave's slabs and staging region lie behind them;
//   - a slot that takes an LP has the whole wave copy that LP's matrix, m x (n - m) contiguous doubles, into its image before
//     c, u, b are loaded.  The embedding starts at y = 0, A'y = 0, so the column sums that ipm_bounded_pa_kernel recomputes are
//     not formed; their place in the area stays, so that GeoPA and the launch plans (kPaBdPlans) hold as they are;
//   - w.Aimg is group g's area around gram_one(g, ..) and the lane's own area everywhere else.
// A parked slot has u = 0: none of its columns takes part, and its image -- zeros, or the last LP's matrix -- only ever meets
// x = 0 and d = 0.  Where that last matrix held a NaN, 0 * NaN makes the parked group's rho, p, q and step NaN all the same; what
// keeps that inside the group is the masks: its Gram product is skipped (the `live` test in do_gram), the factor's pivot test and the
// refinement's `need` are masked by `live`, every reduction runs per lane group, and a slot that is not live stores nothing.
// Launch bounds, waves per workgroup (4 / 4 / 4 / 4 / 3 / 2) and arguments are those of ipm_bounded_pa_kernel;
// statuses and output scaling those of ipm_bounded_hsd_kernel.

template <int MP, int NP>
__global__ void __launch_bounds__((GeoPA<GeoG<MP, NP, true>>::wpb_capped(PYCLLP_WPB_BOUNDED) * 64))
ipm_bounded_pa_hsd_kernel(int m, int n, long B, const double* __restrict__ Ag, const double* __restrict__ bg,
                          const double* __restrict__ cg, const double* __restrict__ ug, double* __restrict__ xg,
                          double* __restrict__ yg, double* __restrict__ zg, double* __restrict__ sg, double* __restrict__ pobj,
                          double* __restrict__ dobj, int* __restrict__ status, int* __restrict__ iters, int* __restrict__ queue,
                          DevOpts o) {
    constexpr bool SL = true, BD = true, PA = true;
#include "ipm_group_hsd_body.inc"
}
