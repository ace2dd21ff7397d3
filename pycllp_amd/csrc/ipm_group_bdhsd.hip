// ipm_group_bdhsd.hip -- translation unit of ipm_bounded_hsd_kernel (ipm_group_bdhsd.inc): the lane-group kernel for LPs with
// upper bounds on a shared A = [A_dense | I], on the homogeneous self-dual embedding.  A unit of its own (as ipm_group_pabd.o is
// for its kernel), so that the code objects of every other kernel of the library are what they were before this kernel existed.
// abi_dense.hip owns the handle and the C ABI (pycllp_hip_dense_solve_bounded_hsd), ipm_dense.hip the launch plan and the row of
// SlackVariant (dense_tab.h), which reaches the kernels through launch_solve_bounded_hsd<MP, NP>, instantiated here for the
// shapes of BDHSD_SHAPES.
#include "dense_tab.h"
#include "ipm_group.inc"
#include "ipm_group_hsd.inc"
#ifndef PYCLLP_WPB_BOUNDED
#define PYCLLP_WPB_BOUNDED 4
#endif
#include "ipm_group_bdhsd.inc"

template <int MP, int NP>
hipError_t launch_solve_bounded_hsd(const GroupPaArgs& a, const LaunchPlan& p, DevOpts o, hipStream_t st) {
    auto kernel = ipm_bounded_hsd_kernel<MP, NP>;
    if (p.block > PYCLLP_WPB_BOUNDED * WAVE || (size_t)p.lds < GeoG<MP, NP, true>::lds_bytes(p.block / WAVE))
        return hipErrorInvalidConfiguration;
    const hipError_t e = set_dyn_lds((const void*)kernel, p.lds);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(kernel, dim3(p.grid), dim3(p.block), p.lds, st, a.m, a.n, a.B, a.A, a.b, a.c, a.u, a.x, a.y, a.z, a.s,
                       a.pobj, a.dobj, a.status, a.iters, a.queue, o);
    return hipGetLastError();
}

#define BDHSD_INSTANTIATE(MP, NP) \
    template hipError_t launch_solve_bounded_hsd<MP, NP>(const GroupPaArgs&, const LaunchPlan&, DevOpts, hipStream_t);
BDHSD_SHAPES(BDHSD_INSTANTIATE)
