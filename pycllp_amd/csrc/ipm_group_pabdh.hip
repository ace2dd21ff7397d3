// ipm_group_pabdh.hip -- translation unit of ipm_bounded_pa_hsd_kernel (ipm_group_pabdhsd.inc): the lane-group kernel for batches
// of LPs with upper bounds and per-problem dense A, on the homogeneous self-dual embedding.  A unit of its own (as
// ipm_group_pabd.o and ipm_group_bdhsd.o are for their kernels), so that the code objects of every other kernel of the library
// are what they were before this kernel existed.  abi_dense.hip owns the handle and the C ABI
// (pycllp_hip_dense_solve_batch_bounded_hsd), ipm_dense.hip the launch plans (kPaBdPlans, dense_tab.h); the kernels are reached
// through kGroupPABDH (group_pa.h), whose launcher is null for a shape left out of PABDHSD_SHAPES (dense_tab.h).
#include "dense_tab.h"
#include "ipm_group.inc"
#include "ipm_group_hsd.inc"
#ifndef PYCLLP_WPB_BOUNDED
#define PYCLLP_WPB_BOUNDED 4
#endif
#include "ipm_group_pabdhsd.inc"

template <int MP, int NP>
static hipError_t launch_group_pabdh(const GroupPaArgs& a, int grid, int block, int lds, DevOpts o, hipStream_t st) {
    using P = GeoPA<GeoG<MP, NP, true>>;
    auto kernel = ipm_bounded_pa_hsd_kernel<MP, NP>;
    if (block > P::wpb_capped(PYCLLP_WPB_BOUNDED) * WAVE || (size_t)lds < P::lds_bytes(block / WAVE))
        return hipErrorInvalidConfiguration;
    hipError_t e = set_dyn_lds((const void*)kernel, lds);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(kernel, dim3(grid), dim3(block), lds, st, a.m, a.n, a.B, a.A, a.b, a.c, a.u, a.x, a.y, a.z, a.s, a.pobj,
                       a.dobj, a.status, a.iters, a.queue, o);
    return hipGetLastError();
}
template <int MP, int NP>
static constexpr gpa_launch_fn pabdh_launcher() {
    if constexpr (pabdhsd_ships(MP, NP)) return launch_group_pabdh<MP, NP>; else return nullptr;
}

// one row per GROUP_SHAPES shape (group_pa.h); the launcher of a shape left out of PABDHSD_SHAPES is null
#define GROUP_PABDH_VARIANT(MP, NP) { MP, NP, 1, pabdh_launcher<MP, NP>() },
// (the device pass gets a file-local copy of the table, as in ipm_group_pa.hip: referencing the launchers instantiates the kernels)
#ifdef __HIP_DEVICE_COMPILE__
namespace { [[maybe_unused]] const GroupPaVariant kGroupPABDH_instantiate[] = { GROUP_SHAPES(GROUP_PABDH_VARIANT) }; }
#else
namespace { const GroupPaVariant kGroupPABDH_v[] = { GROUP_SHAPES(GROUP_PABDH_VARIANT) }; }
extern const GroupPaVariants kGroupPABDH = { kGroupPABDH_v, (int)(sizeof(kGroupPABDH_v) / sizeof(kGroupPABDH_v[0])) };
#endif
