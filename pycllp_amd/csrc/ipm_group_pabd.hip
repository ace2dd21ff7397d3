// ipm_group_pabd.hip -- translation unit of ipm_bounded_pa_kernel (ipm_group_slot.inc): the lane-group kernel for batches of LPs
// with upper bounds AND per-problem dense A.  A unit of its own (as ipm_group_pa.o is for the kernel without bounds), so that
// the code objects of every other kernel of the library are what they were before this kernel existed.  abi_dense.hip owns the
// handle and the C ABI (pycllp_hip_dense_solve_batch_bounded), ipm_dense.hip the launch plan (dense_tab.h); the kernels are
// reached through kGroupPABD (group_pa.h).
#include "group_pa.h"
#include "ipm_group.inc"
#include "ipm_group_slot.inc"

template <int MP, int NP>
static hipError_t launch_group_pabd(const GroupPaArgs& a, int grid, int block, int lds, DevOpts o, hipStream_t st) {
    using P = GeoPA<GeoG<MP, NP, true>>;
    auto kernel = ipm_bounded_pa_kernel<MP, NP>;
    if (block > P::wpb_capped(PYCLLP_WPB_BOUNDED) * WAVE || (size_t)lds < P::lds_bytes(block / WAVE))
        return hipErrorInvalidConfiguration;
    hipError_t e = set_dyn_lds((const void*)kernel, lds);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(kernel, dim3(grid), dim3(block), lds, st, a.m, a.n, a.B, a.A, a.b, a.c, a.u, a.x, a.y, a.z, a.s, a.pobj,
                       a.dobj, a.status, a.iters, a.queue, o);
    return hipGetLastError();
}

// one launcher per GROUP_SHAPES shape (group_pa.h)
#define GROUP_PABD_VARIANT(MP, NP) { MP, NP, 1, launch_group_pabd<MP, NP> },
// (the device pass gets a file-local copy of the table, as in ipm_group_pa.hip: referencing the launchers instantiates the kernels)
#ifdef __HIP_DEVICE_COMPILE__
namespace { [[maybe_unused]] const GroupPaVariant kGroupPABD_instantiate[] = { GROUP_SHAPES(GROUP_PABD_VARIANT) }; }
#else
namespace { const GroupPaVariant kGroupPABD_v[] = { GROUP_SHAPES(GROUP_PABD_VARIANT) }; }
extern const GroupPaVariants kGroupPABD = { kGroupPABD_v, (int)(sizeof(kGroupPABD_v) / sizeof(kGroupPABD_v[0])) };
#endif
