// ipm_group_pa.hip -- translation unit of ipm_group_pa_kernel (ipm_group_slot.inc): the lane-group kernel for batches of LPs
// with per-problem dense A.  A unit of its own (as ipm_wreg_bd.o is for the bounded wave kernel), so that the code objects of
// every other kernel of the library are what they were before this kernel existed.  abi_dense.hip owns the handle and the C ABI
// (pycllp_hip_dense_solve_batch), ipm_dense.hip the launch plan (dense_tab.h); the kernels are reached through kGroupPA (group_pa.h).
#include "group_pa.h"
#include "ipm_group.inc"
#include "ipm_group_slot.inc"

template <int MP, int NP, bool SL>
static hipError_t launch_group_pa(const GroupPaArgs& a, int grid, int block, int lds, DevOpts o, hipStream_t st) {
    auto kernel = ipm_group_pa_kernel<MP, NP, SL>;
    if (block > GeoPA<GeoG<MP, NP, SL>>::WPB_MAX * WAVE || (size_t)lds < GeoPA<GeoG<MP, NP, SL>>::lds_bytes(block / WAVE))
        return hipErrorInvalidConfiguration;
    hipError_t e = set_dyn_lds((const void*)kernel, lds);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(kernel, dim3(grid), dim3(block), lds, st, a.m, a.n, a.B, a.A, a.b, a.c, a.x, a.y, a.z, a.pobj, a.dobj,
                       a.status, a.iters, a.queue, o);
    return hipGetLastError();
}

// one launcher per GROUP_SHAPES shape (group_pa.h) and SL
#define GROUP_PA_VARIANT(MP, NP) { MP, NP, 0, launch_group_pa<MP, NP, false> }, { MP, NP, 1, launch_group_pa<MP, NP, true> },
// The device pass gets a file-local copy of the table: it is never emitted, but referencing the launchers is what makes the
// kernels get instantiated (an external table of host function pointers would be emitted into the device object and fail to
// link there; as WREG_TABLE of wreg_wave.h).
#ifdef __HIP_DEVICE_COMPILE__
namespace { [[maybe_unused]] const GroupPaVariant kGroupPA_instantiate[] = { GROUP_SHAPES(GROUP_PA_VARIANT) }; }
#else
namespace { const GroupPaVariant kGroupPA_v[] = { GROUP_SHAPES(GROUP_PA_VARIANT) }; }
extern const GroupPaVariants kGroupPA = { kGroupPA_v, (int)(sizeof(kGroupPA_v) / sizeof(kGroupPA_v[0])) };
#endif
