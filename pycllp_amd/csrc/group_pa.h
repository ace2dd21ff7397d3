// group_pa.h -- internal interface between ipm_dense.hip (C ABI, handles, launch plans) and ipm_group_pa.hip, the translation
// unit of the lane-group kernel for per-problem dense A (ipm_group_slot.inc).  Not part of the public ABI.
#ifndef PYCLLP_GROUP_PA_H
#define PYCLLP_GROUP_PA_H
#include "wave_common.h"

// Per-wave LDS and the waves of a workgroup: G areas + the wave's slabs and staging region (GeoG::WSZ); G_ is a GeoG<MP, NP, SL>.
// WPB_MAX, the launch bounds: as many waves as fit into the 160 KB of a CU, eight at most.  Up to four, every wave has a SIMD
// and the 512-entry register file per lane to itself (as PYCLLP_WPB_BOUNDED); five fit at (16, 32) general and (16, 48)
// slack-aware, whose kernels stay below 256 registers (measured: 2.27 -> 2.02 ms per 65 536 LPs against four waves).
template <class G_>
struct GeoPA {
    static constexpr int G = G_::G;                               // slots (lane groups) per wave
    static constexpr int AREA = G_::SHARED;                      // doubles per slot: image, column sums, Gram table
    static constexpr int PW = G_::G * AREA + G_::WSZ;             // doubles per wave
    static constexpr int FIT = (int)((160 * 1024) / (sizeof(double) * PW));
    static constexpr int WPB_MAX = FIT >= 8 ? 8 : FIT;
    static_assert(FIT >= 1, "one wave must fit into the LDS of a CU");
    static_assert(AREA % 2 == 0 && PW % 2 == 0, "areas and slabs stay 16-byte aligned");
    static constexpr size_t lds_bytes(int wpb) { return sizeof(double) * (size_t)wpb * PW; }
    // the waves of a kernel on these areas that must not exceed `cap` for another reason (ipm_bounded_pa_kernel: registers)
    static constexpr int wpb_capped(int cap) { return WPB_MAX < cap ? WPB_MAX : cap; }
};

// One launch of ipm_group_pa_kernel<MP, NP, SL>: A [B, m, a_cols] row-major, a_cols = n - m (SL) or n; the outputs of
// pycllp_hip_dense_solve; queue: a zeroed work-queue head.  Sets the kernel's dynamic LDS itself.
struct GroupPaArgs {
    int m, n; long B;
    const double *A, *b, *c;
    double *x, *y, *z, *pobj, *dobj;
    int *status, *iters, *queue;
};
typedef hipError_t (*gpa_launch_fn)(const GroupPaArgs&, int grid, int block, int lds, DevOpts, hipStream_t);
struct GroupPaVariant { int mp, np, sl; gpa_launch_fn launch; };
struct GroupPaVariants { const GroupPaVariant* v; int n; };
// every GROUP_SHAPES shape (ipm_dense.hip) with SL = 0 and SL = 1; matched by (mp, np, sl), never by position
extern const GroupPaVariants kGroupPA;

// One launch of ipm_bounded_pa_kernel<MP, NP> (ipm_group_pabd.hip): upper bounds on per-problem A.  A [B, m, n - m] row-major,
// u [B, n]; the outputs of pycllp_hip_dense_solve_bounded.  Sets the kernel's dynamic LDS itself.
struct GroupPaBdArgs {
    int m, n; long B;
    const double *A, *b, *c, *u;
    double *x, *y, *z, *s, *pobj, *dobj;
    int *status, *iters, *queue;
};
typedef hipError_t (*gpabd_launch_fn)(const GroupPaBdArgs&, int grid, int block, int lds, DevOpts, hipStream_t);
struct GroupPaBdVariant { int mp, np; gpabd_launch_fn launch; };
struct GroupPaBdVariants { const GroupPaBdVariant* v; int n; };
// every GROUP_SHAPES shape (slack-aware only: the bounded equality form ends in the identity); matched by (mp, np)
extern const GroupPaBdVariants kGroupPABD;
#endif
