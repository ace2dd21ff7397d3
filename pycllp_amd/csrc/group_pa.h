// group_pa.h -- internal interface between abi_dense.hip (C ABI, handles; the launch plans are dense_tab.h's) and ipm_group_pa.hip /
// ipm_group_pabd.hip / ipm_group_pabdh.hip, the translation units of the lane-group kernels for per-problem dense A
// (ipm_group_slot.inc; on the self-dual embedding ipm_group_pabdhsd.inc), and the home of GROUP_SHAPES, the shape list of them all.
// Not part of the public ABI.
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

// the lane-group shapes (MP, NP), ordered by cost: the first that covers (m, n) is used, in every table of ipm_dense.hip,
// ipm_group_pa.hip, ipm_group_pabd.hip and ipm_group_pabdh.hip (the one list; tests/test_kernel_variants.py compares it with the Python side's)
#if defined(PYCLLP_DEV_ONLY_3296)   // development builds (tools/ab_*.sh): only the headline shape, compiles in a fraction of the time
#define GROUP_SHAPES(X) X(32, 96)
#elif defined(PYCLLP_DEV_ONLY_1648)
#define GROUP_SHAPES(X) X(16, 48)
#else
#define GROUP_SHAPES(X) X(16, 32) X(16, 48) X(16, 64) X(32, 64) X(32, 96) X(32, 128)
#endif

// One launch of ipm_group_pa_kernel<MP, NP, SL> (ipm_group_pa.hip) or, with upper bounds, of ipm_bounded_pa_kernel<MP, NP>
// (ipm_group_pabd.hip): A [B, m, a_cols] row-major, a_cols = n - m (SL) or n; u [B, n] and s: null without bounds; the outputs
// of pycllp_hip_dense_solve / pycllp_hip_dense_solve_bounded; queue: a zeroed work-queue head.  Sets the kernel's dynamic LDS
// itself.  `first` is dense_tab.h's (ipm_group_kernel on a shared A alone reads it).
struct GroupPaArgs {
    int m, n; long B;
    const double *A, *b, *c, *u;
    double *x, *y, *z, *s, *pobj, *dobj;
    int *status, *iters, *queue;
    const double* first = nullptr;   // shared A, plain and predictor-corrector kernels: the handle's first-pass image, or null
};
typedef hipError_t (*gpa_launch_fn)(const GroupPaArgs&, int grid, int block, int lds, DevOpts, hipStream_t);
struct GroupPaVariant { int mp, np, sl; gpa_launch_fn launch; };
struct GroupPaVariants { const GroupPaVariant* v; int n; };
// every GROUP_SHAPES shape with SL = 0 and SL = 1; matched by (mp, np, sl), never by position
extern const GroupPaVariants kGroupPA;
// ... and with upper bounds: every GROUP_SHAPES shape, slack-aware only (sl = 1: the bounded equality form ends in the identity)
extern const GroupPaVariants kGroupPABD;
// ... with upper bounds on the homogeneous self-dual embedding (ipm_bounded_pa_hsd_kernel, ipm_group_pabdh.hip): every
// GROUP_SHAPES shape, sl = 1; the launcher is null for a shape the kernel does not ship in (PABDHSD_SHAPES, dense_tab.h)
extern const GroupPaVariants kGroupPABDH;
#endif
