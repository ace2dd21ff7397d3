// dense_tab.h -- internal interface between abi_dense.hip (C ABI, handle, queue ring) and ipm_dense.hip, the translation unit of
// the lane-group kernels on a shared dense A: its launcher tables, and the launch plans of every lane-group kernel (those of
// ipm_group_pa.hip and ipm_group_pabd.hip included: the plans need the kernels' geometry).  Not part of the public ABI.
#ifndef PYCLLP_DENSE_TAB_H
#define PYCLLP_DENSE_TAB_H
#include "group_pa.h"
#include "host.h"

// A plan depends on the kernel's compile-time geometry, so the rows hold it as a function
typedef LaunchPlan (*dense_plan_fn)(const DeviceLimits&, long B, const DevOpts&);
// One launch on its plan; sets the kernel's dynamic LDS itself.  GroupPaArgs (group_pa.h) with A = the handle's row-major copy
// [m, n]; the queue-ring slot behind a.queue and the plan's publication are the caller's.
typedef hipError_t (*dense_launch_fn)(const GroupPaArgs&, const LaunchPlan&, DevOpts, hipStream_t);
struct DenseKernel { dense_plan_fn plan; dense_launch_fn launch; };

struct NewtonArgs { int m, n; long B; const double *pack, *x, *z, *y, *b, *c; double mu; double* dy; int* nref; };
typedef hipError_t (*newton_launch_fn)(const NewtonArgs&, const LaunchPlan&, DevOpts, hipStream_t);
typedef hipError_t (*pack_launch_fn)(int m, int n, const double* A, double* pack, hipStream_t);

// The image of an LP's first Gram pass (first_gram_kernel, ipm_dense.hip): its length in doubles and the launch that fills it
// from the handle's row-major A [m, n]; read by the plain and predictor-corrector kernels of the same table row
typedef hipError_t (*first_launch_fn)(int m, int n, const double* A, double* img, hipStream_t);
struct FirstGram { int len; first_launch_fn launch; };   // len 0, launch null: the shape's kernels read no image

struct Variant {
    int mp, np, apack;
    pack_launch_fn pack;
    DenseKernel solve_group;  // group-per-LP kernel (default)
    DenseKernel solve_hsd;    // group-per-LP kernel on the homogeneous self-dual embedding (PYCLLP_FLAG_HSD)
    DenseKernel solve_pc;     // group-per-LP kernel with Mehrotra's predictor-corrector (PYCLLP_FLAG_PREDCORR)
    dense_plan_fn newton_plan;
    newton_launch_fn newton;
    FirstGram first;
};
// slack-aware group kernels: (MP, NP) with NP - MP padded dense columns + the m identity columns
// full_group: the full-shape instantiation of solve_group, launched on its plan, for a matrix with m == mp and n == np
// exactly; null where none was compiled (ipm_dense.hip full_group_kernel)
// solve_bounded_hsd: the bounded kernel on the homogeneous self-dual embedding (ipm_group_bdhsd.hip); its launcher is null for a
// shape that was left out of BDHSD_SHAPES
struct SlackVariant {
    int mp, np;
    DenseKernel solve_group, solve_hsd, solve_pc, solve_bounded;
    dense_launch_fn full_group;
    FirstGram first;          // (the full-shape instantiation reads it too: its Gram bits are the generic ones)
    DenseKernel solve_bounded_hsd;
};

// The shapes ipm_bounded_hsd_kernel ships in: those of GROUP_SHAPES whose instantiation has no scratch (tools/kernel_resources.py;
// DESIGN.md section 26).  ipm_group_bdhsd.hip instantiates the launcher for these; ipm_dense.hip puts it into the table.
#if defined(PYCLLP_DEV_ONLY_3296)
#define BDHSD_SHAPES(X) X(32, 96)
#elif defined(PYCLLP_DEV_ONLY_1648)
#define BDHSD_SHAPES(X) X(16, 48)
#else
#define BDHSD_SHAPES(X) X(16, 32) X(16, 48) X(16, 64) X(32, 64) X(32, 96) X(32, 128)
#endif
template <int MP, int NP>
hipError_t launch_solve_bounded_hsd(const GroupPaArgs&, const LaunchPlan&, DevOpts, hipStream_t);
constexpr bool bdhsd_ships(int mp, int np) {
#define BDHSD_IS(MP, NP) if (mp == MP && np == NP) return true;
    BDHSD_SHAPES(BDHSD_IS)
#undef BDHSD_IS
    return false;
}
template <int MP, int NP>
constexpr dense_launch_fn bounded_hsd_launcher() {
    if constexpr (bdhsd_ships(MP, NP)) return launch_solve_bounded_hsd<MP, NP>; else return nullptr;
}

// The shapes ipm_bounded_pa_hsd_kernel (ipm_group_pabdhsd.inc: the same embedding on per-problem matrices) ships in, by the same
// rule.  ipm_group_pabdh.hip instantiates the launchers for these and puts them into kGroupPABDH
// (group_pa.h); a shape left out has a null launcher there.
#if defined(PYCLLP_DEV_ONLY_3296)
#define PABDHSD_SHAPES(X) X(32, 96)
#elif defined(PYCLLP_DEV_ONLY_1648)
#define PABDHSD_SHAPES(X) X(16, 48)
#else
#define PABDHSD_SHAPES(X) X(16, 32) X(16, 48) X(16, 64) X(32, 64) X(32, 96) X(32, 128)
#endif
constexpr bool pabdhsd_ships(int mp, int np) {
#define PABDHSD_IS(MP, NP) if (mp == MP && np == NP) return true;
    PABDHSD_SHAPES(PABDHSD_IS)
#undef PABDHSD_IS
    return false;
}

// one row per lane-group shape of GROUP_SHAPES (group_pa.h), in its order: the first that covers (m, n) is used, in both tables
extern const Variant kVariants[];
extern const int kNumVariants;
extern const SlackVariant kSlackVariants[];
extern const int kNumSlackVariants;

// launch plans of the kernels for per-problem dense A; their launchers are kGroupPA's and kGroupPABD's (group_pa.h)
struct PaPlan { int mp, np, sl; dense_plan_fn plan; };
struct PaPlans { const PaPlan* v; int n; };
extern const PaPlans kPaPlans;
extern const PaPlans kPaBdPlans;   // ... and with upper bounds
#endif
