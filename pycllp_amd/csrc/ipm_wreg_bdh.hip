// ipm_wreg_bdh.hip -- the wavefront-per-LP kernel for LPs with upper bounds on the homogeneous self-dual embedding, on term tables
// and on a dense image of A (kWBDH, kWBDHDA)
#include "wreg_wave.h"
#include "ipm_wreg_bdhsd.inc"

// a shape whose instantiation does not stay free of scratch has a null launcher (wreg_bdhsd_ships, wreg.h): the entry answers
// PYCLLP_E_UNSUPPORTED for it
template <int MB, int NQ, bool DA>
constexpr wbsolve_fn bdhsd_launcher() {
    if constexpr (wreg_bdhsd_ships(MB, NQ, DA)) return wlaunch<ipm_wreg_bounded_hsd_kernel<MB, NQ, DA>>; else return nullptr;
}
#define WV_BDH(MB, NQ) { MB, NQ, nullptr, nullptr, nullptr, bdhsd_launcher<MB, NQ, false>() },
#define WV_BDHDA(MB, NQ) { MB, NQ, nullptr, nullptr, nullptr, bdhsd_launcher<MB, NQ, true>() },
WREG_TABLE(kWBDH, WREG_TAB_SHAPES, WV_BDH)
WREG_TABLE(kWBDHDA, WREG_DA_SHAPES, WV_BDHDA)
