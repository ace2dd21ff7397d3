// ipm_wreg_pc.hip -- the predictor-corrector kernels of the wavefront-per-LP family on term tables (kWPC)
#include "wreg_wave.h"
#include "ipm_wreg_solve.inc"

#define WV_PC(MB, NQ) { MB, NQ, wlaunch<ipm_wreg_kernel<MB, NQ, false, false, true>>, nullptr, nullptr, nullptr },
WREG_TABLE(kWPC, WREG_TAB_SHAPES, WV_PC)
