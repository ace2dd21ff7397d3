// ipm_wreg_pcpa.hip -- the predictor-corrector kernels of the wavefront-per-LP family for per-problem values of A (kWPCPA)
#include "wreg_wave.h"
#include "ipm_wreg_solve.inc"

#define WV_PCPA(MB, NQ) { MB, NQ, wlaunch<ipm_wreg_kernel<MB, NQ, false, true, true>>, nullptr, nullptr, nullptr },
WREG_TABLE(kWPCPA, WREG_TAB_SHAPES, WV_PCPA)
