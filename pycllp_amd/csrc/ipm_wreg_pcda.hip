// ipm_wreg_pcda.hip -- the predictor-corrector kernels of the wavefront-per-LP family on a dense image of A (kWPCDA)
#include "wreg_wave.h"
#include "ipm_wreg_solve.inc"

#define WV_PCDA(MB, NQ) { MB, NQ, wlaunch<ipm_wreg_kernel<MB, NQ, true, false, true>>, nullptr, nullptr, nullptr },
WREG_TABLE(kWPCDA, WREG_DA_SHAPES, WV_PCDA)
