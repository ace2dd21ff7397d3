// ipm_wreg_pa.hip -- the wavefront-per-LP kernels for per-problem values of A: every (MB, NQ) of the table variants, plain and HSD (kWPA)
#include "wreg_wave.h"
#include "ipm_wreg_solve.inc"
#include "ipm_wreg_hsd.inc"

#define WV_PA(MB, NQ) { MB, NQ, wlaunch<ipm_wreg_kernel<MB, NQ, false, true>>, wlaunch<hsd_wreg_kernel<MB, NQ, false, true>>, nullptr, nullptr },
WREG_TABLE(kWPA, WREG_TAB_SHAPES, WV_PA)
