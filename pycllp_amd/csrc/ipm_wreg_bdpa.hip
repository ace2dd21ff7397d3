// ipm_wreg_bdpa.hip -- the wavefront-per-LP kernel for LPs with upper bounds on per-problem values of A (structure tables; kWBDPA)
#include "wreg_wave.h"
#define PYCLLP_WREG_BOUNDED_PA
#include "ipm_wreg_bounded.inc"

#define WV_BDPA(MB, NQ) { MB, NQ, nullptr, nullptr, nullptr, nullptr, wlaunch<ipm_wreg_bounded_pa_kernel<MB, NQ>> },
WREG_TABLE(kWBDPA, WREG_TAB_SHAPES, WV_BDPA)
