// ipm_wreg_da.hip -- the wavefront-per-LP kernels on a dense image of A: plain, HSD, stand-alone Newton step (kWDA)
#include "wreg_wave.h"
#include "ipm_wreg_solve.inc"
#include "ipm_wreg_hsd.inc"
#include "ipm_wreg_newton.inc"

#define WV_DA(MB, NQ) WV_PLAIN(MB, NQ, true)
WREG_TABLE(kWDA, WREG_DA_SHAPES, WV_DA)
