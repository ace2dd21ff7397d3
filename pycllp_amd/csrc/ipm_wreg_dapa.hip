// ipm_wreg_dapa.hip -- the wavefront-per-LP kernel for per-problem DENSE matrices: the plain solve kernel on a dense image that belongs to the wave (kWDAPA)
#include "wreg_wave.h"
#include "ipm_wreg_solve.inc"

#define WV_DAPA(MB, NQ) { MB, NQ, wlaunch<ipm_wreg_kernel<MB, NQ, true, true>>, nullptr, nullptr, nullptr, nullptr },
WREG_TABLE(kWDAPA, WREG_DAPA_SHAPES, WV_DAPA)
