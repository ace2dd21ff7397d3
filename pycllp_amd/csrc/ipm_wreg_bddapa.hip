// ipm_wreg_bddapa.hip -- the wavefront-per-LP kernel for LPs with upper bounds on per-problem DENSE matrices: the bounded text on a dense image that belongs to the wave (kWBDDAPA)
#include "wreg_wave.h"
#define PYCLLP_WREG_BOUNDED_DAPA
#include "ipm_wreg_bounded.inc"

#define WV_BDDAPA(MB, NQ) { MB, NQ, nullptr, nullptr, nullptr, nullptr, wlaunch<ipm_wreg_bounded_dapa_kernel<MB, NQ>> },
WREG_TABLE(kWBDDAPA, WREG_BDDAPA_SHAPES, WV_BDDAPA)
