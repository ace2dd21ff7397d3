// ipm_wreg_bd.hip -- the wavefront-per-LP kernel for LPs with upper bounds, on term tables and on a dense image of A (kWBD, kWBDDA)
#include "wreg_wave.h"
#include "ipm_wreg_bounded.inc"

#define WV_BD(MB, NQ) { MB, NQ, nullptr, nullptr, nullptr, wlaunch<ipm_wreg_bounded_kernel<MB, NQ, false>> },
#define WV_BDDA(MB, NQ) { MB, NQ, nullptr, nullptr, nullptr, wlaunch<ipm_wreg_bounded_kernel<MB, NQ, true>> },
WREG_TABLE(kWBD, WREG_TAB_SHAPES, WV_BD)
WREG_TABLE(kWBDDA, WREG_DA_SHAPES, WV_BDDA)
