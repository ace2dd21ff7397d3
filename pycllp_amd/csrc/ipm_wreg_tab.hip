// ipm_wreg_tab.hip -- the wavefront-per-LP kernels on term tables: plain, HSD, stand-alone Newton step (kWTab)
#include "wreg_wave.h"
#include "ipm_wreg_solve.inc"
#include "ipm_wreg_hsd.inc"
#include "ipm_wreg_newton.inc"

#define WV_TAB(MB, NQ) WV_PLAIN(MB, NQ, false)
#ifdef PYCLLP_DEV_ONLY_W86   // development builds: only the (8, 6) table variant (BASELINE config 5), compiles in a fraction of the time
#define WREG_W86_SHAPES(X) X(8, 6)
WREG_TABLE(kWTab, WREG_W86_SHAPES, WV_TAB)
#else
WREG_TABLE(kWTab, WREG_TAB_SHAPES, WV_TAB)
#endif
