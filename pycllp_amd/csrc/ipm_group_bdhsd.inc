// ipm_group_bdhsd.inc -- ipm_bounded_hsd_kernel<MP, NP>: the lane-group kernel for LPs with UPPER BOUNDS on one shared
// A = [A_dense | I], on the homogeneous self-dual embedding (DESIGN.md section 26).
//   maximise c'x  subject to  A x = b,  0 <= x <= u        (u_j = +inf: no bound;  u_j = 0: the column is fixed at 0)
// The kernel is the text of ipm_group_hsd_body.inc under SL = true, BD = true: hsd_group_kernel's machinery (ipm_group_hsd.inc:
// GWaveH, one factorisation with two right-hand sides carried through the sweep, At_times2, backward2, the own-diagonal pivot
// floor) with the t, s, u phases that BD adds, as BD adds them in ipm_group_slot_body.inc.  What BD brings here is
// the reduced Newton system with bounds -- the exact Schur complement of hsd_one_raw (oracle/ipm_dense_ref.c) on the explicit
// expansion Ae = [[A_act, 0], [E_bnd, I]], be = (b; u_bnd), ce = (c_act; 0), duals (y; .), dual slacks (z; s):
//     rho = b tau - A x,   omega = u tau - x - t (bnd),   sigma = c tau - A'y + z - s,   phi = b'y + u's - c'x + kappa
//     mu = (x'z + s't + tau kappa) / (N_act + N_bnd + 1),   dmu = delta mu,   eta = 1 - delta
//     zx = z/x,  st = s/t,  d = 1/(zx + st),  w = d st,  h = t - dmu/s + eta omega,  r0 = eta sigma + dmu/x - z
//     dr = d r0 + w h,  dc = d c + w u
//     M = A d A',  M p = A dc - b,  M q = A dr - eta rho                      (ONE factorisation, two right-hand sides)
//     e = c - A'p,  uu = d e + w u,  v = dr - d A'q
//     dtau = (eta phi + b'q + dmu/tau - kappa - c'v + sum_bnd u w (r0 - A'q - zx h)) / (sum d e^2 + sum_bnd zx w u^2 + kappa/tau)
//     dy = p dtau + q,  dx = uu dtau + v,  dz = (dmu - z dx)/x - z,  dkappa = dmu/tau - kappa - (kappa/tau) dtau
//     t >= s:  dt = eta omega + u dtau - dx,  ds = (dmu - s dt)/t - s
//     t <  s:  ds = dz + eta sigma + c dtau - A'dy,  dt = dmu/s - t - (t/s) ds
// (bnd(q): 0 < u < inf; everything indexed by bnd is absent elsewhere).  The two branches for dt, ds are not a refinement: with
// the first pair alone an active upper bound (t ~ 1e-11) multiplies dt's rounding error, ~eps u, by s/t into ds and the dual
// residual grows before the stop test is met; with the second alone a basic column (s ~ 1e-13) does the same to dt through
// t/s.  Switched at t < s neither multiplier exceeds 1.
// Statuses 2 and 4 leave the certificate as it stands; 0 and 5 divide x, y, z, s and the objectives by tau.  A fixed column ends
// at x = 0 with z = max(-r, 0), s = max(r, 0), r = c tau - A'y, on the same scaling.
// Registers: seven N-vectors per slot (x, z, t, s, u, c, A'y) plus tau, kappa; the kernel runs PYCLLP_WPB_BOUNDED waves per
// workgroup, one per SIMD, with the whole register file per lane, as ipm_bounded_kernel.

template <int MP, int NP>
__global__ void __launch_bounds__(PYCLLP_WPB_BOUNDED * 64)
ipm_bounded_hsd_kernel(int m, int n, long B, const double* __restrict__ Ag, const double* __restrict__ bg,
                       const double* __restrict__ cg, const double* __restrict__ ug, double* __restrict__ xg,
                       double* __restrict__ yg, double* __restrict__ zg, double* __restrict__ sg, double* __restrict__ pobj,
                       double* __restrict__ dobj, int* __restrict__ status, int* __restrict__ iters, int* __restrict__ queue,
                       DevOpts o) {
    constexpr bool SL = true, BD = true, PA = false;
#include "ipm_group_hsd_body.inc"
}
