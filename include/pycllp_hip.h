/*
 * pycllp_hip.h -- C ABI of libpycllp_hip.so, the MI355X (gfx950) implementation of pycllp's batched
 * dense primal-normal-equations interior-point path.
 *
 * This is the drop-in boundary: plain pointers and sizes, no torch types.  Every pointer argument
 * named *_dev is a DEVICE pointer owned by the caller (the Python host passes torch tensors'
 * data_ptr()); `stream` is a hipStream_t passed as void* (NULL = default stream).  No entry point
 * synchronises the host with the device except where stated; all of them are re-entrant per handle: solves
 * may be issued from several host threads and on several streams with one handle (the caller keeps their output
 * buffers apart).  A handle keeps 64 device work-queue counters; when 64 launches of one handle are still in flight
 * the next call waits on the host for the oldest of them (the only place a solve entry may block).
 * *_launch_info and *_variant_info report the plan of the LAST launch on the handle.
 *
 * Alignment: a device array needs only the natural alignment of its element type -- 8 bytes for double, 4 for int.  No kernel
 * reads or writes a caller's array through a wider vector type, so an array may start anywhere such an element may (a
 * double array at an address = 8 mod 16, an int array at one = 4 mod 8), e.g. inside a packed allocation of the caller's.
 *
 * Footprint: an entry reads its input arrays and writes its output arrays, element [0] to the last element of the shapes given
 * below, and no other byte of the caller's memory -- no padded row or column of a kernel reaches memory.  An optional output
 * passed as NULL is not written and costs nothing; an input array is never written.  Outputs per status: every LP of a solve
 * entry gets ALL of x, y, z (s), pobj, dobj, status and iters written, whatever its status (OPTIMAL, PRIMAL_INFEASIBLE,
 * NUMERICAL, DUAL_INFEASIBLE, ITERATION_LIMIT): for a status other than OPTIMAL they hold the last iterate (with
 * PYCLLP_FLAG_HSD and status 2 / 4: the certificate) and its objectives.  A Newton entry writes dy and nrefine of every state.
 * ONE EXCEPTION: pycllp_hip_sparse_solve_batch on a structure whose per-problem values only the wavefront-per-LP kernel serves
 * (A's arrays beside the packed factor do not fit the block kernel's 160 KB of LDS, e.g. m = 128, n = 512 from 3 324
 * non-zeros on).  An LP whose LDL' would need the Nocedal-Wright guard there -- every LP with PYCLLP_FLAG_FORCE_GUARD_PATH --
 * has no guarded kernel to go to: it ends PYCLLP_STATUS_NUMERICAL and its status is ALL that is written; its x, y, z, pobj,
 * dobj and iters keep what the caller's arrays held.  Read them only where status != PYCLLP_STATUS_NUMERICAL on that entry.
 * The same holds for pycllp_hip_dense_solve_batch beyond the lane-group kernels (m > 32 or n > 128: the wavefront-per-LP
 * kernel with a dense image per wave), for the same reason.
 * A call that returns a negative PYCLLP_E_* code has written nothing.  tests/test_memory_footprint.py pins all of this.
 * Return value: 0 on success, a negative PYCLLP_E_* code for argument errors, or a positive
 * hipError_t for runtime failures (pycllp_hip_last_error() gives the text).
 *
 * Reference interfaces replaced (paths relative to the reference tree):
 *   pycllp_hip_dense_init   <- ClDensePrimalNormalSolver.init      pycllp/solvers/cl.py:28-83
 *                              (densify+upload A once, allocate per-solver device state)
 *   pycllp_hip_dense_solve  <- ClDensePrimalNormalSolver.solve     pycllp/solvers/cl.py:85-124
 *                              kernels initialize_xzyw              pycllp/cl/primal_normal.cl:14-28
 *                                      standard_primal_normal       pycllp/cl/primal_normal.cl:201-284
 *                                      (-> solve_primal_normal      pycllp/cl/ldl.cl:602-653,
 *                                          primal_normal_step       pycllp/cl/primal_normal.cl:122-156)
 *   pycllp_hip_dense_newton <- kernel solve_primal_normal launched stand-alone by the reference's
 *                              tests/test_ldl.py:219-273            pycllp/cl/ldl.cl:602-653
 *   pycllp_hip_dense_free   <- release of ClDensePrimalNormalSolver.buffers  pycllp/solvers/cl.py:26
 *   pycllp_hip_ldl          <- test kernels ldl / modified_ldl                pycllp/cl/ldl.cl:28-55, 57-107
 *                              (host: pycllp/ldl.py:58-128, launched by tests/test_ldl.py:139-193)
 *
 * Layouts are the problem-major ones of the LP container (pycllp/lp.py:338-347), NOT the
 * batch-interleaved transposes the OpenCL host builds (pycllp/solvers/cl.py:99,102):
 *   A [m, n] row-major (shared by the batch);  b [B, m];  c [B, n];  x, z [B, n];  y [B, m].
 * The LP is in equality form: maximise c'x subject to A x = b, x >= 0 (pycllp/lp.py:306-330).
 */
#ifndef PYCLLP_HIP_H
#define PYCLLP_HIP_H

#ifdef __cplusplus
extern "C" {
#endif

#define PYCLLP_HIP_ABI_VERSION 1

/* per-LP status codes, identical to the reference (pycllp/cl/primal_normal.cl:225,257,262,267;
 * pycllp/solvers/normal_eqns.py:85-87; names in pycllp/common/main.c:21-30) */
#define PYCLLP_STATUS_OPTIMAL 0
#define PYCLLP_STATUS_PRIMAL_INFEASIBLE 2
#define PYCLLP_STATUS_NUMERICAL 3
#define PYCLLP_STATUS_DUAL_INFEASIBLE 4
#define PYCLLP_STATUS_ITERATION_LIMIT 5
/* Non-finite data.  An LP with a non-finite entry (NaN, +Inf, -Inf) in its b, its c, its own values of A (the entries with
 * per-problem matrices) or its warm start (PYCLLP_FLAG_WARM_START: x, y, z) ends with PYCLLP_STATUS_NUMERICAL, and so does
 * an LP whose arithmetic stops being finite on the way (data many decades away from 1 without PYCLLP_FLAG_AUTOSCALE).  Every
 * output of such an LP is written (the one exception stated at the top aside): its x, y, z (and s) hold the last finite
 * iterate or non-finite values, its objectives are unspecified, its iteration count is that of the iteration that noticed.
 * No other LP of the batch is affected: each carries the bits it has in the same call without the bad LP.  u is read as
 * "> 0 or fixed", as everywhere: a NaN or a negative upper bound fixes its variable at 0 and is no error.
 * tests/test_nonfinite.py pins this for every kernel family. */

#define PYCLLP_E_BADARG (-1)      /* NULL pointer / non-positive size                     */
#define PYCLLP_E_UNSUPPORTED (-2) /* (m, n) outside what the compiled kernels cover        */
#define PYCLLP_E_NOMEM (-3)

/* flags */
#define PYCLLP_FLAG_WARM_START 1 /* x, z, y are in/out: start from the caller's point instead of
                                    x=z=y=1 (intent of pycllp/cl/primal_normal.cl:213-219)  */
#define PYCLLP_FLAG_AUTOSCALE 8 /* solve every LP with b/max|b| and c/max|c| and scale the results back: makes the
                                   unit-floored tolerances and the x=z=y=1 start scale invariant (not in the reference;
                                   not available with PYCLLP_FLAG_WAVE_KERNEL)                                       */
#define PYCLLP_FLAG_AUTOSCALE_PER_LP 256 /* PYCLLP_FLAG_AUTOSCALE decided per LP, inside the kernels: an LP is solved exactly as
                                   under PYCLLP_FLAG_AUTOSCALE (same divisions, same scale-back) if and only if it is OUT OF BAND
                                   -- max|b|, max|c| over all n columns or, on the entries with upper bounds, the largest finite
                                   positive u of the LP (an LP without one is left out of that test) is finite and lies outside
                                   [0.1, 10]; 0.1 and 10 themselves are in band, b = 0 is out of band -- and with the scale
                                   factors 1 otherwise.  Division and multiplication by 1.0 are exact: an in-band LP carries the
                                   bits of the call without either flag, an out-of-band LP those of the call with
                                   PYCLLP_FLAG_AUTOSCALE, whatever else is in the batch -- no caller-side band test, no
                                   device-to-host sync.  (An LP with a NaN in b, c or u may get either verdict; it ends with
                                   PYCLLP_STATUS_NUMERICAL under both.)  Every solve entry honours it where it honours
                                   PYCLLP_FLAG_AUTOSCALE and refuses it where it refuses that flag, with the same code; both
                                   flags together: PYCLLP_E_BADARG, before the handle is read.  The stand-alone Newton / LDL'
                                   entries ignore both.  pycllp_amd.solvers.hip.autoscale_mask restates the rule
                                   (DESIGN.md section 23).                                                                    */
#define PYCLLP_FLAG_HSD 32 /* solve on the homogeneous self-dual embedding (the model of the reference's CPU solver,
                              pycllp/ipo/hsd.c:27-312, re-derived on the normal equations): infeasible
                              and unbounded LPs end with a certificate after ~12-15 iterations -- status 2 with (y, z):
                              b'y < 0, A'y - z ~ 0; status 4 with x: c'x > 0, A x ~ 0 -- instead of through the
                              heuristic 10x-growth exits.  x, y, z of a status 2/4 LP are the certificate in homogeneous
                              scaling.  The LDL' pivot floor of column j on this path is pivot_floor^2 * |M_jj| (own original diagonal).
                              Dense and sparse solvers; not available with PYCLLP_FLAG_WAVE_KERNEL.                */
#define PYCLLP_FLAG_PREDCORR 128 /* Mehrotra's predictor-corrector on the reference's path (not in its OpenCL kernel; its CPU solver
                                    alternates predictor and centering iterations, pycllp/ipo/hsd.c:133-143, 222-260): per
                                    iteration ONE factorisation and two solves -- a predictor with mu = 0, the centering parameter
                                    (gamma_affine / gamma)^3 from how far it gets, the corrector with the second-order term.  Same
                                    optimum to the same tolerance in ~27 % fewer iterations at r = 0.9, ~45 % fewer at r = 0.99
                                    (45-50 % on config 5's structure).  An option: the default path stays the reference's rule.
                                    Not with PYCLLP_FLAG_HSD.  oracle/ipm_dense_ref.c ipm_one_pc is its restatement.
                                    The workgroup-per-LP block kernel has no such step: with PYCLLP_FLAG_BLOCK_KERNEL the option is
                                    refused (PYCLLP_E_UNSUPPORTED), and an LP that the wavefront-per-LP kernel DEFERS to it during a
                                    predictor-corrector solve -- the Nocedal-Wright guard would have bitten, or every LP with
                                    PYCLLP_FLAG_FORCE_GUARD_PATH -- is solved from its start again on the reference's plain rule:
                                    the same optimum and statuses, the plain rule's iterates and iteration count for that LP.
                                    The lane-group and large-LP kernels keep the step under their guard.
                                    tests/test_option_pairs.py pins this.                                                     */
#define PYCLLP_FLAG_NO_SLACK_PATH 16 /* do not use the slack-aware kernel even when the last m columns of A are the
                                        identity (diagnostic: results must agree to rounding)                    */
#define PYCLLP_FLAG_FORCE_GUARD_PATH 4 /* diagnostic: always run the guarded (cold) LDL' path of the group
                                          kernel; results must not change when the guard is inactive */
#define PYCLLP_FLAG_GENERIC_SHAPE 512 /* diagnostic: pycllp_hip_dense_solve keeps the generic instantiation of the slack-aware
                                         lane-group kernel where the LP fills a compiled shape exactly (m = MP, n = NP) and a
                                         full-shape instantiation would serve it; the results are the same bits.  The other
                                         entries have no such instantiation and ignore the flag. */
#define PYCLLP_FLAG_EXACT_NORMS 1024 /* diagnostic: the lane-group kernels of pycllp_hip_dense_solve (plain and predictor-corrector
                                        step) take their stop and growth tests on the square roots of the two residual norms in
                                        every pass, as they do of themselves only where the tests on the squared norms are not
                                        decided (csrc/ipm_group.inc, stop_verdict); status, iteration counts and vectors are the
                                        same bits.  The kernels that keep their square roots (PYCLLP_FLAG_HSD, upper bounds,
                                        per-problem matrices, the sparse path) ignore it; pycllp_hip_sparse_solve_bounded and
                                        pycllp_hip_sparse_solve_batch_bounded, which refuse PYCLLP_FLAG_FORCE_GUARD_PATH, refuse it
                                        likewise (PYCLLP_E_BADARG). */
#define PYCLLP_FLAG_PER_LP_FIRST_GRAM 2048 /* diagnostic: the lane-group kernels of pycllp_hip_dense_solve (plain and
                                              predictor-corrector step) form the Gram matrix and A x of every LP's first iteration
                                              on the matrix cores, as they do of themselves under PYCLLP_FLAG_WARM_START, instead of
                                              taking them from the image that pycllp_hip_dense_init made of A (every LP starts at
                                              x = z = 1; csrc/ipm_group.inc, GWave::gram_first; the 32-row shapes -- the others
                                              form the product anyway); status, iteration counts and vectors are the same bits.  Ignored and refused where PYCLLP_FLAG_EXACT_NORMS is. */
#define PYCLLP_FLAG_BLOCK_KERNEL 64 /* sparse solver: use the workgroup-per-LP kernel (ipm_block_kernel) even where the
                                       register-resident wavefront-per-LP kernel covers the problem (diagnostic / A-B runs;
                                       results agree to rounding)                                                  */
#define PYCLLP_FLAG_WAVE_KERNEL 2 /* the first-generation kernel (one LP per wavefront), since removed:
                                     pycllp_hip_dense_solve answers it with PYCLLP_E_UNSUPPORTED  */

#define PYCLLP_MAX_REFINE_AUTO (-1)
#define PYCLLP_MAX_REFINE_PLAIN 5
#define PYCLLP_MAX_REFINE_HSD 20

typedef struct pycllp_hip_opts {
    double eps;         /* relative stopping tolerance on |rho|,|sigma|,gamma; default 1e-10.
                           (reference: absolute EPS 1e-7f, primal_normal.cl:8,256)           */
    double delta;       /* centering parameter DELTA, default 0.02 (primal_normal.cl:10)     */
    double r;           /* step fraction R, default 0.9 (primal_normal.cl:11)                */
    double pivot_floor; /* LDL' diagonal floor, default 1e-6 (primal_normal.cl:275)          */
    double refine_tol;  /* refinement tolerance on max|b-Ax-A dx|, relative to 1+|b|, default
                           1e-11 (reference: 1e-8 absolute on rhs-M dy, ldl.cl:645)          */
    int max_iter;       /* default 200 (primal_normal.cl:9)                                  */
    int max_refine;     /* refinement passes per Newton system.  Default PYCLLP_MAX_REFINE_AUTO (-1): resolved inside
                           every entry point to 5 (ldl.cl:645) on the reference's path and to 20 with PYCLLP_FLAG_HSD
                           (DESIGN.md section 9); any value >= 0 is taken as given               */
    int flags;          /* PYCLLP_FLAG_*                                                     */
    int reserve_cus;    /* compute units the solve leaves idle (default 0).  The solve kernels are persistent and fill every CU
                           completely (LDS and registers), so a kernel on another stream -- e.g. the RCCL copy kernels of the
                           result gather that overlaps the next solve -- finds no free CU until a solve ends; reserving a few
                           (8 = one per XCD) lets it run beside the solve                                    */
} pycllp_hip_opts;

typedef struct pycllp_hip_dense pycllp_hip_dense; /* opaque per-solver device state */

int pycllp_hip_abi_version(void);
const char *pycllp_hip_last_error(void);
void pycllp_hip_default_opts(pycllp_hip_opts *opts);

/* Largest (m, n) the compiled kernels accept (n counts ALL columns of the equality form). */
int pycllp_hip_dense_max_rows(void);
int pycllp_hip_dense_max_cols(void);

/* Upload/pack the shared constraint matrix.  A_dev: [m, n] row-major f64 on the device.
 * Synchronises `stream` before returning (A_dev may be freed by the caller afterwards). */
int pycllp_hip_dense_init(int m, int n, const double *A_dev, void *stream, pycllp_hip_dense **handle);

/* Solve B LPs.  Inputs b_dev [B,m], c_dev [B,n].  Outputs (any of y/z/pobj/dobj/iters may be NULL):
 *   x_dev [B,n], y_dev [B,m], z_dev [B,n]  primal, dual and dual-slack solutions
 *   pobj_dev, dobj_dev [B]                 c'x and b'y at exit (objective offset f NOT added).  An LP that ends at the
 *                                          iteration limit (status 5) returns the x, y, z of its last step and the objectives
 *                                          of the point that step started from (with PYCLLP_FLAG_HSD: divided by the final
 *                                          tau), as the reference's loop leaves them (pycllp/cl/primal_normal.cl:245-248)
 *   status_dev [B] i32, iters_dev [B] i32  status code and IPM iterations used
 * Asynchronous on `stream`. */
int pycllp_hip_dense_solve(pycllp_hip_dense *handle, long B, const double *b_dev, const double *c_dev,
                           double *x_dev, double *y_dev, double *z_dev, double *pobj_dev,
                           double *dobj_dev, int *status_dev, int *iters_dev,
                           const pycllp_hip_opts *opts, void *stream);

/* Solve B LPs with UPPER BOUNDS, maximise c'x s.t. A x = b, 0 <= x <= u (the bounded equality form of a GeneralLP,
 * pycllp_amd/lp.py GeneralLP.to_bounded_equality_form), on the bounded slack-aware lane-group kernel.  The handle's A must be
 * [A_dense | I_m] with m <= 32 and at most 96 dense columns (the slack-aware kernels of pycllp_hip_dense_solve).
 *   u_dev [B,n]      upper bounds: +inf = no bound, 0 = the column is fixed at 0 (it ends at x = 0)
 *   s_dev [B,n]      (optional) duals of x <= u; z_dev (optional) those of x >= 0: A'y - z + s = c
 *   dobj_dev [B]     b'y + u's over the finite u; the other arguments as pycllp_hip_dense_solve, except that at the iteration
 *                    limit pobj and dobj are those of the x, y, s returned (likewise pycllp_hip_sparse_solve_bounded)
 * Options: PYCLLP_FLAG_AUTOSCALE (u scales with b) and PYCLLP_FLAG_FORCE_GUARD_PATH apply.
 * Returns PYCLLP_E_BADARG for a NULL u_dev or any of the flags HSD, PREDCORR, WARM_START, WAVE_KERNEL, NO_SLACK_PATH, and
 * PYCLLP_E_UNSUPPORTED when the handle has no slack-aware lane-group kernel; both before any HIP call.
 * Asynchronous on `stream`. */
int pycllp_hip_dense_solve_bounded(pycllp_hip_dense *handle, long B, const double *b_dev, const double *c_dev,
                                   const double *u_dev, double *x_dev, double *y_dev, double *z_dev, double *s_dev,
                                   double *pobj_dev, double *dobj_dev, int *status_dev, int *iters_dev,
                                   const pycllp_hip_opts *opts, void *stream);

/* The same LPs -- maximise c'x s.t. A x = b, 0 <= x <= u on a handle whose A is [A_dense | I_m] -- on the HOMOGENEOUS SELF-DUAL
 * EMBEDDING with bounds (csrc/ipm_group_bdhsd.inc): an infeasible or unbounded LP ends with a certificate
 * instead of the 10x-growth heuristic of pycllp_hip_dense_solve_bounded.  Arguments as pycllp_hip_dense_solve_bounded; outputs:
 *   status 0 (and 5)  x, y, z, s, pobj, dobj are divided by the final tau: the solution of the LP (at the iteration limit the
 *                     objectives are those of the point returned, as for every bounded entry)
 *   status 2          the certificate as it stands: y, z, s with -b'y - u's > 0 and |A'y - z + s| <= 1e-8 (-b'y - u's)
 *   status 4          the certificate as it stands: a ray x with c'x > 0 and max(|A x|, |x_j| over finite u_j) <= 1e-8 c'x
 *                     (eps = 1e-10: the rule is 100 eps; under autoscale both hold for the LP as the kernel scaled it, b, u / max|b|
 *                     and c / max|c|: in the caller's units the first ratio is divided by max|b|, the second by max|c|)
 *   a fixed column (u = 0) ends at x = 0 with z = max(-r, 0), s = max(r, 0), r = c tau - A'y, on the same scaling
 * Options: PYCLLP_FLAG_HSD is accepted and implied; PYCLLP_FLAG_AUTOSCALE and _AUTOSCALE_PER_LP apply exactly as for
 * pycllp_hip_dense_solve_bounded (b, u, c are divided on load, the results scaled back); PYCLLP_FLAG_FORCE_GUARD_PATH applies;
 * max_refine = PYCLLP_MAX_REFINE_AUTO resolves to 20.
 * Returns PYCLLP_E_BADARG for a NULL handle or u_dev, both autoscale flags together, or any of the flags PREDCORR, WARM_START,
 * WAVE_KERNEL, NO_SLACK_PATH -- before the handle is read --, and PYCLLP_E_UNSUPPORTED when the handle has no slack-aware
 * lane-group shape or that shape's kernel was not compiled.  Asynchronous on `stream`. */
int pycllp_hip_dense_solve_bounded_hsd(pycllp_hip_dense *handle, long B, const double *b_dev, const double *c_dev,
                                       const double *u_dev, double *x_dev, double *y_dev, double *z_dev, double *s_dev,
                                       double *pobj_dev, double *dobj_dev, int *status_dev, int *iters_dev,
                                       const pycllp_hip_opts *opts, void *stream);

/* Solve B LPs that each have their OWN dense matrix, on the lane-group kernel for per-problem A (every lane group keeps the
 * image of its LP's matrix in LDS and refills it from A_dev when it takes its next LP).  The handle comes from
 * pycllp_hip_dense_init with any one matrix of the batch: that matrix fixes m, n and whether the last m columns are the
 * identity (as the handle of pycllp_hip_sparse_solve_batch fixes the structure); its values are not read here.
 *   A_dev [B, m, a_cols]  row-major.  a_cols = n - m on a handle whose tail is the identity (the tail is implied and not
 *                         stored), a_cols = n otherwise -- and with PYCLLP_FLAG_NO_SLACK_PATH on such a handle, where the
 *                         caller passes the full [m, n] matrices, identity included
 * The other arguments, the status codes and the outputs as pycllp_hip_dense_solve, except that at the iteration limit pobj
 * and dobj are those of the x, y returned (as pycllp_hip_dense_solve_bounded).
 * Options: PYCLLP_FLAG_AUTOSCALE, PYCLLP_FLAG_FORCE_GUARD_PATH and PYCLLP_FLAG_NO_SLACK_PATH apply.
 * Beyond the lane-group kernels (m > 32 or n > 128), up to m = 128 and n = 256: the wavefront-per-LP kernel with a dense
 * image PER WAVE (one LP per wavefront; the wave copies its LP's m x a_cols matrix from A_dev into its own LDS area when it
 * takes the LP).  The image counts against the LDS, so the range ends where not even one wave fits 160 KB: e.g. (128, 256)
 * with an identity tail runs (1 wave per workgroup), (64, 128) without one runs, (80, 256) without one and (113, 257) do
 * not.  At the iteration limit pobj and dobj are, as with pycllp_hip_dense_solve, those of the iterate before the last step.
 * PYCLLP_FLAG_AUTOSCALE and _AUTOSCALE_PER_LP apply; an LP whose factorisation would have needed the Nocedal-Wright
 * guard -- every LP under PYCLLP_FLAG_FORCE_GUARD_PATH -- ends PYCLLP_STATUS_NUMERICAL with status its only output.
 * pycllp_hip_dense_launch_info / _variant_info / _kernel_kind report the launch as a wave kernel on a dense image: (MB, NQ),
 * block = 64 x waves per workgroup, the plan's LDS bytes.
 * Returns PYCLLP_E_BADARG for any of the flags HSD, PREDCORR, WARM_START, WAVE_KERNEL or an a_cols other than the above, and
 * PYCLLP_E_UNSUPPORTED for a handle beyond both ranges (m > 128, n > 256, or a shape whose image leaves no room for a wave:
 * use pycllp_hip_sparse_solve_batch); all before any HIP call.  Uses the handle's launch-queue ring;
 * pycllp_hip_dense_launch_info / _variant_info report the launch as they do for the other lane-group kernels.  Asynchronous
 * on `stream`. */
int pycllp_hip_dense_solve_batch(pycllp_hip_dense *handle, long B, const double *A_dev, long a_cols,
                                 const double *b_dev, const double *c_dev, double *x_dev, double *y_dev, double *z_dev,
                                 double *pobj_dev, double *dobj_dev, int *status_dev, int *iters_dev,
                                 const pycllp_hip_opts *opts, void *stream);

/* Solve B LPs with UPPER BOUNDS that each have their OWN dense matrix: maximise c'x s.t. [A_k | I] x = b, 0 <= x <= u, the
 * bounded equality form of a GeneralLP whose A has per-problem values, on the lane-group kernel that has both (the text of
 * pycllp_hip_dense_solve_bounded's kernel on the per-slot matrix images of pycllp_hip_dense_solve_batch's).  The handle comes
 * from pycllp_hip_dense_init with any one [A_k | I_m] of the batch: it fixes m, n and the identity tail (m <= 32, at most 96
 * dense columns); its values are not read here.
 *   A_dev [B, m, a_cols]  row-major, a_cols = n - m: the columns before the identity tail, which is implied and never stored
 *   u_dev [B,n], s_dev [B,n], dobj_dev [B] = b'y + u's and the objectives at the iteration limit: as
 *                         pycllp_hip_dense_solve_bounded; the other arguments as pycllp_hip_dense_solve
 * Options: PYCLLP_FLAG_AUTOSCALE (u scales with b) and PYCLLP_FLAG_FORCE_GUARD_PATH apply.
 * Beyond the lane-group kernels (m > 32 or n > 128) a handle with m <= 128 and n <= 256 whose tail is the identity is served by
 * the bounded wavefront-per-LP kernel with a dense image per wave (ipm_wreg_bddapa.hip: the image of the wave's LP, then its t
 * and s, behind every wave area; fewer waves per workgroup the larger the image -- DESIGN.md section 25), on a plan built by
 * the first call: same arguments; an LP whose factorisation the guard would have changed ends PYCLLP_STATUS_NUMERICAL, and
 * PYCLLP_FLAG_FORCE_GUARD_PATH has no effect there.
 * Returns PYCLLP_E_BADARG for a NULL u_dev, any of the flags HSD, PREDCORR, WARM_START, WAVE_KERNEL, NO_SLACK_PATH or an a_cols
 * other than n - m, and PYCLLP_E_UNSUPPORTED when the handle has no slack-aware lane-group kernel (m <= 32 with 96 < n - m and
 * n <= 128 included) or, beyond them, no shape or LDS plan of the wave kernel (m > 128, n > 256); all before any HIP call.
 * Uses the handle's launch-queue ring; pycllp_hip_dense_launch_info / _variant_info report the launch (slack = 1; on the wave
 * kernel: pycllp_hip_dense_kernel_kind 2, (MB, NQ), block = 64 x waves, the plan's LDS bytes).
 * Asynchronous on `stream`. */
int pycllp_hip_dense_solve_batch_bounded(pycllp_hip_dense *handle, long B, const double *A_dev, long a_cols,
                                         const double *b_dev, const double *c_dev, const double *u_dev,
                                         double *x_dev, double *y_dev, double *z_dev, double *s_dev, double *pobj_dev,
                                         double *dobj_dev, int *status_dev, int *iters_dev,
                                         const pycllp_hip_opts *opts, void *stream);

/* The same LPs -- upper bounds, every LP its OWN dense matrix [A_k | I] -- on the HOMOGENEOUS SELF-DUAL EMBEDDING with bounds
 * (csrc/ipm_group_pabdhsd.inc, DESIGN.md section 28: the system of pycllp_hip_dense_solve_bounded_hsd on the per-slot matrix
 * images of pycllp_hip_dense_solve_batch_bounded): an infeasible or unbounded LP ends with a certificate instead of the
 * 10x-growth heuristic.  Arguments as pycllp_hip_dense_solve_batch_bounded (A_dev [B, m, a_cols], a_cols = n - m); outputs,
 * statuses and certificates as pycllp_hip_dense_solve_bounded_hsd: statuses 0 and 5 divided by the final tau, statuses 2 and 4
 * the certificate as it stands (with A_k in place of A), a fixed column at x = 0.
 * Options: PYCLLP_FLAG_HSD is accepted and implied; PYCLLP_FLAG_AUTOSCALE and _AUTOSCALE_PER_LP apply as for
 * pycllp_hip_dense_solve_bounded_hsd; PYCLLP_FLAG_FORCE_GUARD_PATH applies; max_refine = PYCLLP_MAX_REFINE_AUTO resolves to 20.
 * Returns PYCLLP_E_BADARG for a NULL handle or u_dev, B < 0, both autoscale flags together, or any of the flags PREDCORR,
 * WARM_START, WAVE_KERNEL, NO_SLACK_PATH -- before the handle is read --, and for an a_cols other than n - m;
 * PYCLLP_E_UNSUPPORTED for a handle beyond the lane-group kernels (m > 32 or n > 128: the wave kernel with an image per wave
 * has no embedding), for one without a slack-aware lane-group shape, and for a shape whose kernel was not compiled; all before
 * any HIP call, with nothing touched.  Uses the handle's launch-queue ring; pycllp_hip_dense_launch_info / _variant_info report
 * the launch (slack = 1).  Asynchronous on `stream`. */
int pycllp_hip_dense_solve_batch_bounded_hsd(pycllp_hip_dense *handle, long B, const double *A_dev, long a_cols,
                                             const double *b_dev, const double *c_dev, const double *u_dev,
                                             double *x_dev, double *y_dev, double *z_dev, double *s_dev, double *pobj_dev,
                                             double *dobj_dev, int *status_dev, int *iters_dev,
                                             const pycllp_hip_opts *opts, void *stream);

/* One Newton step of the primal normal equations for B independent states:
 *   dy <- solve( A diag(x/z) A' , -(b - A x - A diag(x/z) (c - A'y + mu/x)) )
 * x,z,c [B,n]; y,b,dy [B,m].  nrefine_dev [B] (optional) receives the refinement passes used. */
int pycllp_hip_dense_newton(pycllp_hip_dense *handle, long B, const double *x_dev, const double *z_dev,
                            const double *y_dev, const double *b_dev, const double *c_dev, double mu,
                            double *dy_dev, int *nrefine_dev, const pycllp_hip_opts *opts, void *stream);

/* Kernel-level statistics of the last launch (solve, bounded solve or Newton step) on this handle (host values).
 * m_pad, n_pad: the (MP, NP) of the lane-group kernel that ran -- of the slack-aware table when that one ran -- and, before
 * the first launch, the shape of the general table's kernel that covers (m, n).  A handle handed to the sparse path's
 * kernels reports 128, 512 there (pycllp_hip_dense_variant_info gives the shape that served). */
int pycllp_hip_dense_launch_info(const pycllp_hip_dense *handle, int *grid, int *block, int *lds_bytes,
                                 int *m_pad, int *n_pad);

/* Which kernel family serves this handle: -1 = the lane-group kernels (m <= 32, n <= 128); otherwise the LP was handed to
 * the sparse path's kernels at init and the value is that of pycllp_hip_sparse_launch_info's `kernel` for the last launch
 * (0 = workgroup-per-LP block kernel, 1 = wavefront-per-LP kernel on term tables, 2 = the same on a dense image of A,
 * 3 = the large-LP kernel with its Gram from a term list, 4 = the same on the matrix cores). */
int pycllp_hip_dense_kernel_kind(const pycllp_hip_dense *handle);

/* The compiled instantiation that served the last launch on this handle.  Lane-group kernels: *a, *b = its (MP, NP) and
 * *slack = 1 when it is one of the slack-aware kernels (every bounded solve), 0 when it is one of the general ones (every
 * Newton step); (0, 0, 0) before the first launch.  A handle handed to the sparse path's kernels: *a, *b = the (MB, NQ) of
 * pycllp_hip_sparse_variant_info and *slack = -1. */
int pycllp_hip_dense_variant_info(const pycllp_hip_dense *handle, int *a, int *b, int *slack);

/* 1 when the last launch on this handle ran a full-shape instantiation of a lane-group kernel -- pycllp_hip_dense_solve on
 * the slack-aware path, without PYCLLP_FLAG_HSD or PYCLLP_FLAG_PREDCORR, for an LP whose m and n (equality form) are exactly the
 * (MP, NP) of a compiled shape, e.g. 32 x 64 -> (32, 96), without PYCLLP_FLAG_GENERIC_SHAPE -- else 0. */
int pycllp_hip_dense_full_shape(const pycllp_hip_dense *handle);

/* pycllp_hip_sparse_plan_info of a handle handed to the sparse path's kernels; (0, 0, -1, -1) on the lane-group kernels. */
int pycllp_hip_dense_plan_info(const pycllp_hip_dense *handle, int *wgpc, int *bnc, int *factor_in_lds, int *a_in_lds);

void pycllp_hip_dense_free(pycllp_hip_dense *handle);

/* Stand-alone batched LDL' (modified != 0: Nocedal-Wright modified LDL' with the given beta and delta) of B
 * explicit symmetric matrices A_dev [B, n, n] (row-major, only the lower triangle is read), n <= 128.
 * L_dev [B, n(n+1)/2]: packed lower triangle with unit diagonal, entry (i, j) at i(i+1)/2 + j; D_dev [B, n].
 * Replaces the reference's test kernels `ldl` / `modified_ldl` (pycllp/cl/ldl.cl:28-55, 57-107). */
int pycllp_hip_ldl(int n, long B, const double *A_dev, double *L_dev, double *D_dev, int modified, double beta,
                   double delta, void *stream);

/* Stand-alone LDL' solves of B explicit symmetric systems (numpy prototypes pycllp/ldl.py:147-281).
 * pycllp_hip_ldl_solve: x = A^-1 rhs through A = L D L' -- `solve_ldl` (ldl.py:202-239) when modified == 0 (one matrix
 *   per wavefront, factor held in registers), `forward_backward_modified_ldl` (ldl.py:242-281: Nocedal-Wright guard with
 *   the given beta and delta) when modified != 0.  A_dev [B, n, n] (lower triangle read), rhs_dev, x_dev [B, n]; n <= 128.
 * pycllp_hip_forward_backward_ldl: x = (L D L')^-1 b for given factors -- `forward_backward_ldl` (ldl.py:165-180).
 *   L_dev [B, n(n+1)/2] packed lower triangle as written by pycllp_hip_ldl (unit diagonal), D_dev, b_dev, x_dev [B, n]. */
int pycllp_hip_ldl_solve(int n, long B, const double *A_dev, const double *rhs_dev, double *x_dev, int modified,
                         double beta, double delta, void *stream);
int pycllp_hip_forward_backward_ldl(int n, long B, const double *L_dev, const double *D_dev, const double *b_dev,
                                    double *x_dev, void *stream);

/* ---- sparse shared-A path (BASELINE config 5): one LP per workgroup, A in CSR, dense packed factor in LDS ----
 * Replaces ClSparsePrimalNormalSolver (pycllp/solvers/cl.py:127-278) and the sparse_* kernels
 * (pycllp/cl/primal_normal.cl:287-375, pycllp/cl/ldl.cl:140-196,221-257,381-502,540-574,656-712).
 * init takes the CSR arrays the reference uploads (cl.py:175-178: Adata f64[nnz], Aindptr i32[m+1], Aindices i32[nnz],
 * device pointers); A' and the structure of A diag(x/z) A' are derived inside (cl.py:180-196 does this on the host).
 * Limits: m <= 128, n <= 512 (equality form).  solve has the semantics and layouts of pycllp_hip_dense_solve. */
typedef struct pycllp_hip_sparse pycllp_hip_sparse;
int pycllp_hip_sparse_max_rows(void);
int pycllp_hip_sparse_max_cols(void);
int pycllp_hip_sparse_init(int m, int n, int nnz, const double *Adata_dev, const int *Aindptr_dev,
                           const int *Aindices_dev, void *stream, pycllp_hip_sparse **handle);
int pycllp_hip_sparse_solve(pycllp_hip_sparse *handle, long B, const double *b_dev, const double *c_dev,
                            double *x_dev, double *y_dev, double *z_dev, double *pobj_dev, double *dobj_dev,
                            int *status_dev, int *iters_dev, const pycllp_hip_opts *opts, void *stream);
/* The same solve with PER-PROBLEM VALUES of A on the shared structure -- SparseMatrix.data[nproblems, nnz] of the
 * reference's container (pycllp/lp.py:16-54, 274-281), which its LP classes still refuse (lp.py:335-336).
 * Adata_dev [B, nnz]: the values of LP k in the CSR order of the arrays given to pycllp_hip_sparse_init (whose values
 * only fixed the structure).  One LP per workgroup; its values travel HBM -> LDS once per LP (8 nnz bytes, next to the
 * 16 (m + n) + 24 of b, c, x, y). */
int pycllp_hip_sparse_solve_batch(pycllp_hip_sparse *handle, long B, const double *Adata_dev, const double *b_dev,
                                  const double *c_dev, double *x_dev, double *y_dev, double *z_dev, double *pobj_dev,
                                  double *dobj_dev, int *status_dev, int *iters_dev, const pycllp_hip_opts *opts,
                                  void *stream);
/* Solve B LPs with UPPER BOUNDS, maximise c'x s.t. A x = b, 0 <= x <= u (the bounded equality form of a GeneralLP), on the
 * register-resident one-LP-per-wavefront kernel (csrc/ipm_wreg_bounded.inc).  Any shared A of the handle with m <= 128 rows
 * and n <= 512 columns that a variant of that kernel covers; no identity tail is required.  The arguments mean what they
 * mean for pycllp_hip_dense_solve_bounded:
 *   u_dev [B,n]      upper bounds: +inf = no bound, 0 = the column is fixed at 0 (it ends at x = 0)
 *   s_dev [B,n]      (optional) duals of x <= u; z_dev (optional) those of x >= 0: A'y - z + s = c
 *   dobj_dev [B]     b'y + u's over the finite u
 * Option: PYCLLP_FLAG_AUTOSCALE (u scales with b).  An LP whose LDL' would need the Nocedal-Wright guard ends
 * PYCLLP_STATUS_NUMERICAL.  The kernel's plan is built on the first call and kept with the handle.
 * Returns PYCLLP_E_BADARG for a NULL handle, a NULL u_dev or any of the flags HSD, PREDCORR, WARM_START, WAVE_KERNEL,
 * BLOCK_KERNEL, NO_SLACK_PATH, FORCE_GUARD_PATH (before the handle is read and before any HIP call), and
 * PYCLLP_E_UNSUPPORTED when no variant of the bounded kernel or LDS plan covers A (m > 128 or n > 512 among them).
 * Asynchronous on `stream`. */
int pycllp_hip_sparse_solve_bounded(pycllp_hip_sparse *handle, long B, const double *b_dev, const double *c_dev,
                                    const double *u_dev, double *x_dev, double *y_dev, double *z_dev, double *s_dev,
                                    double *pobj_dev, double *dobj_dev, int *status_dev, int *iters_dev,
                                    const pycllp_hip_opts *opts, void *stream);
/* The same LPs on the HOMOGENEOUS SELF-DUAL EMBEDDING with bounds, on the wavefront-per-LP kernel
 * (csrc/ipm_wreg_bdhsd.inc; the system of section 26): an infeasible or unbounded LP ends with a certificate
 * instead of the 10x-growth heuristic of pycllp_hip_sparse_solve_bounded.  Arguments as pycllp_hip_sparse_solve_bounded, on the
 * same handle and the same plan (built by whichever of the two entries runs first); the outputs mean what they mean for
 * pycllp_hip_dense_solve_bounded_hsd:
 *   status 0 (and 5)  x, y, z, s, pobj, dobj are divided by the final tau (at the iteration limit the objectives are those of
 *                     the point returned)
 *   status 2          the certificate as it stands: y, z, s with -b'y - u's > 0 and |A'y - z + s| <= 1e-8 (-b'y - u's)
 *   status 4          the certificate as it stands: a ray x with c'x > 0 and max(|A x|, |x_j| over finite u_j) <= 1e-8 c'x
 *                     (under autoscale both hold for the LP as the kernel scaled it)
 *   a fixed column (u = 0) ends at x = 0 with z = max(-r, 0), s = max(r, 0), r = c tau - A'y, on the same scaling
 * y_dev, z_dev, s_dev, pobj_dev, dobj_dev, iters_dev may be NULL.  Options: PYCLLP_FLAG_HSD is accepted and implied;
 * PYCLLP_FLAG_AUTOSCALE and _AUTOSCALE_PER_LP apply exactly as for pycllp_hip_sparse_solve_bounded; max_refine =
 * PYCLLP_MAX_REFINE_AUTO resolves to 20.  An LP whose LDL' would need the Nocedal-Wright guard, or whose norms, tau, kappa or
 * step turn non-finite, ends PYCLLP_STATUS_NUMERICAL.
 * Returns PYCLLP_E_BADARG for a NULL handle or u_dev, B < 0, both autoscale flags together, or any of the flags PREDCORR,
 * WARM_START, WAVE_KERNEL, BLOCK_KERNEL, NO_SLACK_PATH, FORCE_GUARD_PATH -- before the handle is read and before any HIP call --,
 * and PYCLLP_E_UNSUPPORTED for a handle on the large-LP kernel (m > 128 or n > 512), when no variant of the bounded kernel or
 * LDS plan covers A, or when the kernel of the plan's shape was not compiled (an instantiation with scratch is not shipped).
 * pycllp_hip_sparse_launch_info / _variant_info report the launch as they do for pycllp_hip_sparse_solve_bounded.
 * Asynchronous on `stream`. */
int pycllp_hip_sparse_solve_bounded_hsd(pycllp_hip_sparse *handle, long B, const double *b_dev, const double *c_dev,
                                        const double *u_dev, double *x_dev, double *y_dev, double *z_dev, double *s_dev,
                                        double *pobj_dev, double *dobj_dev, int *status_dev, int *iters_dev,
                                        const pycllp_hip_opts *opts, void *stream);
/* The bounded solve with PER-PROBLEM VALUES of A on the shared structure: the union of pycllp_hip_sparse_solve_batch and
 * pycllp_hip_sparse_solve_bounded, on the same kernel text compiled for per-problem values (csrc/ipm_wreg_bdpa.hip).
 *   Adata_dev [B, nnz]   the values of LP k in the CSR order of the arrays given to pycllp_hip_sparse_init (whose values only
 *                        fixed the structure); the ones of slack columns are among them, as the sparse path stores them
 * u, s, dobj = b'y + u's, the objectives at the iteration limit and PYCLLP_FLAG_AUTOSCALE mean what they mean for
 * pycllp_hip_sparse_solve_bounded.  An LP whose LDL' would need the Nocedal-Wright guard ends PYCLLP_STATUS_NUMERICAL.  The
 * kernel's plan (structure tables; every wavefront keeps its LP's values, t and s behind its area, 1 to 4 wavefronts per
 * workgroup as the LDS takes) is built on the first call and kept with the handle.
 * Returns PYCLLP_E_BADARG for a NULL handle, Adata_dev or u_dev, B < 0, or any of the flags HSD, PREDCORR, WARM_START,
 * WAVE_KERNEL, BLOCK_KERNEL, NO_SLACK_PATH, FORCE_GUARD_PATH (before the handle is read and before any HIP call), and
 * PYCLLP_E_UNSUPPORTED for a handle of the large-LP kernel (m > 128 or n > 512) or when no variant or LDS plan covers the
 * structure.  Asynchronous on `stream`. */
int pycllp_hip_sparse_solve_batch_bounded(pycllp_hip_sparse *handle, long B, const double *Adata_dev, const double *b_dev,
                                          const double *c_dev, const double *u_dev, double *x_dev, double *y_dev,
                                          double *z_dev, double *s_dev, double *pobj_dev, double *dobj_dev, int *status_dev,
                                          int *iters_dev, const pycllp_hip_opts *opts, void *stream);
/* One Newton step of the primal normal equations for B independent states with the sparse shared A: the reference's
 * stand-alone kernel sparse_solve_primal_normal (pycllp/cl/ldl.cl:656-712) as launched by its tests/test_ldl.py:276-361.
 * Arguments as pycllp_hip_dense_newton. */
int pycllp_hip_sparse_newton(pycllp_hip_sparse *handle, long B, const double *x_dev, const double *z_dev,
                             const double *y_dev, const double *b_dev, const double *c_dev, double mu, double *dy_dev,
                             int *nrefine_dev, const pycllp_hip_opts *opts, void *stream);
/* grid (workgroups), threads per workgroup, LDS bytes per workgroup and kernel (0 = workgroup-per-LP block kernel,
 * 1 = register-resident wavefront-per-LP kernel on term tables, 2 = the same on a dense image of A, 3 = the large-LP kernel
 * with its Gram from a term list, 4 = the same on the matrix cores) of the last launch (solve or Newton step) on this handle
 * (host values). */
int pycllp_hip_sparse_launch_info(const pycllp_hip_sparse *handle, int *grid, int *block, int *lds_bytes, int *kernel);
/* (MB, NQ) -- 16-row blocks, 64-column registers -- of the wavefront-per-LP kernel's plan that served the last launch on
 * this handle; (0, 0) when that launch ran on the block or the large-LP kernel, or before the first launch. */
int pycllp_hip_sparse_variant_info(const pycllp_hip_sparse *handle, int *mb, int *nq);
/* The LDS plan of the workgroup-per-LP kernel that served the last launch on this handle (any pointer may be NULL).
 * Large-LP kernel: *wgpc, *bnc = the compiled instantiation ipm_big_kernel<WGPC, BNC> that was launched (WGPC workgroups per
 * CU, BNC N-vector registers per thread) and *factor_in_lds = 1 when the blocks of the factor sat in LDS, 0 when they sat in
 * the L2-resident workspace; (0, 0, -1) otherwise.  Block kernel: *a_in_lds = 1 when the CSR / CSC copy of A sat in LDS, 0
 * when it was read through L2; -1 otherwise (a launch of the wavefront-per-LP kernel leaves it at -1 although the block
 * kernel stands behind it for the LPs it defers). */
int pycllp_hip_sparse_plan_info(const pycllp_hip_sparse *handle, int *wgpc, int *bnc, int *factor_in_lds, int *a_in_lds);
void pycllp_hip_sparse_free(pycllp_hip_sparse *handle);

/* ---- GeneralLP batches to and from the bounded equality form, on the device ----
 * B LPs  optimise c'x + f  s.t.  a <= A x <= b,  l <= x <= u  with one shared A [m, n] become the LPs  max c^'x^ + f^  s.t.
 * [+-A | I] x^ = b^,  0 <= x^ <= u^  that pycllp_hip_dense_solve_bounded / pycllp_hip_sparse_solve_bounded take, and their
 * solutions the GeneralLP's: GeneralLP.to_bounded_equality_form and BoundedMap.general of pycllp_amd/lp.py as two kernels.  No
 * handle.  The plan that is one for the batch comes from the caller (GeneralLP.bounded_structure, lp.bounded_rowmap):
 *   rowmap_dev [m] i32   for row i of the LP: k + 1 where it is row k of the bounded form with +A (b finite in every LP),
 *                        -(k + 1) where it is row k with -A (b = +inf, a finite in every LP), 0 where it is dropped (neither
 *                        bound finite in any LP); k = 0 .. mk-1 in the order of the rows.  N = n + mk columns, slacks last.
 *   Adata_dev f64 [nnz], Aindptr_dev i32 [m+1], Aindices_dev i32 [nnz]   CSR of the ORIGINAL A; a row's terms are summed in
 *                        the order they stand in (SparseMatrix.csr_term_order: that of the coordinate lists, so the sums carry
 *                        the host's bits).  With nnz = 0 the two [nnz] arrays may be NULL.
 * pycllp_hip_general_to_bounded:  a_dev, b_dev [B,m], c_dev, l_dev, u_dev [B,n], f_dev [B]  (l_dev, f_dev may be NULL = 0;
 * a non-finite a means "no lower bound") ->
 *   bh_dev [B,mk]        b - A l for a + row, -(a - A l) for a - row; A l = the sequential sum of the separately rounded products
 *   ch_dev [B,N]         [c | 0]
 *   uh_dev [B,N]         u - l where u is finite, else +inf; the slack of a + row (b - A l) - (a - A l) where a is finite, else
 *                        +inf; the slack of a - row +inf.  0 = fixed (l == u, an equality row's slack)
 *   fh_dev [B]           f + c'l (summed in an order of the kernel's own: not the host's bits, to rounding)
 *   invalid_dev [B] i32  0, or the first check LP k fails: 1 a non-finite l, 2 u < l, 3 a > b with a finite, 4 a row whose finite
 *                        bounds do not match rowmap (+: b finite; -: b = +inf and a finite; dropped: neither finite), 5 a
 *                        non-finite c or f.  Such an LP is replaced by a harmless one -- b^ = A^ 1 (row sums, slack included),
 *                        c^ = 0, u^ = +inf, f^ = 0: x^ = 1 is feasible and optimal -- so that no solve kernel meets a NaN.
 * pycllp_hip_general_from_bounded:  xh_dev, zh_dev, sh_dev [B,N], yh_dev [B,mk] as a bounded solve entry wrote them, l_dev (may
 * be NULL = 0), fh_dev and invalid_dev as above ->
 *   x_dev [B,n] = l + x^;  y_dev [B,m] = +-y^ by rowmap, 0 for a dropped row;  z_dev, s_dev [B,n] (optional) the first n columns
 *   of z^, s^ (zh_dev / sh_dev may be NULL, then z_dev / s_dev must be);  pobj_dev, dobj_dev [B] (optional, IN/OUT) += f^;
 *   status_dev, iters_dev (optional) [B] i32 IN/OUT: left as the solve wrote them, except that an LP with invalid != 0 gets
 *   status PYCLLP_STATUS_NUMERICAL, iters 0 and quiet NaNs in x, y, z, s, pobj, dobj.
 * Both: PYCLLP_E_BADARG for a NULL required pointer, m, n or mk < 1, mk > m, B < 0 or nnz < 0, PYCLLP_E_UNSUPPORTED for
 * m > 256 or n + mk > 1280 (beyond every bounded solve entry), all before any HIP call; B = 0 returns 0 and launches nothing.
 * One launch each, asynchronous on `stream`; alignment and footprint as stated at the top. */
int pycllp_hip_general_to_bounded(int m, int n, int mk, long B, const int *rowmap_dev, int nnz, const double *Adata_dev,
                                  const int *Aindptr_dev, const int *Aindices_dev, const double *a_dev, const double *b_dev,
                                  const double *c_dev, const double *l_dev, const double *u_dev, const double *f_dev,
                                  double *bh_dev, double *ch_dev, double *uh_dev, double *fh_dev, int *invalid_dev, void *stream);
int pycllp_hip_general_from_bounded(int m, int n, int mk, long B, const int *rowmap_dev, const double *l_dev,
                                    const double *fh_dev, const int *invalid_dev, const double *xh_dev, const double *yh_dev,
                                    const double *zh_dev, const double *sh_dev, double *x_dev, double *y_dev, double *z_dev,
                                    double *s_dev, double *pobj_dev, double *dobj_dev, int *status_dev, int *iters_dev,
                                    void *stream);

/* ---- The same for LPs that each have their OWN values of A on one shared structure ----
 * pycllp_hip_general_to_bounded_batch: B LPs  a <= A_k x <= b,  l <= x <= u  become the LPs  [+-A_k | I] x^ = b^,  0 <= x^ <= u^
 * that pycllp_hip_dense_solve_batch_bounded / pycllp_hip_sparse_solve_batch_bounded take -- b^, c^, u^, f^, invalid as
 * pycllp_hip_general_to_bounded writes them, and the matrix of every LP in the layout the solve entry wants.  A C caller's
 * three steps: this entry, the solve entry on Ah_dev, bh_dev, ch_dev, uh_dev, then pycllp_hip_general_from_bounded (which
 * needs no matrix).  rowmap_dev, a_dev .. f_dev, bh_dev .. invalid_dev, the checks 1 .. 5 and the sizes: as above.
 *   Avals_dev f64 [B,nnz]   every LP's values in the order of the caller's coordinate lists (rows, cols); read as they are
 *   Aindptr_dev i32 [m+1], Aindices_dev i32 [nnz]   the structure's CSR with a row's terms in the order of the coordinate lists
 *                           (SparseMatrix.csr_term_order); Aorder_dev i32 [nnz]: the position in the coordinate lists of the
 *                           q-th term of that order (a stable sort of rows).  (A_k l_k)_i starts at 0.0 and adds the separately
 *                           rounded products Avals[k, Aorder[q]] * l[k, Aindices[q]] for q = Aindptr[i] .. Aindptr[i+1]-1 in
 *                           turn: the host's bits.  With nnz = 0 the [nnz] arrays may be NULL.
 *   gather_dev i32 [out_len]   the plan of ONE LP's matrix output (lp.bounded_gather_dense / lp.bounded_gather_csr): slot p of
 *                           Ah_dev[k] holds +Avals[k, t] where gather[p] = t + 1, -Avals[k, t] where gather[p] = -(t + 1), 0.0
 *                           where gather[p] = 0 and 1.0 where gather[p] = INT32_MAX (the one of a slack column).  An index
 *                           outside 1 .. nnz yields 0.0.
 *   Ah_dev f64 [B,out_len]  for pycllp_hip_dense_solve_batch_bounded: out_len = mk n, the kept rows of +-A_k as [mk, n]
 *                           row-major (a_cols = n: no slack columns); for pycllp_hip_sparse_solve_batch_bounded: out_len =
 *                           nnz of the handle's [+-A | I], its values in the handle's CSR order.
 * An LP with a code gets b^ = A^_k 1 from its OWN values (the row's signed values summed in term order, plus 1.0), c^ = 0,
 * u^ = +inf, f^ = 0; its matrix is written like every other LP's.  Non-finite values of A are not checked here: the solve
 * kernels end such an LP with PYCLLP_STATUS_NUMERICAL.  PYCLLP_E_BADARG for a NULL required pointer, nnz < 0, out_len < 1, m, n
 * or mk < 1, mk > m, B < 0; PYCLLP_E_UNSUPPORTED for m > 256, n + mk > 1280 or out_len > 256 * 1280; all before any HIP call;
 * B = 0 returns 0 and launches nothing.  One launch, asynchronous on `stream`; alignment and footprint as stated at the top. */
int pycllp_hip_general_to_bounded_batch(int m, int n, int mk, long B, const int *rowmap_dev, int nnz, const int *Aorder_dev,
                                        const int *Aindptr_dev, const int *Aindices_dev, const double *Avals_dev, long out_len,
                                        const int *gather_dev, const double *a_dev, const double *b_dev, const double *c_dev,
                                        const double *l_dev, const double *u_dev, const double *f_dev, double *Ah_dev,
                                        double *bh_dev, double *ch_dev, double *uh_dev, double *fh_dev, int *invalid_dev,
                                        void *stream);

#ifdef __cplusplus
}
#endif
#endif /* PYCLLP_HIP_H */
