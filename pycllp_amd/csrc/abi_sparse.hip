// abi_sparse.hip -- the C ABI of the sparse handle (include/pycllp_hip.h: pycllp_hip_sparse_*), the three LDL' entries, the
// entries that belong to no handle (ABI version, default options, last error) and the thread's error message.  Host code only:
// the kernels are reached through wreg.h (the wave kernels), big.h (the large-LP kernel) and block.h (the block kernel, LDL').
// The block kernel's plan comes from block_plan.h; pycllp_hip_debug_plan (last in this file) builds any plan without a HIP call.
#include "host.h"
#include "wreg_plan.h"
#include "big_plan.h"
#include "block_plan.h"
#include "plan_upload.h"

static thread_local char g_err[512] = "";

int pycllp_runtime_error(int code, const char* what) {   // host_error.h
    if (code > 0) snprintf(g_err, sizeof(g_err), "%s: %s", what, hipGetErrorString((hipError_t)code));
    else snprintf(g_err, sizeof(g_err), "%s", what);
    return code;
}

int pycllp_entry_error(int code, const char* entry, const char* what) {
    snprintf(g_err, sizeof(g_err), "%s: %s", entry, what);
    return code;
}

int pycllp_exceeds_error(const char* entry, int m, int n, int max_m, int max_n) {
    if (max_m) snprintf(g_err, sizeof(g_err), "%s: (m=%d, n=%d) exceeds the compiled kernels (m<=%d, n<=%d)", entry, m, n, max_m, max_n);
    else snprintf(g_err, sizeof(g_err), "%s: n=%d exceeds the compiled kernel (n<=%d)", entry, n, max_n);
    return PYCLLP_E_UNSUPPORTED;
}

int pycllp_a_cols_error(const char* entry, long a_cols, int expected, bool tail) {
    snprintf(g_err, sizeof(g_err), "%s: a_cols = %ld, expected %d (%s)", entry, a_cols, expected,
             tail ? "the columns before the identity tail" : "every column");
    return PYCLLP_E_BADARG;
}

static unsigned long long* g_prof = nullptr;  // diagnostic build only
#ifdef PYCLLP_PROFILE
extern "C" void pycllp_hip_debug_set_prof(void* p) { g_prof = (unsigned long long*)p; }
#endif

DevOpts to_dev(const pycllp_hip_opts* opts) {
    pycllp_hip_opts d;
    pycllp_hip_default_opts(&d);
    if (opts) d = *opts;
    DevOpts o;
    o.eps = d.eps; o.delta = d.delta; o.r = d.r; o.pivot_floor = d.pivot_floor; o.refine_tol = d.refine_tol;
    o.max_iter = d.max_iter; o.flags = d.flags;
    // PYCLLP_FLAG_AUTOSCALE_PER_LP reaches the kernels WITH PYCLLP_FLAG_AUTOSCALE (wave_common.h autoscale_lp): they test the
    // flag they always tested for "the scaling code runs", and the new one only inside it
    if (o.flags & PYCLLP_FLAG_AUTOSCALE_PER_LP) o.flags |= PYCLLP_FLAG_AUTOSCALE;
    // PYCLLP_MAX_REFINE_AUTO: the reference's cap of 5 passes (ldl.cl:645) on its own path; 20 on the homogeneous self-dual
    // variant, whose last systems are harder (with 5, LP 7557 of config 5's share stalls for 70-150 iterations)
    o.max_refine = d.max_refine >= 0 ? d.max_refine : ((d.flags & PYCLLP_FLAG_HSD) ? PYCLLP_MAX_REFINE_HSD : PYCLLP_MAX_REFINE_PLAIN);
    o.reserve_cus = d.reserve_cus < 0 ? 0 : d.reserve_cus;
    o.prof = g_prof;
    return o;
}

// what launch_info reports: the last solve ran on the wave kernel with `plan` (null: on the block or large-LP kernel; the
// block kernel with `a_in_lds` and `lds` bytes of LDS)
static void record_launch(pycllp_hip_sparse* h, WregPlan* plan, int grid, int a_in_lds = -1, int lds = 0) {
    std::lock_guard<std::mutex> g(h->info_mu);
    h->last_plan = plan; h->grid = grid; h->last_a_in_lds = a_in_lds; h->last_lds = lds;
}

// A wave-kernel plan built by its first user (under info_mu; once any call has returned, lp->plan no longer changes), null when
// no variant covers A.  Returns 0, or the set_err code of a HIP error of the build.
template <typename Create>
static int lazy_plan(pycllp_hip_sparse* h, LazyPlan* lp, const char* what, Create create) {
    std::lock_guard<std::mutex> g(h->info_mu);
    if (lp->tried) return 0;
    lp->tried = true;
    WregPlan* wp = nullptr;
    const int rc = create(&wp);
    if (rc >= 1000) return set_err(rc - 1000, what);
    lp->plan = (rc == 0) ? wp : nullptr;
    return 0;
}

// The wave kernel on `plan` with a worklist of the LPs it defers (guard would have bitten), which then(worklist) takes: the
// block kernel's guarded path, or deferred_to_numerical_kernel where no guarded kernel can.  wave_what / then_what: the launches
// as a HIP error names them.
template <typename Then>
static int wave_solve_deferring(pycllp_hip_sparse* h, WregPlan* plan, long B, const double* a_batch, const double* b_dev,
                                const double* c_dev, double* x_dev, double* y_dev, double* z_dev, double* pobj_dev, double* dobj_dev,
                                int* status_dev, int* iters_dev, const DevOpts& o, hipStream_t st, const char* wave_what,
                                const char* then_what, Then&& then) {
    int* worklist = nullptr;
    int grid = 0;
    HIP_TRY(hipMallocAsync((void**)&worklist, sizeof(int) * (size_t)(B + 1), st));
    hipError_t e = h->ring.run(st, [&](int* qw) {
        return wreg_launch_solve(plan, B, a_batch, b_dev, c_dev, x_dev, y_dev, z_dev, pobj_dev, dobj_dev, status_dev, iters_dev, qw,
                                 worklist, o, h->num_cu, st, &grid);
    });
    if (e != hipSuccess) { (void)hipFreeAsync(worklist, st); return set_err((int)e, wave_what); }
    e = then(worklist);
    const hipError_t e2 = hipFreeAsync(worklist, st); if (e == hipSuccess) e = e2;
    record_launch(h, plan, grid);
    if (e != hipSuccess) return set_err((int)e, then_what);
    return 0;
}

// The block kernel's launch plan: four, two or one workgroups per CU by their LDS on `cus` CUs, one per LP at most
static long block_plan(int lds, long cus, long B) {
    const long per_cu = (160 * 1024) / lds >= 4 ? 4 : ((160 * 1024) / lds >= 2 ? 2 : 1);
    const long blocks = cus * per_cu;
    return blocks > B ? B : blocks;
}

int sparse_init_host(int m, int n, int nnz, const std::vector<double>& val, const std::vector<int>& ptr, const std::vector<int>& col,
                     void* stream, pycllp_hip_sparse** handle) {
    hipStream_t st = (hipStream_t)stream;
    if (m > BLK_MAX_M || n > BLK_MAX_N) {
        // beyond the wavefront-per-LP and block kernels: the workgroup-per-LP kernel of ipm_big.hip (blocks of the factor in
        // LDS or an L2-resident workspace)
        pycllp_hip_sparse* hb = new (std::nothrow) pycllp_hip_sparse();
        if (!hb) return set_err(PYCLLP_E_NOMEM, "pycllp_hip_sparse_init: out of host memory");
        DeviceLimits lim;
        hipError_t eb = device_limits(&lim);
        if (eb == hipSuccess) eb = hb->ring.create();
        if (eb != hipSuccess) { pycllp_hip_sparse_free(hb); return set_err((int)eb, "pycllp_hip_sparse_init (large LP)"); }
        hb->num_cu = lim.num_cu; hb->max_lds = lim.max_lds;
        hb->desc.m = m; hb->desc.n = n; hb->desc.nnz = nnz;
        const int rc = big_plan_create(m, n, nnz, val.data(), ptr.data(), col.data(), lim.max_lds, st, &hb->big);
        if (rc != 0) {
            pycllp_hip_sparse_free(hb);
            if (rc >= 1000) return set_err(rc - 1000, "big_plan_create");
            return set_err(PYCLLP_E_UNSUPPORTED, "pycllp_hip_sparse_init: the LP does not fit the large-LP kernel");
        }
        hb->lds = big_lds_bytes(hb->big);
        *handle = hb;
        return 0;
    }
    pycllp_hip_sparse* h = new (std::nothrow) pycllp_hip_sparse();
    if (!h) return set_err(PYCLLP_E_NOMEM, "pycllp_hip_sparse_init: out of host memory");
    // on failure the partly built handle goes through pycllp_hip_sparse_free, which skips what was not made
    DeviceLimits lim;
    hipError_t e = device_limits(&lim);
    if (e != hipSuccess) { pycllp_hip_sparse_free(h); return set_err((int)e, "hipGetDeviceProperties"); }
    h->num_cu = lim.num_cu;
    const int max_lds = lim.max_lds;
    // the block kernel's plan (block_plan.h), its tables uploaded, the device pointers set
    BlockHostPlan H;
    const int brc = block_host_plan(m, n, nnz, val.data(), ptr.data(), col.data(), max_lds, H);
    if (brc != BLOCK_PLAN_OK) {
        pycllp_hip_sparse_free(h);
        return set_err(PYCLLP_E_UNSUPPORTED, brc == BLOCK_PLAN_TOO_DENSE ? "pycllp_hip_sparse_init: A is too dense for the term-list Gram assembly"
                                                                         : "pycllp_hip_sparse_init: problem does not fit in LDS");
    }
    e = h->ring.create();
    if (e != hipSuccess) { pycllp_hip_sparse_free(h); return set_err((int)e, "hipMalloc(sparse A)"); }
    e = plan_upload(H.blob, st, &h->dev_blob);
    if (e != hipSuccess) { pycllp_hip_sparse_free(h); return set_err((int)e, "upload sparse A"); }
    const char* db = (const char*)h->dev_blob;
    BlockA& d = h->desc;
    d = H.desc;
    d.csr_val = (const double*)(db + H.a_csr_val); d.csr_ptr = (const int*)(db + H.a_csr_ptr); d.csr_col = (const int*)(db + H.a_csr_col);
    d.csc_val = (const double*)(db + H.a_csc_val); d.csc_ptr = (const int*)(db + H.a_csc_ptr); d.csc_row = (const int*)(db + H.a_csc_row);
    d.ent_tri = (const int*)(db + H.a_ent_tri); d.ent_ptr = (const int*)(db + H.a_ent_ptr);
    d.term_w = (const double*)(db + H.a_term_w); d.term_col = (const int*)(db + H.a_term_col);
    d.csc_src = (const int*)(db + H.a_csc_src);
    d.term_ia = (const int*)(db + H.a_term_ia); d.term_ib = (const int*)(db + H.a_term_ib);
    h->lds = H.lds; h->lds_with_a = H.lds_with_a;
    // the register-resident one-LP-per-wavefront kernel takes over whenever its tables fit (ipm_wreg.hip)
    {
        WregPlan* wp = nullptr;
        const int rc = wreg_plan_create(m, n, nnz, val.data(), ptr.data(), col.data(), max_lds, 0, st, &wp);
        if (rc >= 1000) { pycllp_hip_sparse_free(h); return set_err(rc - 1000, "wreg_plan_create"); }
        h->wreg = (rc == 0) ? wp : nullptr;
    }
    h->max_lds = max_lds;
    h->host_val = val; h->host_ptr = ptr; h->host_col = col;
    *handle = h;
    return 0;
}

// (host.h) The wave kernel on per-problem dense matrices (ipm_wreg_dapa.hip), on the plan for the implied identity tail or, with
// PYCLLP_FLAG_NO_SLACK_PATH, the one with every column in the image -- each built on first use.  Where no variant or LDS plan
// covers the LP (every handle of the large-LP kernel included) the entry declines as it always did.  An LP the kernel defers (the guard would have bitten; every LP under
// PYCLLP_FLAG_FORCE_GUARD_PATH) ends PYCLLP_STATUS_NUMERICAL with status its only output: the block kernel reads per-problem
// values in CSR order, which the dense [m, a_cols] layout is not.
int dense_solve_batch_wave(pycllp_hip_sparse* h, long B, const double* A_dev, long a_cols, const double* b_dev, const double* c_dev,
                           double* x_dev, double* y_dev, double* z_dev, double* pobj_dev, double* dobj_dev, int* status_dev,
                           int* iters_dev, const pycllp_hip_opts* opts, void* stream) {
    static const char* const kStops = "pycllp_hip_dense_solve_batch: per-problem dense matrices stop at m = 32, n = 128 "
                                      "(beyond: pycllp_hip_sparse_solve_batch)";
    if (h->big) return set_err(PYCLLP_E_UNSUPPORTED, kStops);
    hipStream_t st = (hipStream_t)stream;
    const int keep = ((opts ? opts->flags : 0) & PYCLLP_FLAG_NO_SLACK_PATH) ? 1 : 0;
    LazyPlan* lp = &h->lazy[keep ? LAZY_DAPA_KEEP : LAZY_DAPA];
    const int rc = lazy_plan(h, lp, "wreg_plan_create_dense_pa", [&](WregPlan** wp) {
        return wreg_plan_create_dense_pa(h->desc.m, h->desc.n, h->desc.nnz, h->host_val.data(), h->host_ptr.data(),
                                         h->host_col.data(), h->max_lds, keep, st, wp);
    });
    if (rc != 0) return rc;
    if (!lp->plan) return set_err(PYCLLP_E_UNSUPPORTED, kStops);
    const int nd = wreg_image_cols(lp->plan);
    if (a_cols != (long)nd) return pycllp_a_cols_error("pycllp_hip_dense_solve_batch", a_cols, nd, nd != h->desc.n);
    if (B == 0) return 0;
    return wave_solve_deferring(h, lp->plan, B, A_dev, b_dev, c_dev, x_dev, y_dev, z_dev, pobj_dev, dobj_dev, status_dev, iters_dev,
                                to_dev(opts), st, "ipm_wreg_kernel (per-problem dense A) launch",
                                "deferred_to_numerical_kernel launch",
                                [&](const int* worklist) { return block_launch_deferred_to_numerical(worklist, status_dev, st); });
}

// (host.h) The bounded wave kernel on per-problem dense matrices (ipm_wreg_bddapa.hip), on a plan of its own built on first use:
// the image per wave with the identity tail implied, t and s behind it.  A handle of the large-LP kernel and an LP no variant or
// LDS plan covers are declined.  An LP whose factorisation the guard would have changed ends PYCLLP_STATUS_NUMERICAL in the kernel.
int dense_solve_batch_bounded_wave(pycllp_hip_sparse* h, long B, const double* A_dev, long a_cols, const double* b_dev,
                                   const double* c_dev, const double* u_dev, double* x_dev, double* y_dev, double* z_dev,
                                   double* s_dev, double* pobj_dev, double* dobj_dev, int* status_dev, int* iters_dev,
                                   const pycllp_hip_opts* opts, void* stream) {
    static const char* const kStops = "pycllp_hip_dense_solve_batch_bounded: upper bounds on per-problem dense matrices beyond the "
                                      "lane-group kernels stop at m = 128, n = 256 with [A_dense | I]";
    if (h->big) return set_err(PYCLLP_E_UNSUPPORTED, kStops);
    hipStream_t st = (hipStream_t)stream;
    LazyPlan* lp = &h->lazy[LAZY_BDDAPA];
    const int rc = lazy_plan(h, lp, "wreg_plan_create_bounded_dense_pa", [&](WregPlan** wp) {
        return wreg_plan_create_bounded_dense_pa(h->desc.m, h->desc.n, h->desc.nnz, h->host_val.data(), h->host_ptr.data(),
                                                 h->host_col.data(), h->max_lds, st, wp);
    });
    if (rc != 0) return rc;
    if (!lp->plan) return set_err(PYCLLP_E_UNSUPPORTED, kStops);
    const int nd = wreg_image_cols(lp->plan);
    if (a_cols != (long)nd) return pycllp_a_cols_error("pycllp_hip_dense_solve_batch_bounded", a_cols, nd, nd != h->desc.n);
    if (B == 0) return 0;
    DevOpts o = to_dev(opts);
    int grid = 0;
    const hipError_t e = h->ring.run(st, [&](int* qw) {
        return wreg_launch_solve_bounded(lp->plan, B, A_dev, b_dev, c_dev, u_dev, x_dev, y_dev, z_dev, s_dev, pobj_dev, dobj_dev,
                                         status_dev, iters_dev, qw, o, h->num_cu, st, &grid);
    });
    record_launch(h, lp->plan, grid);
    if (e != hipSuccess) return set_err((int)e, "ipm_wreg_bounded_dapa_kernel launch");
    return 0;
}

// which kernels of the sparse path implement the predictor-corrector step
static bool sparse_predcorr_available(const pycllp_hip_sparse* h, bool per_problem_a, int flags) {
    if (h->big) return true;
    if (flags & PYCLLP_FLAG_BLOCK_KERNEL) return false;
    // (per-problem A: the PA plan is built lazily by the first solve_batch; its kernels all have the variant)
    return per_problem_a ? true : wreg_has_predcorr(h->wreg) != 0;
}

static int sparse_solve_impl(pycllp_hip_sparse* h, long B, const double* a_batch, const double* b_dev, const double* c_dev,
                             double* x_dev, double* y_dev, double* z_dev, double* pobj_dev, double* dobj_dev, int* status_dev,
                             int* iters_dev, const pycllp_hip_opts* opts, void* stream) {
    if (!h || B < 0) return set_err(PYCLLP_E_BADARG, "pycllp_hip_sparse_solve: bad argument");
    if (both_autoscales(opts)) return entry_err(PYCLLP_E_BADARG, "pycllp_hip_sparse_solve", kBothAutoscales);
    if (B == 0) return 0;
    if (!b_dev || !c_dev || !x_dev || !status_dev) return set_err(PYCLLP_E_BADARG, "pycllp_hip_sparse_solve: bad argument");
    DevOpts o = to_dev(opts);
    if ((o.flags & PYCLLP_FLAG_WARM_START) && (!y_dev || !z_dev))
        return set_err(PYCLLP_E_BADARG, "pycllp_hip_sparse_solve: warm start needs y_dev and z_dev");
    hipStream_t st = (hipStream_t)stream;
    if ((o.flags & PYCLLP_FLAG_PREDCORR) && (o.flags & PYCLLP_FLAG_HSD))
        return set_err(PYCLLP_E_BADARG, "pycllp_hip_sparse_solve: PYCLLP_FLAG_PREDCORR is an option of the reference's path (not with PYCLLP_FLAG_HSD)");
    if ((o.flags & PYCLLP_FLAG_PREDCORR) && !sparse_predcorr_available(h, a_batch != nullptr, o.flags))
        return set_err(PYCLLP_E_UNSUPPORTED, "pycllp_hip_sparse_solve: PYCLLP_FLAG_PREDCORR is not available on the kernel that serves this LP");
    if (h->big) {
        if (a_batch) return set_err(PYCLLP_E_UNSUPPORTED, "pycllp_hip_sparse_solve_batch: per-problem values of A stop at m = 128, n = 512");
        int grid_b = 0;
        const hipError_t eb = h->ring.run(st, [&](int* qb) {
            return big_launch_solve(h->big, B, b_dev, c_dev, x_dev, y_dev, z_dev, pobj_dev, dobj_dev, status_dev, iters_dev, qb, o,
                                    h->num_cu, st, &grid_b);
        });
        record_launch(h, nullptr, grid_b);
        if (eb != hipSuccess) return set_err((int)eb, "ipm_big_kernel launch");
        return 0;
    }
    BlockA desc = h->desc;
    int lds = h->lds;
    if (a_batch && h->lds_with_a) { desc.a_in_lds = 1; lds = h->lds_with_a; }
    // per-problem values: the PA plan of the wave kernel (structure tables; built on first use), else the shared-A plan
    if (a_batch && !(o.flags & PYCLLP_FLAG_BLOCK_KERNEL)) {
        const int rc = lazy_plan(h, &h->lazy[LAZY_PA], "wreg_plan_create (per-problem A)", [&](WregPlan** wp) {
            return wreg_plan_create(h->desc.m, h->desc.n, h->desc.nnz, h->host_val.data(), h->host_ptr.data(), h->host_col.data(),
                                    h->max_lds, 1, st, wp);
        });
        if (rc != 0) return rc;
    }
    WregPlan* wplan = a_batch ? h->lazy[LAZY_PA].plan : h->wreg;
    const bool use_wreg = wplan && !(o.flags & PYCLLP_FLAG_BLOCK_KERNEL);
    // per-problem values on the block kernel need A's arrays in LDS next to the packed factor; a matrix too large for that is
    // served by the wave kernel's PA plan alone, and an LP it defers (guard would have bitten: never observed) ends NUMERICAL
    if ((o.flags & PYCLLP_FLAG_PREDCORR) && !use_wreg)
        return set_err(PYCLLP_E_UNSUPPORTED, "pycllp_hip_sparse_solve: PYCLLP_FLAG_PREDCORR is not available on the kernel that serves this LP");
    const bool block_can = !a_batch || h->lds_with_a != 0;
    if (!block_can && !use_wreg)
        return set_err(PYCLLP_E_UNSUPPORTED, "pycllp_hip_sparse_solve_batch: per-problem values of this A fit neither the wavefront-per-LP kernel's tables nor the block kernel's LDS");
    long blocks = 0;
    if (block_can) {
        hipError_t e = block_set_lds(lds);
        if (e != hipSuccess) return set_err((int)e, "set_dyn_lds((const void*)ipm_block_kernel, lds)");
        // on the CUs the caller did not reserve (Newton mode below takes them all)
        blocks = block_plan(lds, (long)h->num_cu - o.reserve_cus > 0 ? (long)h->num_cu - o.reserve_cus : 1, B);
    }
    const auto block_solve = [&](const int* worklist) {
        return h->ring.run(st, [&](int* qhead) {
            return block_launch_solve(desc, blocks, lds, B, b_dev, c_dev, x_dev, y_dev, z_dev, pobj_dev, dobj_dev, status_dev,
                                      iters_dev, qhead, worklist, a_batch, o, st);
        });
    };
    if (use_wreg)   // wave kernel first; whatever it defers (guard would have bitten) goes through the block kernel's guarded path
        return wave_solve_deferring(h, wplan, B, a_batch, b_dev, c_dev, x_dev, y_dev, z_dev, pobj_dev, dobj_dev, status_dev, iters_dev,
                                    o, st, "ipm_wreg_kernel launch",
                                    block_can ? "ipm_block_kernel launch" : "deferred_to_numerical_kernel launch",
                                    [&](const int* worklist) {
                                        return block_can ? block_solve(worklist)
                                                         : block_launch_deferred_to_numerical(worklist, status_dev, st);
                                    });
    const hipError_t e = block_solve(nullptr);
    record_launch(h, nullptr, (int)blocks, desc.a_in_lds, lds);
    if (e != hipSuccess) return set_err((int)e, "ipm_block_kernel launch");
    return 0;
}

// The body of pycllp_hip_sparse_solve_bounded and, with a_batch, of pycllp_hip_sparse_solve_batch_bounded, behind their
// argument checks (as sparse_solve_impl is of the entries without bounds).  lp: the entry's plan slot of the handle;
// create: its constructor, named create_what in a HIP error of the build.  hsd: the batch runs on the homogeneous self-dual
// embedding (ipm_wreg_bounded_hsd_kernel, on the same plan; shared A only) and `opts` carries PYCLLP_FLAG_HSD.
typedef int (*bounded_plan_fn)(int, int, int, const double*, const int*, const int*, int, hipStream_t, WregPlan**);
static int sparse_solve_bounded_impl(const char* entry, pycllp_hip_sparse* h, long B, const double* a_batch, LazyPlan* lp,
                                     bounded_plan_fn create, const char* create_what, const double* b_dev,
                                     const double* c_dev, const double* u_dev, double* x_dev, double* y_dev, double* z_dev,
                                     double* s_dev, double* pobj_dev, double* dobj_dev, int* status_dev, int* iters_dev,
                                     const pycllp_hip_opts* opts, void* stream, bool hsd = false) {
    if (h->big) return entry_err(PYCLLP_E_UNSUPPORTED, entry, "the bounded wave kernel stops at m = 128, n = 512");
    hipStream_t st = (hipStream_t)stream;
    const int rc = lazy_plan(h, lp, create_what, [&](WregPlan** wp) {
        return create(h->desc.m, h->desc.n, h->desc.nnz, h->host_val.data(), h->host_ptr.data(), h->host_col.data(), h->max_lds, st, wp);
    });
    if (rc != 0) return rc;
    if (!lp->plan)
        return entry_err(PYCLLP_E_UNSUPPORTED, entry,
                         a_batch ? "no variant of the bounded wave kernel covers this structure on per-problem values (rows, "
                                   "columns, or its tables in LDS)"
                                 : "no variant of the bounded wave kernel covers this A (rows, columns, or its tables in LDS)");
    if (hsd && !wreg_has_bounded_hsd(lp->plan))
        return entry_err(PYCLLP_E_UNSUPPORTED, entry, "no kernel of this shape was compiled (the instantiation does not stay free of scratch)");
    if (B == 0) return 0;
    DevOpts o = to_dev(opts);
    int grid = 0;
    const hipError_t e = h->ring.run(st, [&](int* qw) {
        if (hsd)
            return wreg_launch_solve_bounded_hsd(lp->plan, B, b_dev, c_dev, u_dev, x_dev, y_dev, z_dev, s_dev, pobj_dev, dobj_dev,
                                                 status_dev, iters_dev, qw, o, h->num_cu, st, &grid);
        return wreg_launch_solve_bounded(lp->plan, B, a_batch, b_dev, c_dev, u_dev, x_dev, y_dev, z_dev, s_dev, pobj_dev, dobj_dev,
                                         status_dev, iters_dev, qw, o, h->num_cu, st, &grid);
    });
    record_launch(h, lp->plan, grid);
    if (e != hipSuccess)
        return set_err((int)e, hsd ? "ipm_wreg_bounded_hsd_kernel launch"
                                   : (a_batch ? "ipm_wreg_bounded_pa_kernel launch" : "ipm_wreg_bounded_kernel launch"));
    return 0;
}

extern "C" {

int pycllp_hip_abi_version(void) { return PYCLLP_HIP_ABI_VERSION; }

const char* pycllp_hip_last_error(void) { return g_err; }

void pycllp_hip_default_opts(pycllp_hip_opts* o) {
    if (!o) return;
    o->eps = 1e-10;
    o->delta = 0.02;
    o->r = 0.9;
    o->pivot_floor = 1e-6;
    o->refine_tol = 1e-11;
    o->max_iter = 200;
    o->max_refine = PYCLLP_MAX_REFINE_AUTO;
    o->flags = 0;
    o->reserve_cus = 0;
}

int pycllp_hip_sparse_init(int m, int n, int nnz, const double* Adata_dev, const int* Aindptr_dev,
                           const int* Aindices_dev, void* stream, pycllp_hip_sparse** handle) {
    if (!handle || !Adata_dev || !Aindptr_dev || !Aindices_dev || m <= 0 || n <= 0 || nnz <= 0)
        return set_err(PYCLLP_E_BADARG, "pycllp_hip_sparse_init: bad argument");
    if (m > BIG_MAX_M || n > BIG_MAX_N) return pycllp_exceeds_error("pycllp_hip_sparse_init", m, n, BIG_MAX_M, BIG_MAX_N);
    hipStream_t st = (hipStream_t)stream;
    std::vector<double> val(nnz);
    std::vector<int> ptr(m + 1), col(nnz);
    HIP_TRY(hipMemcpyAsync(val.data(), Adata_dev, sizeof(double) * nnz, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipMemcpyAsync(ptr.data(), Aindptr_dev, sizeof(int) * (m + 1), hipMemcpyDeviceToHost, st));
    HIP_TRY(hipMemcpyAsync(col.data(), Aindices_dev, sizeof(int) * nnz, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    if (ptr[0] != 0 || ptr[m] != nnz) return set_err(PYCLLP_E_BADARG, "pycllp_hip_sparse_init: malformed CSR row pointer");
    for (int i = 0; i < m; i++) if (ptr[i + 1] < ptr[i]) return set_err(PYCLLP_E_BADARG, "pycllp_hip_sparse_init: malformed CSR row pointer");
    for (int e = 0; e < nnz; e++) if (col[e] < 0 || col[e] >= n) return set_err(PYCLLP_E_BADARG, "pycllp_hip_sparse_init: column index out of range");
    return sparse_init_host(m, n, nnz, val, ptr, col, stream, handle);
}

int pycllp_hip_sparse_solve(pycllp_hip_sparse* h, long B, const double* b_dev, const double* c_dev, double* x_dev,
                            double* y_dev, double* z_dev, double* pobj_dev, double* dobj_dev, int* status_dev,
                            int* iters_dev, const pycllp_hip_opts* opts, void* stream) {
    return sparse_solve_impl(h, B, nullptr, b_dev, c_dev, x_dev, y_dev, z_dev, pobj_dev, dobj_dev, status_dev, iters_dev, opts, stream);
}

int pycllp_hip_sparse_solve_batch(pycllp_hip_sparse* h, long B, const double* Adata_dev, const double* b_dev,
                                  const double* c_dev, double* x_dev, double* y_dev, double* z_dev, double* pobj_dev,
                                  double* dobj_dev, int* status_dev, int* iters_dev, const pycllp_hip_opts* opts, void* stream) {
    if (B > 0 && !Adata_dev) return set_err(PYCLLP_E_BADARG, "pycllp_hip_sparse_solve_batch: bad argument");
    return sparse_solve_impl(h, B, Adata_dev, b_dev, c_dev, x_dev, y_dev, z_dev, pobj_dev, dobj_dev, status_dev, iters_dev, opts, stream);
}

int pycllp_hip_sparse_solve_bounded(pycllp_hip_sparse* h, long B, const double* b_dev, const double* c_dev, const double* u_dev,
                                    double* x_dev, double* y_dev, double* z_dev, double* s_dev, double* pobj_dev, double* dobj_dev,
                                    int* status_dev, int* iters_dev, const pycllp_hip_opts* opts, void* stream) {
    const int rc = check_restricted("pycllp_hip_sparse_solve_bounded", h, B, u_dev, opts, kWaveBoundedRejected,
                                    "HSD, PREDCORR, WARM_START, WAVE_KERNEL, BLOCK_KERNEL, NO_SLACK_PATH and FORCE_GUARD_PATH are "
                                    "not available with upper bounds", b_dev && c_dev && x_dev && status_dev);
    if (rc != 0) return rc;
    return sparse_solve_bounded_impl("pycllp_hip_sparse_solve_bounded", h, B, nullptr, &h->lazy[LAZY_BD],
                                     wreg_plan_create_bounded, "wreg_plan_create_bounded", b_dev, c_dev, u_dev, x_dev, y_dev, z_dev,
                                     s_dev, pobj_dev, dobj_dev, status_dev, iters_dev, opts, stream);
}

int pycllp_hip_sparse_solve_bounded_hsd(pycllp_hip_sparse* h, long B, const double* b_dev, const double* c_dev, const double* u_dev,
                                        double* x_dev, double* y_dev, double* z_dev, double* s_dev, double* pobj_dev,
                                        double* dobj_dev, int* status_dev, int* iters_dev, const pycllp_hip_opts* opts, void* stream) {
    const int rc = check_restricted("pycllp_hip_sparse_solve_bounded_hsd", h, B, u_dev, opts, kWaveBoundedRejected & ~PYCLLP_FLAG_HSD,
                                    "PREDCORR, WARM_START, WAVE_KERNEL, BLOCK_KERNEL, NO_SLACK_PATH and FORCE_GUARD_PATH are not "
                                    "available with upper bounds on the self-dual embedding", b_dev && c_dev && x_dev && status_dev);
    if (rc != 0) return rc;
    pycllp_hip_opts ho;     // PYCLLP_FLAG_HSD is implied: max_refine AUTO resolves to the embedding's 20 passes
    pycllp_hip_default_opts(&ho);
    if (opts) ho = *opts;
    ho.flags |= PYCLLP_FLAG_HSD;
    return sparse_solve_bounded_impl("pycllp_hip_sparse_solve_bounded_hsd", h, B, nullptr, &h->lazy[LAZY_BD],
                                     wreg_plan_create_bounded, "wreg_plan_create_bounded", b_dev, c_dev, u_dev, x_dev, y_dev, z_dev,
                                     s_dev, pobj_dev, dobj_dev, status_dev, iters_dev, &ho, stream, true);
}

int pycllp_hip_sparse_solve_batch_bounded(pycllp_hip_sparse* h, long B, const double* Adata_dev, const double* b_dev,
                                          const double* c_dev, const double* u_dev, double* x_dev, double* y_dev, double* z_dev,
                                          double* s_dev, double* pobj_dev, double* dobj_dev, int* status_dev, int* iters_dev,
                                          const pycllp_hip_opts* opts, void* stream) {
    const int rc = check_restricted("pycllp_hip_sparse_solve_batch_bounded", h, B, Adata_dev && u_dev, opts, kWaveBoundedRejected,
                                    "HSD, PREDCORR, WARM_START, WAVE_KERNEL, BLOCK_KERNEL, NO_SLACK_PATH and FORCE_GUARD_PATH are "
                                    "not available with upper bounds on per-problem matrices",
                                    b_dev && c_dev && x_dev && status_dev);
    if (rc != 0) return rc;
    return sparse_solve_bounded_impl("pycllp_hip_sparse_solve_batch_bounded", h, B, Adata_dev, &h->lazy[LAZY_BDPA],
                                     wreg_plan_create_bounded_pa, "wreg_plan_create_bounded_pa", b_dev, c_dev, u_dev, x_dev, y_dev,
                                     z_dev, s_dev, pobj_dev, dobj_dev, status_dev, iters_dev, opts, stream);
}

int pycllp_hip_sparse_newton(pycllp_hip_sparse* h, long B, const double* x_dev, const double* z_dev, const double* y_dev,
                             const double* b_dev, const double* c_dev, double mu, double* dy_dev, int* nrefine_dev,
                             const pycllp_hip_opts* opts, void* stream) {
    if (!h || B < 0) return set_err(PYCLLP_E_BADARG, "pycllp_hip_sparse_newton: bad argument");
    if (B == 0) return 0;
    if (!x_dev || !z_dev || !y_dev || !b_dev || !c_dev || !dy_dev)
        return set_err(PYCLLP_E_BADARG, "pycllp_hip_sparse_newton: bad argument");
    DevOpts o = to_dev(opts);
    hipStream_t st = (hipStream_t)stream;
    if (h->big) {
        int grid_b = 0;
        const hipError_t eb = h->ring.run(st, [&](int* qb) {
            return big_launch_newton(h->big, B, x_dev, z_dev, y_dev, b_dev, c_dev, mu, dy_dev, nrefine_dev, qb, o, h->num_cu, st,
                                     &grid_b);
        });
        record_launch(h, nullptr, grid_b);
        if (eb != hipSuccess) return set_err((int)eb, "ipm_big_kernel (Newton mode) launch");
        return 0;
    }
    if (h->wreg && !(o.flags & PYCLLP_FLAG_BLOCK_KERNEL)) {
        int grid_w = 0;
        hipError_t e = wreg_launch_newton(h->wreg, B, x_dev, z_dev, y_dev, b_dev, c_dev, mu, dy_dev, nrefine_dev, o, h->num_cu, st,
                                          &grid_w);
        record_launch(h, h->wreg, grid_w);
        if (e != hipSuccess) return set_err((int)e, "newton_wreg_kernel launch");
        return 0;
    }
    // matrices the wave kernel does not cover (dense, or tables larger than LDS): the block kernel in its Newton mode
    hipError_t e = block_set_lds(h->lds);
    if (e != hipSuccess) return set_err((int)e, "set_dyn_lds((const void*)ipm_block_kernel, h->lds)");
    const long blocks = block_plan(h->lds, h->num_cu, B);   // on every CU: Newton mode ignores reserve_cus (the solve does not)
    e = h->ring.run(st, [&](int* qhead) {
        return block_launch_newton(h->desc, blocks, h->lds, B, x_dev, z_dev, y_dev, b_dev, c_dev, mu, dy_dev, nrefine_dev, qhead, o, st);
    });
    record_launch(h, nullptr, (int)blocks, h->desc.a_in_lds, h->lds);
    if (e != hipSuccess) return set_err((int)e, "ipm_block_kernel (Newton mode) launch");
    return 0;
}

int pycllp_hip_sparse_launch_info(const pycllp_hip_sparse* h, int* grid, int* block, int* lds_bytes, int* kernel) {
    if (!h) return set_err(PYCLLP_E_BADARG, "pycllp_hip_sparse_launch_info: bad argument");
    std::lock_guard<std::mutex> g(h->info_mu);
    if (grid) *grid = h->grid;
    if (block) *block = h->last_plan ? wreg_block_threads(h->last_plan) : BLK_T;
    if (lds_bytes) *lds_bytes = h->last_plan ? wreg_lds_bytes(h->last_plan) : (h->last_lds ? h->last_lds : h->lds);
    if (kernel) *kernel = h->big ? (big_dense_mode(h->big) ? 4 : 3) : (h->last_plan ? wreg_variant(h->last_plan) : 0);
    return 0;
}

int pycllp_hip_sparse_variant_info(const pycllp_hip_sparse* h, int* mb, int* nq) {
    if (!h) return set_err(PYCLLP_E_BADARG, "pycllp_hip_sparse_variant_info: bad argument");
    std::lock_guard<std::mutex> g(h->info_mu);
    wreg_shape(h->last_plan, mb, nq);
    return 0;
}

int pycllp_hip_sparse_plan_info(const pycllp_hip_sparse* h, int* wgpc, int* bnc, int* factor_in_lds, int* a_in_lds) {
    if (!h) return set_err(PYCLLP_E_BADARG, "pycllp_hip_sparse_plan_info: bad argument");
    std::lock_guard<std::mutex> g(h->info_mu);
    big_shape(h->big, wgpc, bnc, factor_in_lds);
    if (a_in_lds) *a_in_lds = h->last_a_in_lds;
    return 0;
}

void pycllp_hip_sparse_free(pycllp_hip_sparse* h) {
    if (!h) return;
    if (h->dev_blob) (void)hipFree(h->dev_blob);
    h->ring.destroy();
    wreg_plan_free(h->wreg);
    for (const LazyPlan& lp : h->lazy) wreg_plan_free(lp.plan);
    big_plan_free(h->big);
    delete h;
}

int pycllp_hip_sparse_max_rows(void) { return BIG_MAX_M; }
int pycllp_hip_sparse_max_cols(void) { return BIG_MAX_N; }

int pycllp_hip_ldl(int n, long B, const double* A_dev, double* L_dev, double* D_dev, int modified, double beta,
                   double delta, void* stream) {
    if (n <= 0 || B < 0) return set_err(PYCLLP_E_BADARG, "pycllp_hip_ldl: bad argument");
    if (B == 0) return 0;
    if (!A_dev || !L_dev || !D_dev) return set_err(PYCLLP_E_BADARG, "pycllp_hip_ldl: bad argument");
    if (n > LDL_MAX_N) return pycllp_exceeds_error("pycllp_hip_ldl", 0, n, 0, LDL_MAX_N);
    if (modified && !(beta > 0.0)) return set_err(PYCLLP_E_BADARG, "pycllp_hip_ldl: beta must be positive");
    const char* what;
    const hipError_t e = ldl_launch_factor(n, B, A_dev, L_dev, D_dev, modified, beta, delta, (hipStream_t)stream, &what);
    if (e != hipSuccess) return set_err((int)e, what);
    return 0;
}

int pycllp_hip_ldl_solve(int n, long B, const double* A_dev, const double* rhs_dev, double* x_dev, int modified, double beta,
                         double delta, void* stream) {
    if (n <= 0 || B < 0) return set_err(PYCLLP_E_BADARG, "pycllp_hip_ldl_solve: bad argument");
    if (B == 0) return 0;
    if (!A_dev || !rhs_dev || !x_dev) return set_err(PYCLLP_E_BADARG, "pycllp_hip_ldl_solve: bad argument");
    if (n > LDL_MAX_N) return pycllp_exceeds_error("pycllp_hip_ldl_solve", 0, n, 0, LDL_MAX_N);
    if (modified && !(beta > 0.0)) return set_err(PYCLLP_E_BADARG, "pycllp_hip_ldl_solve: beta must be positive");
    hipStream_t st = (hipStream_t)stream;
    if (!modified) {
        int dev = 0, ncu = 256;
        if (hipGetDevice(&dev) == hipSuccess) (void)hipDeviceGetAttribute(&ncu, hipDeviceAttributeMultiprocessorCount, dev);
        hipError_t e = wreg_launch_ldl_solve(n, B, A_dev, rhs_dev, x_dev, 0.0, ncu, st);
        if (e != hipSuccess) return set_err((int)e, "ldl_solve_wreg_kernel launch");
        return 0;
    }
    const char* what;
    const hipError_t e = ldl_launch_solve(n, B, A_dev, rhs_dev, x_dev, modified, beta, delta, st, &what);
    if (e != hipSuccess) return set_err((int)e, what);
    return 0;
}

int pycllp_hip_forward_backward_ldl(int n, long B, const double* L_dev, const double* D_dev, const double* b_dev, double* x_dev,
                                    void* stream) {
    if (n <= 0 || B < 0) return set_err(PYCLLP_E_BADARG, "pycllp_hip_forward_backward_ldl: bad argument");
    if (B == 0) return 0;
    if (!L_dev || !D_dev || !b_dev || !x_dev) return set_err(PYCLLP_E_BADARG, "pycllp_hip_forward_backward_ldl: bad argument");
    if (n > LDL_MAX_N) return pycllp_exceeds_error("pycllp_hip_forward_backward_ldl", 0, n, 0, LDL_MAX_N);
    const char* what;
    const hipError_t e = ldl_launch_forward_backward(n, B, L_dev, D_dev, b_dev, x_dev, (hipStream_t)stream, &what);
    if (e != hipSuccess) return set_err((int)e, what);
    return 0;
}

}  // extern "C"

// Not part of the public ABI (absent from include/pycllp_hip.h): the plan a creator would build for the matrix given as HOST CSR
// arrays, with no HIP call and nothing uploaded.  kind: 0 the block kernel's plan; 1 .. 6 the wave kernel's creators (wreg_plan_create,
// the same with pa, _bounded, _bounded_pa, _dense_pa without and with keep_tail); 7 the large-LP kernel's; 8 the wave kernel's
// _bounded_dense_pa (the later creator takes the next free number: 0 .. 7 keep their meaning).  Returns the creator's
// code (the block plan: BLOCK_PLAN_*) and, where it is 0, scalars[PLAN_NSCALARS] and the digest as the plan's header documents them.
extern "C" int pycllp_hip_debug_plan(int kind, int m, int n, int nnz, const double* val, const int* ptr, const int* col, int max_lds,
                                     long long* scalars, unsigned long long* digest) {
    if (kind < 0 || kind > 8 || m < 0 || n < 0 || nnz < 0 || !ptr || !scalars || !digest || (nnz > 0 && (!val || !col))) return -1;
    memset(scalars, 0, sizeof(long long) * PLAN_NSCALARS);
    *digest = 0;
    int rc;
    if (kind == 0) {
        BlockHostPlan P;
        if ((rc = block_host_plan(m, n, nnz, val, ptr, col, max_lds, P)) == 0) *digest = block_plan_report(P, scalars);
    } else if (kind == 7) {
        BigHostPlan P;
        if ((rc = big_host_plan(m, n, nnz, val, ptr, col, max_lds, P)) == 0) *digest = big_plan_report(P, scalars);
    } else {
        WregHostPlan P;
        const WregPlanKind wk = kind == 8 ? WPLAN_BOUNDED_DENSE_PA : (WregPlanKind)(kind - 1);
        if ((rc = wreg_plan_host(wk, m, n, nnz, val, ptr, col, max_lds, &P)) == 0) *digest = wreg_plan_report(P, scalars);
    }
    return rc;
}
