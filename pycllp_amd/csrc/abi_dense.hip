// abi_dense.hip -- the C ABI of the dense handle (include/pycllp_hip.h: pycllp_hip_dense_*).  Host code only: the lane-group
// kernels are reached through the tables of dense_tab.h (ipm_dense.hip) and group_pa.h (ipm_group_pa.hip, ipm_group_pabd.hip, ipm_group_pabdh.hip);
// a matrix beyond them (m > 32 or n > 128) gets a sparse handle, whose entries and bodies are abi_sparse.hip's (host.h).
#include "dense_tab.h"

static void publish(pycllp_hip_dense* h, const LaunchPlan& p, bool full = false) {
    std::lock_guard<std::mutex> g(h->info_mu);
    h->grid = p.grid; h->block = p.block; h->lds = p.lds; h->mp = p.mp; h->np = p.np; h->sl = p.sl; h->full = full ? 1 : 0;
}

// Plans k for a.B LPs, launches it on a queue-ring slot (a.queue) and publishes the plan for launch_info.  full: k.launch is a
// full-shape instantiation
static hipError_t run_group(pycllp_hip_dense* h, const DenseKernel& k, GroupPaArgs a, const DevOpts& o, hipStream_t st,
                            bool full = false) {
    const LaunchPlan p = k.plan(h->lim, a.B, o);
    return h->ring.run(st, [&](int* qhead) {
        a.queue = qhead;
        const hipError_t el = k.launch(a, p, o, st);
        publish(h, p, full);
        return el;
    });
}

// the row of a per-problem-A table (PaPlans, GroupPaVariants) for (mp, np, sl) -- never by position --, or null
template <typename Table>
static auto find_pa(const Table& t, int mp, int np, bool sl) -> decltype(t.v) {
    for (int i = 0; i < t.n; i++)
        if (t.v[i].mp == mp && t.v[i].np == np && t.v[i].sl == (sl ? 1 : 0)) return &t.v[i];
    return nullptr;
}

// The body of pycllp_hip_dense_solve_batch and, with u_dev, of pycllp_hip_dense_solve_batch_bounded and (hsd: on the
// self-dual embedding, kGroupPABDH on the plans of kPaBdPlans) of pycllp_hip_dense_solve_batch_bounded_hsd, behind their argument
// checks and their look at the handle.  sl: the matrices come without the identity tail (the slack-aware kernels).
static int dense_solve_batch_impl(const char* entry, pycllp_hip_dense* h, long B, bool sl, const double* A_dev, long a_cols,
                                  const double* b_dev, const double* c_dev, const double* u_dev, double* x_dev, double* y_dev,
                                  double* z_dev, double* s_dev, double* pobj_dev, double* dobj_dev, int* status_dev, int* iters_dev,
                                  const pycllp_hip_opts* opts, void* stream, bool hsd = false) {
    const bool bd = u_dev != nullptr;
    if (a_cols != (long)(sl ? h->n - h->m : h->n)) return pycllp_a_cols_error(entry, a_cols, sl ? h->n - h->m : h->n, sl);
    const int mp = sl ? kSlackVariants[h->variant_sl].mp : kVariants[h->variant].mp;
    const int np = sl ? kSlackVariants[h->variant_sl].np : kVariants[h->variant].np;
    const PaPlan* pp = find_pa(bd ? kPaBdPlans : kPaPlans, mp, np, sl);
    const GroupPaVariant* pv = find_pa(hsd ? kGroupPABDH : (bd ? kGroupPABD : kGroupPA), mp, np, sl);
    if (!pp || !pv || !pv->launch) return entry_err(PYCLLP_E_UNSUPPORTED, entry, "no kernel of this shape was compiled");
    if (B == 0) return 0;
    DevOpts o = to_dev(opts);
    hipStream_t st = (hipStream_t)stream;
    const LaunchPlan p = pp->plan(h->lim, B, o);
    const hipError_t e = h->ring.run(st, [&](int* qhead) {
        const GroupPaArgs a = {h->m, h->n, B, A_dev, b_dev, c_dev, u_dev, x_dev, y_dev, z_dev, s_dev, pobj_dev, dobj_dev,
                               status_dev, iters_dev, qhead};
        const hipError_t el = pv->launch(a, p.grid, p.block, p.lds, o, st);
        publish(h, p);
        return el;
    });
    if (e != hipSuccess)
        return set_err((int)e, hsd ? "bounded per-problem self-dual solve kernel launch"
                                   : (bd ? "bounded per-problem solve kernel launch" : "per-problem solve kernel launch"));
    return 0;
}

extern "C" {

int pycllp_hip_dense_max_rows(void) { return BIG_MAX_M; }   // m <= 32, n <= 128: lane-group kernels; beyond: the sparse path's kernels
int pycllp_hip_dense_max_cols(void) { return BIG_MAX_N; }

int pycllp_hip_dense_init(int m, int n, const double* A_dev, void* stream, pycllp_hip_dense** handle) {
    if (!A_dev || !handle || m <= 0 || n <= 0) return set_err(PYCLLP_E_BADARG, "pycllp_hip_dense_init: bad argument");
    int vi = -1;
    for (int i = 0; i < kNumVariants; i++)
        if (m <= kVariants[i].mp && n <= kVariants[i].np) { vi = i; break; }
    if (vi < 0) {
        // Beyond the lane-group kernels (m <= 32, n <= 128).  The reference's dense host has no size limit
        // (pycllp/solvers/cl.py:28-83; its own kernel test runs m = 100, N = 180): up to m = 256, n = 1280 the LP is handed
        // to the kernels of the sparse path -- the structural non-zeros of the dense A become its CSR arrays (m <= 128,
        // n <= 512: the wavefront-per-LP kernel on a dense image; beyond: the workgroup-per-LP kernel of ipm_big.hip).
        if (m > BIG_MAX_M || n > BIG_MAX_N) return pycllp_exceeds_error("pycllp_hip_dense_init", m, n, BIG_MAX_M, BIG_MAX_N);
        hipStream_t st = (hipStream_t)stream;
        std::vector<double> Ah((size_t)m * n);
        HIP_TRY(hipMemcpyAsync(Ah.data(), A_dev, sizeof(double) * (size_t)m * n, hipMemcpyDeviceToHost, st));
        HIP_TRY(hipStreamSynchronize(st));
        std::vector<double> val; std::vector<int> ptr(m + 1, 0), col;
        for (int i = 0; i < m; i++) {
            for (int j = 0; j < n; j++) if (Ah[(size_t)i * n + j] != 0.0) { val.push_back(Ah[(size_t)i * n + j]); col.push_back(j); }
            ptr[i + 1] = (int)val.size();
        }
        if (val.empty()) return set_err(PYCLLP_E_BADARG, "pycllp_hip_dense_init: A is all zero");
        pycllp_hip_sparse* sp = nullptr;
        const int rc = sparse_init_host(m, n, (int)val.size(), val, ptr, col, stream, &sp);
        if (rc != 0) return rc;
        pycllp_hip_dense* hs = new (std::nothrow) pycllp_hip_dense();
        if (!hs) { pycllp_hip_sparse_free(sp); return set_err(PYCLLP_E_NOMEM, "pycllp_hip_dense_init: out of host memory"); }
        hs->m = m; hs->n = n; hs->variant = -1; hs->variant_sl = -1; hs->sp = sp;
        *handle = hs;
        return 0;
    }
    pycllp_hip_dense* h = new (std::nothrow) pycllp_hip_dense();
    if (!h) return set_err(PYCLLP_E_NOMEM, "pycllp_hip_dense_init: out of host memory");
    h->m = m; h->n = n; h->variant = vi; h->mp = kVariants[vi].mp; h->np = kVariants[vi].np;
    // on failure the partly built handle goes through pycllp_hip_dense_free, which skips what was not made
    hipError_t e = device_limits(&h->lim);
    if (e != hipSuccess) { pycllp_hip_dense_free(h); return set_err((int)e, "hipGetDeviceProperties"); }
    e = hipMalloc((void**)&h->pack, sizeof(double) * kVariants[vi].apack);
    if (e != hipSuccess) { pycllp_hip_dense_free(h); return set_err((int)e, "hipMalloc(pack)"); }
    e = hipMalloc((void**)&h->a_rm, sizeof(double) * (size_t)m * n);
    if (e != hipSuccess) { pycllp_hip_dense_free(h); return set_err((int)e, "hipMalloc(A)"); }
    e = h->ring.create();
    if (e != hipSuccess) { pycllp_hip_dense_free(h); return set_err((int)e, "hipMalloc(queue)"); }
    hipStream_t st = (hipStream_t)stream;
    e = hipMemcpyAsync(h->a_rm, A_dev, sizeof(double) * (size_t)m * n, hipMemcpyDeviceToDevice, st);
    if (e == hipSuccess) e = kVariants[vi].pack(m, n, A_dev, h->pack, st);
    // is A = [A_dense | I_m]?  (equality form of a StandardLP, pycllp/lp.py:551-567)
    h->variant_sl = -1;
    if (e == hipSuccess && n > m) {
        std::vector<double> Ah((size_t)m * n);
        e = hipMemcpyAsync(Ah.data(), A_dev, sizeof(double) * (size_t)m * n, hipMemcpyDeviceToHost, st);
        if (e == hipSuccess) e = hipStreamSynchronize(st);
        if (e == hipSuccess) {
            bool ident = true;
            for (int i = 0; i < m && ident; i++)
                for (int k = 0; k < m; k++)
                    if (Ah[(size_t)i * n + (n - m) + k] != (i == k ? 1.0 : 0.0)) { ident = false; break; }
            if (ident)
                for (int i = 0; i < kNumSlackVariants; i++)
                    if (m <= kSlackVariants[i].mp && n - m <= kSlackVariants[i].np - kSlackVariants[i].mp) { h->variant_sl = i; break; }
        }
    }
    if (e == hipSuccess) e = hipStreamSynchronize(st);
    if (e != hipSuccess) { pycllp_hip_dense_free(h); return set_err((int)e, "pack_A_kernel"); }
    // the images of an LP's first Gram pass: the general variant's and, for [A_dense | I], the slack-aware variant's
    const FirstGram& fg = kVariants[vi].first;
    const int sl_len = h->variant_sl >= 0 ? kSlackVariants[h->variant_sl].first.len : 0;
    if (fg.len + sl_len > 0) {
        e = hipMalloc((void**)&h->first, sizeof(double) * (size_t)(fg.len + sl_len));
        if (e != hipSuccess) { pycllp_hip_dense_free(h); return set_err((int)e, "hipMalloc(first Gram image)"); }
        if (fg.len > 0) {
            h->first_gen = h->first;
            e = fg.launch(m, n, h->a_rm, h->first_gen, st);
        }
        if (e == hipSuccess && sl_len > 0) {
            h->first_sl = h->first + fg.len;
            e = kSlackVariants[h->variant_sl].first.launch(m, n, h->a_rm, h->first_sl, st);
        }
        if (e == hipSuccess) e = hipStreamSynchronize(st);
        if (e != hipSuccess) { pycllp_hip_dense_free(h); return set_err((int)e, "first_gram_kernel"); }
    }
    *handle = h;
    return 0;
}

int pycllp_hip_dense_solve(pycllp_hip_dense* h, long B, const double* b_dev, const double* c_dev, double* x_dev,
                           double* y_dev, double* z_dev, double* pobj_dev, double* dobj_dev, int* status_dev,
                           int* iters_dev, const pycllp_hip_opts* opts, void* stream) {
    if (!h || B < 0) return set_err(PYCLLP_E_BADARG, "pycllp_hip_dense_solve: bad argument");
    if (both_autoscales(opts)) return entry_err(PYCLLP_E_BADARG, "pycllp_hip_dense_solve", kBothAutoscales);
    if (B == 0) return 0;  // empty batch: nothing to do (pointers may be NULL)
    if (!b_dev || !c_dev || !x_dev || !status_dev)
        return set_err(PYCLLP_E_BADARG, "pycllp_hip_dense_solve: bad argument");
    if (h->sp) {   // beyond the lane-group kernels: the sparse path's kernels (flags that select lane-group variants do not apply)
        pycllp_hip_opts so;
        pycllp_hip_default_opts(&so);
        if (opts) so = *opts;
        if (so.flags & PYCLLP_FLAG_WAVE_KERNEL)
            return set_err(PYCLLP_E_BADARG, "pycllp_hip_dense_solve: PYCLLP_FLAG_WAVE_KERNEL is not available beyond m = 32, n = 128");
        so.flags &= ~PYCLLP_FLAG_NO_SLACK_PATH;
        return pycllp_hip_sparse_solve(h->sp, B, b_dev, c_dev, x_dev, y_dev, z_dev, pobj_dev, dobj_dev, status_dev, iters_dev, &so, stream);
    }
    DevOpts o = to_dev(opts);
    if ((o.flags & PYCLLP_FLAG_WARM_START) && (!y_dev || !z_dev))
        return set_err(PYCLLP_E_BADARG, "pycllp_hip_dense_solve: warm start needs y_dev and z_dev");
    if ((o.flags & PYCLLP_AUTOSCALE_ANY) && (o.flags & PYCLLP_FLAG_WAVE_KERNEL))
        return set_err(PYCLLP_E_BADARG, "pycllp_hip_dense_solve: PYCLLP_FLAG_AUTOSCALE (and _PER_LP) is not available with PYCLLP_FLAG_WAVE_KERNEL");
    if ((o.flags & PYCLLP_FLAG_HSD) && (o.flags & PYCLLP_FLAG_WAVE_KERNEL))
        return set_err(PYCLLP_E_BADARG, "pycllp_hip_dense_solve: PYCLLP_FLAG_HSD is not available with PYCLLP_FLAG_WAVE_KERNEL");
    if ((o.flags & PYCLLP_FLAG_PREDCORR) && (o.flags & (PYCLLP_FLAG_HSD | PYCLLP_FLAG_WAVE_KERNEL)))
        return set_err(PYCLLP_E_BADARG, "pycllp_hip_dense_solve: PYCLLP_FLAG_PREDCORR is an option of the reference's path (not with PYCLLP_FLAG_HSD)");
    if (o.flags & PYCLLP_FLAG_WAVE_KERNEL)
        return set_err(PYCLLP_E_UNSUPPORTED, "pycllp_hip_dense_solve: the first-generation kernel (PYCLLP_FLAG_WAVE_KERNEL) has been removed");
    const Variant& v = kVariants[h->variant];
    const bool hsd = (o.flags & PYCLLP_FLAG_HSD) != 0, pc = (o.flags & PYCLLP_FLAG_PREDCORR) != 0;
    DenseKernel k = hsd ? v.solve_hsd : (pc ? v.solve_pc : v.solve_group);
    bool full = false;
    const double* first = h->first_gen;
    if (h->variant_sl >= 0 && !(o.flags & PYCLLP_FLAG_NO_SLACK_PATH)) {
        first = h->first_sl;
        const SlackVariant& s = kSlackVariants[h->variant_sl];
        k = hsd ? s.solve_hsd : (pc ? s.solve_pc : s.solve_group);
        // an LP that fills the shape exactly goes to its full-shape instantiation, on the same plan
        const dense_launch_fn f = (hsd || pc) ? nullptr : s.full_group;
        if (f && h->m == s.mp && h->n == s.np && !(o.flags & PYCLLP_FLAG_GENERIC_SHAPE)) { k.launch = f; full = true; }
    }
    // a warm start does not begin at x = z = 1, and the diagnostic flag asks for the product itself (the HSD kernel has no such path)
    if (o.flags & (PYCLLP_FLAG_WARM_START | PYCLLP_FLAG_PER_LP_FIRST_GRAM)) first = nullptr;
    const GroupPaArgs a = {h->m, h->n, B, h->a_rm, b_dev, c_dev, nullptr, x_dev, y_dev, z_dev, nullptr, pobj_dev, dobj_dev,
                           status_dev, iters_dev, nullptr, first};
    hipError_t e = run_group(h, k, a, o, (hipStream_t)stream, full);
    if (e != hipSuccess) return set_err((int)e, "solve kernel launch");
    return 0;
}

int pycllp_hip_dense_solve_bounded(pycllp_hip_dense* h, long B, const double* b_dev, const double* c_dev, const double* u_dev,
                                   double* x_dev, double* y_dev, double* z_dev, double* s_dev, double* pobj_dev, double* dobj_dev,
                                   int* status_dev, int* iters_dev, const pycllp_hip_opts* opts, void* stream) {
    const int rc = check_restricted("pycllp_hip_dense_solve_bounded", h, B, u_dev, opts, kBoundedRejected,
                                    "HSD, PREDCORR, WARM_START, WAVE_KERNEL and NO_SLACK_PATH are not available with upper bounds",
                                    b_dev && c_dev && x_dev && status_dev);
    if (rc != 0) return rc;
    if (h->sp || h->variant_sl < 0)
        return set_err(PYCLLP_E_UNSUPPORTED, "pycllp_hip_dense_solve_bounded: A is not [A_dense | I] with m <= 32 and at most 96 "
                                             "dense columns (48 when m <= 16 on the 16-row kernels)");
    if (B == 0) return 0;
    DevOpts o = to_dev(opts);
    const GroupPaArgs a = {h->m, h->n, B, h->a_rm, b_dev, c_dev, u_dev, x_dev, y_dev, z_dev, s_dev, pobj_dev, dobj_dev,
                           status_dev, iters_dev, nullptr};
    hipError_t e = run_group(h, kSlackVariants[h->variant_sl].solve_bounded, a, o, (hipStream_t)stream);
    if (e != hipSuccess) return set_err((int)e, "bounded solve kernel launch");
    return 0;
}

int pycllp_hip_dense_solve_bounded_hsd(pycllp_hip_dense* h, long B, const double* b_dev, const double* c_dev, const double* u_dev,
                                       double* x_dev, double* y_dev, double* z_dev, double* s_dev, double* pobj_dev,
                                       double* dobj_dev, int* status_dev, int* iters_dev, const pycllp_hip_opts* opts, void* stream) {
    const int rc = check_restricted("pycllp_hip_dense_solve_bounded_hsd", h, B, u_dev, opts, kBoundedRejected & ~PYCLLP_FLAG_HSD,
                                    "PREDCORR, WARM_START, WAVE_KERNEL and NO_SLACK_PATH are not available with upper bounds on "
                                    "the self-dual embedding", b_dev && c_dev && x_dev && status_dev);
    if (rc != 0) return rc;
    if (h->sp || h->variant_sl < 0)
        return set_err(PYCLLP_E_UNSUPPORTED, "pycllp_hip_dense_solve_bounded_hsd: A is not [A_dense | I] with m <= 32 and at most "
                                             "96 dense columns (48 when m <= 16 on the 16-row kernels)");
    const DenseKernel& k = kSlackVariants[h->variant_sl].solve_bounded_hsd;
    if (!k.launch)
        return set_err(PYCLLP_E_UNSUPPORTED, "pycllp_hip_dense_solve_bounded_hsd: no kernel of this shape was compiled");
    if (B == 0) return 0;
    pycllp_hip_opts ho;     // PYCLLP_FLAG_HSD is implied: max_refine AUTO resolves to the embedding's 20 passes
    pycllp_hip_default_opts(&ho);
    if (opts) ho = *opts;
    ho.flags |= PYCLLP_FLAG_HSD;
    DevOpts o = to_dev(&ho);
    const GroupPaArgs a = {h->m, h->n, B, h->a_rm, b_dev, c_dev, u_dev, x_dev, y_dev, z_dev, s_dev, pobj_dev, dobj_dev,
                           status_dev, iters_dev, nullptr};
    hipError_t e = run_group(h, k, a, o, (hipStream_t)stream);
    if (e != hipSuccess) return set_err((int)e, "bounded self-dual solve kernel launch");
    return 0;
}

int pycllp_hip_dense_solve_batch(pycllp_hip_dense* h, long B, const double* A_dev, long a_cols, const double* b_dev,
                                 const double* c_dev, double* x_dev, double* y_dev, double* z_dev, double* pobj_dev, double* dobj_dev,
                                 int* status_dev, int* iters_dev, const pycllp_hip_opts* opts, void* stream) {
    const int rc = check_restricted("pycllp_hip_dense_solve_batch", h, B, true, opts, kBoundedRejected & ~PYCLLP_FLAG_NO_SLACK_PATH,
                                    "HSD, PREDCORR, WARM_START and WAVE_KERNEL are not available with per-problem matrices",
                                    A_dev && b_dev && c_dev && x_dev && status_dev);
    if (rc != 0) return rc;
    if (h->sp)      // beyond the lane-group kernels: the wave kernel with an image per wave, where a variant and an LDS plan cover the LP
        return dense_solve_batch_wave(h->sp, B, A_dev, a_cols, b_dev, c_dev, x_dev, y_dev, z_dev, pobj_dev, dobj_dev, status_dev,
                                      iters_dev, opts, stream);
    const bool sl = h->variant_sl >= 0 && !((opts ? opts->flags : 0) & PYCLLP_FLAG_NO_SLACK_PATH);
    return dense_solve_batch_impl("pycllp_hip_dense_solve_batch", h, B, sl, A_dev, a_cols, b_dev, c_dev, nullptr, x_dev, y_dev,
                                  z_dev, nullptr, pobj_dev, dobj_dev, status_dev, iters_dev, opts, stream);
}

int pycllp_hip_dense_solve_batch_bounded(pycllp_hip_dense* h, long B, const double* A_dev, long a_cols, const double* b_dev,
                                         const double* c_dev, const double* u_dev, double* x_dev, double* y_dev, double* z_dev,
                                         double* s_dev, double* pobj_dev, double* dobj_dev, int* status_dev, int* iters_dev,
                                         const pycllp_hip_opts* opts, void* stream) {
    const int rc = check_restricted("pycllp_hip_dense_solve_batch_bounded", h, B, u_dev, opts, kBoundedRejected,
                                    "HSD, PREDCORR, WARM_START, WAVE_KERNEL and NO_SLACK_PATH are not available with upper bounds "
                                    "on per-problem matrices", A_dev && b_dev && c_dev && x_dev && status_dev);
    if (rc != 0) return rc;
    if (h->sp)      // beyond the lane-group kernels: the bounded wave kernel with an image per wave, where a variant and an LDS plan cover the LP
        return dense_solve_batch_bounded_wave(h->sp, B, A_dev, a_cols, b_dev, c_dev, u_dev, x_dev, y_dev, z_dev, s_dev, pobj_dev,
                                              dobj_dev, status_dev, iters_dev, opts, stream);
    if (h->variant_sl < 0)
        return set_err(PYCLLP_E_UNSUPPORTED, "pycllp_hip_dense_solve_batch_bounded: A is not [A_dense | I] with m <= 32 and at most "
                                             "96 dense columns (48 when m <= 16 on the 16-row kernels)");
    return dense_solve_batch_impl("pycllp_hip_dense_solve_batch_bounded", h, B, true, A_dev, a_cols, b_dev, c_dev, u_dev, x_dev,
                                  y_dev, z_dev, s_dev, pobj_dev, dobj_dev, status_dev, iters_dev, opts, stream);
}

int pycllp_hip_dense_solve_batch_bounded_hsd(pycllp_hip_dense* h, long B, const double* A_dev, long a_cols, const double* b_dev,
                                             const double* c_dev, const double* u_dev, double* x_dev, double* y_dev, double* z_dev,
                                             double* s_dev, double* pobj_dev, double* dobj_dev, int* status_dev, int* iters_dev,
                                             const pycllp_hip_opts* opts, void* stream) {
    static const char* const entry = "pycllp_hip_dense_solve_batch_bounded_hsd";
    const int rc = check_restricted(entry, h, B, u_dev, opts, kBoundedRejected & ~PYCLLP_FLAG_HSD,
                                    "PREDCORR, WARM_START, WAVE_KERNEL and NO_SLACK_PATH are not available with upper bounds on "
                                    "per-problem matrices on the self-dual embedding",
                                    A_dev && b_dev && c_dev && x_dev && status_dev);
    if (rc != 0) return rc;
    if (h->sp)      // beyond the lane-group kernels: the wave kernel with an image per wave has no embedding
        return entry_err(PYCLLP_E_UNSUPPORTED, entry, "the self-dual embedding on per-problem matrices exists on the lane-group "
                                                      "kernels only (m <= 32, n <= 128)");
    if (h->variant_sl < 0)
        return entry_err(PYCLLP_E_UNSUPPORTED, entry, "A is not [A_dense | I] with m <= 32 and at most 96 dense columns (48 when "
                                                      "m <= 16 on the 16-row kernels)");
    pycllp_hip_opts ho;     // PYCLLP_FLAG_HSD is implied: max_refine AUTO resolves to the embedding's 20 passes
    pycllp_hip_default_opts(&ho);
    if (opts) ho = *opts;
    ho.flags |= PYCLLP_FLAG_HSD;
    return dense_solve_batch_impl(entry, h, B, true, A_dev, a_cols, b_dev, c_dev, u_dev, x_dev, y_dev, z_dev, s_dev, pobj_dev,
                                  dobj_dev, status_dev, iters_dev, &ho, stream, true);
}

int pycllp_hip_dense_newton(pycllp_hip_dense* h, long B, const double* x_dev, const double* z_dev,
                            const double* y_dev, const double* b_dev, const double* c_dev, double mu, double* dy_dev,
                            int* nrefine_dev, const pycllp_hip_opts* opts, void* stream) {
    if (!h || B < 0) return set_err(PYCLLP_E_BADARG, "pycllp_hip_dense_newton: bad argument");
    if (B == 0) return 0;
    if (!x_dev || !z_dev || !y_dev || !b_dev || !c_dev || !dy_dev)
        return set_err(PYCLLP_E_BADARG, "pycllp_hip_dense_newton: bad argument");
    if (h->sp) return pycllp_hip_sparse_newton(h->sp, B, x_dev, z_dev, y_dev, b_dev, c_dev, mu, dy_dev, nrefine_dev, opts, stream);
    DevOpts o = to_dev(opts);
    const Variant& v = kVariants[h->variant];
    const LaunchPlan p = v.newton_plan(h->lim, B, o);
    const NewtonArgs a = {h->m, h->n, B, h->pack, x_dev, z_dev, y_dev, b_dev, c_dev, mu, dy_dev, nrefine_dev};
    hipError_t e = v.newton(a, p, o, (hipStream_t)stream);
    publish(h, p);
    if (e != hipSuccess) return set_err((int)e, "newton_kernel launch");
    return 0;
}

int pycllp_hip_dense_launch_info(const pycllp_hip_dense* h, int* grid, int* block, int* lds_bytes, int* m_pad,
                                 int* n_pad) {
    if (!h) return set_err(PYCLLP_E_BADARG, "pycllp_hip_dense_launch_info: bad argument");
    if (h->sp) {
        int kern = 0;
        const int rc = pycllp_hip_sparse_launch_info(h->sp, grid, block, lds_bytes, &kern);
        if (m_pad) *m_pad = BLK_MAX_M;
        if (n_pad) *n_pad = BLK_MAX_N;
        return rc;
    }
    std::lock_guard<std::mutex> g(h->info_mu);
    if (grid) *grid = h->grid;
    if (block) *block = h->block;
    if (lds_bytes) *lds_bytes = h->lds;
    if (m_pad) *m_pad = h->mp;
    if (n_pad) *n_pad = h->np;
    return 0;
}

int pycllp_hip_dense_variant_info(const pycllp_hip_dense* h, int* a, int* b, int* slack) {
    if (!h) return set_err(PYCLLP_E_BADARG, "pycllp_hip_dense_variant_info: bad argument");
    if (h->sp) {
        if (slack) *slack = -1;
        return pycllp_hip_sparse_variant_info(h->sp, a, b);
    }
    std::lock_guard<std::mutex> g(h->info_mu);
    const bool ran = h->sl >= 0;
    if (a) *a = ran ? h->mp : 0;
    if (b) *b = ran ? h->np : 0;
    if (slack) *slack = ran ? h->sl : 0;
    return 0;
}

int pycllp_hip_dense_full_shape(const pycllp_hip_dense* h) {
    if (!h || h->sp) return 0;
    std::lock_guard<std::mutex> g(h->info_mu);
    return h->full;
}

int pycllp_hip_dense_plan_info(const pycllp_hip_dense* h, int* wgpc, int* bnc, int* factor_in_lds, int* a_in_lds) {
    if (!h) return set_err(PYCLLP_E_BADARG, "pycllp_hip_dense_plan_info: bad argument");
    if (h->sp) return pycllp_hip_sparse_plan_info(h->sp, wgpc, bnc, factor_in_lds, a_in_lds);
    if (wgpc) *wgpc = 0;
    if (bnc) *bnc = 0;
    if (factor_in_lds) *factor_in_lds = -1;
    if (a_in_lds) *a_in_lds = -1;
    return 0;
}

int pycllp_hip_dense_kernel_kind(const pycllp_hip_dense* h) {
    if (!h || !h->sp) return -1;
    int kern = 0;
    if (pycllp_hip_sparse_launch_info(h->sp, nullptr, nullptr, nullptr, &kern) != 0) return -1;
    return kern;
}

void pycllp_hip_dense_free(pycllp_hip_dense* h) {
    if (!h) return;
    if (h->sp) pycllp_hip_sparse_free(h->sp);
    if (h->pack) (void)hipFree(h->pack);
    if (h->a_rm) (void)hipFree(h->a_rm);
    if (h->first) (void)hipFree(h->first);
    h->ring.destroy();
    delete h;
}

}  // extern "C"
