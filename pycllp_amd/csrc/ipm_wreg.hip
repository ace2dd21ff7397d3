// ipm_wreg.hip -- host side of the register-resident one-LP-per-wavefront kernels (wreg_wave.h): the plan of one constraint
// matrix (term tables or dense image, LDS layout: built by wreg_plan.h, uploaded here), the choice of a launcher from the tables of the kernel units
// (ipm_wreg_{tab,da,pa,dapa,pc,pcda,pcpa,bd,bdpa,bddapa}.hip), grid sizing and the wreg_launch_* entry points of wreg.h.  The only kernels
// compiled here are the two that have no table: the stand-alone LDL' solve and the selftest of the cross-lane primitives.
#include "wreg_wave.h"
#include "wreg_plan.h"
#include "plan_upload.h"

namespace {

// ------------------------------------------------------------------------------------------------------------------
// stand-alone LDL' solve of explicit dense symmetric matrices: the register factor + block substitution on their own
// (pycllp/ldl.py:202-239 solve_ldl; also the bring-up check of factor()/solve())
// ------------------------------------------------------------------------------------------------------------------
template <int MB>
__global__ void __launch_bounds__(256, 1)
ldl_solve_wreg_kernel(int n, long B, const double* __restrict__ Ag, const double* __restrict__ rhs, double* __restrict__ out,
                      double floor_, int* __restrict__ queue) {
    using G = WGeo<MB>;
    constexpr int MP = G::MP;
    extern __shared__ __attribute__((aligned(16))) unsigned char lraw[];
    WReg<MB, 1> w;
    USE_AGPR_FORM();
    const int tid = threadIdx.x;
    wreg_carve(w, (double*)lraw + (size_t)(tid >> 6) * G::WAVE_D(1), tid);
    const int &lane = w.lane, &q = w.q, &c16 = w.c16;
    long mat = next_item(queue, lane);
    while (mat < B) {
        const double* A = Ag + mat * (long)n * n;
        // off-diagonal blocks: U[K][I] register r = M[i = 16I + c16][k = 16K + 4r + q] (i > k); padded rows are zero
        static_for<0, MB>([&](auto Kc) {
            constexpr int K = decltype(Kc)::value;
            static_for<K + 1, MB>([&](auto Ic) {
                constexpr int I = decltype(Ic)::value;
                double4_t blk;
#pragma unroll
                for (int r = 0; r < 4; r++) {
                    const int i = 16 * I + c16, k = 16 * K + 4 * r + q;
                    blk[r] = (i < n) ? A[(long)i * n + k] : 0.0;
                }
                park(w.P[G::bix(K, I)], blk);
            });
        });
        for (int i = lane; i < MP; i += 64) w.um_()[i] = (i < n) ? rhs[mat * n + i] : 0.0;
        // diagonal blocks into their slots: element [row][col], col <= row, of block K at K WL + row (row + 1) / 2 + col
        static_for<0, MB>([&](auto Kc) {
            constexpr int K = decltype(Kc)::value;
#pragma unroll
            for (int r = 0; r < 4; r++) {
                const int il = 4 * r + q, row = 16 * K + il, col = 16 * K + c16;
                if (c16 <= il) w.wl_()[K * WL + il * (il + 1) / 2 + c16] = (row < n) ? A[(long)row * n + col] : ((row == col) ? 1.0 : 0.0);
            }
        });
        wave_lds_sync();
        STAMP_DECL
        (void)w.template factor<false>(1e300, floor_ STAMP_PASS);
        w.solve();
        for (int i = lane; i < n; i += 64) out[mat * n + i] = w.um_()[i];
        wave_lds_sync();
        mat = next_item(queue, lane);
    }
}

// ---- selftest of the cross-lane primitives (bring-up aid) --------------------------------------------------------
__global__ void wreg_selftest_kernel(double* out) {
    const int lane = threadIdx.x & 63;
    const double v = 1.0 + lane;
    out[lane] = quad_sum(v);                 // expect sum over l' = l mod 16 + 16 k
    out[64 + lane] = row_sum(v);             // expect sum over the 16-lane row
    out[128 + lane] = wsum(v);               // expect 2080
    out[192 + lane] = row_bcast<5>(v);       // expect 1 + (lane & ~15) + 5
    // MFMA layout: A[m][k] = 100 m + k (k = 0..3), B[k][n] = (k == 1) ? n + 1 : 0  ->  C[m][n] = (100 m + 1)(n + 1)
    const int c16 = lane & 15, qd = lane >> 4;
    const double a = 100.0 * c16 + qd, b = (qd == 1) ? c16 + 1.0 : 0.0;
    double4_t acc = {0.0, 0.0, 0.0, 0.0};
    acc = __builtin_amdgcn_mfma_f64_16x16x4f64(a, b, acc, 0, 0, 0);
    for (int r = 0; r < 4; r++) out[256 + 64 * r + lane] = acc[r];   // expect (100 (4r + q) + 1)(c16 + 1)
    out[512 + lane] = wmax(v);               // expect 64
}

}  // namespace

// ------------------------------------------------------------------------------------------------------------------
// host side
// ------------------------------------------------------------------------------------------------------------------
struct WregPlan {
    WregTab tab;
    int mb, nq;
    bool da = false, pa = false;
    bool bd = false;      // the plan of the bounded kernel (wreg_plan_create_bounded): 2 NP more doubles per wave
    void* dev_blob;
};

// the launcher table of a plan's kind; pc: its predictor-corrector kernels (plans of the bounded kernel have none)
static const WVariants& table_of(bool da, bool pa, bool bd, bool pc = false) {
    static const WVariants none = { nullptr, 0 };
    if (da && pa) return pc ? none : (bd ? kWBDDAPA : kWDAPA);      // per-problem dense matrices: the plain and the bounded kernel
    if (bd) return pa ? kWBDPA : (da ? kWBDDA : kWBD);
    if (pc) return pa ? kWPCPA : (da ? kWPCDA : kWPC);
    return pa ? kWPA : (da ? kWDA : kWTab);
}

// (wreg_plan.h) the plan of a creator below, on the shapes its kind's launcher table holds; no HIP call
int wreg_plan_host(WregPlanKind kind, int m, int n, int nnz, const double* val, const int* ptr, const int* col, int max_lds,
                   WregHostPlan* out) {
    auto shapes_of = [](bool da, bool pa, bool bd) {
        const WVariants& t = table_of(da, pa, bd);
        std::vector<WShape> s;
        for (int i = 0; i < t.n; i++) s.push_back({t.v[i].mb, t.v[i].nq});
        return s;
    };
    return wreg_host_plan(kind, shapes_of, m, n, nnz, val, ptr, col, max_lds, *out);
}

// a creator of wreg.h: the host plan, its tables uploaded, the device pointers set (an empty table's points behind the one before)
static int wreg_plan_upload(WregPlanKind kind, int m, int n, int nnz, const double* val, const int* ptr, const int* col, int max_lds,
                            hipStream_t st, WregPlan** out) {
    WregHostPlan H;
    const int rc = wreg_plan_host(kind, m, n, nnz, val, ptr, col, max_lds, &H);
    if (rc != 0) return rc;
    WregPlan* P = new WregPlan();
    P->tab = H.tab; P->mb = H.mb; P->nq = H.nq; P->da = H.da; P->pa = H.pa; P->bd = H.bd;
    P->dev_blob = nullptr;
    if (!H.blob.sec.empty()) {      // (a plan on per-problem dense matrices has no table)
        const hipError_t e = plan_upload(H.blob, st, &P->dev_blob);
        if (e != hipSuccess) { delete P; return 1000 + (int)e; }
        const char* db = (const char*)P->dev_blob;
        WregTab& T = P->tab;
        if (H.da) T.img = (const double*)(db + H.a_img);
        else {
            T.csr_val = (const double*)(db + H.a_csr_val); T.ec_val = (const double*)(db + H.a_ec_val); T.t_w = (const double*)(db + H.a_t_w);
            T.lev = (const int*)(db + H.a_lev);
            T.csr_col = (const unsigned short*)(db + H.a_csr_col); T.csr_ptr = (const unsigned short*)(db + H.a_csr_ptr);
            T.csr_len = (const unsigned short*)(db + H.a_csr_len); T.ec_row = (const unsigned short*)(db + H.a_ec_row);
            T.colmap = (const unsigned*)(db + H.a_colmap);
            T.t_cd = (const unsigned*)(db + H.a_t_cd);
            T.ec_src = (const unsigned short*)(db + H.a_ec_src); T.t_ab = (const unsigned*)(db + H.a_t_ab);
        }
    }
    *out = P;
    return 0;
}

int wreg_plan_create(int m, int n, int nnz, const double* val, const int* ptr, const int* col, int max_lds, int pa,
                     hipStream_t st, WregPlan** out) {
    return wreg_plan_upload(pa ? WPLAN_PA : WPLAN_SHARED, m, n, nnz, val, ptr, col, max_lds, st, out);
}

int wreg_plan_create_bounded(int m, int n, int nnz, const double* val, const int* ptr, const int* col, int max_lds,
                             hipStream_t st, WregPlan** out) {
    return wreg_plan_upload(WPLAN_BOUNDED, m, n, nnz, val, ptr, col, max_lds, st, out);
}

int wreg_plan_create_dense_pa(int m, int n, int nnz, const double* val, const int* ptr, const int* col, int max_lds,
                              int keep_tail, hipStream_t st, WregPlan** out) {
    return wreg_plan_upload(keep_tail ? WPLAN_DENSE_PA_KEEP : WPLAN_DENSE_PA, m, n, nnz, val, ptr, col, max_lds, st, out);
}

int wreg_plan_create_bounded_pa(int m, int n, int nnz, const double* val, const int* ptr, const int* col, int max_lds,
                                hipStream_t st, WregPlan** out) {
    return wreg_plan_upload(WPLAN_BOUNDED_PA, m, n, nnz, val, ptr, col, max_lds, st, out);
}


int wreg_plan_create_bounded_dense_pa(int m, int n, int nnz, const double* val, const int* ptr, const int* col, int max_lds,
                                      hipStream_t st, WregPlan** out) {
    return wreg_plan_upload(WPLAN_BOUNDED_DENSE_PA, m, n, nnz, val, ptr, col, max_lds, st, out);
}

void wreg_plan_free(WregPlan* p) {
    if (!p) return;
    if (p->dev_blob) (void)hipFree(p->dev_blob);
    delete p;
}

int wreg_lds_bytes(const WregPlan* p) { return p ? p->tab.lds_bytes : 0; }
int wreg_block_threads(const WregPlan* p) { return p ? 64 * p->tab.wpb : 0; }
int wreg_variant(const WregPlan* p) { return p ? (p->da ? 2 : 1) : 0; }
int wreg_image_cols(const WregPlan* p) { return (p && p->da) ? p->tab.nd : 0; }
void wreg_shape(const WregPlan* p, int* mb, int* nq) {
    if (mb) *mb = p ? p->mb : 0;
    if (nq) *nq = p ? p->nq : 0;
}
int wreg_has_predcorr(const WregPlan* p) { return p ? 1 : 0; }

// the launchers of the plan's (MB, NQ) among the plain (pc: predictor-corrector, bd: bounded) kernels of its kind, or null
static const WVariant* plan_launchers(const WregPlan* p, bool bd, bool pc = false) {
    if (!p || p->bd != bd) return nullptr;
    const WVariants& t = table_of(p->da, p->pa, p->bd, pc);
    for (int i = 0; i < t.n; i++)
        if (t.v[i].mb == p->mb && t.v[i].nq == p->nq) return &t.v[i];
    return nullptr;
}

// persistent grid of the solve kernels: one workgroup per CU left to the solve; the m <= 64 variants need fewer than half the
// registers (234 of 512 per lane): two workgroups per CU -- two waves per SIMD -- where the LDS allows it
static int solve_grid(const WregPlan* p, long B, const DevOpts& o, int num_cu) {
    long cus = resident_cus(num_cu, o);
    if (p->mb <= 4 && 2 * (long)p->tab.lds_bytes <= 160 * 1024 && p->tab.wpb == 4) cus *= 2;
    const long grid = std::min(cus, (B + p->tab.wpb - 1) / p->tab.wpb);
    return grid < 1 ? 1 : (int)grid;
}

hipError_t wreg_launch_solve(WregPlan* p, long B, const double* a_batch, const double* b, const double* c, double* x, double* y, double* z,
                             double* pobj, double* dobj, int* status, int* iters, int* qhead, int* defer, DevOpts o,
                             int num_cu, hipStream_t st, int* grid_out) {
    const WVariant* v = plan_launchers(p, false);
    if (!v || (p->pa != (a_batch != nullptr))) return hipErrorInvalidValue;
    hipError_t e = hipMemsetAsync(defer, 0, sizeof(int), st);
    if (e != hipSuccess) return e;
    const int grid = solve_grid(p, B, o, num_cu);
    if (grid_out) *grid_out = grid;
    wsolve_fn fn = (o.flags & PYCLLP_FLAG_HSD) ? v->solve_hsd : v->solve;
    if ((o.flags & PYCLLP_FLAG_PREDCORR) && !(o.flags & PYCLLP_FLAG_HSD)) {
        const WVariant* pc = plan_launchers(p, false, true);
        if (!pc) return hipErrorNotSupported;
        fn = pc->solve;
    }
    if (!fn) return hipErrorNotSupported;      // (a kind without that kernel: per-problem dense matrices have the plain one only)
    return fn(p->tab, B, a_batch, b, c, x, y, z, pobj, dobj, status, iters, qhead, defer, o, grid, st);
}

hipError_t wreg_launch_solve_bounded(WregPlan* p, long B, const double* a_batch, const double* b, const double* c, const double* u, double* x, double* y,
                                     double* z, double* s, double* pobj, double* dobj, int* status, int* iters, int* qhead,
                                     DevOpts o, int num_cu, hipStream_t st, int* grid_out) {
    const WVariant* v = plan_launchers(p, true);
    if (!v || (p->pa != (a_batch != nullptr))) return hipErrorInvalidValue;
    const int grid = solve_grid(p, B, o, num_cu);
    if (grid_out) *grid_out = grid;
    if (a_batch) return v->solve_bounded_pa(p->tab, B, a_batch, b, c, u, x, y, z, s, pobj, dobj, status, iters, qhead, o, grid, st);
    return v->solve_bounded(p->tab, B, b, c, u, x, y, z, s, pobj, dobj, status, iters, qhead, o, grid, st);
}

// the launcher of the bounded kernel on the self-dual embedding for a shared-A bounded plan's (MB, NQ), or null
static wbsolve_fn bounded_hsd_launcher(const WregPlan* p) {
    if (!p || !p->bd || p->pa) return nullptr;
    const WVariants& t = p->da ? kWBDHDA : kWBDH;
    for (int i = 0; i < t.n; i++)
        if (t.v[i].mb == p->mb && t.v[i].nq == p->nq) return t.v[i].solve_bounded;
    return nullptr;
}
int wreg_has_bounded_hsd(const WregPlan* p) { return bounded_hsd_launcher(p) ? 1 : 0; }

hipError_t wreg_launch_solve_bounded_hsd(WregPlan* p, long B, const double* b, const double* c, const double* u, double* x, double* y,
                                         double* z, double* s, double* pobj, double* dobj, int* status, int* iters, int* qhead,
                                         DevOpts o, int num_cu, hipStream_t st, int* grid_out) {
    if (!p || !p->bd || p->pa) return hipErrorInvalidValue;
    const wbsolve_fn fn = bounded_hsd_launcher(p);
    if (!fn) return hipErrorNotSupported;
    const int grid = solve_grid(p, B, o, num_cu);
    if (grid_out) *grid_out = grid;
    return fn(p->tab, B, b, c, u, x, y, z, s, pobj, dobj, status, iters, qhead, o, grid, st);
}

hipError_t wreg_launch_newton(WregPlan* p, long B, const double* x, const double* z, const double* y, const double* b,
                              const double* c, double mu, double* dy, int* nref, DevOpts o, int num_cu, hipStream_t st,
                              int* grid_out) {
    const WVariant* v = plan_launchers(p, false);
    if (!v || !v->newton) return hipErrorInvalidValue;
    int* qhead = nullptr;
    hipError_t e = hipMallocAsync((void**)&qhead, sizeof(int), st);
    if (e != hipSuccess) return e;
    e = hipMemsetAsync(qhead, 0, sizeof(int), st);
    long grid = std::min((long)num_cu, (B + p->tab.wpb - 1) / p->tab.wpb);
    if (grid < 1) grid = 1;
    if (grid_out) *grid_out = (int)grid;
    if (e == hipSuccess) e = v->newton(p->tab, B, x, z, y, b, c, mu, dy, nref, qhead, o, (int)grid, st);
    hipError_t e2 = hipFreeAsync(qhead, st);
    return e != hipSuccess ? e : e2;
}

hipError_t wreg_launch_ldl_solve(int n, long B, const double* A, const double* rhs, double* out, double floor_,
                                 int num_cu, hipStream_t st) {
    if (n > 128) return hipErrorInvalidValue;
    int* qhead = nullptr;
    hipError_t e = hipMallocAsync((void**)&qhead, sizeof(int), st);
    if (e != hipSuccess) return e;
    e = hipMemsetAsync(qhead, 0, sizeof(int), st);
    long grid = std::min((long)num_cu, (B + 3) / 4);
    if (grid < 1) grid = 1;
    const int lds = (int)(sizeof(double) * 4 * WGeo<8>::WAVE_D(1));
    if (e == hipSuccess) e = set_dyn_lds((const void*)ldl_solve_wreg_kernel<8>, lds);
    if (e == hipSuccess) {
        hipLaunchKernelGGL((ldl_solve_wreg_kernel<8>), dim3((unsigned)grid), dim3(256), lds, st, n, B, A, rhs, out, floor_, qhead);
        e = hipGetLastError();
    }
    hipError_t e2 = hipFreeAsync(qhead, st);
    return e != hipSuccess ? e : e2;
}

extern "C" int pycllp_hip_debug_wreg_selftest(double* out_dev, void* stream) {
    hipLaunchKernelGGL(wreg_selftest_kernel, dim3(1), dim3(64), 0, (hipStream_t)stream, out_dev);
    return (int)hipGetLastError();
}
