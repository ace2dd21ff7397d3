// host.h -- what the units of the C ABI (abi_dense.hip, abi_sparse.hip) share: the two handles, the work-queue ring, the
// device's limits, launch plans and the argument checks of the entries.  Host code only; not part of the public ABI.
#ifndef PYCLLP_HOST_H
#define PYCLLP_HOST_H
#include "wreg.h"
#include "big.h"
#include "block.h"
#include "host_error.h"
#include <mutex>

inline int set_err(int code, const char* what) { return pycllp_runtime_error(code, what); }
// the messages of entries that share a body keep the entry's own name
inline int entry_err(int code, const char* entry, const char* what) { return pycllp_entry_error(code, entry, what); }

#define HIP_TRY(expr)                                             \
    do {                                                          \
        hipError_t e_ = (expr);                                   \
        if (e_ != hipSuccess) return set_err((int)e_, #expr);     \
    } while (0)

static constexpr unsigned kQueueRing = 64;   // work-queue counters per handle = launches that may be in flight at once

// Device work-queue heads of the persistent kernels: a ring of kQueueRing counters, one per launch in flight, so that solves
// issued on different streams / from different host threads with one handle never share a counter.  Every slot carries an
// event recorded behind the launch that used it; a slot is handed out again only once that launch has finished (the
// 65th launch in flight makes its caller wait for the oldest one instead of silently sharing its counter).
struct QueueRing {
    int* dev = nullptr;
    hipEvent_t ev[kQueueRing] = {};
    bool armed[kQueueRing] = {};
    std::atomic<unsigned> next{0};
    std::mutex mu[kQueueRing];
    hipError_t create() {
        hipError_t e = hipMalloc((void**)&dev, sizeof(int) * kQueueRing);
        for (unsigned i = 0; e == hipSuccess && i < kQueueRing; i++) e = hipEventCreateWithFlags(&ev[i], hipEventDisableTiming);
        return e;
    }
    void destroy() {
        for (unsigned i = 0; i < kQueueRing; i++) if (ev[i]) (void)hipEventDestroy(ev[i]);
        if (dev) (void)hipFree(dev);
        dev = nullptr;
    }
    // zeroed counter for a launch on `st`; *slot identifies it for release()
    hipError_t acquire(hipStream_t st, int** head, unsigned* slot) {
        const unsigned s = next.fetch_add(1u) % kQueueRing;
        mu[s].lock();                                   // held until release(): two threads 64 launches apart
        if (armed[s]) {
            hipError_t q = hipEventSynchronize(ev[s]);   // returns at once unless 64 later launches overtook this one
            if (q != hipSuccess) { mu[s].unlock(); return q; }
        }
        *head = dev + s; *slot = s;
        hipError_t e = hipMemsetAsync(dev + s, 0, sizeof(int), st);
        if (e != hipSuccess) mu[s].unlock();
        return e;
    }
    hipError_t release(unsigned s, hipStream_t st) {
        hipError_t e = hipEventRecord(ev[s], st);
        armed[s] = (e == hipSuccess);
        mu[s].unlock();
        return e;
    }
    // launch(head) on a slot of its own: acquire, launch, release on every path once acquired; the launch's error comes first
    template <typename Launch>
    hipError_t run(hipStream_t st, Launch&& launch) {
        int* head = nullptr; unsigned slot = 0;
        hipError_t e = acquire(st, &head, &slot);
        if (e != hipSuccess) return e;
        e = launch(head);
        const hipError_t er = release(slot, st);
        return e != hipSuccess ? e : er;
    }
};

// What the launch plans need to know of the current device: its CU count and the LDS one workgroup may take.  The LDS cap
// is 160 KB, also where a device reports none: every code object of this library is built for gfx950, which has 160 KB.
struct DeviceLimits { int num_cu = 0, max_lds = 0; };
inline hipError_t device_limits(DeviceLimits* d) {
    int dev = 0;
    hipDeviceProp_t prop;
    hipError_t e = hipGetDevice(&dev);
    if (e == hipSuccess) e = hipGetDeviceProperties(&prop, dev);
    if (e != hipSuccess) return e;
    d->num_cu = prop.multiProcessorCount;
    d->max_lds = (int)prop.maxSharedMemoryPerMultiProcessor;
    if (d->max_lds > 160 * 1024 || d->max_lds <= 0) d->max_lds = 160 * 1024;
    return hipSuccess;
}

struct LaunchPlan { int grid, block, lds, mp, np, sl; };   // sl: a kernel of the slack-aware table

// The persistent lane-group kernels run one workgroup per CU (its 8 waves already use the whole register file, so a second
// workgroup could not become resident whatever the LDS says), on the CUs the caller did not reserve (wave_common.h)
inline long resident_cus(const DeviceLimits& d, const DevOpts& o) { return resident_cus(d.num_cu, o); }
// A batch too small to fill every CU's eight waves (round 3): the waves per workgroup, wpb at most, of a kernel with G lane
// groups per wave.  Two waves on one SIMD share its issue port and the lane groups of a wave share its
// instruction stream, so: up to one wave per SIMD everywhere (4 per CU) every LP gets a wavefront of its own -- the kernel's
// slots are group-major, idle lane groups skip their Gram product -- then the lane groups fill, and only then does a SIMD get
// its second wave.
inline int small_batch_wpb(long B, long resident, int G, int wpb) {
    const long per_cu = (B + resident - 1) / resident;                               // LPs per CU
    long want = (per_cu <= 4 * (long)G) ? (per_cu < 4 ? per_cu : 4) : (per_cu + G - 1) / G;
    if (want < 1) want = 1;
    return want < wpb ? (int)want : wpb;
}
// workgroups: enough for one LP per wave while the batch is that small, else enough for all lane groups
inline int resident_blocks(long B, int wpb, long resident) {
    long blocks = (B + wpb - 1) / wpb;
    if (blocks > resident) blocks = resident;
    return blocks < 1 ? 1 : (int)blocks;
}

struct pycllp_hip_dense {
    int m = 0, n = 0, mp = 0, np = 0, variant = -1;
    double* pack = nullptr;
    double* a_rm = nullptr;   // row-major copy of A [m,n] for the group kernel
    double* first = nullptr;  // images of an LP's first Gram pass (dense_tab.h FirstGram), one allocation: the general variant's
    double* first_gen = nullptr, *first_sl = nullptr;   // (first_gen) and the slack-aware variant's (first_sl); null: none
    QueueRing ring; // device work-queue heads of the group kernel
    mutable std::mutex info_mu;   // guards grid/block/lds/mp/np/sl/full (what launch_info and variant_info report: the LAST launch)
    int variant_sl = -1; // index into kSlackVariants when the last m columns of A are the identity, else -1
    int grid = 0, block = 0, lds = 0;
    int sl = -1;         // the last launch ran a kernel of the slack-aware table (1) or of the general one (0); -1: none yet
    int full = 0;        // ... and that kernel was a full-shape instantiation (SlackVariant::full_group)
    DeviceLimits lim;
    struct pycllp_hip_sparse* sp = nullptr;   // LPs beyond the lane-group kernels (m <= 128, n <= 512): served by the sparse path's kernels
};

// A wave-kernel plan built by its first user (lazy_plan, abi_sparse.hip)
struct LazyPlan { WregPlan* plan = nullptr; bool tried = false; };
// ... each by the first call of: _sparse_solve_batch (structure tables only), _sparse_solve_bounded (t and s behind every wave
// area), _sparse_solve_batch_bounded (both), _dense_solve_batch beyond the lane-group kernels (per-problem DENSE matrices, an
// image per wave: with the identity tail implied, and with every column in the image under PYCLLP_FLAG_NO_SLACK_PATH),
// _dense_solve_batch_bounded beyond the lane-group kernels (that image with t and s behind it)
enum { LAZY_PA, LAZY_BD, LAZY_BDPA, LAZY_DAPA, LAZY_DAPA_KEEP, LAZY_BDDAPA,
       LAZY_N };

// ---- sparse shared-A path (one LP per workgroup) ---------------------------------------------------------------
struct pycllp_hip_sparse {
    BlockA desc = {};
    void* dev_blob = nullptr;     // one allocation holding every device array of desc
    QueueRing ring;     // work-queue heads (see pycllp_hip_dense)
    mutable std::mutex info_mu;
    int lds = 0, num_cu = 0, grid = 0;
    int lds_with_a = 0;     // LDS bytes with A's arrays in LDS (what per-problem values need), 0 when that does not fit
    WregPlan* wreg = nullptr;     // tables of the register-resident wave kernel (wreg_wave.h; host side ipm_wreg.hip), or nullptr when it does not cover A
    BigPlan* big = nullptr;       // LPs beyond m = 128 / n = 512: the workgroup-per-LP kernel of ipm_big.hip serves the handle alone
    LazyPlan lazy[LAZY_N];        // the wave kernel's other plans (under info_mu)
    WregPlan* last_plan = nullptr;   // the wave kernel's plan when the last solve ran on it, else null
    int last_a_in_lds = -1;          // the block kernel served the last launch: whether A's CSR / CSC copy sat in LDS; else -1
    int last_lds = 0;                // ... and the LDS bytes of that launch
    int max_lds = 0;
    std::vector<double> host_val; std::vector<int> host_ptr, host_col;   // host CSR copy (what a PA plan is built from)
};

DevOpts to_dev(const pycllp_hip_opts* opts);   // abi_sparse.hip

// PYCLLP_FLAG_AUTOSCALE scales every LP, PYCLLP_FLAG_AUTOSCALE_PER_LP those out of band: every solve entry refuses the pair, right
// after its handle / B check and before it reads the handle
static const char* const kBothAutoscales = "PYCLLP_FLAG_AUTOSCALE and PYCLLP_FLAG_AUTOSCALE_PER_LP exclude each other";
inline bool both_autoscales(const pycllp_hip_opts* opts) {
    return ((opts ? opts->flags : 0) & PYCLLP_AUTOSCALE_ANY) == PYCLLP_AUTOSCALE_ANY;
}

// The argument checks that open the five restricted entries (pycllp_hip_dense_solve_bounded, _dense_solve_batch,
// _dense_solve_batch_bounded, _sparse_solve_bounded, _sparse_solve_batch_bounded), in their order: the handle and B with the
// pointers the entry needs whatever B is (`always`), the flags it rejects (`rejected`, with the entry's sentence about them),
// the pointers it needs when B > 0 (`with_lps`).  The handle is not read and no HIP call is made: every one of these checks
// comes before either.  Returns 0 or PYCLLP_E_BADARG.
inline int check_restricted(const char* entry, const void* h, long B, bool always, const pycllp_hip_opts* opts, int rejected,
                            const char* rejected_what, bool with_lps) {
    if (!h || B < 0 || !always) return entry_err(PYCLLP_E_BADARG, entry, "bad argument");
    if (both_autoscales(opts)) return entry_err(PYCLLP_E_BADARG, entry, kBothAutoscales);
    if ((opts ? opts->flags : 0) & rejected) return entry_err(PYCLLP_E_BADARG, entry, rejected_what);
    if (B > 0 && !with_lps) return entry_err(PYCLLP_E_BADARG, entry, "bad argument");
    return 0;
}
// what the entries with upper bounds reject: on the lane-group kernels, and on the wave kernel
static constexpr int kBoundedRejected = PYCLLP_FLAG_HSD | PYCLLP_FLAG_PREDCORR | PYCLLP_FLAG_WARM_START | PYCLLP_FLAG_WAVE_KERNEL |
                                        PYCLLP_FLAG_NO_SLACK_PATH;
static constexpr int kWaveBoundedRejected = kBoundedRejected | PYCLLP_FLAG_BLOCK_KERNEL | PYCLLP_FLAG_FORCE_GUARD_PATH |
                                            PYCLLP_FLAG_EXACT_NORMS | PYCLLP_FLAG_PER_LP_FIRST_GRAM;   // (the diagnostic flags; the entries' sentence names the first)

// ---- bodies of abi_sparse.hip that entries of the dense handle run ----
// The sparse handle of a matrix given as host CSR arrays (validated by the caller): what pycllp_hip_sparse_init builds behind
// its download, and pycllp_hip_dense_init for a dense A beyond the lane-group kernels.
int sparse_init_host(int m, int n, int nnz, const std::vector<double>& val, const std::vector<int>& ptr, const std::vector<int>& col,
                     void* stream, pycllp_hip_sparse** handle);
// The body of pycllp_hip_dense_solve_batch for a handle beyond the lane-group kernels (h: its sparse handle), behind its
// argument checks.
int dense_solve_batch_wave(pycllp_hip_sparse* h, long B, const double* A_dev, long a_cols, const double* b_dev, const double* c_dev,
                           double* x_dev, double* y_dev, double* z_dev, double* pobj_dev, double* dobj_dev, int* status_dev,
                           int* iters_dev, const pycllp_hip_opts* opts, void* stream);
// ... and of pycllp_hip_dense_solve_batch_bounded for such a handle.
int dense_solve_batch_bounded_wave(pycllp_hip_sparse* h, long B, const double* A_dev, long a_cols, const double* b_dev,
                                   const double* c_dev, const double* u_dev, double* x_dev, double* y_dev, double* z_dev,
                                   double* s_dev, double* pobj_dev, double* dobj_dev, int* status_dev, int* iters_dev,
                                   const pycllp_hip_opts* opts, void* stream);
#endif
