// wave_common.h -- device helpers shared by the translation units of libpycllp_hip.so (ipm_dense.hip, ipm_wreg*.hip).
#ifndef PYCLLP_WAVE_COMMON_H
#define PYCLLP_WAVE_COMMON_H
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdio.h>
#include <string.h>

#include <algorithm>
#include <atomic>
#include <mutex>
#include <unordered_map>
#include <type_traits>
#include <vector>

#include "../../include/pycllp_hip.h"

// The 10x-growth exits (primal_normal.cl:261-269) keep the reference's own floor -- EPS = 1e-7f absolute, which is
// 1e3 x the relative stopping tolerance used here (for |b|, |c| ~ 1) -- instead of the stopping tolerance itself:
// within a factor 1000 of convergence a residual is rounding noise, and a 10x bump of noise is not divergence.
#define PYCLLP_GROWTH_FLOOR 1e3

typedef double double4_t __attribute__((ext_vector_type(4)));

// hipFuncAttributeMaxDynamicSharedMemorySize, set once per (device, kernel, size): the attribute call costs several
// microseconds of host time, which a small-batch "repeat solve" caller would pay on every launch
inline hipError_t set_dyn_lds(const void* fn, int bytes) {
    static std::mutex mu;
    static std::unordered_map<unsigned long long, int> done;
    int dev = 0;
    (void)hipGetDevice(&dev);
    const unsigned long long key = (unsigned long long)(size_t)fn ^ ((unsigned long long)dev << 56);
    std::lock_guard<std::mutex> g(mu);
    auto it = done.find(key);
    if (it != done.end() && it->second >= bytes) return hipSuccess;
    hipError_t e = hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, bytes);
    if (e == hipSuccess) done[key] = bytes;
    return e;
}

#define WAVE 64

// ------------------------------------------------------------------------------------------------
// small device helpers
// ------------------------------------------------------------------------------------------------
__device__ __forceinline__ double readlane_d(double v, int srclane) {
    int lo = __double2loint(v), hi = __double2hiint(v);
    lo = __builtin_amdgcn_readlane(lo, srclane);
    hi = __builtin_amdgcn_readlane(hi, srclane);
    return __hiloint2double(hi, lo);
}

// 1/a for a normal, positive a: v_rcp_f64 seed + two Newton steps (<= 1 ulp); skips the scaling/fix-up of an
// IEEE division, which the LDL' pivots (floored at pivot_floor) never need
// opaque copies of wave-uniform values that live in SGPRs (kernel arguments): what is derived from them is re-derived at
// every use instead of being hoisted out of a persistent loop into long-lived VGPRs
__device__ __forceinline__ double sopaque(double v) { asm volatile("" : "+s"(v)); return v; }
__device__ __forceinline__ int iopaque(int v) { asm volatile("" : "+s"(v)); return v; }
// The two scaling options as the kernels see them (DevOpts::flags; to_dev in abi_sparse.hip): PYCLLP_FLAG_AUTOSCALE -- the scaling
// code of an LP's load and store runs, as it always has -- and PYCLLP_FLAG_AUTOSCALE_PER_LP beside it -- that code takes a verdict
// per LP.  (A caller sets one of the two; the entries refuse both and hand a caller's PER_LP on as the pair.)
#define PYCLLP_AUTOSCALE_ANY (PYCLLP_FLAG_AUTOSCALE | PYCLLP_FLAG_AUTOSCALE_PER_LP)
// The verdict for ONE LP, taken where the LP's raw maxima are known (load and, where the scale factors are recomputed from the
// inputs, store): without PYCLLP_FLAG_AUTOSCALE_PER_LP every LP is scaled, with it an LP is scaled if and only if it is out of
// band -- max|b| (mb), max|c| over all n columns (mc) or, where mu > 0, the largest finite positive u (mu; 0: none, or an entry
// without bounds) outside [0.1, 10] and finite; the edges are in band.  A caller that gets false solves with sb = sc = 1:
// x / 1.0 and x * 1.0 are exact, so the LP carries the bits of a launch without either flag.  The host's restatement is
// autoscale_mask (solvers/hip.py).  The maxima come from fmax, which passes over a NaN: an LP with a NaN in its data may get
// either verdict and ends with PYCLLP_STATUS_NUMERICAL under both.
// The only f64 constant is 10, which every solve kernel holds anyway (the 10x-growth exits): an f64 literal needs a register
// pair, which the compiler loads once, outside the persistent LP loop, and keeps through every iteration -- a new one costs the
// largest wave kernels scratch.  So "mx < 0.1" is written 10 mx < 1, which is the same set of doubles: rounding is monotone,
// fl(10 * 0.1) = 1 (0.1 is 0x3FB999999999999A, 10 times it 1 + 5.6e-17) and fl(10 * pred(0.1)) = 1 - 2^-53 < 1 (the exact
// product is 1 - 8.3e-17, nearer to 1 - 2^-53 than to 1); an overflowing 10 mx is inf, not below 1.  And "finite" is written
// mx * 0 == 0 (inf * 0 is NaN) for the same reason: isfinite() brings its own constants.
__device__ __forceinline__ bool out_of_band(double mx) { return 10.0 * mx < 1.0 || (mx > 10.0 && mx * 0.0 == 0.0); }
__device__ __forceinline__ bool autoscale_lp(int flags, double mb, double mc, double mu) {
    return (flags & PYCLLP_FLAG_AUTOSCALE_PER_LP) == 0 || out_of_band(mb) || out_of_band(mc) || (mu > 0.0 && out_of_band(mu));
}
__device__ __forceinline__ double fast_rcp(double a) {
    double r = __builtin_amdgcn_rcp(a);
    r = fma(r, fma(-a, r, 1.0), r);
    r = fma(r, fma(-a, r, 1.0), r);
    return r;
}

__device__ __forceinline__ double wave_sum(double v) {
    asm volatile("" : "+v"(v));   // no fma contraction of the first stage with v's producer: see grp_sum
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) v += __shfl_xor(v, o, WAVE);
    return v;
}

__device__ __forceinline__ double wave_max(double v) {
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) v = fmax(v, __shfl_xor(v, o, WAVE));
    return v;
}

// Wave-private LDS hand-off: DS operations of one wave execute in order, so only the compiler has
// to be kept from moving a read above the write it depends on.
__device__ __forceinline__ void wave_lds_sync() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

struct DevOpts {
    double eps, delta, r, pivot_floor, refine_tol;
    int max_iter, max_refine, flags;
    int reserve_cus;           // host side only: CUs left idle by the launch plan
    unsigned long long* prof;  // diagnostic build only (-DPYCLLP_PROFILE): per-wave phase cycle sums
};
// the CUs left to a solve: those the caller did not reserve, one at least
inline long resident_cus(int num_cu, const DevOpts& o) { return (long)num_cu - o.reserve_cus > 0 ? (long)num_cu - o.reserve_cus : 1; }

// In-kernel phase stamps (diagnostic build only; the shipped library has no stamp executing).
#ifdef PYCLLP_PROFILE
#define NPHASE 12
#ifdef PYCLLP_PROFILE_LITE   // fewer live counters: the full set costs registers and distorts a kernel at the VGPR limit
#define PHASE_MAP(i) ((i) <= 1 ? 0 : (i) == 2 ? 2 : (i) <= 4 ? 4 : (i) == 5 ? 5 : (i) <= 7 ? 6 : 8)
#else
#define PHASE_MAP(i) (i)
#endif
#define STAMP_DECL unsigned long long t_prev_ = 0, t_acc_[NPHASE] = {0}; \
    { __builtin_amdgcn_sched_barrier(0); asm volatile("s_memtime %0\n\ts_waitcnt lgkmcnt(0)" : "=s"(t_prev_) :: "memory"); __builtin_amdgcn_sched_barrier(0); }
#define STAMP(i) { unsigned long long t_now_; __builtin_amdgcn_sched_barrier(0); \
    asm volatile("s_memtime %0\n\ts_waitcnt lgkmcnt(0)" : "=s"(t_now_) :: "memory"); __builtin_amdgcn_sched_barrier(0); \
    t_acc_[PHASE_MAP(i)] += t_now_ - t_prev_; t_prev_ = t_now_; }
#define STAMP_ARGS , unsigned long long& t_prev_, unsigned long long (&t_acc_)[NPHASE]
#define STAMP_PASS , t_prev_, t_acc_
#define STAMP_FLUSH(o, wid) if ((o).prof && lane == 0) { for (int i_ = 0; i_ < NPHASE; i_++) (o).prof[(size_t)(wid) * NPHASE + i_] = t_acc_[i_]; }
#define STAMP_FLUSH_BLOCK(o, wid) for (int i_ = 0; i_ < NPHASE; i_++) (o).prof[(size_t)(wid) * NPHASE + i_] = t_acc_[i_];
#else
#define STAMP_FLUSH_BLOCK(o, wid)
#define STAMP_DECL
#define STAMP(i)
#define STAMP_ARGS
#define STAMP_PASS
#define STAMP_FLUSH(o, wid)
#endif

// ---- DPP helpers (the exchanges across 16-lane rows are the lane swaps further down) -------------------------------------------------------------------------------------
template <int CTRL>
__device__ __forceinline__ double dpp_d(double v) {
    int lo = __double2loint(v), hi = __double2hiint(v);
    lo = __builtin_amdgcn_update_dpp(0, lo, CTRL, 0xF, 0xF, true);
    hi = __builtin_amdgcn_update_dpp(0, hi, CTRL, 0xF, 0xF, true);
    return __hiloint2double(hi, lo);
}
// compile-time loop (DPP controls must be immediates)
template <int K, int N, typename F>
__device__ __forceinline__ void static_for(F&& f) {
    if constexpr (K < N) {
        f(std::integral_constant<int, K>{});
        static_for<K + 1, N>(f);
    }
}
// value of lane K of the caller's own 16-lane row (row_newbcast)
template <int K>
__device__ __forceinline__ double row_bcast(double v) { return dpp_d<0x150 + K>(v); }

// ---- 64-bit DPP (gfx90a+: the DP ALU takes row_newbcast) ---------------------------------------------------------
// The compiler builds a row broadcast of a double from two v_mov_b32_dpp and feeds the copy to the FMA; the hardware can
// broadcast inside the 64-bit instruction itself.  The s_nop covers the VALU-write -> DPP-read hazard (2 wait states),
// which the hazard recogniser does not see through inline asm.
#define DPP_STR_(x) #x
#define DPP_STR(x) DPP_STR_(x)
// v of lane K of each 16-lane row
template <int K>
__device__ __forceinline__ double bcast64(double v) {
    double r;
    asm volatile("s_nop 1\n\tv_mov_b64_dpp %0, %1 row_newbcast:" DPP_STR(%2) " row_mask:0xf bank_mask:0xf" : "=v"(r) : "v"(v), "n"(K));
    return r;
}
#include "chain_asm.inc"

// ---- pivot steps under an EXEC mask (ipm_group.inc, round 3) ----
// In the lane-group kernel the mask "lanes below the pivot" and the one-hot "the pivot's lane" are compile-time constants per
// column; taking them as EXEC masks replaces, per column, the compare + two selects that zero the multiplier of the lanes
// on and above the pivot, the compare + two selects that pick the pivot's reciprocal, and the two multiplies + compare of the
// guard test (now one multiply + one max into a running maximum) -- five vector instructions per column that are not FP64 work.
// EXEC is saved and restored inside each statement, so the compiler never sees it change.  Source lanes of the broadcasts
// are always active lanes (k > J: below the pivot).
//   l (in: 0 everywhere) <- u rD in the lanes of the mask, u = Wd[J] (read from the operand list: no copy);  ymax <- max(ymax,
//   |l u|) there (= u^2 / D, the guard's test value);  Wd[k] -= (src of lane k) * l for k = J+1 .. 15 (the negation rides on the
//   FMA's source modifier: the caller stores l itself as the column of L, where rounds 2-3 negated it twice).
//   One function per J (the operand number of u is part of the instruction text).
// (SELF_, SRC_: the operand numbers of SELF and src in the statement that uses the line)
#define CHAIN_COL_FMA_(K, J_, SELF_, SRC_) ".if " #K " > " #J_ "\n\t.if %" #SELF_ "\n\tv_fmac_f64_dpp %" #K ", %" #J_ ", -%16 row_newbcast:" #K " row_mask:0xf bank_mask:0xf\n.else\n\t" \
                             "v_fmac_f64_dpp %" #K ", %" #SRC_ ", -%16 row_newbcast:" #K " row_mask:0xf bank_mask:0xf\n.endif\n.endif\n\t"
#define CHAIN_COL_FMA(K, J_) CHAIN_COL_FMA_(K, J_, 25, 21)
#define DEF_CHAIN_COL(J_) \
template <unsigned MLO, unsigned MHI, int SELF, unsigned ONELO, unsigned ONEHI> \
__device__ __forceinline__ void chain_col_##J_(double (&Wd)[16], double src, double rD, double& l, double& ymax, double& rdiag) { \
    double t; \
    unsigned long long save; \
    asm volatile("s_mov_b64 %19, exec\n\ts_mov_b32 exec_lo, %26\n\ts_mov_b32 exec_hi, %27\n\t" \
                 "v_mov_b64 %20, %22\n\t" \
                 "s_mov_b32 exec_lo, %23\n\ts_mov_b32 exec_hi, %24\n\t" \
                 "v_mul_f64 %16, %" #J_ ", %22\n\t" \
                 "v_mul_f64 %18, %16, %" #J_ "\n\t" \
                 "v_max_f64 %17, %17, |%18|\n\t" \
                 CHAIN_COL_FMA(0, J_) \
                 CHAIN_COL_FMA(1, J_) \
                 CHAIN_COL_FMA(2, J_) \
                 CHAIN_COL_FMA(3, J_) \
                 CHAIN_COL_FMA(4, J_) \
                 CHAIN_COL_FMA(5, J_) \
                 CHAIN_COL_FMA(6, J_) \
                 CHAIN_COL_FMA(7, J_) \
                 CHAIN_COL_FMA(8, J_) \
                 CHAIN_COL_FMA(9, J_) \
                 CHAIN_COL_FMA(10, J_) \
                 CHAIN_COL_FMA(11, J_) \
                 CHAIN_COL_FMA(12, J_) \
                 CHAIN_COL_FMA(13, J_) \
                 CHAIN_COL_FMA(14, J_) \
                 CHAIN_COL_FMA(15, J_) \
                 "s_mov_b64 exec, %19" \
                 : "+v"(Wd[0]), "+v"(Wd[1]), "+v"(Wd[2]), "+v"(Wd[3]), "+v"(Wd[4]), "+v"(Wd[5]), "+v"(Wd[6]), "+v"(Wd[7]), "+v"(Wd[8]), "+v"(Wd[9]), "+v"(Wd[10]), "+v"(Wd[11]), "+v"(Wd[12]), "+v"(Wd[13]), "+v"(Wd[14]), "+v"(Wd[15]), \
                   "+v"(l), "+v"(ymax), "=&v"(t), "=&s"(save), "+v"(rdiag) \
                 : "v"(src), "v"(rD), "n"(MLO), "n"(MHI), "n"(SELF), "n"(ONELO), "n"(ONEHI)); \
}
DEF_CHAIN_COL(0) DEF_CHAIN_COL(1) DEF_CHAIN_COL(2) DEF_CHAIN_COL(3) DEF_CHAIN_COL(4) DEF_CHAIN_COL(5) DEF_CHAIN_COL(6) DEF_CHAIN_COL(7)
DEF_CHAIN_COL(8) DEF_CHAIN_COL(9) DEF_CHAIN_COL(10) DEF_CHAIN_COL(11) DEF_CHAIN_COL(12) DEF_CHAIN_COL(13) DEF_CHAIN_COL(14) DEF_CHAIN_COL(15)
#undef DEF_CHAIN_COL
// The same column without the guard's test value: no l u, no running maximum.  Instead the pivot's own lane (the one-hot mask
// that captures rdiag) keeps its pivot -- Wd[J] there, whatever the other lanes hold -- in `pv`: one move in place of two f64
// instructions of the column statement.  What the caller concludes from the pivots: GWave::factor_sweep.  (A compare into VCC
// gathered by a scalar OR instead of the move lost 0.02 ms on the headline where the move gains 0.04: profiles/guard_sign.)
#define DEF_CHAIN_COLP(J_) \
template <unsigned MLO, unsigned MHI, int SELF, unsigned ONELO, unsigned ONEHI> \
__device__ __forceinline__ void chain_colp_##J_(double (&Wd)[16], double src, double rD, double& l, double& pv, double& rdiag) { \
    unsigned long long save; \
    asm volatile("s_mov_b64 %18, exec\n\ts_mov_b32 exec_lo, %25\n\ts_mov_b32 exec_hi, %26\n\t" \
                 "v_mov_b64 %19, %21\n\t" \
                 "v_mov_b64 %17, %" #J_ "\n\t" \
                 "s_mov_b32 exec_lo, %22\n\ts_mov_b32 exec_hi, %23\n\t" \
                 "v_mul_f64 %16, %" #J_ ", %21\n\t" \
                 CHAIN_COL_FMA_(0, J_, 24, 20) \
                 CHAIN_COL_FMA_(1, J_, 24, 20) \
                 CHAIN_COL_FMA_(2, J_, 24, 20) \
                 CHAIN_COL_FMA_(3, J_, 24, 20) \
                 CHAIN_COL_FMA_(4, J_, 24, 20) \
                 CHAIN_COL_FMA_(5, J_, 24, 20) \
                 CHAIN_COL_FMA_(6, J_, 24, 20) \
                 CHAIN_COL_FMA_(7, J_, 24, 20) \
                 CHAIN_COL_FMA_(8, J_, 24, 20) \
                 CHAIN_COL_FMA_(9, J_, 24, 20) \
                 CHAIN_COL_FMA_(10, J_, 24, 20) \
                 CHAIN_COL_FMA_(11, J_, 24, 20) \
                 CHAIN_COL_FMA_(12, J_, 24, 20) \
                 CHAIN_COL_FMA_(13, J_, 24, 20) \
                 CHAIN_COL_FMA_(14, J_, 24, 20) \
                 CHAIN_COL_FMA_(15, J_, 24, 20) \
                 "s_mov_b64 exec, %18" \
                 : "+v"(Wd[0]), "+v"(Wd[1]), "+v"(Wd[2]), "+v"(Wd[3]), "+v"(Wd[4]), "+v"(Wd[5]), "+v"(Wd[6]), "+v"(Wd[7]), "+v"(Wd[8]), "+v"(Wd[9]), "+v"(Wd[10]), "+v"(Wd[11]), "+v"(Wd[12]), "+v"(Wd[13]), "+v"(Wd[14]), "+v"(Wd[15]), \
                   "+v"(l), "+v"(pv), "=&s"(save), "+v"(rdiag) \
                 : "v"(src), "v"(rD), "n"(MLO), "n"(MHI), "n"(SELF), "n"(ONELO), "n"(ONEHI)); \
}
DEF_CHAIN_COLP(0) DEF_CHAIN_COLP(1) DEF_CHAIN_COLP(2) DEF_CHAIN_COLP(3) DEF_CHAIN_COLP(4) DEF_CHAIN_COLP(5) DEF_CHAIN_COLP(6) DEF_CHAIN_COLP(7)
DEF_CHAIN_COLP(8) DEF_CHAIN_COLP(9) DEF_CHAIN_COLP(10) DEF_CHAIN_COLP(11) DEF_CHAIN_COLP(12) DEF_CHAIN_COLP(13) DEF_CHAIN_COLP(14) DEF_CHAIN_COLP(15)
#undef DEF_CHAIN_COLP
#undef CHAIN_COL_FMA
#undef CHAIN_COL_FMA_
// SELF = 1: the broadcast source is the column itself, Wd[J] (the pivot's DPP row is the lane's own); `src` is then not read
// rdiag <- rD in the pivot's lane (mask ONELO / ONEHI) rides in the same statement: one save / restore of EXEC per column less
template <int J, unsigned MLO, unsigned MHI, int SELF, unsigned ONELO, unsigned ONEHI>
__device__ __forceinline__ void chain_step_exec(double (&Wd)[16], double src, double rD, double& l, double& ymax, double& rdiag) {
#define CHAIN_COL_CASE(J_) if constexpr (J == J_) chain_col_##J_<MLO, MHI, SELF, ONELO, ONEHI>(Wd, src, rD, l, ymax, rdiag);
    CHAIN_COL_CASE(0) CHAIN_COL_CASE(1) CHAIN_COL_CASE(2) CHAIN_COL_CASE(3) CHAIN_COL_CASE(4) CHAIN_COL_CASE(5) CHAIN_COL_CASE(6) CHAIN_COL_CASE(7)
    CHAIN_COL_CASE(8) CHAIN_COL_CASE(9) CHAIN_COL_CASE(10) CHAIN_COL_CASE(11) CHAIN_COL_CASE(12) CHAIN_COL_CASE(13) CHAIN_COL_CASE(14) CHAIN_COL_CASE(15)
#undef CHAIN_COL_CASE
}
template <int J, unsigned MLO, unsigned MHI, int SELF, unsigned ONELO, unsigned ONEHI>
__device__ __forceinline__ void chain_step_piv(double (&Wd)[16], double src, double rD, double& l, double& pv, double& rdiag) {
#define CHAIN_COL_CASE(J_) if constexpr (J == J_) chain_colp_##J_<MLO, MHI, SELF, ONELO, ONEHI>(Wd, src, rD, l, pv, rdiag);
    CHAIN_COL_CASE(0) CHAIN_COL_CASE(1) CHAIN_COL_CASE(2) CHAIN_COL_CASE(3) CHAIN_COL_CASE(4) CHAIN_COL_CASE(5) CHAIN_COL_CASE(6) CHAIN_COL_CASE(7)
    CHAIN_COL_CASE(8) CHAIN_COL_CASE(9) CHAIN_COL_CASE(10) CHAIN_COL_CASE(11) CHAIN_COL_CASE(12) CHAIN_COL_CASE(13) CHAIN_COL_CASE(14) CHAIN_COL_CASE(15)
#undef CHAIN_COL_CASE
}
// Wd[k] -= (src of lane k) * l, k = 0 .. 15, in ALL lanes (no EXEC mask: for callers whose other lanes hold don't-care values)
__device__ __forceinline__ void chain_all_neg(double (&Wd)[16], double src, double l) {
    asm volatile("s_nop 1\n\t"
                 "v_fmac_f64_dpp %0, %16, -%17 row_newbcast:0 row_mask:0xf bank_mask:0xf\n\t"
                 "v_fmac_f64_dpp %1, %16, -%17 row_newbcast:1 row_mask:0xf bank_mask:0xf\n\t"
                 "v_fmac_f64_dpp %2, %16, -%17 row_newbcast:2 row_mask:0xf bank_mask:0xf\n\t"
                 "v_fmac_f64_dpp %3, %16, -%17 row_newbcast:3 row_mask:0xf bank_mask:0xf\n\t"
                 "v_fmac_f64_dpp %4, %16, -%17 row_newbcast:4 row_mask:0xf bank_mask:0xf\n\t"
                 "v_fmac_f64_dpp %5, %16, -%17 row_newbcast:5 row_mask:0xf bank_mask:0xf\n\t"
                 "v_fmac_f64_dpp %6, %16, -%17 row_newbcast:6 row_mask:0xf bank_mask:0xf\n\t"
                 "v_fmac_f64_dpp %7, %16, -%17 row_newbcast:7 row_mask:0xf bank_mask:0xf\n\t"
                 "v_fmac_f64_dpp %8, %16, -%17 row_newbcast:8 row_mask:0xf bank_mask:0xf\n\t"
                 "v_fmac_f64_dpp %9, %16, -%17 row_newbcast:9 row_mask:0xf bank_mask:0xf\n\t"
                 "v_fmac_f64_dpp %10, %16, -%17 row_newbcast:10 row_mask:0xf bank_mask:0xf\n\t"
                 "v_fmac_f64_dpp %11, %16, -%17 row_newbcast:11 row_mask:0xf bank_mask:0xf\n\t"
                 "v_fmac_f64_dpp %12, %16, -%17 row_newbcast:12 row_mask:0xf bank_mask:0xf\n\t"
                 "v_fmac_f64_dpp %13, %16, -%17 row_newbcast:13 row_mask:0xf bank_mask:0xf\n\t"
                 "v_fmac_f64_dpp %14, %16, -%17 row_newbcast:14 row_mask:0xf bank_mask:0xf\n\t"
                 "v_fmac_f64_dpp %15, %16, -%17 row_newbcast:15 row_mask:0xf bank_mask:0xf\n\t"
                 : "+v"(Wd[0]), "+v"(Wd[1]), "+v"(Wd[2]), "+v"(Wd[3]), "+v"(Wd[4]), "+v"(Wd[5]), "+v"(Wd[6]), "+v"(Wd[7]), "+v"(Wd[8]), "+v"(Wd[9]), "+v"(Wd[10]), "+v"(Wd[11]), "+v"(Wd[12]), "+v"(Wd[13]), "+v"(Wd[14]), "+v"(Wd[15])
                 : "v"(src), "v"(l));
}
// Half of that block per DPP row (the split sweep of GWave::factor_sweep): Wd[s] -= (x of lane 8 + s) * (x rD), s = 0 .. 7, in
// ALL lanes.  x rD has the bits of the multiplier chain_col forms from the same two factors.  The multiply and the s_nop stand
// between a DPP move that wrote x just before the statement and the first read of x through DPP (two wait states).
__device__ __forceinline__ void chain_half_neg(double (&Wd)[8], double x, double rD) {
    double lx;
    asm volatile("v_mul_f64 %8, %9, %10\n\t"
                 "s_nop 0\n\t"
                 "v_fmac_f64_dpp %0, %9, -%8 row_newbcast:8 row_mask:0xf bank_mask:0xf\n\t"
                 "v_fmac_f64_dpp %1, %9, -%8 row_newbcast:9 row_mask:0xf bank_mask:0xf\n\t"
                 "v_fmac_f64_dpp %2, %9, -%8 row_newbcast:10 row_mask:0xf bank_mask:0xf\n\t"
                 "v_fmac_f64_dpp %3, %9, -%8 row_newbcast:11 row_mask:0xf bank_mask:0xf\n\t"
                 "v_fmac_f64_dpp %4, %9, -%8 row_newbcast:12 row_mask:0xf bank_mask:0xf\n\t"
                 "v_fmac_f64_dpp %5, %9, -%8 row_newbcast:13 row_mask:0xf bank_mask:0xf\n\t"
                 "v_fmac_f64_dpp %6, %9, -%8 row_newbcast:14 row_mask:0xf bank_mask:0xf\n\t"
                 "v_fmac_f64_dpp %7, %9, -%8 row_newbcast:15 row_mask:0xf bank_mask:0xf\n\t"
                 : "+v"(Wd[0]), "+v"(Wd[1]), "+v"(Wd[2]), "+v"(Wd[3]), "+v"(Wd[4]), "+v"(Wd[5]), "+v"(Wd[6]), "+v"(Wd[7]), "=&v"(lx)
                 : "v"(x), "v"(rD));
}
// max(|a|, b) as ONE instruction (fmax(fabs(a), b) costs a canonicalising v_max_f64 a, a first); BS: b is wave-uniform (SGPR)
template <bool BS>
__device__ __forceinline__ double max_abs(double a, double b) {
    double r;
    if constexpr (BS) asm volatile("v_max_f64 %0, |%1|, %2" : "=v"(r) : "v"(a), "s"(b));
    else asm volatile("v_max_f64 %0, |%1|, %2" : "=v"(r) : "v"(a), "v"(b));
    return r;
}
// Head of a pivot step of the wave kernel's 16-step chain (every 16-lane DPP row holds the same diagonal block, lane = row):
//   nli <- -(u rD) in the lanes below the pivot (mask M16 per DPP row), 0 elsewhere;  ymax <- max(ymax, |nli u|) there (u^2 / D:
//   the guard's test value);  rdiag <- rD in the pivot's lane (mask ONE16).
// Five vector instructions where compares + selects on per-lane predicates took thirteen, and the multiplier no longer passes
// through a select on its way into the trailing FMAs.  EXEC is saved and restored inside the statement.
template <unsigned M16, unsigned ONE16>
__device__ __forceinline__ void chain_head_exec(double u, double rD, double& nli, double& ymax, double& rdiag) {
    double t;
    unsigned long long save;
    asm volatile("v_mov_b64 %0, 0\n\t"
                 "s_mov_b64 %4, exec\n\ts_mov_b32 exec_lo, %7\n\ts_mov_b32 exec_hi, %7\n\t"
                 "v_mul_f64 %0, -%5, %6\n\t"
                 "v_mul_f64 %3, %0, %5\n\t"
                 "v_max_f64 %1, %1, |%3|\n\t"
                 "s_mov_b32 exec_lo, %8\n\ts_mov_b32 exec_hi, %8\n\t"
                 "v_mov_b64 %2, %6\n\t"
                 "s_mov_b64 exec, %4"
                 : "=&v"(nli), "+v"(ymax), "+v"(rdiag), "=&v"(t), "=&s"(save)
                 : "v"(u), "v"(rD), "n"(M16), "n"(ONE16));
}
// dst <- v in the lanes of the mask only
template <unsigned MLO, unsigned MHI>
__device__ __forceinline__ void mov_exec(double& dst, double v) {
    unsigned long long save;
    asm volatile("s_mov_b64 %1, exec\n\ts_mov_b32 exec_lo, %3\n\ts_mov_b32 exec_hi, %4\n\tv_mov_b64 %0, %2\n\ts_mov_b64 exec, %1"
                 : "+v"(dst), "=&s"(save) : "v"(v), "n"(MLO), "n"(MHI));
}

// Unit-triangular substitution inside a 16-lane DPP row with the broadcast fused into the FMA: 15 dependent steps
//   s -= l[k] * (s of lane k),  k = 0 .. 14   (subst15_up: forward, L)        /  k = 15 .. 1  (subst15_down: backward, L')
// one instruction each (the compiler's form is two v_mov_b32_dpp + v_fma_f64 per step, three dependent issues); the s_nop
// covers the VALU-write -> DPP-read hazard between consecutive steps.  Same FMA, same rounding.
__device__ __forceinline__ void subst15_up(double& s, const double* l) {
    asm volatile("s_nop 1\n\tv_fmac_f64_dpp %0, %0, -%1 row_newbcast:0 row_mask:0xf bank_mask:0xf\n\t"
                 "s_nop 1\n\tv_fmac_f64_dpp %0, %0, -%2 row_newbcast:1 row_mask:0xf bank_mask:0xf\n\t"
                 "s_nop 1\n\tv_fmac_f64_dpp %0, %0, -%3 row_newbcast:2 row_mask:0xf bank_mask:0xf\n\t"
                 "s_nop 1\n\tv_fmac_f64_dpp %0, %0, -%4 row_newbcast:3 row_mask:0xf bank_mask:0xf\n\t"
                 "s_nop 1\n\tv_fmac_f64_dpp %0, %0, -%5 row_newbcast:4 row_mask:0xf bank_mask:0xf\n\t"
                 "s_nop 1\n\tv_fmac_f64_dpp %0, %0, -%6 row_newbcast:5 row_mask:0xf bank_mask:0xf\n\t"
                 "s_nop 1\n\tv_fmac_f64_dpp %0, %0, -%7 row_newbcast:6 row_mask:0xf bank_mask:0xf\n\t"
                 "s_nop 1\n\tv_fmac_f64_dpp %0, %0, -%8 row_newbcast:7 row_mask:0xf bank_mask:0xf\n\t"
                 "s_nop 1\n\tv_fmac_f64_dpp %0, %0, -%9 row_newbcast:8 row_mask:0xf bank_mask:0xf\n\t"
                 "s_nop 1\n\tv_fmac_f64_dpp %0, %0, -%10 row_newbcast:9 row_mask:0xf bank_mask:0xf\n\t"
                 "s_nop 1\n\tv_fmac_f64_dpp %0, %0, -%11 row_newbcast:10 row_mask:0xf bank_mask:0xf\n\t"
                 "s_nop 1\n\tv_fmac_f64_dpp %0, %0, -%12 row_newbcast:11 row_mask:0xf bank_mask:0xf\n\t"
                 "s_nop 1\n\tv_fmac_f64_dpp %0, %0, -%13 row_newbcast:12 row_mask:0xf bank_mask:0xf\n\t"
                 "s_nop 1\n\tv_fmac_f64_dpp %0, %0, -%14 row_newbcast:13 row_mask:0xf bank_mask:0xf\n\t"
                 "s_nop 1\n\tv_fmac_f64_dpp %0, %0, -%15 row_newbcast:14 row_mask:0xf bank_mask:0xf\n\t"
                 : "+v"(s) : "v"(l[0]), "v"(l[1]), "v"(l[2]), "v"(l[3]), "v"(l[4]), "v"(l[5]), "v"(l[6]), "v"(l[7]), "v"(l[8]), "v"(l[9]), "v"(l[10]), "v"(l[11]), "v"(l[12]), "v"(l[13]), "v"(l[14]));
}
__device__ __forceinline__ void subst15_down(double& s, const double* l) {      // uses l[15] .. l[1]
    asm volatile("s_nop 1\n\tv_fmac_f64_dpp %0, %0, -%1 row_newbcast:15 row_mask:0xf bank_mask:0xf\n\t"
                 "s_nop 1\n\tv_fmac_f64_dpp %0, %0, -%2 row_newbcast:14 row_mask:0xf bank_mask:0xf\n\t"
                 "s_nop 1\n\tv_fmac_f64_dpp %0, %0, -%3 row_newbcast:13 row_mask:0xf bank_mask:0xf\n\t"
                 "s_nop 1\n\tv_fmac_f64_dpp %0, %0, -%4 row_newbcast:12 row_mask:0xf bank_mask:0xf\n\t"
                 "s_nop 1\n\tv_fmac_f64_dpp %0, %0, -%5 row_newbcast:11 row_mask:0xf bank_mask:0xf\n\t"
                 "s_nop 1\n\tv_fmac_f64_dpp %0, %0, -%6 row_newbcast:10 row_mask:0xf bank_mask:0xf\n\t"
                 "s_nop 1\n\tv_fmac_f64_dpp %0, %0, -%7 row_newbcast:9 row_mask:0xf bank_mask:0xf\n\t"
                 "s_nop 1\n\tv_fmac_f64_dpp %0, %0, -%8 row_newbcast:8 row_mask:0xf bank_mask:0xf\n\t"
                 "s_nop 1\n\tv_fmac_f64_dpp %0, %0, -%9 row_newbcast:7 row_mask:0xf bank_mask:0xf\n\t"
                 "s_nop 1\n\tv_fmac_f64_dpp %0, %0, -%10 row_newbcast:6 row_mask:0xf bank_mask:0xf\n\t"
                 "s_nop 1\n\tv_fmac_f64_dpp %0, %0, -%11 row_newbcast:5 row_mask:0xf bank_mask:0xf\n\t"
                 "s_nop 1\n\tv_fmac_f64_dpp %0, %0, -%12 row_newbcast:4 row_mask:0xf bank_mask:0xf\n\t"
                 "s_nop 1\n\tv_fmac_f64_dpp %0, %0, -%13 row_newbcast:3 row_mask:0xf bank_mask:0xf\n\t"
                 "s_nop 1\n\tv_fmac_f64_dpp %0, %0, -%14 row_newbcast:2 row_mask:0xf bank_mask:0xf\n\t"
                 "s_nop 1\n\tv_fmac_f64_dpp %0, %0, -%15 row_newbcast:1 row_mask:0xf bank_mask:0xf\n\t"
                 : "+v"(s) : "v"(l[15]), "v"(l[14]), "v"(l[13]), "v"(l[12]), "v"(l[11]), "v"(l[10]), "v"(l[9]), "v"(l[8]), "v"(l[7]), "v"(l[6]), "v"(l[5]), "v"(l[4]), "v"(l[3]), "v"(l[2]), "v"(l[1]));
}
// the same for two right-hand sides at once, the two dependency chains interleaved (each step of one chain stands between two
// steps of the other: one s_nop 0 more completes the two wait states of the VALU-write -> DPP-read hazard)
__device__ __forceinline__ void subst15_up2(double& s, double& t, const double* l) {
    asm volatile("s_nop 1\n\t"
                 "s_nop 0\n\tv_fmac_f64_dpp %0, %0, -%2 row_newbcast:0 row_mask:0xf bank_mask:0xf\n\t"
                 "v_fmac_f64_dpp %1, %1, -%2 row_newbcast:0 row_mask:0xf bank_mask:0xf\n\t"
                 "s_nop 0\n\tv_fmac_f64_dpp %0, %0, -%3 row_newbcast:1 row_mask:0xf bank_mask:0xf\n\t"
                 "v_fmac_f64_dpp %1, %1, -%3 row_newbcast:1 row_mask:0xf bank_mask:0xf\n\t"
                 "s_nop 0\n\tv_fmac_f64_dpp %0, %0, -%4 row_newbcast:2 row_mask:0xf bank_mask:0xf\n\t"
                 "v_fmac_f64_dpp %1, %1, -%4 row_newbcast:2 row_mask:0xf bank_mask:0xf\n\t"
                 "s_nop 0\n\tv_fmac_f64_dpp %0, %0, -%5 row_newbcast:3 row_mask:0xf bank_mask:0xf\n\t"
                 "v_fmac_f64_dpp %1, %1, -%5 row_newbcast:3 row_mask:0xf bank_mask:0xf\n\t"
                 "s_nop 0\n\tv_fmac_f64_dpp %0, %0, -%6 row_newbcast:4 row_mask:0xf bank_mask:0xf\n\t"
                 "v_fmac_f64_dpp %1, %1, -%6 row_newbcast:4 row_mask:0xf bank_mask:0xf\n\t"
                 "s_nop 0\n\tv_fmac_f64_dpp %0, %0, -%7 row_newbcast:5 row_mask:0xf bank_mask:0xf\n\t"
                 "v_fmac_f64_dpp %1, %1, -%7 row_newbcast:5 row_mask:0xf bank_mask:0xf\n\t"
                 "s_nop 0\n\tv_fmac_f64_dpp %0, %0, -%8 row_newbcast:6 row_mask:0xf bank_mask:0xf\n\t"
                 "v_fmac_f64_dpp %1, %1, -%8 row_newbcast:6 row_mask:0xf bank_mask:0xf\n\t"
                 "s_nop 0\n\tv_fmac_f64_dpp %0, %0, -%9 row_newbcast:7 row_mask:0xf bank_mask:0xf\n\t"
                 "v_fmac_f64_dpp %1, %1, -%9 row_newbcast:7 row_mask:0xf bank_mask:0xf\n\t"
                 "s_nop 0\n\tv_fmac_f64_dpp %0, %0, -%10 row_newbcast:8 row_mask:0xf bank_mask:0xf\n\t"
                 "v_fmac_f64_dpp %1, %1, -%10 row_newbcast:8 row_mask:0xf bank_mask:0xf\n\t"
                 "s_nop 0\n\tv_fmac_f64_dpp %0, %0, -%11 row_newbcast:9 row_mask:0xf bank_mask:0xf\n\t"
                 "v_fmac_f64_dpp %1, %1, -%11 row_newbcast:9 row_mask:0xf bank_mask:0xf\n\t"
                 "s_nop 0\n\tv_fmac_f64_dpp %0, %0, -%12 row_newbcast:10 row_mask:0xf bank_mask:0xf\n\t"
                 "v_fmac_f64_dpp %1, %1, -%12 row_newbcast:10 row_mask:0xf bank_mask:0xf\n\t"
                 "s_nop 0\n\tv_fmac_f64_dpp %0, %0, -%13 row_newbcast:11 row_mask:0xf bank_mask:0xf\n\t"
                 "v_fmac_f64_dpp %1, %1, -%13 row_newbcast:11 row_mask:0xf bank_mask:0xf\n\t"
                 "s_nop 0\n\tv_fmac_f64_dpp %0, %0, -%14 row_newbcast:12 row_mask:0xf bank_mask:0xf\n\t"
                 "v_fmac_f64_dpp %1, %1, -%14 row_newbcast:12 row_mask:0xf bank_mask:0xf\n\t"
                 "s_nop 0\n\tv_fmac_f64_dpp %0, %0, -%15 row_newbcast:13 row_mask:0xf bank_mask:0xf\n\t"
                 "v_fmac_f64_dpp %1, %1, -%15 row_newbcast:13 row_mask:0xf bank_mask:0xf\n\t"
                 "s_nop 0\n\tv_fmac_f64_dpp %0, %0, -%16 row_newbcast:14 row_mask:0xf bank_mask:0xf\n\t"
                 "v_fmac_f64_dpp %1, %1, -%16 row_newbcast:14 row_mask:0xf bank_mask:0xf\n\t"
                 : "+v"(s), "+v"(t) : "v"(l[0]), "v"(l[1]), "v"(l[2]), "v"(l[3]), "v"(l[4]), "v"(l[5]), "v"(l[6]), "v"(l[7]), "v"(l[8]), "v"(l[9]), "v"(l[10]), "v"(l[11]), "v"(l[12]), "v"(l[13]), "v"(l[14]));
}
__device__ __forceinline__ void subst15_down2(double& s, double& t, const double* l) {      // uses l[15] .. l[1]
    asm volatile("s_nop 1\n\t"
                 "s_nop 0\n\tv_fmac_f64_dpp %0, %0, -%2 row_newbcast:15 row_mask:0xf bank_mask:0xf\n\t"
                 "v_fmac_f64_dpp %1, %1, -%2 row_newbcast:15 row_mask:0xf bank_mask:0xf\n\t"
                 "s_nop 0\n\tv_fmac_f64_dpp %0, %0, -%3 row_newbcast:14 row_mask:0xf bank_mask:0xf\n\t"
                 "v_fmac_f64_dpp %1, %1, -%3 row_newbcast:14 row_mask:0xf bank_mask:0xf\n\t"
                 "s_nop 0\n\tv_fmac_f64_dpp %0, %0, -%4 row_newbcast:13 row_mask:0xf bank_mask:0xf\n\t"
                 "v_fmac_f64_dpp %1, %1, -%4 row_newbcast:13 row_mask:0xf bank_mask:0xf\n\t"
                 "s_nop 0\n\tv_fmac_f64_dpp %0, %0, -%5 row_newbcast:12 row_mask:0xf bank_mask:0xf\n\t"
                 "v_fmac_f64_dpp %1, %1, -%5 row_newbcast:12 row_mask:0xf bank_mask:0xf\n\t"
                 "s_nop 0\n\tv_fmac_f64_dpp %0, %0, -%6 row_newbcast:11 row_mask:0xf bank_mask:0xf\n\t"
                 "v_fmac_f64_dpp %1, %1, -%6 row_newbcast:11 row_mask:0xf bank_mask:0xf\n\t"
                 "s_nop 0\n\tv_fmac_f64_dpp %0, %0, -%7 row_newbcast:10 row_mask:0xf bank_mask:0xf\n\t"
                 "v_fmac_f64_dpp %1, %1, -%7 row_newbcast:10 row_mask:0xf bank_mask:0xf\n\t"
                 "s_nop 0\n\tv_fmac_f64_dpp %0, %0, -%8 row_newbcast:9 row_mask:0xf bank_mask:0xf\n\t"
                 "v_fmac_f64_dpp %1, %1, -%8 row_newbcast:9 row_mask:0xf bank_mask:0xf\n\t"
                 "s_nop 0\n\tv_fmac_f64_dpp %0, %0, -%9 row_newbcast:8 row_mask:0xf bank_mask:0xf\n\t"
                 "v_fmac_f64_dpp %1, %1, -%9 row_newbcast:8 row_mask:0xf bank_mask:0xf\n\t"
                 "s_nop 0\n\tv_fmac_f64_dpp %0, %0, -%10 row_newbcast:7 row_mask:0xf bank_mask:0xf\n\t"
                 "v_fmac_f64_dpp %1, %1, -%10 row_newbcast:7 row_mask:0xf bank_mask:0xf\n\t"
                 "s_nop 0\n\tv_fmac_f64_dpp %0, %0, -%11 row_newbcast:6 row_mask:0xf bank_mask:0xf\n\t"
                 "v_fmac_f64_dpp %1, %1, -%11 row_newbcast:6 row_mask:0xf bank_mask:0xf\n\t"
                 "s_nop 0\n\tv_fmac_f64_dpp %0, %0, -%12 row_newbcast:5 row_mask:0xf bank_mask:0xf\n\t"
                 "v_fmac_f64_dpp %1, %1, -%12 row_newbcast:5 row_mask:0xf bank_mask:0xf\n\t"
                 "s_nop 0\n\tv_fmac_f64_dpp %0, %0, -%13 row_newbcast:4 row_mask:0xf bank_mask:0xf\n\t"
                 "v_fmac_f64_dpp %1, %1, -%13 row_newbcast:4 row_mask:0xf bank_mask:0xf\n\t"
                 "s_nop 0\n\tv_fmac_f64_dpp %0, %0, -%14 row_newbcast:3 row_mask:0xf bank_mask:0xf\n\t"
                 "v_fmac_f64_dpp %1, %1, -%14 row_newbcast:3 row_mask:0xf bank_mask:0xf\n\t"
                 "s_nop 0\n\tv_fmac_f64_dpp %0, %0, -%15 row_newbcast:2 row_mask:0xf bank_mask:0xf\n\t"
                 "v_fmac_f64_dpp %1, %1, -%15 row_newbcast:2 row_mask:0xf bank_mask:0xf\n\t"
                 "s_nop 0\n\tv_fmac_f64_dpp %0, %0, -%16 row_newbcast:1 row_mask:0xf bank_mask:0xf\n\t"
                 "v_fmac_f64_dpp %1, %1, -%16 row_newbcast:1 row_mask:0xf bank_mask:0xf\n\t"
                 : "+v"(s), "+v"(t) : "v"(l[15]), "v"(l[14]), "v"(l[13]), "v"(l[12]), "v"(l[11]), "v"(l[10]), "v"(l[9]), "v"(l[8]), "v"(l[7]), "v"(l[6]), "v"(l[5]), "v"(l[4]), "v"(l[3]), "v"(l[2]), "v"(l[1]));
}
// sum_k l[k] * (src of lane k), k = 0 .. 15, accumulated in that order (as the scalar loop it replaces): sixteen fused FMAs
__device__ __forceinline__ double dot16_bcast(double src, const double* l) {
    double a = 0.0;
    asm volatile("s_nop 1\n\t"
                 "v_fmac_f64_dpp %0, %1, %2 row_newbcast:0 row_mask:0xf bank_mask:0xf\n\t"
                 "v_fmac_f64_dpp %0, %1, %3 row_newbcast:1 row_mask:0xf bank_mask:0xf\n\t"
                 "v_fmac_f64_dpp %0, %1, %4 row_newbcast:2 row_mask:0xf bank_mask:0xf\n\t"
                 "v_fmac_f64_dpp %0, %1, %5 row_newbcast:3 row_mask:0xf bank_mask:0xf\n\t"
                 "v_fmac_f64_dpp %0, %1, %6 row_newbcast:4 row_mask:0xf bank_mask:0xf\n\t"
                 "v_fmac_f64_dpp %0, %1, %7 row_newbcast:5 row_mask:0xf bank_mask:0xf\n\t"
                 "v_fmac_f64_dpp %0, %1, %8 row_newbcast:6 row_mask:0xf bank_mask:0xf\n\t"
                 "v_fmac_f64_dpp %0, %1, %9 row_newbcast:7 row_mask:0xf bank_mask:0xf\n\t"
                 "v_fmac_f64_dpp %0, %1, %10 row_newbcast:8 row_mask:0xf bank_mask:0xf\n\t"
                 "v_fmac_f64_dpp %0, %1, %11 row_newbcast:9 row_mask:0xf bank_mask:0xf\n\t"
                 "v_fmac_f64_dpp %0, %1, %12 row_newbcast:10 row_mask:0xf bank_mask:0xf\n\t"
                 "v_fmac_f64_dpp %0, %1, %13 row_newbcast:11 row_mask:0xf bank_mask:0xf\n\t"
                 "v_fmac_f64_dpp %0, %1, %14 row_newbcast:12 row_mask:0xf bank_mask:0xf\n\t"
                 "v_fmac_f64_dpp %0, %1, %15 row_newbcast:13 row_mask:0xf bank_mask:0xf\n\t"
                 "v_fmac_f64_dpp %0, %1, %16 row_newbcast:14 row_mask:0xf bank_mask:0xf\n\t"
                 "v_fmac_f64_dpp %0, %1, %17 row_newbcast:15 row_mask:0xf bank_mask:0xf\n\t"
                 : "+v"(a) : "v"(src), "v"(l[0]), "v"(l[1]), "v"(l[2]), "v"(l[3]), "v"(l[4]), "v"(l[5]), "v"(l[6]), "v"(l[7]), "v"(l[8]), "v"(l[9]), "v"(l[10]), "v"(l[11]), "v"(l[12]), "v"(l[13]), "v"(l[14]), "v"(l[15]));
    return a;
}

// ---- single steps of the above, for the forward substitution that GWave::factor_dpp_fwd carries through the LDL' sweep ----
// Step K of subst15_up, s -= l * (s of lane K of the DPP row), written only in the DPP rows of RM (the DPP row_mask: no EXEC
// switch; the other rows keep their s).  Same FMA, same operands as the step inside subst15_up.
template <int K, int RM>
__device__ __forceinline__ void fwd_step(double& s, double l) {
    asm volatile("s_nop 1\n\tv_fmac_f64_dpp %0, %0, -%1 row_newbcast:" DPP_STR(%2) " row_mask:" DPP_STR(%3) " bank_mask:0xf"
                 : "+v"(s) : "v"(l), "n"(K), "n"(RM));
}
// Step K of dot16_bcast, a += l * (src of lane K of the DPP row), in the DPP rows of RM; the first step carries the s_nop
template <int K, int RM>
__device__ __forceinline__ void dot_step(double& a, double src, double l) {
    if constexpr (K == 0)
        asm volatile("s_nop 1\n\tv_fmac_f64_dpp %0, %1, %2 row_newbcast:" DPP_STR(%3) " row_mask:" DPP_STR(%4) " bank_mask:0xf"
                     : "+v"(a) : "v"(src), "v"(l), "n"(K), "n"(RM));
    else
        asm volatile("v_fmac_f64_dpp %0, %1, %2 row_newbcast:" DPP_STR(%3) " row_mask:" DPP_STR(%4) " bank_mask:0xf"
                     : "+v"(a) : "v"(src), "v"(l), "n"(K), "n"(RM));
}

// ---- cross-lane helpers ----------------------------------------------------------------------------------------
// Lane swaps move ACTIVE lanes only: v_permlane16_swap needs both 16-lane rows of a 32-lane group in EXEC, v_permlane32_swap the
// whole wave.  Every call site says which it has.  They are VALU instructions: no LDS, no lgkmcnt.
// A swap overwrites BOTH operands, so a double swapped with itself needs two copies of itself first.  Handed over as halves
// (__double2loint / __double2hiint of one value, each swapped with itself) the compiler copies every half: four v_mov_b32 per
// swap where the value stays live.  self_swap16 / self_swap32 make the two copies as doubles -- the pin keeps them 64-bit
// values in registers of their own, one v_mov_b64 each (none where the value dies) -- and swap the halves of those.
//   r0 / r1 <- [0] / [1] of the self-swap: v of rows (0, 0, 2, 2) / (1, 1, 3, 3) for the 16-lane swap, of lanes (0-31, 0-31) /
//   (32-63, 32-63) for the 32-lane swap
__device__ __forceinline__ void self_swap16(double v, double& r0, double& r1) {
    double a = v, b = v;
    asm("" : "+v"(a), "+v"(b));
    auto l = __builtin_amdgcn_permlane16_swap(__double2loint(a), __double2loint(b), false, false);
    auto h = __builtin_amdgcn_permlane16_swap(__double2hiint(a), __double2hiint(b), false, false);
    r0 = __hiloint2double(h[0], l[0]);
    r1 = __hiloint2double(h[1], l[1]);
}
__device__ __forceinline__ void self_swap32(double v, double& r0, double& r1) {
    double a = v, b = v;
    asm("" : "+v"(a), "+v"(b));
    auto l = __builtin_amdgcn_permlane32_swap(__double2loint(a), __double2loint(b), false, false);
    auto h = __builtin_amdgcn_permlane32_swap(__double2hiint(a), __double2hiint(b), false, false);
    r0 = __hiloint2double(h[0], l[0]);
    r1 = __hiloint2double(h[1], l[1]);
}
// v[l] + v[l ^ 16], then + the other 32 lanes: the sum over the four 16-lane rows, identical in all of them.  COPY64: through
// self_swap16 / self_swap32, as the lane-group kernels call it; the wave and large-LP kernels (wreg_wave.h, ipm_big.hip), one
// wavefront per SIMD and bound by latency, keep the halves and with them their machine code.  Same bits either way.
template <bool COPY64 = false>
__device__ __forceinline__ double quad_sum(double v) {
    if constexpr (COPY64) {
        double r0, r1;
        self_swap16(v, r0, r1);
        self_swap32(r0 + r1, r0, r1);
        return r0 + r1;
    } else {
        int lo = __double2loint(v), hi = __double2hiint(v);
        auto a = __builtin_amdgcn_permlane16_swap(lo, lo, false, false);
        auto b = __builtin_amdgcn_permlane16_swap(hi, hi, false, false);
        v = __hiloint2double(b[0], a[0]) + __hiloint2double(b[1], a[1]);
        lo = __double2loint(v); hi = __double2hiint(v);
        auto c = __builtin_amdgcn_permlane32_swap(lo, lo, false, false);
        auto d = __builtin_amdgcn_permlane32_swap(hi, hi, false, false);
        return __hiloint2double(d[0], c[0]) + __hiloint2double(d[1], c[1]);
    }
}
// a and b are partial sums per 16-lane row: the sum of a over the four rows arrives in rows 0 and 2, that of b in rows 1 and 3.
// Per lane (own + lane ^ 16) + (lane ^ 32) with operands commuted: the bits of two __shfl_xor stages.  Whole wave.
__device__ __forceinline__ double quad_sum2(double a, double b) {
    auto l = __builtin_amdgcn_permlane16_swap(__double2loint(a), __double2loint(b), false, false);   // [0] = rows (a0, b0, a2, b2)
    auto h = __builtin_amdgcn_permlane16_swap(__double2hiint(a), __double2hiint(b), false, false);   // [1] = rows (a1, b1, a3, b3)
    double r0, r1;
    self_swap32(__hiloint2double(h[0], l[0]) + __hiloint2double(h[1], l[1]), r0, r1);
    return r0 + r1;
}
// v of the top / of the bottom 16-lane row of the caller's 32-lane group, in both rows.  Both rows of the group active.
// (A caller that needs both takes them from ONE swap: both_rows_d.)
__device__ __forceinline__ double top_row_d(double v) {
    double r0, r1;
    self_swap16(v, r0, r1);
    return r0;
}
__device__ __forceinline__ double bottom_row_d(double v) {
    double r0, r1;
    self_swap16(v, r0, r1);
    return r1;
}
// both halves of ONE self-swap: returns top_row_d(v), `bot` receives bottom_row_d(v).  Both rows of the group active.
__device__ __forceinline__ double both_rows_d(double v, double& bot) {
    double top;
    self_swap16(v, top, bot);
    return top;
}
// v rotated by 8 lanes inside the TOP 16-lane row of every 32-lane group (lane t takes lane t ^ 8's); the bottom rows keep
// theirs: two v_mov_b32_dpp row_ror:8 row_mask:0x5, in place
__device__ __forceinline__ double ror8_top_d(double v) {
    int lo = __double2loint(v), hi = __double2hiint(v);
    lo = __builtin_amdgcn_update_dpp(lo, lo, 0x128, 0x5, 0xF, false);
    hi = __builtin_amdgcn_update_dpp(hi, hi, 0x128, 0x5, 0xF, false);
    return __hiloint2double(hi, lo);
}
// v of the top row + v of the bottom row / the larger of the two, in both rows: [0] and [1] of one self-swap, the last stage of
// a reduction over a 32-lane group.  The swap overwrites both operands, so it costs two copies more than a ds_swizzle pair
// (+4 vector instructions, -2 LDS instructions and their wait): what that buys is latency, 42 against 73 cycles on a dependent
// path (tools/dev/ubench_xchg.hip, profiles/lane_swaps).  Both rows of the group active.
__device__ __forceinline__ double row_pair_sum(double v) {
    double r0, r1;
    self_swap16(v, r0, r1);
    return r0 + r1;
}
__device__ __forceinline__ double row_pair_max(double v) {
    double r0, r1;
    self_swap16(v, r0, r1);
    return fmax(r0, r1);
}
// sum over the 16 lanes of each DPP row (identical inside the row)
__device__ __forceinline__ double row_sum(double v) {
    asm volatile("" : "+v"(v));
    v += dpp_d<0xB1>(v);
    v += dpp_d<0x4E>(v);
    v += dpp_d<0x141>(v);
    v += dpp_d<0x140>(v);
    return v;
}
// four row sums at once, stage by stage: the eight DPP moves of a stage, then its four adds.  One row_sum is a chain of four
// dependent (move, move, add) triples; four of them written one after the other run one after the other (the compiler keeps
// them apart), which a wavefront alone on its SIMD pays in full.  Same operations and order per sum as row_sum.
__device__ __forceinline__ void row_sum4(double (&v)[4]) {
#define ROW_SUM4_STAGE(C)                                                                      \
    {                                                                                          \
        double t_[4];                                                                          \
        _Pragma("unroll") for (int i = 0; i < 4; i++) t_[i] = dpp_d<C>(v[i]);                  \
        _Pragma("unroll") for (int i = 0; i < 4; i++) asm volatile("" : "+v"(t_[i]));          \
        _Pragma("unroll") for (int i = 0; i < 4; i++) v[i] += t_[i];                           \
        _Pragma("unroll") for (int i = 0; i < 4; i++) asm volatile("" : "+v"(v[i]));           \
    }
#pragma unroll
    for (int i = 0; i < 4; i++) asm volatile("" : "+v"(v[i]));
    ROW_SUM4_STAGE(0xB1) ROW_SUM4_STAGE(0x4E) ROW_SUM4_STAGE(0x141) ROW_SUM4_STAGE(0x140)
#undef ROW_SUM4_STAGE
}
__device__ __forceinline__ double row_max(double v) {
    v = fmax(v, dpp_d<0xB1>(v));
    v = fmax(v, dpp_d<0x4E>(v));
    v = fmax(v, dpp_d<0x141>(v));
    v = fmax(v, dpp_d<0x140>(v));
    return v;
}
// a wave-uniform double, moved to a scalar register pair: the f64 arithmetic that produced it left it in VGPRs, where a
// kernel-lifetime scalar (tolerances, mu, theta, ...) costs two registers of every lane -- or a scratch slot
__device__ __forceinline__ double uni(double v) {
    return __hiloint2double(__builtin_amdgcn_readfirstlane(__double2hiint(v)), __builtin_amdgcn_readfirstlane(__double2loint(v)));
}
// whole-wave reductions: DPP inside the rows, then the four row results through SGPRs (wave-uniform result)
__device__ __forceinline__ double wsum(double v) {
    v = row_sum(v);
    return uni((readlane_d(v, 0) + readlane_d(v, 16)) + (readlane_d(v, 32) + readlane_d(v, 48)));
}
__device__ __forceinline__ double wmax(double v) {
    v = row_max(v);
    return uni(fmax(fmax(readlane_d(v, 0), readlane_d(v, 16)), fmax(readlane_d(v, 32), readlane_d(v, 48))));
}

// Step J of the triangular inverse in the A-operand layout: Ws[s] += (Ws[s] of lane J of the row) * nl for the registers
// s <= J / 4 (columns 4s + q <= J)
template <int J>
__device__ __forceinline__ void winv_step(double (&Ws)[4], double nl) {
    asm volatile("s_nop 1\n\t"
                 ".if 0 <= %5\n\tv_fmac_f64_dpp %0, %0, %4 row_newbcast:" DPP_STR(%5) " row_mask:0xf bank_mask:0xf\n.endif\n\t"
                 ".if 4 <= %5\n\tv_fmac_f64_dpp %1, %1, %4 row_newbcast:" DPP_STR(%5) " row_mask:0xf bank_mask:0xf\n.endif\n\t"
                 ".if 8 <= %5\n\tv_fmac_f64_dpp %2, %2, %4 row_newbcast:" DPP_STR(%5) " row_mask:0xf bank_mask:0xf\n.endif\n\t"
                 ".if 12 <= %5\n\tv_fmac_f64_dpp %3, %3, %4 row_newbcast:" DPP_STR(%5) " row_mask:0xf bank_mask:0xf\n.endif\n\t"
                 : "+v"(Ws[0]), "+v"(Ws[1]), "+v"(Ws[2]), "+v"(Ws[3]) : "v"(nl), "n"(J));
}

// ---- batched LDS reads (see wreg_wave.h for the rest of the family) -------------------------------------------
__device__ __forceinline__ unsigned lds_addr(const void* p) {
    return (unsigned)(size_t)(const __attribute__((address_space(3))) char*)p;
}
#define LDS_RD_(i) "ds_read_b64 %" #i ", %16 offset:%17+%18*" #i "\n\t"
// o[i] = *(double*)(a + OFF0 + STRIDE i), i < 16 (byte address / offsets)
template <int OFF0, int STRIDE>
__device__ __forceinline__ void lds_run16(unsigned a, double* o) {
    asm volatile(LDS_RD_(0) LDS_RD_(1) LDS_RD_(2) LDS_RD_(3) LDS_RD_(4) LDS_RD_(5) LDS_RD_(6) LDS_RD_(7) LDS_RD_(8) LDS_RD_(9)
                 LDS_RD_(10) LDS_RD_(11) LDS_RD_(12) LDS_RD_(13) LDS_RD_(14) LDS_RD_(15) "s_waitcnt lgkmcnt(0)"
                 : "=&v"(o[0]), "=&v"(o[1]), "=&v"(o[2]), "=&v"(o[3]), "=&v"(o[4]), "=&v"(o[5]), "=&v"(o[6]), "=&v"(o[7]),
                   "=&v"(o[8]), "=&v"(o[9]), "=&v"(o[10]), "=&v"(o[11]), "=&v"(o[12]), "=&v"(o[13]), "=&v"(o[14]), "=&v"(o[15])
                 : "v"(a), "n"(OFF0), "n"(STRIDE) : "memory");
}
template <int OFF0, int STRIDE>
__device__ __forceinline__ void lds_run8(unsigned a, double* o) {
    asm volatile("ds_read_b64 %0, %8 offset:%9+%10*0\n\tds_read_b64 %1, %8 offset:%9+%10*1\n\tds_read_b64 %2, %8 offset:%9+%10*2\n\t"
                 "ds_read_b64 %3, %8 offset:%9+%10*3\n\tds_read_b64 %4, %8 offset:%9+%10*4\n\tds_read_b64 %5, %8 offset:%9+%10*5\n\t"
                 "ds_read_b64 %6, %8 offset:%9+%10*6\n\tds_read_b64 %7, %8 offset:%9+%10*7\n\ts_waitcnt lgkmcnt(0)"
                 : "=&v"(o[0]), "=&v"(o[1]), "=&v"(o[2]), "=&v"(o[3]), "=&v"(o[4]), "=&v"(o[5]), "=&v"(o[6]), "=&v"(o[7])
                 : "v"(a), "n"(OFF0), "n"(STRIDE) : "memory");
}
#undef LDS_RD_
// o[4 b + s] = *(double*)(a[s] + OFF0 + STRIDE b), s < 4, b < NB (NB = 1, 2 or 4): the same four lane-dependent addresses in NB
// consecutive slots of a table, one round trip
template <int OFF0, int STRIDE, int NB>
__device__ __forceinline__ void lds_gather4xN(const unsigned (&a)[4], double* o) {
    static_assert(NB == 1 || NB == 2 || NB == 4, "1, 2 or 4 slots");
    if constexpr (NB == 4) {
        asm volatile("ds_read_b64 %0, %16 offset:%20\n\tds_read_b64 %1, %17 offset:%20\n\tds_read_b64 %2, %18 offset:%20\n\tds_read_b64 %3, %19 offset:%20\n\t"
                     "ds_read_b64 %4, %16 offset:%20+%21\n\tds_read_b64 %5, %17 offset:%20+%21\n\tds_read_b64 %6, %18 offset:%20+%21\n\tds_read_b64 %7, %19 offset:%20+%21\n\t"
                     "ds_read_b64 %8, %16 offset:%20+2*%21\n\tds_read_b64 %9, %17 offset:%20+2*%21\n\tds_read_b64 %10, %18 offset:%20+2*%21\n\tds_read_b64 %11, %19 offset:%20+2*%21\n\t"
                     "ds_read_b64 %12, %16 offset:%20+3*%21\n\tds_read_b64 %13, %17 offset:%20+3*%21\n\tds_read_b64 %14, %18 offset:%20+3*%21\n\tds_read_b64 %15, %19 offset:%20+3*%21\n\t"
                     "s_waitcnt lgkmcnt(0)"
                     : "=&v"(o[0]), "=&v"(o[1]), "=&v"(o[2]), "=&v"(o[3]), "=&v"(o[4]), "=&v"(o[5]), "=&v"(o[6]), "=&v"(o[7]),
                       "=&v"(o[8]), "=&v"(o[9]), "=&v"(o[10]), "=&v"(o[11]), "=&v"(o[12]), "=&v"(o[13]), "=&v"(o[14]), "=&v"(o[15])
                     : "v"(a[0]), "v"(a[1]), "v"(a[2]), "v"(a[3]), "n"(OFF0), "n"(STRIDE) : "memory");
    } else if constexpr (NB == 2) {
        asm volatile("ds_read_b64 %0, %8 offset:%12\n\tds_read_b64 %1, %9 offset:%12\n\tds_read_b64 %2, %10 offset:%12\n\tds_read_b64 %3, %11 offset:%12\n\t"
                     "ds_read_b64 %4, %8 offset:%12+%13\n\tds_read_b64 %5, %9 offset:%12+%13\n\tds_read_b64 %6, %10 offset:%12+%13\n\tds_read_b64 %7, %11 offset:%12+%13\n\t"
                     "s_waitcnt lgkmcnt(0)"
                     : "=&v"(o[0]), "=&v"(o[1]), "=&v"(o[2]), "=&v"(o[3]), "=&v"(o[4]), "=&v"(o[5]), "=&v"(o[6]), "=&v"(o[7])
                     : "v"(a[0]), "v"(a[1]), "v"(a[2]), "v"(a[3]), "n"(OFF0), "n"(STRIDE) : "memory");
    } else {
        asm volatile("ds_read_b64 %0, %4 offset:%8\n\tds_read_b64 %1, %5 offset:%8\n\tds_read_b64 %2, %6 offset:%8\n\tds_read_b64 %3, %7 offset:%8\n\t"
                     "s_waitcnt lgkmcnt(0)"
                     : "=&v"(o[0]), "=&v"(o[1]), "=&v"(o[2]), "=&v"(o[3])
                     : "v"(a[0]), "v"(a[1]), "v"(a[2]), "v"(a[3]), "n"(OFF0) : "memory");
    }
}
// o[i] = *(double*)(a + OFF0 + STRIDE i), i < N, any N: runs of 16 / 8 and a tail of single reads
template <int OFF0, int STRIDE, int N>
__device__ __forceinline__ void lds_run(unsigned a, double* o) {
    if constexpr (N >= 16) { lds_run16<OFF0, STRIDE>(a, o); lds_run<OFF0 + 16 * STRIDE, STRIDE, N - 16>(a, o + 16); }
    else if constexpr (N >= 8) { lds_run8<OFF0, STRIDE>(a, o); lds_run<OFF0 + 8 * STRIDE, STRIDE, N - 8>(a, o + 8); }
    else if constexpr (N >= 4) {
        asm volatile("ds_read_b64 %0, %4 offset:%5\n\tds_read_b64 %1, %4 offset:%5+%6\n\tds_read_b64 %2, %4 offset:%5+2*%6\n\tds_read_b64 %3, %4 offset:%5+3*%6\n\t"
                     "s_waitcnt lgkmcnt(0)" : "=&v"(o[0]), "=&v"(o[1]), "=&v"(o[2]), "=&v"(o[3]) : "v"(a), "n"(OFF0), "n"(STRIDE) : "memory");
        lds_run<OFF0 + 4 * STRIDE, STRIDE, N - 4>(a, o + 4);
    } else if constexpr (N >= 1) {
        asm volatile("ds_read_b64 %0, %1 offset:%2\n\ts_waitcnt lgkmcnt(0)" : "=&v"(o[0]) : "v"(a), "n"(OFF0) : "memory");
        lds_run<OFF0 + STRIDE, STRIDE, N - 1>(a, o + 1);
    }
}

#endif  // PYCLLP_WAVE_COMMON_H
