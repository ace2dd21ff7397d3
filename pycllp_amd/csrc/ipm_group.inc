// ipm_group.inc -- second-generation solve kernel: one LP per LANE GROUP (MP lanes), G = 64/MP LPs per wavefront.
//
// Why: in the first-generation wave-per-LP kernel (since removed) the LDL' factorisation and the triangular solves kept one
// matrix row per lane, so with m <= 32 only half (m <= 16: a quarter) of the 64 lanes worked during ~50 % of the run time.
// Here the lanes [g*MP, (g+1)*MP) of a wave form a group that owns its own LP for the whole solve:
//   * m-vectors: lane gl = lane % MP holds element gl of its group's LP (no replication);
//   * N-vectors: NCG = NP/MP registers per lane, column j = gl + MP*q;
//   * the row-per-lane phases (LDL', forward/back substitution, A*dx) and the column-per-lane phases (A'u, step,
//     ratio test, norms) are ONE instruction stream serving G LPs;
//   * the Gram product still uses the whole wave per LP on the matrix cores (v_mfma_f64_16x16x4_f64; 32-row groups:
//     the diagonal blocks' lower tiles on v_mfma_f64_4x4x4_4b_f64, see gram_pair()), groups taking turns;
//     its operands now come straight from ONE row-major image of A in LDS (odd row stride: the
//     row-per-lane reads are conflict free, the MFMA-order reads see a harmless 2-way conflict);
//   * an LP's FIRST Gram product is not formed at all without warm start: x = z = 1 there, so it is A A' whatever b and c are,
//     and the wave copies it (and A 1) from an image the handle made once (first_gram_kernel; GWave::gram_first; MP = 32);
//   * group reductions use DPP row operations (+ one lane swap between the two rows of a 32-lane group) instead of ds_bpermute;
//   * the LDL' column sweep hands the RAW column (pivot included) through LDS, so no cross-lane pivot broadcast
//     sits on the critical path: every lane derives 1/D_j itself from the broadcast read;
//   * groups are independent slots: a slot that finishes its LP stores it and immediately loads its next one, so
//     differing iteration counts inside a wave cost nothing.
// SL = true ("slack aware"): when the last m columns of A are the identity -- the equality form of a StandardLP,
// [A | I] (pycllp/lp.py:551-567) -- those columns never enter the dense machinery: their N-vector entries live in
// the LAST register of every lane (slack i in lane gl = i), A'u is u_i, A v adds v_slack_i to row i and the Gram
// product only gets d_slack_i added to its diagonal.  The image of A, the k-layout staging and the MFMA loop then
// cover n - m columns instead of n (16 instead of 24 k-steps per LP-iteration at (32, 64+32)).
// Semantics are those of oracle/ipm_dense_ref.c (see ipm_dense.hip header); x/z, mu/x and the ratio test use
// v_rcp_f64 + 2 Newton steps instead of IEEE division (<= 2 ulp).

#ifndef PYCLLP_SPLITJ
#define PYCLLP_SPLITJ 6    // LDL' columns whose broadcast reads are issued in two batches (register pressure)
#endif
#ifndef PYCLLP_GRAM_UNROLL
#define PYCLLP_GRAM_UNROLL 4   // chunks of 4 k-steps of the Gram loop unrolled together (A/B: 1 -> 7.10 ms, 2 -> 7.06, 4 -> 7.00)
#endif
#ifndef PYCLLP_AT_RB
#define PYCLLP_AT_RB 4     // rows of A per batch of the pipelined A'u
#endif
#ifndef PYCLLP_A_CB
#define PYCLLP_A_CB 8      // columns of A per batch of the pipelined A v
#endif
#ifndef PYCLLP_SOLVE_PRIO
#define PYCLLP_SOLVE_PRIO 2    // s_setprio level inside the substitution (with PYCLLP_FACTOR_PRIO 2: 5.93 -> 5.91 ms; each alone: nothing)
#endif
#ifndef PYCLLP_FACTOR_PRIO
#define PYCLLP_FACTOR_PRIO 2       // s_setprio level of a wave inside the LDL' sweep, plain / predictor-corrector kernels (0: none)
#endif
#ifndef PYCLLP_FACTOR_PRIO_HSD
#define PYCLLP_FACTOR_PRIO_HSD 3   // ... of the HSD kernel (see GWave::factor_dpp)
#endif
#ifndef PYCLLP_WPB
#define PYCLLP_WPB 8        // waves per workgroup of the group kernel (LDS at (32,96) slack-aware: 8 x 17.5 KB + 17.5 KB)
#endif

// Tile schedule of the MP = 32 Gram product's two DIAGONAL 16x16 blocks on v_mfma_f64_4x4x4_4b_f64 (four independent 4x4x4
// products per instruction).  The 32 rows are 8 row tiles of 4; M = A D A' is symmetric and only its lower triangle is read, so a
// diagonal 16-block needs 10 of its 16 tiles.  Five instructions cover the 20 tiles exactly once: block b of instruction r
// multiplies the OWNER tile (its rows scaled by d, the A operand) with the PARTNER tile (plain A, the B operand).  A pair whose
// partner lies below its owner is the transpose of the wanted lower tile and is stored transposed.  The reference scales the
// LOWER row of an entry, (a_ik d_k) a_jk with i >= j, and so does the 16x16 form here; a transposed pair scales the upper one
// (same sum, products rounded differently), so the owner is the lower tile wherever the lane's own tiles allow it: 8 of the 12
// off-diagonal pairs (all twelve would take a multiply or a select per instruction and k-step, more than the tiles save).
// (The off-diagonal 16-block has no waste and stays one v_mfma_f64_16x16x4_f64, whose operands are the two loads the lane makes
// anyway.)
struct GramPair { int own, par; };
constexpr int GRAM_INSTS = 5;
constexpr GramPair gram_pair(int r, int b) {
    return r == 0 ? GramPair{b, b} : r == 1 ? GramPair{b + 4, b + 4} : r == 2 ? GramPair{b, (b + 3) & 3}
         : r == 3 ? GramPair{b + 4, 4 + ((b + 3) & 3)} : (b < 2 ? GramPair{b, b + 2} : GramPair{b + 4, b + 2});
}
constexpr bool gram_pairs_cover_diagonal_blocks() {
    int cnt[8][8] = {};
    for (int r = 0; r < GRAM_INSTS; r++)
        for (int b = 0; b < 4; b++) {
            const GramPair t = gram_pair(r, b);
            cnt[t.own > t.par ? t.own : t.par][t.own > t.par ? t.par : t.own]++;
        }
    for (int i = 0; i < 8; i++)
        for (int j = 0; j < 8; j++)
            if (cnt[i][j] != ((j <= i && i / 4 == j / 4) ? 1 : 0)) return false;
    return true;
}
static_assert(gram_pairs_cover_diagonal_blocks(), "the five instructions must cover the 20 lower tiles of the diagonal blocks exactly once");

template <int MP, int NP, bool SL = false>
struct GeoG {
    static_assert(MP == 16 || MP == 32, "row padding must be 16 or 32");
    static_assert(NP % MP == 0 && NP % 8 == 0 && NP <= 128, "column padding must be a multiple of MP and 8, <= 128");
    static_assert(!SL || NP >= 2 * MP, "the slack-aware variant needs at least one dense register");
    static constexpr int G = 64 / MP;        // LPs per wave
    static constexpr int NCG = NP / MP;      // N-vector registers per lane (dense ones + the slack register if SL)
    static constexpr int ND = SL ? NP - MP : NP;   // (padded) dense columns: what the A image / MFMA loop cover
    static constexpr int NCD = ND / MP;      // dense registers per lane
    static constexpr int JB = MP / 16;
    static constexpr int KS = ND / 4;
    static constexpr int AS = ND + 1;        // odd row stride of the A image
    static constexpr int AIMG = MP * AS;
    // Slab addressing.  MP = 16: rows are MP + 2 doubles apart (the padding spreads a column over the banks).
    // MP = 32: rows are exactly 32 doubles apart and the column index is XOR-swizzled with the row in units of 16-byte
    // pairs, col ^ ((row & 15) << 1): a column (one entry per lane) still hits 16 distinct pairs of banks, pairs stay
    // adjacent and aligned for ds_read_b128, and the 2 padding doubles per row -- 1 KB per wave -- are what lets an 8th
    // wave fit into the 160 KB of a CU at (32, 96).
    static constexpr bool SWZ = (MP == 32);
    static constexpr int MS = SWZ ? MP : MP + 2;
    __host__ __device__ static constexpr int sidx(int row, int col) {
        return SWZ ? row * MS + (col ^ ((row & 15) << 1)) : row * MS + col;
    }
    static constexpr int SLAB = MP * MS;
    static constexpr int STAGE = 3 * ND;     // k-layout x, d, d*t of one LP; also reused for G*ND / G*MP vector staging
    static constexpr int STAGE_A = (G * ND > STAGE) ? G * ND : STAGE;
    static constexpr int STAGE_SZ = (2 * G * MP > STAGE_A) ? 2 * G * MP : STAGE_A;   // 2 G MP: the two-vector A'u of the HSD kernel
    // MP = 32: where lane l of Gram instruction r stores its result, as a byte offset into the LP's slab (swizzle included), one
    // 16-bit entry per (r, lane).  Operand / result lane map of the instruction (tools/dev/ubench_mfma4.hip): A[i][k] in lane
    // 16 k + 4 b + i, B[k][j] in lane 16 k + 4 b + j, D[i][j] in lane 16 i + 4 b + j.  A per-workgroup LDS table: derived from the
    // lane bits in every call the offsets cost several integer instructions each, read from here a load and an add.
    __host__ __device__ static constexpr int gram_store(int r, int lane) {
        const GramPair t = gram_pair(r, (lane >> 2) & 3);
        const int ro = 4 * t.own + (lane >> 4), rp = 4 * t.par + (lane & 3);
        return 8 * (t.par > t.own ? sidx(rp, ro) : sidx(ro, rp));
    }
    // Row GRAM_INSTS of the table: byte offset into the A image of the lane's row of partner tile (b + 3) % 4, which wraps for
    // b = 0 (the same row of tile 4 + (b + 3) % 4 is 16 rows below: an immediate).
    __host__ __device__ static constexpr int gram_wrap(int lane) { return 8 * AS * (((lane & 15) + 12) & 15); }
    static constexpr int GROWS = GRAM_INSTS + 1;
    static constexpr int GTAB = (MP == 32) ? GROWS * 64 / 4 : 0;   // doubles
    static constexpr int GTAB_OFF = AIMG + ND;                     // behind the A image and the column sums
    // (every kernel fills it next to the A image; the workgroup barrier that publishes the image publishes the table)
    __device__ static void fill_gram_table(double* lds, int tid, int nthreads) {
        if constexpr (MP == 32) {
            unsigned short* tab = (unsigned short*)(lds + GTAB_OFF);
            for (int i = tid; i < GROWS * 64; i += nthreads)
                tab[i] = (unsigned short)(i < GRAM_INSTS * 64 ? gram_store(i >> 6, i & 63) : gram_wrap(i & 63));
        }
    }
    static constexpr int SHARED = GTAB_OFF + GTAB;            // A image + column sums (A'1) + Gram store offsets
    static constexpr int WSZ = G * SLAB + STAGE_SZ;            // per-wave doubles
    static constexpr size_t lds_bytes(int wpb) { return sizeof(double) * (size_t)(SHARED + wpb * WSZ); }
    __host__ __device__ static constexpr int kpos(int j) { return (j & 3) * KS + (j >> 2); }
};

// sum / max over the MP lanes of each group; every lane of the group receives the result
// MP = 32: the last stage is a lane swap between the group's two 16-lane rows, which moves active lanes only.  Every call site
// is reached by whole 32-lane groups: the kernels' bodies and GWave's members run under wave-uniform conditions, and the one
// per-group condition (finalize(), whose verdict every lane of a group derives from these very sums) keeps both rows of a group
// together.  A reduction across groups (v_permlane32_swap) would not be allowed there.
template <int MP>
__device__ __forceinline__ double grp_sum(double v) {
    // v is pinned first: were its producer a product, the compiler would contract the first stage into
    // fma(a, b, partner) on one lane and fma(a', b', round(a b)) on the partner -- two different roundings, and the
    // lanes of a group would no longer hold bit-identical sums (every lane takes its own copy of a group-wide scalar
    // such as a step length from these sums)
    asm volatile("" : "+v"(v));
    v += dpp_d<0xB1>(v);    // quad_perm(1,0,3,2): xor 1
    v += dpp_d<0x4E>(v);    // quad_perm(2,3,0,1): xor 2
    v += dpp_d<0x141>(v);   // row_half_mirror: the other quad of each 8
    v += dpp_d<0x140>(v);   // row_mirror: the other 8 of each 16
    if (MP == 32) v = row_pair_sum(v);   // top + bottom in both rows: the bits of own + other
    return v;
}
template <int MP>
__device__ __forceinline__ double grp_max(double v) {
    v = fmax(v, dpp_d<0xB1>(v));
    v = fmax(v, dpp_d<0x4E>(v));
    v = fmax(v, dpp_d<0x141>(v));
    v = fmax(v, dpp_d<0x140>(v));
    if (MP == 32) v = row_pair_max(v);
    return v;
}
// ---- stop and growth tests of ipm_group_kernel on the SQUARES of the two residual norms ----
// The norms |rho| and |sigma| are only ever compared: with the tolerances, with ten times their value one iteration earlier, with
// the growth floor, and for finiteness.  Two correctly rounded square roots per iteration bought nothing else.  The kernel
// carries r2 = |rho|^2 and s2 = |sigma|^2 and keeps the previous pass's as squares (r2_0, s2_0; +inf before the first pass, where
// the norms had 1e300: a finite norm is below 2^512, so "greater than ten times it" is false under either).
//
// ALL CLEAR, the verdict of all but a pass or two of an LP: no test holds, decided on the squares with a factor of two to spare
// where an ulp decides on the square roots.  With h = fl(s / 2) (exact, or the nearest subnormal) and P = fl(T |T|):
//   (a)  h > P    =>  "sqrt(s) <= T" fails                (s >= 2 h - 2^-1074 > T^2: sqrt(s) > T, and rounding is monotone)
//   (b)  h < s0   =>  "sqrt(s) > 10 sqrt(s0)" fails       (s0 > 0 and s <= 3 s0: sqrt(s) < 1.74 sqrt(s0))
//   (c)  h < P    =>  "sqrt(s) > FLOOR T" fails           (T > 0 and s < 4 T^2: sqrt(s) < 2 T)
// and the pass is clear if gam is finite, (a) holds for r2 or for s2 or gam fails its own test, and (b) or (c) holds for each of
// r2 and s2.  All three compares are strict, which is what makes them safe where a product underflows: a P below 2^-1022 is
// within 2^-1075 of T^2, and h and P are then multiples of 2^-1074 that differ.  An overflowed P, a NaN or an infinite square
// fail the compares they stand in ((c) holds against P = +inf, rightly: T > 2^511).  T |T| has the sign of a negative T (a
// negative eps), for which nothing is <= T and everything above FLOOR T.  tests/test_norm_squares.py restates the three in numpy
// against the square roots.  Two multiplies and three compares per norm, no constant but 1/2.
// THE EXACT PATH, every other pass of an LP -- as a rule the one it ends with -- and every pass under PYCLLP_FLAG_EXACT_NORMS: the
// text these kernels had, the square roots of r2, s2, r2_0, s2_0 (the last two are the very norms the previous pass tested) and
// the comparisons on them.  A cold branch of the wave.  (A middle tier that decided each comparison on the squares behind a
// band of 2^-40 was built as well: its mask arithmetic cost the (32, 96) predictor-corrector kernels spilt VGPRs and every
// kernel about twenty SGPRs spilt to lanes, for one pass per LP; profiles/swap_copies_norm_squares.)
// Returns the status the pass ends with, or -1: none of the tests holds.  No cross-lane operation: callable under any mask;
// only `active` lanes send the wave down the exact path.
__device__ __forceinline__ int stop_verdict_exact(double r2, double s2, double gam, double po, double tol_r, double tol_s,
                                                  double r2_0, double s2_0, double eps) {
    const double normr = sqrt(r2), norms = sqrt(s2), normr0 = sqrt(r2_0), norms0 = sqrt(s2_0);
    if (!(isfinite(normr) && isfinite(norms) && isfinite(gam))) return PYCLLP_STATUS_NUMERICAL;
    if (normr <= tol_r && norms <= tol_s && gam <= eps * (1.0 + fabs(po))) return PYCLLP_STATUS_OPTIMAL;
    if (normr > 10.0 * normr0 && normr > PYCLLP_GROWTH_FLOOR * tol_r) return PYCLLP_STATUS_PRIMAL_INFEASIBLE;
    if (norms > 10.0 * norms0 && norms > PYCLLP_GROWTH_FLOOR * tol_s) return PYCLLP_STATUS_DUAL_INFEASIBLE;
    return -1;
}
__device__ __forceinline__ int stop_verdict(double r2, double s2, double gam, double po, double tol_r, double tol_s,
                                            double r2_0, double s2_0, double eps, bool active, bool exact_always) {
    const double Pr = tol_r * fabs(tol_r), Ps = tol_s * fabs(tol_s);
    const double r_h = 0.5 * r2, s_h = 0.5 * s2;
    const bool gam_ok = gam <= eps * (1.0 + fabs(po));
    // (& and |: the compares in a row and mask arithmetic, where && and || become a branch each)
    const bool clear = (bool)isfinite(gam) & ((r_h > Pr) | (s_h > Ps) | !gam_ok) & ((r_h < r2_0) | (r_h < Pr)) & ((s_h < s2_0) | (s_h < Ps));
    const bool exact = active & (exact_always | !clear);
    int v = -1;
    if (__any(exact)) {
        const int ve = stop_verdict_exact(r2, s2, gam, po, tol_r, tol_s, r2_0, s2_0, eps);
        if (exact) v = ve;
    }
    return v;
}

// value held by lane k (0 <= k < MP, wave-uniform) of the caller's own group
template <int MP>
__device__ __forceinline__ double grp_bcast(double v, int k, int grp) {
    if (MP == 32) {
        const double a = readlane_d(v, k), b = readlane_d(v, 32 + k);
        return grp ? b : a;
    } else {
        const double a = readlane_d(v, k), b = readlane_d(v, 16 + k), c = readlane_d(v, 32 + k), d = readlane_d(v, 48 + k);
        return (grp & 2) ? ((grp & 1) ? d : c) : ((grp & 1) ? b : a);
    }
}

template <int MP, int NP, bool SL = false>
struct GWave {
    using G_ = GeoG<MP, NP, SL>;
    static constexpr int G = G_::G, NCG = G_::NCG, NCD = G_::NCD, ND = G_::ND, JB = G_::JB, KS = G_::KS, AS = G_::AS, MS = G_::MS;

    const double* Aimg;   // LDS: row-major A, row stride AS
    static constexpr bool COLB = MP == 32 && NP <= 96;   // (at NP = 128 the sixteen registers are not to spare)
    static constexpr bool ROWB = COLB && SL;     // (the variants without the identity tail carry one more N-vector register each: no room)
    // The sweep stores L column by column and carries the first solve's right-hand side (factor_dpp_fwd) where that is free:
    // the (32, 128) shapes have neither the address registers nor room for the carried values (10-19 registers spilt with them).
    static constexpr bool CARRY = COLB || MP == 16;
    // The sweep shares the rank-1 updates of the bottom-right 16 x 16 block between both DPP rows of the group (factor_sweep).
    static constexpr bool SPLIT = MP == 32;
    unsigned rb[ROWB ? 16 : 1];   // ... and of the sixteen 16-byte pairs of the lane's own ROW (load_own_row), swizzle included
    unsigned xb[COLB ? 16 : 1];   // MP = 32: LDS byte address of slab entry (row c, column gl), c < 16, swizzle included: entry (k, gl) of the
                          // factor's column layout is at xb[k & 15] + 256 (k & 16).  Kernel-lifetime values (16 registers, which the kernel
                          // has to spare since round 3) instead of an XOR and a shift-add per access in the sweep's final store and
                          // in every substitution's column loads.
    double* slab;         // LDS: this lane's GROUP slab (MP x MS)
    double* slab0;        // LDS: slab of group 0 of this wave
    double* stage;        // LDS: wave-private staging region
    int lane, gl, grp, m, n;

    // row gl of the own group's slab into registers, as explicit 16-byte loads (with the swizzle the compiler can no
    // longer see that entries 2p and 2p+1 are neighbours)
    // The lane's index inside its group, opaque to the optimiser.  The swizzled slab addresses are lane ^ constant; taken
    // from the plain `gl` they are loop invariants of the whole solve, get hoisted out of it and then occupy (and spill)
    // registers for good -- recomputing them where they are used costs one VALU op each.
    __device__ __forceinline__ int ogl() const { int g = gl; asm volatile("" : "+v"(g)); return g; }

    __device__ __forceinline__ void load_own_row(double (&out)[MP]) const {
        typedef double double2_t __attribute__((ext_vector_type(2)));
        if constexpr (ROWB) {
#pragma unroll
            for (int p2 = 0; p2 < MP / 2; p2++) {
                const double2_t t = *(const __attribute__((address_space(3))) double2_t*)(size_t)rb[p2];
                out[2 * p2] = t[0]; out[2 * p2 + 1] = t[1];
            }
            return;
        }
        const int g = ogl();
        const double2_t* rp = (const double2_t*)(slab + g * MS);
        const int g15 = G_::SWZ ? (g & 15) : 0;
#pragma unroll
        for (int p2 = 0; p2 < MP / 2; p2++) {
            const double2_t t = rp[p2 ^ g15];
            out[2 * p2] = t[0]; out[2 * p2 + 1] = t[1];
        }
    }

    // The row as the SPLIT sweep wants it.  Bottom lanes (gl >= 16): load_own_row.  Top lane t: its own row, except that W[24 + s],
    // s = 0 .. 7 -- don't-care values of the upper triangle there -- take M[R][16 + s] of row R = 16 + (t ^ 8), the half of the
    // bottom-right block that the lane updates for the bottom lane t ^ 8.  Pair 8 + q, q < 4, of row R sits at pair
    // (8 + q) ^ (R & 15) = q ^ t of that row: the address of the lane's own pair 12 + q plus ONE per-lane offset (the rows are
    // R - t = 24 or 8 apart, and (12 + q) ^ t - (q ^ t) = 12 - 2 (t & 12) whatever q < 4 is), formed here and not held.
    // backward() keeps load_own_row: the top lanes use lb[16 .. 31] there.
    // (Why not rb[q] + 256 (R - t), which needs no swizzle term: the bottom lanes want rb[12 + q], so that form is a select between
    // two address registers per pair; this one is an add of a value that is 0 in the bottom lanes.)
    // The three helpers below are that offset in the two address forms, shared with merge_through_slab.  Bit arithmetic on the
    // opaque g, not selects between constants: those are loop invariants to the compiler, which gives each a register for the
    // whole kernel, and the headline kernel has none to spare.
    __device__ __forceinline__ static unsigned top_lanes(int g) { return (((unsigned)g >> 4) & 1u) - 1u; }   // all ones in the top lanes, 0 in the bottom lanes
    // ROWB: bytes from rb[12 + q] to pair 8 + q of row R: 256 (R - t) - 16 (12 - 2 (t & 12)), R - t = 24 - 2 (t & 8); 0 in the bottom lanes
    __device__ __forceinline__ static unsigned split_off(int g) {
        return (5952u - (((unsigned)g & 8u) << 9) + (((unsigned)g & 12u) << 5)) & top_lanes(g);
    }
    // pointer form: 16-byte pairs from the own row to row R, and the swizzle term of pairs 12 .. 15 ((p2 ^ 12) ^ t = q ^ t for p2 = 12 + q)
    __device__ __forceinline__ static unsigned split_row(int g) { return ((24u - 2u * ((unsigned)g & 8u)) * (unsigned)(MS / 2)) & top_lanes(g); }
    __device__ __forceinline__ static int split_swz(int g) { return (g & 15) ^ (int)(12u & top_lanes(g)); }
    template <bool SP = SPLIT>
    __device__ __forceinline__ void load_row_for_sweep(double (&out)[MP]) const {
        if constexpr (!SP) {
            load_own_row(out);
        } else {
            typedef double double2_t __attribute__((ext_vector_type(2)));
            const int g = ogl();
            if constexpr (ROWB) {
                const unsigned off = split_off(g);
#pragma unroll
                for (int p2 = 0; p2 < MP / 2; p2++) {
                    const double2_t t = *(const __attribute__((address_space(3))) double2_t*)(size_t)(rb[p2] + (p2 >= 12 ? off : 0u));
                    out[2 * p2] = t[0]; out[2 * p2 + 1] = t[1];
                }
            } else {
                const double2_t* rp = (const double2_t*)(slab + g * MS);
                const int g15 = g & 15;
                const double2_t* rs = rp + split_row(g);   // row R (top lanes)
                const int g15s = split_swz(g);
#pragma unroll
                for (int p2 = 0; p2 < MP / 2; p2++) {
                    const double2_t t = p2 >= 12 ? rs[p2 ^ g15s] : rp[p2 ^ g15];
                    out[2 * p2] = t[0]; out[2 * p2 + 1] = t[1];
                }
            }
        }
    }

    // The merge behind column 15 of the SPLIT sweep: every lane puts its W[24 .. 31] back where load_row_for_sweep took them from
    // (the top lanes: columns 16 .. 23 of row R; the bottom lanes: columns 24 .. 31 of their own row, which nobody reads), then
    // re-reads columns 16 .. 23 of its own row into W[16 .. 23]: four ds_write_b128 and four ds_read_b128 at addresses that
    // exist already, no EXEC switch.  Rows 16 .. 31 of the slab are dead between the row load and the stores of columns 16 .. 31
    // (columns 0 .. 15 of L go to rows 0 .. 15; the (32, 128) shapes store L behind the sweep).  The top lanes receive
    // don't-care values, as before.
    __device__ __forceinline__ void merge_through_slab(double (&W)[MP]) const {
        typedef double double2_t __attribute__((ext_vector_type(2)));
        const int g = ogl();
        if constexpr (ROWB) {
            const unsigned off = split_off(g);
#pragma unroll
            for (int q = 0; q < 4; q++) {
                double2_t t; t[0] = W[24 + 2 * q]; t[1] = W[25 + 2 * q];
                *(__attribute__((address_space(3))) double2_t*)(size_t)(rb[12 + q] + off) = t;
            }
            wave_lds_sync();
#pragma unroll
            for (int q = 0; q < 4; q++) {
                const double2_t t = *(const __attribute__((address_space(3))) double2_t*)(size_t)rb[8 + q];
                W[16 + 2 * q] = t[0]; W[17 + 2 * q] = t[1];
            }
        } else {
            double2_t* rp = (double2_t*)(slab + g * MS);
            const int g15 = g & 15;
            double2_t* rs = rp + split_row(g);
            const int g15s = split_swz(g);
#pragma unroll
            for (int q = 0; q < 4; q++) {
                double2_t t; t[0] = W[24 + 2 * q]; t[1] = W[25 + 2 * q];
                rs[(12 + q) ^ g15s] = t;
            }
            wave_lds_sync();
#pragma unroll
            for (int q = 0; q < 4; q++) {
                const double2_t t = rp[(8 + q) ^ g15];
                W[16 + 2 * q] = t[0]; W[17 + 2 * q] = t[1];
            }
        }
    }

    // out_q = sum_i A[i][gl + MP q] * u_i   (u: lane = row of own group)  -- A'u
    // Software pipelined by hand: rows are fetched in batches of RB into two register buffers; a batch is pinned
    // (waited for) only after the next batch's loads have been issued.  Left alone, the scheduler sinks every LDS
    // read next to its FMA and the loop runs at LDS latency.  The partial sums are pinned after every batch too: left free,
    // the scheduler may sink every FMA below the last batch's loads and keep the whole image of A live at once (the
    // predictor-corrector kernel spilled 96-433 registers that way; 6.06 -> 5.45 ms at (32, 96)).
    // u_i comes from registers: a DPP row broadcast (lane i & 15) of the u of the group's top or bottom 16-lane row, which one lane
    // swap hands to both rows (whole wave active at every call site).  STAGED: u through the wave's staging area instead -- a
    // write, a wave sync and MP broadcast reads, as before the lane swaps -- for the kernel that pays for the registers with
    // scratch (AT_STAGED in the HSD kernel).  Same FMAs in the same order either way.
    // FUSED (not with STAGED): no copy of u_i at all -- each FMA takes the row broadcast itself (v_fmac_f64_dpp, as subst15_up):
    // the same two factors and the same addend, so the same bits, for two moves per row of A less.  The s_nop in front of a
    // batch covers the VALU-write -> DPP-read hazard of `ur`, which the hazard recogniser does not see through inline asm.
    // One statement per batch, so that nothing the compiler places (a copy of `ur`, say) can stand between the s_nop and a DPP read.
    template <int K0>
    __device__ __forceinline__ static void at_batch_fused(double (&out)[NCG], double ur, const double (&a)[PYCLLP_AT_RB][NCD]) {
        static_assert(PYCLLP_AT_RB == 4 && NCD == 2, "written for batches of four rows and two dense registers per lane");
        asm volatile("s_nop 1\n\t"
                     "v_fmac_f64_dpp %0, %2, %3 row_newbcast:" DPP_STR(%11) " row_mask:0xf bank_mask:0xf\n\t"
                     "v_fmac_f64_dpp %1, %2, %4 row_newbcast:" DPP_STR(%11) " row_mask:0xf bank_mask:0xf\n\t"
                     "v_fmac_f64_dpp %0, %2, %5 row_newbcast:" DPP_STR(%12) " row_mask:0xf bank_mask:0xf\n\t"
                     "v_fmac_f64_dpp %1, %2, %6 row_newbcast:" DPP_STR(%12) " row_mask:0xf bank_mask:0xf\n\t"
                     "v_fmac_f64_dpp %0, %2, %7 row_newbcast:" DPP_STR(%13) " row_mask:0xf bank_mask:0xf\n\t"
                     "v_fmac_f64_dpp %1, %2, %8 row_newbcast:" DPP_STR(%13) " row_mask:0xf bank_mask:0xf\n\t"
                     "v_fmac_f64_dpp %0, %2, %9 row_newbcast:" DPP_STR(%14) " row_mask:0xf bank_mask:0xf\n\t"
                     "v_fmac_f64_dpp %1, %2, %10 row_newbcast:" DPP_STR(%14) " row_mask:0xf bank_mask:0xf"
                     : "+v"(out[0]), "+v"(out[1])
                     : "v"(ur), "v"(a[0][0]), "v"(a[0][1]), "v"(a[1][0]), "v"(a[1][1]), "v"(a[2][0]), "v"(a[2][1]), "v"(a[3][0]), "v"(a[3][1]),
                       "n"(K0), "n"(K0 + 1), "n"(K0 + 2), "n"(K0 + 3));
    }
    template <bool STAGED = false, bool FUSED = false>
    __device__ __forceinline__ void At_times(double u, double (&out)[NCG]) const {
        static_assert(!(STAGED && FUSED), "FUSED reads u from registers");
        const int g = ogl();
        double ur[2] = {u, u};
        const __attribute__((address_space(3))) double* ub = nullptr;
        if constexpr (STAGED) {
            stage[grp * MP + g] = u;
            wave_lds_sync();
            unsigned uba = lds_addr(stage + grp * MP);      // opaque: see A_times
            asm volatile("" : "+v"(uba));
            ub = (const __attribute__((address_space(3))) double*)(size_t)uba;
        } else if constexpr (MP == 32) {
            ur[0] = both_rows_d(u, ur[1]);     // one swap (two calls would be two: the pinned copies are not shared)
        }
        const double* ac = Aimg + g;
        constexpr int RB = PYCLLP_AT_RB, NB = MP / RB;
        double a0[RB][NCD], a1[RB][NCD], u0[RB], u1[RB];
#define AT_LOAD(A_, U_, I0)                                                                     \
    static_for<0, RB>([&](auto ic_) {                                                           \
        constexpr int ii = decltype(ic_)::value, i_ = (I0) + ii;                                \
        if constexpr (STAGED) U_[ii] = ub[i_ + tok];                                            \
        else if constexpr (!FUSED) U_[ii] = row_bcast<(i_ & 15)>(ur[i_ >> 4]);                  \
        _Pragma("unroll") for (int q = 0; q < NCD; q++) A_[ii][q] = ac[i_ * AS + MP * q + tok]; \
    });
#define AT_USE(A_, U_, I0)                                                                      \
    _Pragma("unroll") for (int ii = 0; ii < RB; ii++) {                                         \
        if constexpr (!FUSED) asm volatile("" : "+v"(U_[ii]));                                  \
        _Pragma("unroll") for (int q = 0; q < NCD; q++) asm volatile("" : "+v"(A_[ii][q]));     \
    }                                                                                           \
    asm volatile("" : "+v"(tok));                                                               \
    if constexpr (FUSED) {                                                                      \
        at_batch_fused<(I0) & 15>(out, ur[(I0) >> 4], A_);                                      \
    } else {                                                                                 \
        _Pragma("unroll") for (int ii = 0; ii < RB; ii++)                                       \
            _Pragma("unroll") for (int q = 0; q < NCD; q++) out[q] = fma(A_[ii][q], U_[ii], out[q]); \
    }                                                                                           \
    _Pragma("unroll") for (int q = 0; q < NCD; q++) asm volatile("" : "+v"(out[q]));
#pragma unroll
        for (int q = 0; q < NCG; q++) out[q] = 0.0;
        if (SL) out[NCG - 1] = u;   // slack column i of lane gl = i: (A'u)_slack = u_i (u is 0 in padded rows)
        // `tok` is an opaque zero refreshed after every pin: the next batch's addresses depend on it, so at most
        // two batches are in flight (without it every load is hoisted to the top and the kernel spills).  It is ADDED to the
        // index, never scaled: (row + tok) * AS cost a 64-bit multiply-add (quarter rate) per batch
        int tok = 0;
        asm volatile("" : "+v"(tok));
        AT_LOAD(a0, u0, 0)
        static_for<0, NB / 2>([&](auto bc) {
            constexpr int b2 = 2 * decltype(bc)::value;
            AT_LOAD(a1, u1, (b2 + 1) * RB)
            AT_USE(a0, u0, b2 * RB)
            if constexpr (b2 + 2 < NB) { AT_LOAD(a0, u0, (b2 + 2) * RB) }
            AT_USE(a1, u1, (b2 + 1) * RB)
        });
#undef AT_LOAD
#undef AT_USE
        if constexpr (STAGED) wave_lds_sync();
    }

    // (A v)_gl with v given per column of the own group's LP -- row-per-lane, conflict-free thanks to the odd stride;
    // pipelined like At_times
    __device__ __forceinline__ double A_times(const double (&vq)[NCG]) const {
        const int g = ogl();
#pragma unroll
        for (int q = 0; q < NCD; q++) stage[grp * ND + g + MP * q] = vq[q];
        wave_lds_sync();
        // (the staged vector through an OPAQUE 32-bit LDS address: from the plain pointer the compiler folds the stage's offset
        // inside the wave's area -- too large for a ds_read2 offset field -- into a fresh base register for EVERY read pair)
        unsigned vba = lds_addr(stage + grp * ND);
        asm volatile("" : "+v"(vba));
        const __attribute__((address_space(3))) double* vb = (const __attribute__((address_space(3))) double*)(size_t)vba;
        const double* row = Aimg + g * AS;
        constexpr int CB = (ND % PYCLLP_A_CB == 0) ? PYCLLP_A_CB : 8, NB = ND / CB;
        double a0[CB], a1[CB], v0[CB], v1[CB];
        double acc[4] = {0.0, 0.0, 0.0, 0.0};
#define A_LOAD(A_, V_, J0) \
    _Pragma("unroll") for (int jj = 0; jj < CB; jj++) { A_[jj] = row[(J0) + jj + tok]; V_[jj] = vb[(J0) + jj + tok]; }
#define A_USE(A_, V_)                                                                                          \
    _Pragma("unroll") for (int jj = 0; jj < CB; jj++) { asm volatile("" : "+v"(A_[jj])); asm volatile("" : "+v"(V_[jj])); } \
    asm volatile("" : "+v"(tok));                                                                              \
    _Pragma("unroll") for (int jj = 0; jj < CB; jj++) acc[jj & 3] = fma(A_[jj], V_[jj], acc[jj & 3]);
        int tok = 0;
        asm volatile("" : "+v"(tok));
        A_LOAD(a0, v0, 0)
        static_for<0, (NB + 1) / 2>([&](auto bc) {
            constexpr int b2 = 2 * decltype(bc)::value;
            if constexpr (b2 + 1 < NB) { A_LOAD(a1, v1, (b2 + 1) * CB) }
            A_USE(a0, v0)
            if constexpr (b2 + 2 < NB) { A_LOAD(a0, v0, (b2 + 2) * CB) }
            if constexpr (b2 + 1 < NB) { A_USE(a1, v1) }
        });
#undef A_LOAD
#undef A_USE
        wave_lds_sync();
        return (acc[0] + acc[1]) + (acc[2] + acc[3]) + (SL ? vq[NCG - 1] : 0.0);   // + v_slack_i for row i
    }

    // Gram product of group g's LP on the matrix cores (whole wave), fused with A*x (AX) and A*(d.t).
    // stage holds that LP's x, d, d*t in k-layout.  M goes to group g's slab; Ax/Adt come back for row l & (MP - 1), in every lane
    // group (ax is left alone without AX).  Reached with the whole wave active, which the lane swaps of its last lines need.
    // LATE: the store offsets are read after the k-loop instead of before it (their latency is then exposed, but they are not live
    // across the loop: the bounded kernel, which has no registers to spare there, spilt four without it).
    template <bool AX = true, bool LATE = false, bool SELB = false>
    __device__ __forceinline__ void gram_one(int g, double& ax, double& ad) const {
        double axp[JB], adp[JB];
        int lo0_ = lane;                      // opaque copy: see ogl()
        asm volatile("" : "+v"(lo0_));
        const int kg = lo0_ >> 4, cc = lo0_ & 15;
#pragma unroll
        for (int I = 0; I < JB; I++) { axp[I] = 0.0; adp[I] = 0.0; }
        const double* px = stage + kg * KS;
        const double* pd = stage + ND + kg * KS;
        const double* pt = stage + 2 * ND + kg * KS;
        const double* arow = Aimg + cc * AS + kg;
        double* sg = slab0 + g * G_::SLAB;
        constexpr int SC = (KS % 4 == 0) ? 4 : 2;
        // Only the LOWER triangle is needed: everything that reads the raw matrix -- load_own_row for the register-resident LDL',
        // the guarded cold path, the diagonal -- uses entries (row, col <= row) only.
        if constexpr (MP == 32) {
            // The off-diagonal 16x16 block on one v_mfma_f64_16x16x4_f64 and the two diagonal blocks' lower tiles on five 4x4x4
            // instructions (gram_pair()): 256 + 320 = 576 entries computed for the 528 needed, where three 16x16 tiles computed
            // 768.  The lane's operand element of row tile t is A[4 t + (l & 3)][4 s + (l >> 4)]: its own tiles
            // b = (l >> 2) & 3 and b + 4 are the two loads the fused A x / A (d t) sums and the 16x16 block take anyway; tile b + 2 sits
            // 8 rows below (an immediate), tiles (b + 3) % 4 and 4 + (b + 3) % 4 wrap for b = 0 and get an address of their own
            // (GeoG::gram_wrap).  Three more reads per k-step, not the six of an all-4x4 schedule: the LDS pipe, 44 % busy before,
            // is what that schedule's gain drowned in (profiles/r04).
            const unsigned short* tab = (const unsigned short*)(Aimg + G_::GTAB_OFF) + lo0_;
            const __attribute__((address_space(3))) double* wrow =
                (const __attribute__((address_space(3))) double*)(size_t)(lds_addr(Aimg + kg) + tab[64 * GRAM_INSTS]);
            unsigned so[GRAM_INSTS];
            if constexpr (!LATE) {
#pragma unroll
                for (int r = 0; r < GRAM_INSTS; r++) so[r] = tab[64 * r];
            }
            const bool top = cc < 8;              // instruction 4: blocks 0, 1 own tile b, blocks 2, 3 own tile b + 4
            // SELB: that choice as a lane-dependent base formed once, read and scaled again in every k-step (one read and one
            // multiply on the factors of ad[0] or ad[1]: the same product) instead of two selects per k-step
            const double* asel = arow + (top ? 0 : 16 * AS);
            double4_t acc10 = (double4_t){0.0, 0.0, 0.0, 0.0};
            double acc[GRAM_INSTS];
#pragma unroll
            for (int r = 0; r < GRAM_INSTS; r++) acc[r] = 0.0;
#pragma unroll PYCLLP_GRAM_UNROLL
            for (int s0 = 0; s0 < KS; s0 += SC) {
#pragma unroll
                for (int ss = 0; ss < SC; ss++) {
                    const int s = s0 + ss;
                    const double xk = AX ? px[s] : 0.0, dk = pd[s], tk = pt[s];
                    double a[2], ad[2];
#pragma unroll
                    for (int J = 0; J < 2; J++) {
                        a[J] = arow[16 * J * AS + 4 * s];      // A[16J + (l&15)][4s + (l>>4)]
                        if (AX) axp[J] = fma(a[J], xk, axp[J]);
                        adp[J] = fma(a[J], tk, adp[J]);
                        ad[J] = a[J] * dk;
                    }
                    const double p3 = wrow[4 * s], p7 = wrow[16 * AS + 4 * s], p2 = arow[8 * AS + 4 * s];
                    acc10 = __builtin_amdgcn_mfma_f64_16x16x4f64(ad[1], a[0], acc10, 0, 0, 0);
                    acc[0] = __builtin_amdgcn_mfma_f64_4x4x4f64(ad[0], a[0], acc[0], 0, 0, 0);
                    acc[1] = __builtin_amdgcn_mfma_f64_4x4x4f64(ad[1], a[1], acc[1], 0, 0, 0);
                    acc[2] = __builtin_amdgcn_mfma_f64_4x4x4f64(ad[0], p3, acc[2], 0, 0, 0);
                    acc[3] = __builtin_amdgcn_mfma_f64_4x4x4f64(ad[1], p7, acc[3], 0, 0, 0);
                    if constexpr (SELB) acc[4] = __builtin_amdgcn_mfma_f64_4x4x4f64(asel[4 * s] * dk, p2, acc[4], 0, 0, 0);
                    else acc[4] = __builtin_amdgcn_mfma_f64_4x4x4f64(top ? ad[0] : ad[1], p2, acc[4], 0, 0, 0);
                }
            }
            int lo_ = lane;                       // opaque copy: see ogl()
            asm volatile("" : "+v"(lo_));
            if constexpr (LATE) {
                const unsigned short* tab2 = (const unsigned short*)(Aimg + G_::GTAB_OFF) + lo_;
#pragma unroll
                for (int r = 0; r < GRAM_INSTS; r++) so[r] = tab2[64 * r];
            }
            const unsigned sga = lds_addr(sg);
#pragma unroll
            for (int r = 0; r < GRAM_INSTS; r++) *(__attribute__((address_space(3))) double*)(size_t)(sga + so[r]) = acc[r];
            // the 16x16 block, entry (16 + kg + 4 r, cc): (row & 15) << 1 = 2 kg + 8 r, so the swizzled column is
            // 16 (r >> 1) + ((cc ^ 2 kg) ^ 8 (r & 1)): TWO lane-dependent bases and an immediate per store
            const int kg2 = lo_ >> 4, c0 = (lo_ & 15) ^ (kg2 << 1);
            double* e0 = sg + kg2 * G_::MS + c0;
            double* e1 = sg + kg2 * G_::MS + (c0 ^ 8);
#pragma unroll
            for (int r4 = 0; r4 < 4; r4++) ((r4 & 1) ? e1 : e0)[(16 + 4 * r4) * G_::MS + 16 * (r4 >> 1)] = acc10[r4];
        } else {
            // one 16x16 tile (both triangles) on v_mfma_f64_16x16x4_f64
            double4_t acc = (double4_t){0.0, 0.0, 0.0, 0.0};
#pragma unroll PYCLLP_GRAM_UNROLL
            for (int s0 = 0; s0 < KS; s0 += SC) {
#pragma unroll
                for (int ss = 0; ss < SC; ss++) {
                    const int s = s0 + ss;
                    const double xk = AX ? px[s] : 0.0, dk = pd[s], tk = pt[s];
                    const double a = arow[4 * s];          // A[l & 15][4s + (l >> 4)]
                    if (AX) axp[0] = fma(a, xk, axp[0]);
                    adp[0] = fma(a, tk, adp[0]);
                    acc = __builtin_amdgcn_mfma_f64_16x16x4f64(a * dk, a, acc, 0, 0, 0);
                }
            }
            int lo_ = lane;                       // opaque copy: see ogl()
            asm volatile("" : "+v"(lo_));
            const int kg2 = lo_ >> 4, cc2 = lo_ & 15;
#pragma unroll
            for (int r4 = 0; r4 < 4; r4++) sg[G_::sidx(kg2 + 4 * r4, cc2)] = acc[r4];
        }
        // The partial sums over k = kg mod 4 of the four 16-lane rows, summed on lane swaps (whole wave: see the head of the function).
        // MP = 32: lane (kg, cc) holds rows cc and 16 + cc; the total of row cc comes back in the even 16-lane rows, that of row 16 + cc
        // in the odd ones, which is the lane -> row map of a group (gl = l & 31).  MP = 16: the total of row cc in all four rows.
        if constexpr (MP == 32) {
            if (AX) ax = quad_sum2(axp[0], axp[1]);
            ad = quad_sum2(adp[0], adp[1]);
        } else {
            if (AX) ax = quad_sum<true>(axp[0]);
            ad = quad_sum<true>(adp[0]);
        }
    }

    // The Gram pass of an LP's FIRST iteration without warm start, from the handle's image (first_gram_kernel, ipm_dense.hip).
    // Every LP starts at x = z = 1, so d is 1 in the real columns and 0 in padding whatever b and c are: the matrix gram_one<true>
    // leaves in the slab and the A x it returns depend on A, m and n alone.  `img` holds them as first_gram_kernel got them from
    // gram_one<true> itself: FIRST_SLAB doubles, the slab as that call left a zeroed one, then A x of row i at FIRST_SLAB + i.
    // The whole wave copies the slab image into group g's slab, 16 bytes per lane and load, every load issued before the k-loop,
    // which hides them (up to 32 registers across the loop, where gram_one holds more).  ad, the A (d t) sums -- they depend on
    // c --, come from gram_one's k-loop without its multiplies, selects and MFMAs: the same fma chain over s on the same operands
    // and the same sums across the 16-lane rows, so the same bits.  stage holds d t of the LP in k-layout (x and d are not read).
    // Whole wave active, as gram_one.  (The slack columns' d on M's diagonal is the caller's, behind either route.)
    // The 32-row shapes only.  At MP = 16 the pass has 8 to 16 MFMAs to save per LP and the copy costs as much: measured on
    // 16 x 32, 65 536 LPs 1.337 -> 1.330 / 1.340 ms (inside the scatter), and 4 096 LPs -- every LP in a slot of its own, one wave
    // per SIMD, nothing to hide a load behind -- 0.169 -> 0.171 ms, 0.172 with one load for the four groups (profiles/first_gram).
    static constexpr bool FIRST_IMAGE = MP == 32;
    static constexpr int FIRST_SLAB = (G_::SLAB + 1) & ~1;     // (16-byte pairs)
    static constexpr int FIRST_LEN = FIRST_SLAB + MP;          // doubles of an image
    __device__ __forceinline__ void gram_first(int g, const double* __restrict__ img, double& ax, double& ad) const {
        typedef double double2_t __attribute__((ext_vector_type(2)));
        constexpr int PAIRS = G_::SLAB / 2, NLD = (PAIRS + 63) / 64;
        static_assert(G_::SLAB % 2 == 0, "the slab is copied in 16-byte pairs");
        int lo_ = lane;                       // opaque copy: see ogl()
        asm volatile("" : "+v"(lo_));
        const double2_t* src = (const double2_t*)img + lo_;
        double2_t* dst = (double2_t*)(slab0 + g * G_::SLAB) + lo_;
        double2_t cp[NLD];
#pragma unroll
        for (int i = 0; i < NLD; i++)
            if (PAIRS % 64 == 0 || 64 * i + lo_ < PAIRS) cp[i] = src[64 * i];
        ax = img[FIRST_SLAB + (lo_ & (MP - 1))];
        const int kg = lo_ >> 4, cc = lo_ & 15;
        const double* pt = stage + 2 * ND + kg * KS;
        const double* arow = Aimg + cc * AS + kg;
        double adp[JB];
#pragma unroll
        for (int J = 0; J < JB; J++) adp[J] = 0.0;
#pragma unroll
        for (int s = 0; s < KS; s++) {
            const double tk = pt[s];
#pragma unroll
            for (int J = 0; J < JB; J++) adp[J] = fma(arow[16 * J * AS + 4 * s], tk, adp[J]);
        }
#pragma unroll
        for (int i = 0; i < NLD; i++)
            if (PAIRS % 64 == 0 || 64 * i + lo_ < PAIRS) dst[64 * i] = cp[i];
        if constexpr (MP == 32) ad = quad_sum2(adp[0], adp[1]);
        else ad = quad_sum<true>(adp[0]);
    }

    // Modified LDL' of every group's matrix at once, WITHOUT the Nocedal-Wright guard D_j = max(|D_j|, (theta_j/beta)^2, floor)
    // on the hot path: the sweep records whether it WOULD have bitten (some u_i^2 > beta^2 max(|D_j|, floor)) and returns that
    // verdict for the whole wave; if so (rare) the caller re-forms M and runs factor_guarded_inplace, which applies the guard
    // exactly as the reference does -- when nothing bites the two are the same arithmetic.  RELF (HSD kernel): the pivot floor of
    // column j is fl[j] (LDS, written by the caller: pivot_floor^2 |M_jj|) instead of the scalar floor_.
    // (Rounds 1-2 also carried factor<GUARD>, the round-1 sweep that handed every raw column through LDS; nothing called it.)
    // No LDS in a column's updates (the SP sweep, below, has one round trip behind column 15).  Lane gl keeps row gl of the trailing matrix in W; by symmetry
    // the entry M[j][k] that column j's update of W[k] needs is the column-j entry u = W[j] of LANE k, i.e. a broadcast
    // inside the lane's 16-lane DPP row -- which the DP ALU does inside the FMA itself (v_fmac_f64_dpp row_newbcast, see
    // wave_common.h): one instruction per trailing entry, where factor() above pays an LDS broadcast read (496 per
    // factorisation of a 32-row LP, with 8 waves per CU the LDS pipe was the bound of this phase) plus the FMA.
    // A 32-row group is two DPP rows: the bottom row's columns k < 16 (the L21 panel) need the TOP row's u, which one
    // v_permlane16_swap per half (gfx950) copies into both rows; columns k >= 16 only matter in the bottom row and take
    // its own u.  (Tried: leaving the rank-16 update of the bottom-right block to plain FMAs on LDS broadcast reads after
    // column 15 -- the 64-bit DPP FMA issues at half the rate of a plain one -- but the 32 extra round trips cost more than
    // the FP64 cycles saved: 9.3 M instead of 10.2 M LPs/s.  Also tried: that update as ONE product on the matrix cores (raw and
    // scaled column halves collected in two LDS tiles, 4 MFMAs per LP, result back through a third tile): correct, 9.6 M --
    // three more wave-level round trips per factorisation outweigh 1.6 k FP64 cycles with only two waves per SIMD.)
    // L ends up in W (W[j] = L[gl][j], 0 on and above the diagonal) and is written to the slab column by column, as
    // each becomes final, in the layout the substitution reads.  Arithmetic: u_i u_k / D_j as fma(-(u_i / D_j), u_k, .).
    // top row's value of u in both DPP rows of a 32-lane group (gfx950 v_permlane16_swap: [0] = rows (0, 0, 2, 2))
    __device__ __forceinline__ static double top_row_of(double u) { return top_row_d(u); }

    // The sweep takes "below the pivot" / "the pivot's lane" as EXEC masks (wave_common.h, round 3).  Tried and removed:
    // software-pipelining the next pivot's chain into column j's updates (6.314 against 6.26 ms per 65 536 LPs: with two waves
    // per SIMD the other wave already hides that latency, profiles/r03/dense_factor_pipelined.txt), and handing the top DPP
    // row's entries to the bottom row through LDS instead of v_permlane16_swap (6.02-6.09 against 5.94 ms).
    //
    // The sweep can take NR right-hand sides along (factor_dpp_fwd): forward substitution is elimination applied to one more
    // column, and its step j, r -= L[.][j] * (r of lane j), needs only the multiplier l that column j has just formed -- the
    // FMA of step j of subst15_up with the same operands, issued where the sweep waits on its pivot chain instead of in three
    // serial chains behind the factor's round trip through the slab (31 column loads and their wait go away).  Per lane the
    // floating-point operations and their order are those of forward(); the rows a step writes are chosen by the DPP row_mask,
    // so EXEC is not touched and lanes on and above a pivot still execute r -= 0 * r_j as they do there.
    //   MP = 16: step j follows column j, j = 0 .. 14.
    //   MP = 32: the top DPP row's steps follow columns 0 .. 14; its finished values then cross to the bottom row (one
    //   lane swap, issued after column 14) for the 16 accumulate steps of dot16_bcast, the subtraction and the bottom row's 15
    //   steps.  These 32 dependent operations are dealt two to a column over columns 16 .. 31, one behind the pivot's broadcast
    //   and one behind its reciprocal, so that none of their latency stands in front of a pivot: the step of column c runs
    //   inside column 17 + c / 2, on the W[c] that the lane still holds, and only the last one (c = 30) follows column 31.
    // Column j of L goes to the slab as soon as it is final, in the layout the substitution reads; one wave_lds_sync() follows the
    // last column.  The stores are plain C++ stores between the sweep's asm volatile statements.  Those have no memory clobber, so
    // nothing in the language keeps a store next to its column: the scheduler treats a volatile asm as a barrier for memory
    // operations, and the shipped code has one ds_write_b64 behind every column (llvm-objdump -d of the library's gfx950 code object).  Correctness
    // does not depend on it -- a store that sank would still precede the final sync -- only the overlap does; check the
    // disassembly after a compiler change.
    //
    // SP (MP = 32): the split sweep.  The rank-1 updates of the bottom-right 16 x 16 block M22 during columns j < 16 are useful in
    // the bottom DPP row only, and there only in the lower triangle.  With SP the top row of the group works as a rotated clone of
    // the bottom row during these columns and carries half of M22's columns: eight block FMAs per column in place of sixteen.
    //   Lane map (t: index inside the 16-lane row).  Bottom lane i keeps row 16 + i as before, but only its columns 24 .. 31
    //   (W[24 + s] = M[16 + i][24 + s]) are updated during columns j < 16.  Top lane t keeps its own row's left half W[0 .. 15] as
    //   before; its W[24 + s], s = 0 .. 7, don't-care values until now, hold M[R][16 + s] of row R = 16 + (t ^ 8)
    //   (load_row_for_sweep).
    //   Column j < 16.  The self-swap of u = W[j] that yields the top row's u in both rows (the pivot chain's operand) also yields
    //   the bottom row's u in both rows (both_rows_d).  In the top rows that copy is rotated by 8 lanes (ror8_top_d): X is the
    //   lane's own u in bottom lane i and the u of row R in top lane t.  X rD has the bits of the multiplier l that the masked
    //   chain forms in the bottom lane of row R (same two factors; rD is one value per group).  Then, in all lanes and without
    //   an EXEC switch, W[24 + s] -= (X of lane 8 + s of the DPP row) * (X rD): lane 8 + s of the bottom row's X is u of row
    //   24 + s, so bottom lane i updates column 24 + s of its row; lane 8 + s of the top row's X is u of row 16 + s, so top lane t
    //   updates column 16 + s of row R (chain_half_neg).  Every entry of M22 gets the sixteen FMAs it got, in column order, on
    //   the same two multiplicands: the lower triangle of the block is what the plain sweep computes, bit for bit.  Nothing is
    //   added to the pivot's dependent path: the rotation, the multiply and the eight FMAs follow the chain of W[0 .. 15].
    //   Behind column 15 the halves meet again through rows 16 .. 31 of the slab, which are dead at that point (merge_through_slab:
    //   4 + 4 128-bit LDS operations per lane; measured against 16 rotations and 16 v_permlane16_swap in registers, which need no
    //   LDS but cost 0.011 ms of the 0.089 ms this split gains on 65 536 LPs of 32 x 64, profiles/sweep_split).  Columns 16 .. 31,
    //   the carried forward substitution, the column stores of L and the guard's running maximum are those of the plain sweep.
    // A kernel takes SP where it costs no scratch and no spilt register (its `SPLIT` constant, next to `CARRY`).
    // SIGN: the verdict "the Nocedal-Wright guard would have bitten" (some u_i^2 / D_j > beta^2) from the pivots instead of a
    // running maximum of y_ij = l_i u_i per column and lane.  If no pivot of a group is <= 0 or NaN, nothing bit:
    //   1. rD > 0 and l_i = fl(u_i rD) has the sign of u_i (or is a zero of that sign), so every product l_i u_i is >= 0.
    //   2. A trailing diagonal entry changes only by W_ii <- fma(-l_i, u_i, W_ii): the exact value does not grow, and rounding
    //      is monotone, so W_ii never increases.  It starts at M_ii <= beta^2 = max |diag M|.
    //   3. fl(l_i u_i) > beta^2 implies that the exact product exceeds beta^2 (rounding is monotone and beta^2 is a double), so
    //      at that column the exact W_ii - l_i u_i is below zero and W_ii comes out negative (or -0: a sign bit that no later
    //      update clears, since -l_i u_i always carries it) and stays at or below that value.
    //   4. So row i's own pivot is not > 0 when its column comes.  A NaN on the diagonal stays NaN and fails `> 0` as well.
    // The converse does not hold: a pivot <= 0 where nothing bit (M singular to rounding) now takes the redo too.  The redo is
    // factor_guarded_inplace, whose arithmetic is the sweep's wherever the guard does not bite (what PYCLLP_FLAG_FORCE_GUARD_PATH
    // and tests/test_fused_forward.py rest on), so the results keep their bits (tests/test_guard_sign.py).  Two limits.  That
    // equality is not a theorem at every magnitude: on the diverging LPs of tests/golden/status_cases.npz the forced path leaves
    // the sweep's trajectory (in the parent too), so there "the parent's bits" is a measurement (the eight shapes and three
    // singular batches of tools/dev/outputs_vs_parent.py, byte for byte), not an argument.  And the redo costs time: a batch whose
    // M has a zero or a redundant row has a pivot that is zero or negative by rounding in most iterations, and every such wave
    // re-forms M and runs the run-time loops of the guarded path, where the parent stayed on the hot sweep -- 16 384 LPs of
    // 32 x 96 with a duplicated and a zero row 2.02 -> 9.00 ms, of 12 x 40 0.50 -> 1.30 ms (profiles/guard_sign).  Only the pivot's own
    // lane votes (chain_colp_*: the one-hot mask that captures rdiag): in columns 16 .. 31 the top DPP row's W[j] is a don't-care
    // value.  Padded rows are identity rows, pivot 1.
    template <bool RELF = false, bool SP = SPLIT, bool SIGN = false>
    __device__ __forceinline__ bool factor_dpp(double (&W)[MP], double beta2, double floor_, bool live, double& rdiag,
                                               const double* fl = nullptr) const {
        return factor_sweep<RELF, 0, SP, SIGN>(W, beta2, floor_, live, rdiag, fl, nullptr);
    }
    // r <- L^-1 r for the NR right-hand sides r (lane = row) along with the factorisation; the caller goes on with backward()
    template <bool RELF = false, bool SP = SPLIT, bool SIGN = false, int NR>
    __device__ __forceinline__ bool factor_dpp_fwd(double (&W)[MP], double beta2, double floor_, bool live, double& rdiag,
                                                   double (&r)[NR], const double* fl = nullptr) const {
        return factor_sweep<RELF, NR, SP, SIGN>(W, beta2, floor_, live, rdiag, fl, r);
    }
    // operation `op` (0 .. 31) of the bottom DPP row's part of the carried forward substitution, MP = 32 (see above)
    template <int OP, int NR>
    __device__ __forceinline__ static void fwd_bottom_op(const double (&W)[MP], double* r, const double* so, double* a) {
        if constexpr (OP >= 0 && OP < 16) {
#pragma unroll
            for (int i = 0; i < NR; i++) dot_step<OP, 0xA>(a[i], so[i], W[OP]);      // a += L21[.][OP] * t1_OP (a stays 0 in the top row)
        } else if constexpr (OP == 16) {
#pragma unroll
            for (int i = 0; i < NR; i++) r[i] -= a[i];                               // r2 -= L21 t1 (top row: r1 - 0)
        } else if constexpr (OP > 16 && OP < 32) {
#pragma unroll
            for (int i = 0; i < NR; i++) fwd_step<OP - 17, 0xA>(r[i], W[OP - 1]);    // step of column OP - 1
        }
    }
    template <bool RELF, int NR, bool SP, bool SIGN>
    __device__ __forceinline__ bool factor_sweep(double (&W)[MP], double beta2, double floor_, bool live, double& rdiag,
                                                 const double* fl, double* r) const {
        rdiag = 1.0;
        // the sweep is a chain of dependent operations: s_setprio lets it go first when both waves of the SIMD are ready.
        // Measured: 6.82 -> 6.75 ms for the HSD kernel (RELF); for the plain kernel nothing alone (5.93-5.95 ms at levels 0, 2, 3),
        // 5.93 -> 5.91 ms together with the same level inside the substitution (PYCLLP_SOLVE_PRIO); raising the priority of the
        // Gram product's MFMA loop instead costs 0.3-0.6 %.
        constexpr int PRIO_ = RELF ? PYCLLP_FACTOR_PRIO_HSD : PYCLLP_FACTOR_PRIO;
        if constexpr (PRIO_ != 0) __builtin_amdgcn_s_setprio(PRIO_);
        const int go = ogl();      // COLB: unused, but this opaque copy shapes the register allocation of the (32, .) kernels
        (void)go;
        constexpr int NR1 = NR ? NR : 1;
        double so[NR1], acc[NR1];  // MP = 32: the top row's finished values as the bottom row sees them / the L21 t1 accumulators
#pragma unroll
        for (int i = 0; i < NR1; i++) { so[i] = 0.0; acc[i] = 0.0; }
        double ymax = 0.0;         // running max of u^2 / D over the lanes below the pivots: the guard bites iff it exceeds beta^2
        double pv = 1.0;           // SIGN: the lane's own pivot, kept when its column comes (see above)
        static_for<0, MP>([&](auto jc) {
            constexpr int j = decltype(jc)::value;
            const double u = W[j];
            double src = u;        // the u whose lane j % 16 is the pivot row as seen from this lane's DPP row
            double ub = u;         // SPLIT: the bottom row's u in both rows, the other half of the same swap
            if constexpr (SP && j < 16) src = both_rows_d(u, ub);
            else if constexpr (MP == 32 && j < 16) src = top_row_of(u);
            const double piv = bcast64<j % 16>(src);
            if constexpr (NR > 0 && MP == 32 && j > 16) fwd_bottom_op<2 * (j - 16) - 1, NR>(W, r, so, acc);
            const double aD = RELF ? max_abs<false>(piv, fl[j]) : max_abs<true>(piv, floor_);
            double rD = fast_rcp(aD);
            if constexpr (NR > 0 && MP == 32 && j >= 16) {
                asm volatile("" : "+v"(rD));   // behind the Newton steps, not between the maximum and the reciprocal
                fwd_bottom_op<2 * (j - 16), NR>(W, r, so, acc);
            }
            // lanes of every group with gl > j / the lane gl == j
            constexpr unsigned below32 = (j + 1 < 32) ? (0xFFFFFFFFu << ((j + 1) & 31)) : 0u;
            constexpr unsigned below16 = (j + 1 < 16) ? (((0xFFFFu << ((j + 1) & 15)) & 0xFFFFu) * 0x10001u) : 0u;
            constexpr unsigned MB_ = (MP == 32) ? below32 : below16;
            constexpr unsigned ONE_ = (MP == 32) ? (1u << (j % 32)) : ((1u << (j % 16)) * 0x10001u);
            double l = 0.0;        // L[gl][j] = u / D below the pivot, 0 on and above it
            asm volatile("" : "+v"(l));
            if constexpr (MP == 16) {
                if constexpr (SIGN) chain_step_piv<j, MB_, MB_, 1, ONE_, ONE_>(W, 0.0, rD, l, pv, rdiag);
                else chain_step_exec<j, MB_, MB_, 1, ONE_, ONE_>(W, 0.0, rD, l, ymax, rdiag);
            } else if constexpr (j < 16) {
                if constexpr (SIGN) chain_step_piv<j, MB_, MB_, 0, ONE_, ONE_>(*reinterpret_cast<double (*)[16]>(&W[0]), src, rD, l, pv, rdiag);
                else chain_step_exec<j, MB_, MB_, 0, ONE_, ONE_>(*reinterpret_cast<double (*)[16]>(&W[0]), src, rD, l, ymax, rdiag);
                // the bottom-right block's columns.  SP: half of them per DPP row (see above; the top lanes' W[24 .. 31] are M22's
                // columns 16 .. 23 of row R).  Plain: all sixteen in ALL lanes -- what the top row's lanes hold in W[16..31] is then
                // never read (upper triangle; overwritten with 0 when its column comes), so the EXEC mask of rounds 2-3 only cost
                // its switches
                if constexpr (SP) chain_half_neg(*reinterpret_cast<double (*)[8]>(&W[24]), ror8_top_d(ub), rD);
                else chain_all_neg(*reinterpret_cast<double (*)[16]>(&W[16]), W[j], l);
            } else {
                if constexpr (SIGN) chain_step_piv<j - 16, MB_, MB_, 1, ONE_, ONE_>(*reinterpret_cast<double (*)[16]>(&W[16]), 0.0, rD, l, pv, rdiag);
                else chain_step_exec<j - 16, MB_, MB_, 1, ONE_, ONE_>(*reinterpret_cast<double (*)[16]>(&W[16]), 0.0, rD, l, ymax, rdiag);
            }
            W[j] = l;
            if constexpr (COLB) *(__attribute__((address_space(3))) double*)(size_t)(xb[j & 15] + 256u * (unsigned)(j & ~15)) = l;
            else if constexpr (MP == 16) slab[G_::sidx(j, go)] = l;
            if constexpr (NR > 0 && j < 15) {
#pragma unroll
                for (int i = 0; i < NR; i++) fwd_step<j, (MP == 32) ? 0x5 : 0xF>(r[i], l);
                if constexpr (MP == 32 && j == 14) {
#pragma unroll
                    for (int i = 0; i < NR; i++) so[i] = top_row_d(r[i]);   // (whole wave, like top_row_of above)
                }
            }
            if constexpr (SP && j == 15) merge_through_slab(W);
        });
        if constexpr (NR > 0 && MP == 32) fwd_bottom_op<31, NR>(W, r, so, acc);
        // SIGN: every lane is the pivot lane of one column of its group and votes with its own pivot (zero, negative or NaN);
        // the lanes of an idle group do not vote, as before
        const bool viol = SIGN ? live && !(pv > 0.0) : live && (ymax > beta2);
        if constexpr (PRIO_ != 0) __builtin_amdgcn_s_setprio(0);
        if constexpr (!CARRY) {    // (32, 128): the swizzled addresses are formed here, not held across the sweep
            const int g = ogl();
#pragma unroll
            for (int j = 0; j < MP; j++) slab[G_::sidx(j, g)] = W[j];
        }
        wave_lds_sync();
        return __any(viol);
    }

    // Cold path: the reference's modified LDL' with the Nocedal-Wright guard applied at every column, run IN PLACE on
    // the group's slab (lower triangle = trailing matrix, upper triangle receives L', exactly the layout the
    // substitution reads) with plain runtime loops: compact code, no register-resident row, only executed when
    // factor_dpp reported that the guard would have bitten.
    __device__ __forceinline__ double factor_guarded_inplace(bool rowok, double beta2, double floor_,
                                                             const double* fl = nullptr) const {
        if (!rowok) slab[G_::sidx(gl, gl)] = 1.0;   // padded rows of A are zero rows/columns of M: identity
        wave_lds_sync();
        double rdiag = 1.0;
#pragma unroll 1
        for (int j = 0; j < MP; j++) {
            const bool below = gl > j;
            const double u = below ? slab[G_::sidx(gl, j)] : 0.0;
            const double piv = slab[G_::sidx(j, j)];
            const double theta = grp_max<MP>(fabs(u));
            const double aD = fmax(fmax(fabs(piv), fl ? fl[j] : floor_), theta * theta / beta2);   // ldl.cl:368
            const double rD = fast_rcp(aD);
            const double li = u * rD;
            if (gl == j) rdiag = rD;
#pragma unroll 1
            for (int k = j + 1; k < MP; k++) {
                const double uk = slab[G_::sidx(k, j)];        // raw column entry of row k (broadcast read)
                if (gl >= k) slab[G_::sidx(gl, k)] = fma(-li, uk, slab[G_::sidx(gl, k)]);
            }
            wave_lds_sync();
            slab[G_::sidx(j, gl)] = below ? li : 0.0;          // L' row j; columns <= j of row j are zeroed below
            wave_lds_sync();
        }
        // the substitution expects zeros on and below the diagonal of the slab
#pragma unroll 1
        for (int k = 0; k < MP; k++) if (k <= gl) slab[G_::sidx(gl, k)] = 0.0;
        wave_lds_sync();
        return rdiag;
    }

    // s <- (L D L')^-1 s for every group.  Substitution runs in 16x16 blocks so that every broadcast stays inside
    // a 16-lane DPP row (row_newbcast: 2 moves, no SGPR round trip); a 32-lane group does top block, the 16x16
    // off-diagonal product (operand fetched across the rows by one lane swap, top_row_d / bottom_row_d) and bottom block.
    // forward(s): s <- L^-1 s from the slab's column layout; backward(s, rdiag): s <- L^-T D^-1 s from its rows.  fwd_back is the
    // whole solve, for callers that have no sweep to carry their right-hand side (refinement, the corrector, the guarded path);
    // behind factor_dpp_fwd the caller runs back_after_sweep() on what the sweep returned: the row loads are then the first
    // thing behind the sweep's final sync.  (s_setprio as before the split: the 16-row kernels leave the substitution's level on
    // until the next sweep ends.)
    __device__ __forceinline__ double fwd_back(double s, double rdiag) const {
        if constexpr (PYCLLP_SOLVE_PRIO != 0) __builtin_amdgcn_s_setprio(PYCLLP_SOLVE_PRIO);
        forward(s);
        backward(s, rdiag);
        if constexpr (MP == 32 && PYCLLP_SOLVE_PRIO != 0) __builtin_amdgcn_s_setprio(0);
        return s;
    }
    __device__ __forceinline__ double back_after_sweep(double s, double rdiag) const {
        if constexpr (PYCLLP_SOLVE_PRIO != 0) __builtin_amdgcn_s_setprio(PYCLLP_SOLVE_PRIO);
        backward(s, rdiag);
        if constexpr (MP == 32 && PYCLLP_SOLVE_PRIO != 0) __builtin_amdgcn_s_setprio(0);
        return s;
    }
    __device__ __forceinline__ void forward(double& s) const {
        // all factor entries a lane needs are fetched up front and pinned in registers: left to itself the
        // scheduler sinks each ds_read next to its FMA and every step of the serial chain pays an LDS round trip
        double lf[MP];
        if constexpr (COLB) {
#pragma unroll
            for (int k = 0; k < MP - 1; k++) lf[k] = *(const __attribute__((address_space(3))) double*)(size_t)(xb[k & 15] + 256u * (unsigned)(k & ~15));
        } else {
            const int g = ogl();
#pragma unroll
            for (int k = 0; k < MP - 1; k++) lf[k] = slab[G_::sidx(k, g)];    // column entries L[gl][k]
        }
#pragma unroll
        for (int k = 0; k < MP - 1; k++) asm volatile("" : "+v"(lf[k]));
        if constexpr (MP == 16) {
            subst15_up(s, lf);
        } else {
            const bool top = gl < 16;
            if (top) subst15_up(s, lf);           // t1 = L11^-1 r1
            const double so = top_row_d(s);       // bottom rows see t1 (outside the branches: the swap needs both rows active)
            if (!top) {
                s -= dot16_bcast(so, lf);         // r2 -= L21 t1 (no serial dependence)
                subst15_up(s, lf + 16);           // t2 = L22^-1 r2
            }
        }
    }
    __device__ __forceinline__ void backward(double& s, double rdiag) const {
        s *= rdiag;
        double lb[MP];
        load_own_row(lb);   // lb[i] = L[i][gl] for i > gl, else 0 (lb[0] is not used)
#pragma unroll
        for (int i = 1; i < MP; i++) asm volatile("" : "+v"(lb[i]));
        if constexpr (MP == 16) {
            subst15_down(s, lb);
        } else {
            const bool top = gl < 16;
            if (!top) subst15_down(s, lb + 16);   // x2 = L22^-T s2
            const double so = bottom_row_d(s);    // top rows see x2 (outside the branches: the swap needs both rows active)
            if (top) {
                s -= dot16_bcast(so, lb + 16);    // s1 -= L21^T x2
                subst15_down(s, lb);              // x1 = L11^-T s1
            }
        }
    }
};

// PC = true (PYCLLP_FLAG_PREDCORR): Mehrotra's predictor-corrector on the same machinery -- oracle ipm_one_pc: after the ONE
// factorisation of an iteration a predictor solve with mu = 0, the centering parameter from how far that step gets
// (sigma = (gamma_a / gamma)^3), then the corrector solve with the second-order term dx_a dz_a; a second forward/back
// substitution, A'u and A v per iteration buy ~27 % fewer iterations at the reference's step fraction (0.9), ~45 % at 0.99.
// FULL = true (slack-aware kernels only): the instantiation for LPs that fill it exactly, m = MP and n = NP (so n - m = ND dense
// columns), which the host guarantees (abi_dense.hip launches SlackVariant::full_group for no other LP).  No column is
// padding then: every `ok[q]` is true, the selects on them fold away (35 v_cndmask of the (32, 96) kernel's text), and
// the identity rows of a padded M are never written.  A select on a true condition is the identity: the results are those of
// the generic instantiation, bit for bit (tests/test_full_shape.py).  `rowok`, m and n stay run-time values although they are
// known as well: with `rowok` true -- even at the one select on the hot path, M's diagonal before the sweep -- or with m = MP
// as a constant (which makes `rowok` one), the (32, 96) kernel spills 2-11 VGPRs (DESIGN section 13.8); as it stands no
// full-shape kernel has scratch or a spilt VGPR.  Where a select stood between a product and a sum it also kept the two from
// contracting into an fma; the two places of the plain step (gam, d_slack onto M's diagonal) pin the product for FULL.  That
// rests on what the compiler contracts (DESIGN section 13.8); tests/test_full_shape.py holds the two texts together.  Plain
// step only: the predictor-corrector text with FULL did not give the generic bits, for a reason not found, and is not built.
// Without FULL the text is what it was, and so is every generic kernel's machine code.
template <int MP, int NP, bool SL, bool PC = false, bool FULL = false>
__global__ void __launch_bounds__(PYCLLP_WPB * 64)
ipm_group_kernel(int m, int n, long B, const double* __restrict__ Ag, const double* __restrict__ bg,
                 const double* __restrict__ cg, double* __restrict__ xg, double* __restrict__ yg,
                 double* __restrict__ zg, double* __restrict__ pobj, double* __restrict__ dobj,
                 int* __restrict__ status, int* __restrict__ iters, int* __restrict__ queue, DevOpts o,
                 const double* __restrict__ first) {
    using G_ = GeoG<MP, NP, SL>;
    constexpr int G = G_::G, NCG = G_::NCG, NCD = G_::NCD, ND = G_::ND, JB = G_::JB, AS = G_::AS;
    static_assert(!FULL || (SL && !PC), "full-shape instantiations exist for the plain slack-aware kernels only");
    // `first` (the handle's image of an LP's first Gram pass, or null: GWave::gram_first) is read by the 32-row instantiations
    // (GWave::FIRST_IMAGE) but the two predictor-corrector kernels that fill the register file: with the path the slack-aware
    // (32, 96) one and the general (32, 128) one spill 2 VGPRs each (the copy after the k-loop, rolled, or half of it: 11 to
    // 49), so they keep the product
    constexpr bool FIRST_IMAGE = GWave<MP, NP, SL>::FIRST_IMAGE && !(PC && ((SL && NP == 96) || (!SL && NP == 128)));
    // Three cuts of vector issue that the plain-step instantiations take (profiles/guard_sign; the predictor-corrector kernels sit
    // at the register limit -- the slack-aware (32, 96) one spills 2 to 3 VGPRs with GRAM_SELB or AT_FUSED, the general one 1 with
    // PIVOT_SIGN -- and keep the parent's text): the guard's verdict from the pivots' signs (GWave::factor_sweep), the Gram loop's
    // fifth tile without its selects (GWave::gram_one) and A'u with the row broadcast inside the FMA where a lane holds two
    // dense registers (GWave::At_times)
    constexpr bool PIVOT_SIGN = !PC, GRAM_SELB = !PC;
    constexpr bool AT_FUSED = !PC && NCD == 2 && PYCLLP_AT_RB == 4;
    const int nd = SL ? n - m : n;          // dense columns of A (the last m columns are the identity when SL)
    extern __shared__ __attribute__((aligned(16))) double lds[];
    const int tid = threadIdx.x;
    const int wpb = blockDim.x / WAVE;
    double* Aimg = lds;
    double* colsum = lds + G_::AIMG;
    // stage the row-major image of A (zero padded) and its column sums A'1
    for (int i = tid; i < G_::AIMG; i += blockDim.x) {
        const int r = i / AS, cidx = i % AS;
        Aimg[i] = (r < m && cidx < nd) ? Ag[(size_t)r * n + cidx] : 0.0;
    }
    G_::fill_gram_table(lds, tid, blockDim.x);
    __syncthreads();
    for (int j = tid; j < ND; j += blockDim.x) {
        double sacc = 0.0;
        for (int i = 0; i < MP; i++) sacc += Aimg[i * AS + j];
        colsum[j] = sacc;
    }
    __syncthreads();

    GWave<MP, NP, SL> w;
    const int wave = tid / WAVE;
    const int lane = tid & 63, gl = lane & (MP - 1), grp = lane / MP;
    w.lane = lane; w.gl = gl; w.grp = grp; w.m = m; w.n = n;
    w.Aimg = Aimg;
    w.slab0 = lds + G_::SHARED + wave * G_::WSZ;
    w.slab = w.slab0 + grp * G_::SLAB;
    w.stage = w.slab0 + G * G_::SLAB;
    if constexpr (GWave<MP, NP, SL>::COLB) {
#pragma unroll
        for (int cidx = 0; cidx < 16; cidx++) w.xb[cidx] = lds_addr(w.slab) + 8u * (unsigned)G_::sidx(cidx, gl);
    }
    if constexpr (GWave<MP, NP, SL>::ROWB) {
#pragma unroll
        for (int p2 = 0; p2 < 16; p2++) w.rb[p2] = lds_addr(w.slab + gl * G_::MS) + 16u * (unsigned)(p2 ^ (gl & 15));
    }
    // the Gram pass writes the lower block triangle only; the rest of a slab is read (load_own_row) but never used: zero once,
    // so that no NaN pattern of uninitialised LDS ever travels through the registers
    for (int i = lane; i < G * G_::SLAB; i += WAVE) w.slab0[i] = 0.0;
    wave_lds_sync();
    const bool rowok = gl < m;
    const bool warm = (o.flags & PYCLLP_FLAG_WARM_START) != 0;
    const bool autoscale = (o.flags & PYCLLP_FLAG_AUTOSCALE) != 0;
    const unsigned long long gmask = (MP == 32) ? 0xFFFFFFFFull : 0xFFFFull;
    STAMP_DECL

    // slots in GROUP-major order: the first gridDim.x * wpb LPs go to lane group 0 of every wave, the next to group 1, ... -- a
    // batch smaller than the launch's slots leaves whole lane groups idle (their Gram products are skipped below) instead of
    // whole waves: B <= waves means one LP per wavefront and the single-LP latency for every LP (round 3)
    const long nslots = (long)gridDim.x * wpb * G;
    long lp = (long)grp * ((long)gridDim.x * wpb) + (long)blockIdx.x * wpb + wave;
    bool live = lp < B, fresh = live;

    // per-slot state
    double x[NCG], z[NCG], c[NCG], v[NCG];
    bool ok[NCG];
#pragma unroll
    for (int q = 0; q < NCG; q++) {
        ok[q] = FULL || ((q < NCD) ? (gl + MP * q < nd) : (gl < m));
        x[q] = 1.0; z[q] = 1.0; c[q] = 0.0; v[q] = 0.0;
    }
    // global column of register q (dense registers first, then (SL) the slack column of row gl) from an OPAQUE lane index: the
    // cold paths that need it (loading / storing an LP) must not leave per-lane 64-bit addresses alive across the iterations
    // (hoisted out of the persistent loop they cost ~30 registers and, at 256, scratch)
    auto gcol = [&](int q, int g_) { return (q < NCD) ? g_ + MP * q : nd + g_; };
    double b = 0.0, y = 0.0;
    double tol_r = 0.0, tol_s = 0.0, etol = 0.0;
    double r2_0 = __builtin_inf(), s2_0 = __builtin_inf();   // the squared norms of the previous pass (stop_verdict)
    const bool exact_norms = (o.flags & PYCLLP_FLAG_EXACT_NORMS) != 0;
    double rho_pred = 0.0;     // b - A x of the CURRENT point, predicted exactly from the previous step:
    bool have_pred = false;    // rho+ = (1-theta) rho + theta (rho - A dx); lets the stop test run BEFORE the Newton work
    int it = 0;

    while (__any(live)) {
        if (__any(fresh)) {
            if (fresh) {
                const int go = w.ogl();
#pragma unroll
                for (int q = 0; q < NCG; q++) {
                    const int j = gcol(q, go);
                    c[q] = ok[q] ? cg[lp * n + j] : 0.0;
                    x[q] = (warm && ok[q]) ? xg[lp * n + j] : 1.0;
                    z[q] = (warm && ok[q]) ? zg[lp * n + j] : 1.0;
                    v[q] = (q < NCD) ? colsum[go + MP * q] : (rowok ? 1.0 : 0.0);   // A'y for y = 1
                }
                b = rowok ? bg[lp * m + go] : 0.0;
                y = rowok ? ((warm && yg) ? yg[lp * m + go] : 1.0) : 0.0;
            }
            if (autoscale) {   // solve the LP with b/max|b| and c/max|c| (PYCLLP_FLAG_AUTOSCALE); undone when storing
                double cm = 0.0;
#pragma unroll
                for (int q = 0; q < NCG; q++) cm = fmax(cm, fabs(c[q]));
                double sb = grp_max<MP>(fabs(b)), sc = grp_max<MP>(cm);
                const bool scaled = autoscale_lp(o.flags, sb, sc, 0.0);
                sb = (scaled && sb > 0.0) ? sb : 1.0; sc = (scaled && sc > 0.0) ? sc : 1.0;
                if (fresh) {
                    b = b / sb;
#pragma unroll
                    for (int q = 0; q < NCG; q++) c[q] = c[q] / sc;
                    if (warm) {
                        y = y / sc;
#pragma unroll
                        for (int q = 0; q < NCG; q++) { x[q] = x[q] / sb; z[q] = z[q] / sc; }
                    }
                }
            }
            double c2 = 0.0;
#pragma unroll
            for (int q = 0; q < NCG; q++) c2 = fma(c[q], c[q], c2);
            const double nb2 = grp_sum<MP>(b * b), nc2 = grp_sum<MP>(c2);
            double vw[NCG];
            if (warm) w.template At_times<false, AT_FUSED>(y, vw);
            if (fresh) {
                tol_r = o.eps * (1.0 + sqrt(nb2));
                tol_s = o.eps * (1.0 + sqrt(nc2));
                etol = o.refine_tol * (1.0 + sqrt(nb2));
                r2_0 = __builtin_inf(); s2_0 = __builtin_inf(); it = 0; have_pred = false;
                if (warm) {
#pragma unroll
                    for (int q = 0; q < NCG; q++) v[q] = vw[q];
                }
            }
            fresh = false;
            STAMP(9)
        }

        // ---- dual infeasibility, complementarity, objectives (primal_normal.cl:76-94, 245-248) ----
        double s2 = 0.0, gam = 0.0, pp = 0.0;
#pragma unroll
        for (int q = 0; q < NCG; q++) {
            const double sg = ok[q] ? c[q] - v[q] + z[q] : 0.0;
            s2 = fma(sg, sg, s2);
            if constexpr (FULL) {
                // without the select nothing keeps the product from contracting into the sum; the generic text adds the ROUNDED
                // product, so this one must (the pin is no instruction, it only forbids the fma).  A branch of its own: the
                // generic line written with a named product compiles to other machine code in every generic kernel
                double xz = x[q] * z[q];
                asm volatile("" : "+v"(xz));
                gam += xz;
            } else {
                gam += ok[q] ? x[q] * z[q] : 0.0;
            }
            pp += c[q] * (ok[q] ? x[q] : 0.0);
        }
        s2 = grp_sum<MP>(s2); gam = grp_sum<MP>(gam);
        const double po = grp_sum<MP>(pp);
        double mu = PC ? 0.0 : o.delta * gam / (double)(n + m);     // PC: 0 for the predictor, set from its outcome below

        // store a finished LP and hand the slot its next one from the device-wide queue.  du = b'y of the point whose objectives
        // are returned: summed by the caller, where an LP ends, and not in every pass (it is read nowhere else)
        auto finalize = [&](int stat_, double du) {
            double sb = 1.0, sc = 1.0;
            const int go = w.ogl();
            int gro = grp;
            asm volatile("" : "+v"(gro));
            if (autoscale) {   // recover the scale factors from the inputs (cheaper than carrying them in registers)
                double cm = 0.0;
#pragma unroll
                for (int q = 0; q < NCG; q++) cm = fmax(cm, ok[q] ? fabs(cg[lp * n + gcol(q, go)]) : 0.0);
                // (under a per-group condition: both rows of the group are active, which is all grp_max's lane swap needs)
                sb = grp_max<MP>(rowok ? fabs(bg[lp * m + go]) : 0.0);
                sc = grp_max<MP>(cm);
                const bool scaled = autoscale_lp(o.flags, sb, sc, 0.0);      // (the verdict of the load: the same maxima)
                sb = (scaled && sb > 0.0) ? sb : 1.0; sc = (scaled && sc > 0.0) ? sc : 1.0;
            }
#pragma unroll
            for (int q = 0; q < NCG; q++) {
                const int j = gcol(q, go);
                if (ok[q]) {
                    xg[lp * n + j] = x[q] * sb;
                    if (zg) zg[lp * n + j] = z[q] * sc;
                }
            }
            if (yg && rowok) yg[lp * m + go] = y * sc;
            if (go == 0) {
                if (pobj) pobj[lp] = po * (sb * sc);
                if (dobj) dobj[lp] = du * (sb * sc);
                status[lp] = stat_;
                if (iters) iters[lp] = it;
            }
            int nxt = 0;
            if (go == 0) nxt = atomicAdd(queue, 1);
            nxt = __shfl(nxt, gro * MP, WAVE);
            lp = nslots + (long)nxt;
            live = lp < B;
            fresh = live;
            have_pred = false;
            if (!live) {   // park the slot on harmless values
#pragma unroll
                for (int q = 0; q < NCG; q++) { x[q] = 1.0; z[q] = 1.0; c[q] = 0.0; v[q] = 0.0; }
                b = 0.0; y = 0.0;
            }
        };

        // ---- stop tests of THIS point (primal_normal.cl:256-269) before any Newton work, when rho is known ----
        // rho_pred follows the recurrence rho+ = rho + theta (e - rho) and never sees the rounding of x += theta dx
        // (about eps |x| |A| N): where |x| >> |b| the true |b - A x| can sit above tol_r while the predicted one passes.
        // So the prediction only NOMINATES a slot for finishing; the verdict is taken on rho = b - A x recomputed from x
        // (what the oracle tests every iteration, ipm_dense_ref.c ipm_one_path) -- one A*x for the wave, on the passes where
        // some slot is about to finish, i.e. about once per LP.
        double r2_pred = grp_sum<MP>(rho_pred * rho_pred);
        {
            // (a candidate is a slot for which one of the tests holds: the verdict's status is taken again below, on the true rho)
            const bool tested = have_pred && live;
            const bool cand = tested & (stop_verdict(r2_pred, s2, gam, po, tol_r, tol_s, r2_0, s2_0, o.eps, tested, exact_norms) >= 0);
            if (__any(cand)) {
                double xs[NCG];
#pragma unroll
                for (int q = 0; q < NCG; q++) xs[q] = ok[q] ? x[q] : 0.0;
                const double rho_true = b - w.A_times(xs);
                const double r2_true = grp_sum<MP>(rho_true * rho_true);
                const int verdict_e = stop_verdict(r2_true, s2, gam, po, tol_r, tol_s, r2_0, s2_0, o.eps, cand, exact_norms);
                int stat_e = PYCLLP_STATUS_ITERATION_LIMIT;
                bool fin_e = false;
                if (cand) {
                    rho_pred = rho_true; r2_pred = r2_true;     // re-seed the recurrence with the true residual
                    if (verdict_e >= 0) { stat_e = verdict_e; fin_e = true; }
                }
                if (__any(fin_e)) {
                    if (fin_e) finalize(stat_e, grp_sum<MP>(b * y));    // (per group, as grp_max inside finalize)
                    continue;   // the freed slot loads its next LP first, so the Newton pass below is never wasted
                }
            }
        }
        STAMP(0)

        // ---- d = x/z, t = c - A'y + mu/x ----
        double Ax = 0.0, Adt = 0.0;
        // 1/x and 1/z are computed once per iteration and kept (12 VGPRs at (32, 96)) instead of being re-derived in each place
        // that needs them (round 3: 18 -> 6 fast_rcp per LP-iteration)
        double rxk[NCG], rzk[NCG];
#pragma unroll
        for (int q = 0; q < NCG; q++) { rxk[q] = fast_rcp(x[q]); rzk[q] = fast_rcp(z[q]); }
        auto do_gram = [&](double& Ax_, double& Adt_) {
            double d[NCG], t[NCG];
#pragma unroll
            for (int q = 0; q < NCG; q++) {
                const double rx = rxk[q], rz = rzk[q];
                d[q] = ok[q] ? x[q] * rz : 0.0;
                t[q] = ok[q] ? c[q] - v[q] + mu * rx : 0.0;
            }
            // ---- Gram products, one group at a time on the whole wave ----
#pragma unroll 1
            for (int g = 0; g < G; g++) {
                if (__shfl((int)live, g * MP, WAVE) == 0) continue;      // an idle lane group (small batch, or the batch's tail)
                // (a slot that carries rho -- every pass but an LP's first -- needs no A x from the Gram pass: -32 FMAs,
                // -16 LDS reads, -4 shuffles per LP-iteration, round 3)
                const bool carried = __shfl((int)have_pred, g * MP, WAVE) != 0;
                // an LP's first pass (have_pred is cleared where a slot loads an LP and nowhere else) starts from x = z = 1: its
                // M and A x are the handle's (GWave::gram_first); `first` is null under warm start
                const bool from_image = FIRST_IMAGE && first != nullptr && !carried;
                if (grp == g) {
#pragma unroll
                    for (int q = 0; q < NCD; q++) {
                        const int p = G_::kpos(gl + MP * q);
                        if (!carried && !from_image) w.stage[p] = ok[q] ? x[q] : 0.0;
                        if (!from_image) w.stage[ND + p] = d[q];
                        w.stage[2 * ND + p] = d[q] * t[q];
                    }
                }
                wave_lds_sync();
                double axg = 0.0, adg;
                if (carried) w.template gram_one<false, false, GRAM_SELB>(g, axg, adg);
                else if (from_image) w.gram_first(g, first, axg, adg);
                else w.template gram_one<true, false, GRAM_SELB>(g, axg, adg);
                wave_lds_sync();
                if (grp == g) { Ax_ = axg; Adt_ = adg; }
            }
            if (SL) {   // identity columns: x_slack and (d t)_slack go straight to row gl, d_slack onto the diagonal of M
                Ax_ += ok[NCG - 1] ? x[NCG - 1] : 0.0;
                Adt_ += d[NCG - 1] * t[NCG - 1];
                if constexpr (FULL) {   // d_slack is a bare product here: added rounded, as the generic text adds it (see gam above)
                    double ds = d[NCG - 1];
                    asm volatile("" : "+v"(ds));
                    w.slab[G_::sidx(gl, gl)] += ds;
                } else {
                    w.slab[G_::sidx(gl, gl)] += d[NCG - 1];
                }
                wave_lds_sync();
            }
        };
        do_gram(Ax, Adt);
        STAMP(2)
        const double rho = have_pred ? rho_pred : b - Ax;
        const double rhs = Adt - rho;
        double rdiag;
        double fs[1] = {rhs};     // the first solve's right-hand side rides through the sweep: L^-1 rhs when it returns
        // (the slack-aware (32, 96) predictor-corrector kernel alone has no registers for it: 10 -> 18 spilt; it keeps the plain sweep)
        constexpr bool CARRY = GWave<MP, NP, SL>::CARRY && !(PC && SL && MP == 32 && NP == 96);
        // `fused` is a run-time flag, not `if constexpr`: whether the guarded path replaces the factor is known only when the sweep
        // returns, so both back_after_sweep() and the whole fwd_back() are inlined at the first solve of a carrying kernel
        bool fused = CARRY;      // (wave-uniform) ... unless the guarded path replaced the factor
        // the split sweep (GWave::factor_sweep) wherever it costs no register: the same kernel as above goes from 2 to 10 spilt with it
        constexpr bool SPLIT = GWave<MP, NP, SL>::SPLIT && !(PC && SL && MP == 32 && NP == 96);
        {
            double W[MP];
            const int gd = w.ogl();
            if (!FULL && m < MP) {   // padded rows of A are zero rows/columns of M: make them identity rows -- in the slab, before the rows
                            // are fetched (one masked LDS write; as 32 selects on the fetched row it was 98 vector instructions
                            // per iteration, executed whether or not m < MP: the compiler had if-converted the branch)
                if (!rowok) w.slab[G_::sidx(gd, gd)] = 1.0;
                wave_lds_sync();
            }
            w.template load_row_for_sweep<SPLIT>(W);
            double diag = rowok ? w.slab[G_::sidx(gd, gd)] : 0.0;
            const double beta2 = grp_max<MP>(fabs(diag));
            wave_lds_sync();
            STAMP(3)
            bool redo;
            if constexpr (CARRY) redo = w.template factor_dpp_fwd<false, SPLIT, PIVOT_SIGN>(W, beta2, o.pivot_floor, live, rdiag, fs);
            else redo = w.template factor_dpp<false, SPLIT, PIVOT_SIGN>(W, beta2, o.pivot_floor, live, rdiag);
            if (redo || (o.flags & PYCLLP_FLAG_FORCE_GUARD_PATH)) {
                // the Nocedal-Wright guard would have bitten somewhere: re-form M and factor with the guard applied
                double Ax2, Adt2;
                do_gram(Ax2, Adt2);
                rdiag = w.factor_guarded_inplace(rowok, beta2, o.pivot_floor);
                fused = false;    // the carried forward half belongs to the dropped factor
            }
            STAMP(4)
        }
        double cor[NCG];          // PC: mu - dx_a dz_a per column (the corrector's complementarity target)
        double rhs_c = rhs;
        if constexpr (PC) {
            // ---- predictor (mu = 0): dy_a, dx_a, dz_a; how far it gets; centering; the corrector's right-hand side ----
            const double dya = fused ? w.back_after_sweep(fs[0], rdiag) : w.fwd_back(rhs, rdiag);
            double wva[NCG], dxa[NCG], dza[NCG], dt[NCG];
            w.template At_times<false, AT_FUSED>(dya, wva);
            double tha = 0.0;
#pragma unroll
            for (int q = 0; q < NCG; q++) {
                const double rx = rxk[q], rz = rzk[q];
                const double dq = ok[q] ? x[q] * rz : 0.0;
                const double ta = ok[q] ? c[q] - v[q] : 0.0;
                dxa[q] = (ta - wva[q]) * dq;
                dza[q] = ok[q] ? (-z[q] * dxa[q]) * rx - z[q] : 0.0;
                if (ok[q]) tha = fmax(tha, fmax(-dza[q] * rz, -dxa[q] * rx));
            }
            tha = grp_max<MP>(tha);
            const double theta_a = fmin(1.0 / tha, 1.0);
            double ga = 0.0;
#pragma unroll
            for (int q = 0; q < NCG; q++) ga += ok[q] ? fma(theta_a, dxa[q], x[q]) * fma(theta_a, dza[q], z[q]) : 0.0;
            ga = grp_sum<MP>(ga);
            const double sg = ga / gam;
            mu = sg * sg * sg * gam / (double)n;
#pragma unroll
            for (int q = 0; q < NCG; q++) {
                const double rx = rxk[q], rz = rzk[q];
                cor[q] = ok[q] ? mu - dxa[q] * dza[q] : 0.0;
                const double tq = ok[q] ? c[q] - v[q] + cor[q] * rx : 0.0;
                dt[q] = (ok[q] ? x[q] * rz : 0.0) * tq;
            }
            rhs_c = w.A_times(dt) - rho;
        }
        double dy = (!PC && fused) ? w.back_after_sweep(fs[0], rdiag) : w.fwd_back(rhs_c, rdiag);
        STAMP(5)
        double wv[NCG], dx[NCG], d[NCG];
        w.template At_times<false, AT_FUSED>(dy, wv);
        // d and t are recomputed (bit-identical) rather than kept alive across the factorisation: 12 VGPRs
#pragma unroll
        for (int q = 0; q < NCG; q++) {
            const double rx = rxk[q], rz = rzk[q];
            d[q] = ok[q] ? x[q] * rz : 0.0;
            const double tq = ok[q] ? c[q] - v[q] + (PC ? cor[q] : mu) * rx : 0.0;
            dx[q] = (tq - wv[q]) * d[q];
        }
        STAMP(6)
        // ---- x-space iterative refinement (oracle newton_dy) ----
        int nref = 0;
        double e;
        for (;;) {
            e = rho - w.A_times(dx);
            const double maxe = grp_max<MP>(fabs(e));
            const bool need = live && (maxe > etol) && (nref < o.max_refine);
            STAMP(7)
            if (!__any(need)) break;
            const double eta = w.fwd_back(need ? e : 0.0, rdiag);
            double w2[NCG];
            w.template At_times<false, AT_FUSED>(eta, w2);
#pragma unroll
            for (int q = 0; q < NCG; q++) {
                dx[q] = fma(d[q], w2[q], dx[q]);
                wv[q] -= w2[q];
            }
            dy -= eta;
            nref += need ? 1 : 0;
        }
        // ---- stop tests after the Newton work: only for a slot's first pass (no predicted rho yet), plus the NaN guard ----
        double r2 = r2_pred;
        const unsigned long long nf = __ballot(!isfinite(dy));
        const bool dy_bad = ((nf >> (grp * MP)) & gmask) != 0ull;
        int stat = PYCLLP_STATUS_ITERATION_LIMIT;
        bool fin = true;
        if (__all(have_pred || !live)) {    // (wave-uniform: no slot of the wave is on its first pass -- all but one pass in ~12)
            if (dy_bad) stat = PYCLLP_STATUS_NUMERICAL; else fin = false;
        } else {
            const double r2_first = grp_sum<MP>(rho * rho);      // (whole groups, under a wave-uniform condition)
            if (!have_pred) r2 = r2_first;
            const int verdict = stop_verdict(r2, s2, gam, po, tol_r, tol_s, r2_0, s2_0, o.eps, live && !have_pred, exact_norms);
            if (!have_pred && verdict >= 0) stat = verdict;
            else if (dy_bad) stat = PYCLLP_STATUS_NUMERICAL;
            else fin = false;
        }

        double du_start = 0.0;       // b'y of the point this pass started from, for the LP that its step takes to the iteration limit
        bool at_limit = false;
        if (!fin) {
            // ---- step (primal_normal.cl:122-156) ----
            if (it + 1 >= o.max_iter) { du_start = grp_sum<MP>(b * y); at_limit = true; }     // (per group; before y moves)
            double dz[NCG];
            double th = 0.0;
#pragma unroll
            for (int q = 0; q < NCG; q++) {
                const double rx = rxk[q], rz = rzk[q];
                dz[q] = ok[q] ? ((PC ? cor[q] : mu) - z[q] * dx[q]) * rx - z[q] : 0.0;
                if (ok[q]) th = fmax(th, fmax(-dz[q] * rz, -dx[q] * rx));
            }
            th = grp_max<MP>(th);
            const double theta = fmin(o.r / th, 1.0);
            y = fma(theta, dy, y);
#pragma unroll
            for (int q = 0; q < NCG; q++) {
                x[q] = fma(theta, dx[q], x[q]);
                z[q] = fma(theta, dz[q], z[q]);
                v[q] = fma(theta, wv[q], v[q]);
            }
            r2_0 = r2; s2_0 = s2;
            rho_pred = fma(theta, e - rho, rho);   // b - A(x + theta dx) = (1-theta) rho + theta (rho - A dx)
            have_pred = true;
            it++;
            if (it >= o.max_iter) fin = true;   // status stays ITERATION_LIMIT
        }
        STAMP(8)
        if (fin && live) finalize(stat, at_limit ? du_start : grp_sum<MP>(b * y));
    }
    STAMP_FLUSH(o, blockIdx.x * wpb + wave)
}
