// wreg.h -- internal interface between abi_sparse.hip (C ABI, handles; host.h), ipm_wreg.hip (host side of the register-resident
// one-LP-per-wavefront kernels of the sparse shared-A path) and the units that compile those kernels (ipm_wreg_*.hip on
// wreg_wave.h).  Not part of the public ABI.
#ifndef PYCLLP_WREG_H
#define PYCLLP_WREG_H
#include "wave_common.h"

// ---- shared between the host unit (ipm_wreg.hip) and the eleven units the wave kernels are compiled in (ipm_wreg_*.hip) ----
constexpr int MAX_NQ = 8;
constexpr int META_COFF = MAX_NQ, META_SEG = 2 * MAX_NQ, META_N = META_SEG + 16;

// Geometry of a wave's LDS area: the kernels (wreg_wave.h) and the plan builders of the host (wreg_plan.h) call the same functions.
// stage proper: N-vector staging; during factor/solve t, x and z parked at 0, NP, 2 NP and the stride-17 tile of the current
// diagonal block behind them
constexpr int TILE_D = 272;
__host__ __device__ constexpr int tile_off(int NQ) { return 192 * NQ > 768 ? 192 * NQ : 768; }
__host__ __device__ constexpr int stage_d(int NQ) { return tile_off(NQ) + TILE_D; }
constexpr int HB = 8;            // 16 x 16 blocks per Gram staging chunk: the stage and, behind it, the still unused W area (16 KB)
constexpr int WL = 144;          // doubles per diagonal-block slot: first the ORIGINAL diagonal block of M (lower triangle with
                                 // diagonal, row i at i(i+1)/2: 136), from stage K on W_K (strictly lower triangle, row i at i(i-1)/2)
// per-wave LDS doubles of an (MB, NQ) kernel: the stage, an N-vector, five m-vectors, the diagonal-block slots (a plan adds
// what its kind keeps behind them: t and s of the bounded kernel, an LP's own values or image)
__host__ __device__ constexpr int wave_doubles(int MB, int NQ) { return stage_d(NQ) + 64 * NQ + 5 * 16 * MB + MB * WL; }
// the diagonal blocks' entries ride with the last Gram staging chunk when its blocks end in front of the W area (where they go)
__host__ __device__ constexpr bool merge_diag(int MB, int NQ) {
    return MB * (MB - 1) / 2 > 0 && (MB * (MB - 1) / 2 - HB * ((MB * (MB - 1) / 2 + HB - 1) / HB - 1)) * 256 <= stage_d(NQ);
}
template <int MB>
struct WGeo {
    static constexpr int MP = 16 * MB;
    static constexpr int MR = (MP + 63) / 64;    // m-vector registers per lane in "lane = row" form
    static constexpr int MPL = 64 * MR;
    static constexpr int NBLK = MB * (MB - 1) / 2;
    // off-diagonal block (K, I), K < I, of U = L'
    __host__ __device__ static constexpr int bix(int K, int I) { return K * MB - K * (K + 1) / 2 + (I - K - 1); }
    // Gram staging chunks: the off-diagonal blocks in bix order, HB at a time; chunk NCHUNK = the diagonal blocks
    static constexpr int NCHUNK = (NBLK + HB - 1) / HB;
    __host__ __device__ static constexpr bool MERGE_DIAG(int NQ) { return merge_diag(MB, NQ); }
    static constexpr int WAVE_D(int NQ) { return wave_doubles(MB, NQ); }
};
// byte offset of a padded position of the N-vectors inside an LP's row: past the row, where a buffer load reads 0 and a
// store is dropped (row_rsrc, wreg_wave.h)
constexpr unsigned PAD_OFF = 0x7ffffff0u;

// Device view of the tables of one constraint matrix (built by wreg_plan_create).
struct WregTab {
    int m, n, nnz;
    int rmax, n_lev, n_term;
    int meta[META_N];     // [0..8) ELL depth of column register q, [META_COFF..) its first ELL slot, [META_SEG..) first level
                          // (index into lev) of Gram group g: the NCHUNK staging chunks of off-diagonal blocks, then the
                          // diagonal blocks; NCHUNK + 2 used -- copied to LDS
    const double* csr_val; const unsigned short* csr_col; const unsigned short* csr_ptr; const unsigned short* csr_len;
    // A by columns in ELL form over column POSITIONS: the columns are dealt to the (lane, register) positions of the
    // N-vectors sorted by length, so that each register's 64 columns are about equally long (JDS); colmap[pos] = 8 x column
    const double* ec_val; const unsigned short* ec_row; const unsigned* colmap; int ctot;   // (a byte offset; PAD_OFF for pos >= n)
    // Gram terms a_ij a_kj d_j of the strictly lower triangle of M, one record per term: weight a_ij a_kj, column position
    // of j, destination offset inside the group's staging area.  Inside a group the terms are ordered by LEVEL = rank of
    // the term inside its entry (i, k): level 0 holds the first term of every entry, level 1 the second term of the
    // entries that have one, ...; lev[] holds the item boundaries, level l of the table = items [lev[l], lev[l + 1]).
    // Destinations are distinct inside a level, so a level is one flat pass with no inner loop; level 0 stores, the
    // later levels accumulate in the same order a per-entry loop would.
    const double* t_w; const unsigned* t_cd; const int* lev;     // t_cd = column position | destination << 16
    int o_csr_val, o_ec_val, o_t_w, o_wave, o_lev, o_meta, o_csr_col, o_csr_ptr, o_csr_len, o_ec_row, o_colmap,
        o_t_cd;                                           // LDS byte offsets
    int wave_doubles, lds_bytes;
    // per-problem values of A (PA variants; SparseMatrix.data[nproblems, nnz], pycllp/lp.py:16-54): the tables above hold
    // the STRUCTURE only -- csr_val, ec_val and t_w are absent; every wavefront keeps the values of ITS LP (CSR order,
    // nnzp = nnz + 1 rounded up to even doubles, entry [nnz] = 0 for the padded slots) behind its wave area, and finds an
    // ELL slot's value through ec_src (CSR index of the slot) and a Gram term's weight as the product of the two entries
    // t_ab names (CSR index of a_ij | CSR index of a_kj << 16)
    int pa, nnzp, o_ec_src, o_t_ab;
    const unsigned short* ec_src; const unsigned* t_ab;
    // dense variant (DA): no tables, A as a row-major image [img_rows][as] of its first nd columns (the remaining n - nd
    // columns are the identity, column nd + i = e_i, or there are none), as = nd rounded up to 8, + 1
    int nd, as, img_rows, o_img, wpb;
    const double* img;
    // dense variant on per-problem matrices (DA && PA, pa != 0): no device copy (img null) -- every wavefront keeps the image
    // of ITS LP behind its wave area (wave_doubles includes img_rows x as) and fills it from a_batch [B, m, nd] per LP
};


typedef hipError_t (*wsolve_fn)(const WregTab&, long, const double*, const double*, const double*, double*, double*, double*,
                                double*, double*, int*, int*, int*, int*, DevOpts, int, hipStream_t);
typedef hipError_t (*wnewton_fn)(const WregTab&, long, const double*, const double*, const double*, const double*,
                                 const double*, double, double*, int*, int*, DevOpts, int, hipStream_t);
// the kernel for LPs with upper bounds (ipm_wreg_bounded.inc): argument meaning of pycllp_hip_sparse_solve_bounded
typedef hipError_t (*wbsolve_fn)(const WregTab&, long, const double*, const double*, const double*, double*, double*, double*,
                                 double*, double*, double*, int*, int*, int*, DevOpts, int, hipStream_t);
// ... on per-problem values of A: a_batch [B, nnz] in front of b (argument meaning of pycllp_hip_sparse_solve_batch_bounded)
typedef hipError_t (*wbpsolve_fn)(const WregTab&, long, const double*, const double*, const double*, const double*, double*,
                                  double*, double*, double*, double*, double*, int*, int*, int*, DevOpts, int, hipStream_t);

// The (MB, NQ) geometries of the wave kernels (MB 16-row blocks, NQ 64-column N-vector registers), ordered by cost: a plan
// takes the first of its kind with 16 MB >= m and 64 NQ >= n.  One list for the kernels on term tables, one for those on a
// dense image; every table below is derived from one of them.
#define WREG_TAB_SHAPES(X) X(1, 4) X(2, 4) X(3, 4) X(4, 2) X(4, 4) X(5, 6) X(6, 6) X(7, 6) X(8, 4) X(8, 6) X(8, 8)
#define WREG_DA_SHAPES(X)  X(1, 4) X(2, 4) X(3, 4) X(4, 2) X(4, 4) X(5, 4) X(6, 4) X(7, 4) X(8, 4) X(8, 6)
// ... and the dense-image shapes of the kernel on per-problem dense matrices (kWDAPA): the list above without (8, 6), whose
// instantiation does not stay free of scratch (28 bytes, like the shared-A kernel of that shape) -- DESIGN.md sections 10, 24
#define WREG_DAPA_SHAPES(X) X(1, 4) X(2, 4) X(3, 4) X(4, 2) X(4, 4) X(5, 4) X(6, 4) X(7, 4) X(8, 4)
// ... and those of the bounded kernel on per-problem dense matrices (kWBDDAPA): a list of its own, under the same rule -- DESIGN.md section 25
#define WREG_BDDAPA_SHAPES(X) X(1, 4) X(2, 4) X(3, 4) X(4, 2) X(4, 4) X(5, 4) X(6, 4) X(7, 4) X(8, 4)
// The bounded kernel on the homogeneous self-dual embedding (kWBDH, kWBDHDA; ipm_wreg_bdh.hip) runs on the plans of the bounded
// kernel, so its tables list the shapes of WREG_TAB_SHAPES / WREG_DA_SHAPES; a shape whose instantiation does not stay free of
// scratch (tools/kernel_resources.py, profiles/bounded_wave_hsd/kernel_resources.txt) keeps its row with a null launcher --
// the five shapes with MB = 8 (m' > 112) spill 10 to 82 VGPRs past the 512 registers of a lane
__host__ __device__ constexpr bool wreg_bdhsd_ships(int MB, int NQ, bool DA) { return MB < 8; }

// The launchers of one (MB, NQ) of one kernel kind; a launcher the kind does not have is null.
struct WVariant { int mb, nq; wsolve_fn solve, solve_hsd; wnewton_fn newton; wbsolve_fn solve_bounded; wbpsolve_fn solve_bounded_pa; };
struct WVariants { const WVariant* v; int n; };
// One table per kind, each defined by the translation unit that compiles its kernels; launchers are matched across tables
// by (MB, NQ), never by position.
extern const WVariants kWTab;      // ipm_wreg_tab.hip:  term tables (plain, HSD, Newton)
extern const WVariants kWDA;       // ipm_wreg_da.hip:   dense image (plain, HSD, Newton)
extern const WVariants kWPA;       // ipm_wreg_pa.hip:   per-problem A on structure tables (plain, HSD)
extern const WVariants kWDAPA;     // ipm_wreg_dapa.hip: per-problem dense A, a dense image per wave (plain)
extern const WVariants kWPC;       // ipm_wreg_pc.hip:   predictor-corrector kernels of kWTab's kind
extern const WVariants kWPCDA;     // ipm_wreg_pcda.hip: ... of kWDA's kind
extern const WVariants kWPCPA;     // ipm_wreg_pcpa.hip: ... of kWPA's kind
extern const WVariants kWBD;       // ipm_wreg_bd.hip:   upper bounds, term tables
extern const WVariants kWBDDA;     // ipm_wreg_bd.hip:   upper bounds, dense image
extern const WVariants kWBDPA;     // ipm_wreg_bdpa.hip: upper bounds, per-problem A on structure tables
extern const WVariants kWBDDAPA;   // ipm_wreg_bddapa.hip: upper bounds, per-problem dense A, a dense image per wave
extern const WVariants kWBDH;      // ipm_wreg_bdh.hip:  upper bounds on the self-dual embedding, term tables (solve_bounded; null: not shipped)
extern const WVariants kWBDHDA;    // ipm_wreg_bdh.hip:  upper bounds on the self-dual embedding, dense image

struct WregPlan;   // host tables + device copies for one shared constraint matrix

// Builds the plan from a host CSR copy of A (m rows, n columns, equality form).  Returns 0 and *out on success,
// 1 when the register-resident kernel does not cover the problem (too many rows/columns, tables larger than LDS):
// the caller then stays on ipm_block_kernel.  A positive hipError_t is returned as (1000 + error).
// pa != 0: the plan of the per-problem-A variants (structure tables only; `val` is not read).
int wreg_plan_create(int m, int n, int nnz, const double* val, const int* ptr, const int* col, int max_lds, int pa,
                     hipStream_t st, WregPlan** out);
// The plan of the bounded kernel for the same A: the tables or dense image of wreg_plan_create with 2 NP more doubles per
// wave (t and s), as many waves per workgroup (4 at most) as the LDS then takes.  Returns 1 when no bounded variant or LDS plan
// covers A.
int wreg_plan_create_bounded(int m, int n, int nnz, const double* val, const int* ptr, const int* col, int max_lds,
                             hipStream_t st, WregPlan** out);
// The plan of the bounded kernel on per-problem values of A: structure-only tables with nnzp + 2 NP doubles behind every wave
// area (the LP's values, then t and s), as many waves per workgroup (4 at most, 1 at least) as the LDS takes.  Returns 1 when
// no variant covers (m, n), when nnz >= 65535 or when not even one wave fits.  `val` is not read.
int wreg_plan_create_bounded_pa(int m, int n, int nnz, const double* val, const int* ptr, const int* col, int max_lds,
                                hipStream_t st, WregPlan** out);
// The plan of the wave kernel on per-problem DENSE matrices (kWDAPA): the geometry of wreg_plan_create's dense plan (identity
// tail detection on the CSR arrays given, R, AS, first covering variant) with no device copy of an image -- the image sits
// behind every wave area (wave_doubles enlarged by img_rows x AS) -- and as many waves per workgroup, 4 down to 1, as max_lds
// takes.  keep_tail: all n columns go into the image (nd = n) even where the matrix ends in the identity
// (PYCLLP_FLAG_NO_SLACK_PATH).  Returns 1 when no variant covers (m, n) or not even one wave fits.
int wreg_plan_create_dense_pa(int m, int n, int nnz, const double* val, const int* ptr, const int* col, int max_lds,
                              int keep_tail, hipStream_t st, WregPlan** out);
// The plan of the bounded kernel on per-problem DENSE matrices (kWBDDAPA): wreg_plan_create_dense_pa's without keep_tail (the
// bounded form always ends in the identity) and with 2 NP more doubles per wave, t and s, BEHIND the wave's image.  Returns 1
// when no variant covers (m, n) or not even one wave fits.
int wreg_plan_create_bounded_dense_pa(int m, int n, int nnz, const double* val, const int* ptr, const int* col, int max_lds,
                                      hipStream_t st, WregPlan** out);
void wreg_plan_free(WregPlan* p);

// Solve B LPs (same argument meaning as pycllp_hip_sparse_solve).  LPs whose factorisation would have needed the
// Nocedal-Wright guard are NOT solved: their indices are appended to defer[1..] (defer[0] = count, zeroed here) and
// their status is left at -1; the caller runs them through the guarded kernel afterwards.
// a_batch: [B, nnz] values of every LP in the CSR order of the arrays the plan was built from (PA plans only, else null); on a
// plan of wreg_plan_create_dense_pa: the dense matrices [B, m, nd], row-major.
hipError_t wreg_launch_solve(WregPlan* p, long B, const double* a_batch, const double* b, const double* c, double* x, double* y, double* z,
                             double* pobj, double* dobj, int* status, int* iters, int* qhead, int* defer, DevOpts o,
                             int num_cu, hipStream_t st, int* grid_out);

// Solve B LPs with upper bounds on a plan of wreg_plan_create_bounded (argument meaning of pycllp_hip_sparse_solve_bounded).
// An LP whose factorisation would have needed the Nocedal-Wright guard ends PYCLLP_STATUS_NUMERICAL.
// a_batch: [B, nnz] values of every LP in the plan's CSR order, on a plan of wreg_plan_create_bounded_pa; the dense matrices
// [B, m, nd], row-major, on a plan of wreg_plan_create_bounded_dense_pa; else null.
hipError_t wreg_launch_solve_bounded(WregPlan* p, long B, const double* a_batch, const double* b, const double* c, const double* u, double* x, double* y,
                                     double* z, double* s, double* pobj, double* dobj, int* status, int* iters, int* qhead,
                                     DevOpts o, int num_cu, hipStream_t st, int* grid_out);
// The same batch on the homogeneous self-dual embedding (ipm_wreg_bounded_hsd_kernel; argument meaning of
// pycllp_hip_sparse_solve_bounded_hsd), on a plan of wreg_plan_create_bounded: the kernel keeps nothing more behind the wave area.
// hipErrorInvalidValue on any other plan (a per-problem plan has no such kernel), hipErrorNotSupported where the plan's shape is
// not shipped (wreg_has_bounded_hsd says so beforehand).
hipError_t wreg_launch_solve_bounded_hsd(WregPlan* p, long B, const double* b, const double* c, const double* u, double* x, double* y,
                                         double* z, double* s, double* pobj, double* dobj, int* status, int* iters, int* qhead,
                                         DevOpts o, int num_cu, hipStream_t st, int* grid_out);
int wreg_has_bounded_hsd(const WregPlan* p);   // 1 when p is a shared-A bounded plan whose shape ipm_wreg_bounded_hsd_kernel ships in

// One Newton step for B states (semantics of pycllp_hip_dense_newton).  guard_hit[0] is set to 1 if any state would
// have needed the guard (the stand-alone step then simply ran without it).  *grid_out (optional): the workgroups launched.
hipError_t wreg_launch_newton(WregPlan* p, long B, const double* x, const double* z, const double* y, const double* b,
                              const double* c, double mu, double* dy, int* nref, DevOpts o, int num_cu, hipStream_t st,
                              int* grid_out);

// out = (L D L')^-1 rhs with L D L' = A for B explicit dense symmetric matrices A [B, n, n] (lower triangle read),
// n <= 128, pivots floored at floor_ (0: plain LDL'); one matrix per wavefront, factor held in registers.
hipError_t wreg_launch_ldl_solve(int n, long B, const double* A, const double* rhs, double* out, double floor_,
                                 int num_cu, hipStream_t st);
int wreg_lds_bytes(const WregPlan* p);
int wreg_block_threads(const WregPlan* p);   // 64 x waves per workgroup
int wreg_variant(const WregPlan* p);         // 1 = term tables, 2 = dense image
int wreg_image_cols(const WregPlan* p);      // the columns of a dense image (nd: n - m with an implied identity tail, else n); 0 on term tables
void wreg_shape(const WregPlan* p, int* mb, int* nq);   // the plan's (MB, NQ); (0, 0) for a null plan
int wreg_has_predcorr(const WregPlan* p);   // 1 when the plan's kernels have a PYCLLP_FLAG_PREDCORR variant (every plan of the wave kernel)
#endif
