// big.h -- internal interface between abi_sparse.hip (C ABI, handles; host.h) and ipm_big.hip (the workgroup-per-LP kernel for LPs
// beyond the register-resident kernels: 128 < m <= 256 rows or 512 < n <= 1280 columns).  Not part of the public ABI.
#ifndef PYCLLP_BIG_H
#define PYCLLP_BIG_H
#include "wave_common.h"

constexpr int BIG_MAX_M = 256;    // rows (16 x 16 blocks: MB <= 16)
constexpr int BIG_MAX_N = 1280;   // columns of the equality form (5 per thread)

// Device view of the tables of one constraint matrix (built by big_plan.h, uploaded by big_plan_create)
struct BigTab {
    int m, n, nnz, MB, dense, m_in_lds, lds_bytes;
    int nd, ks, imgR, n_sl;              // dense mode: nd dense columns, ks = k-steps of 4 columns, image rows, identity columns behind them
    const double* csr_val; const int* csr_ptr; const int* csr_col;   // A by rows
    const double* csc_val; const int* csc_ptr; const int* csc_row;   // A by columns
    const double* img;                   // [ks][imgR][4]
    const double* img_rm;                // dense mode: the dense columns row-major [m][nd] (A'u: thread = column, coalesced)
    const double* img_cm;                // ... and column-major [nd][imgR] (A v: thread = row, coalesced)
    int n_ent;                           // term-list mode: entries (i, k), i >= k, of M with their terms a_ij a_kj, column j
    const int* ent_dst; const int* ent_dst2; const int* ent_ptr; const double* term_w; const int* term_col;
};

__host__ __device__ inline int bidx(int K, int I) { return I * (I + 1) / 2 + K; }     // block (K, I), K <= I, of U = L'
// offset of element [kl][il] inside a block
__host__ __device__ inline int boff(int kl, int il) { return (kl >> 2) * 64 + (kl & 3) * 16 + il; }

// doubles of LDS the kernel carves (host and device agree through this one function)
__host__ __device__ constexpr size_t big_lds_doubles(int MB, int n, bool m_in_lds) {
    const size_t MP = 16 * (size_t)MB, NPv = ((size_t)n + 7) & ~(size_t)7;
    return (m_in_lds ? (size_t)MB * (MB + 1) / 2 * 256 : 0) + (size_t)MB * 256 + 2 * NPv + 9 * MP + 272 + 256 + 32;
}

struct BigPlan;   // host tables + device copies for one shared constraint matrix

// Builds the plan from a host CSR copy of A (m rows, n columns, equality form).  0 and *out on success, 1 when the problem is
// outside the kernel's limits; a positive hipError_t is returned as (1000 + error).
int big_plan_create(int m, int n, int nnz, const double* val, const int* ptr, const int* col, int max_lds, hipStream_t st,
                    BigPlan** out);
void big_plan_free(BigPlan* p);

// Solve B LPs (argument meaning of pycllp_hip_sparse_solve).
hipError_t big_launch_solve(BigPlan* p, long B, const double* b, const double* c, double* x, double* y, double* z,
                            double* pobj, double* dobj, int* status, int* iters, int* qhead, DevOpts o, int num_cu,
                            hipStream_t st, int* grid_out);
// One Newton step for B states (semantics of pycllp_hip_dense_newton).
hipError_t big_launch_newton(BigPlan* p, long B, const double* x, const double* z, const double* y, const double* b,
                             const double* c, double mu, double* dy, int* nref, int* qhead, DevOpts o, int num_cu,
                             hipStream_t st, int* grid_out);
int big_lds_bytes(const BigPlan* p);
int big_dense_mode(const BigPlan* p);   // 1: Gram product on the matrix cores from a dense image; 0: term list
// the instantiation ipm_big_kernel<WGPC, BNC> the plan's last launch ran ((0, 0) before the first) and whether the factor
// blocks sat in LDS (-1 before the first launch)
void big_shape(const BigPlan* p, int* wgpc, int* bnc, int* m_in_lds);
#endif
