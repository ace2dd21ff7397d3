// block.h -- internal interface between abi_sparse.hip (C ABI, handles) and the units that compile the workgroup-per-LP kernel
// of the sparse shared-A path (ipm_block.inc) with the kernel that ends the LPs a wave kernel deferred -- ipm_dense.hip, which
// says why -- and the three batched LDL' kernels (ldl_batched.inc; ipm_block.hip).  Not part of the public ABI.
#ifndef PYCLLP_BLOCK_H
#define PYCLLP_BLOCK_H
#include "wave_common.h"

#define BLK_T 256
#define BLK_MAX_M 128
#define BLK_MAX_N 512
#define LDL_MAX_N 128

struct BlockA {            // device-side description of the shared constraint matrix
    int m, n, nnz;
    const double* csr_val; const int* csr_ptr; const int* csr_col;   // A by rows
    const double* csc_val; const int* csc_ptr; const int* csc_row;   // A by columns
    int n_entries, n_terms;                                          // Gram term list
    const int* ent_tri; const int* ent_ptr;                          // packed index of entry e, its term range
    const double* term_w; const int* term_col;                       // weight a_ij a_kj and column j
    int a_in_lds;                                                    // CSR/CSC copied to LDS at block start
    // per-problem values of A (SparseMatrix.data[nproblems, nnz], pycllp/lp.py:16-54): the structure above is shared, the
    // values of LP `lp` are a_batch[lp, :] in CSR order (kernel argument); what the kernel then needs besides them:
    const int* csc_src;                                              // CSC position -> CSR index of the same entry
    const int* term_ia; const int* term_ib;                          // Gram term = val[term_ia] * val[term_ib]
};

// LDS bytes of a workgroup of ipm_block_kernel: an upper bound of the carve-up at the top of ipm_block.inc -- the packed
// triangle of M, two N-vectors, seven m-vectors padded to 8 rows, the reduction scratch; with_a: also A's CSR / CSC copy
inline size_t block_lds_bytes(int m, int n, int nnz, bool with_a) {
    const size_t mp8 = ((size_t)m + 7) & ~(size_t)7;
    const size_t base = sizeof(double) * ((size_t)m * (m + 1) / 2 + 1 + 2 * ((size_t)n + 1) + 7 * mp8 + 8);
    return with_a ? base + sizeof(double) * 2 * (size_t)nnz + sizeof(int) * (2 * (size_t)nnz + m + n + 2) + 16 : base;
}

// Solve B LPs on `blocks` workgroups with `lds` bytes of LDS each (argument meaning of pycllp_hip_sparse_solve; qhead: a zeroed
// work-queue head).  worklist: null, or the LPs to solve (worklist[0] = count) -- those a wave kernel deferred.  a_batch: null,
// or [B, nnz] per-problem values in CSR order.  block_set_lds(lds) comes first: the kernel's dynamic LDS, set apart from the
// launches because the entries report its failure in words of their own.
hipError_t block_set_lds(int lds);
hipError_t block_launch_solve(const BlockA& A, long blocks, int lds, long B, const double* b, const double* c, double* x, double* y,
                              double* z, double* pobj, double* dobj, int* status, int* iters, int* qhead, const int* worklist,
                              const double* a_batch, DevOpts o, hipStream_t st);
// One Newton step for B states (semantics of pycllp_hip_dense_newton) on the same kernel.
hipError_t block_launch_newton(const BlockA& A, long blocks, int lds, long B, const double* x, const double* z, const double* y,
                               const double* b, const double* c, double mu, double* dy, int* nref, int* qhead, DevOpts o,
                               hipStream_t st);
// status <- PYCLLP_STATUS_NUMERICAL for the LPs of a wave kernel's worklist when no guarded kernel can take them
hipError_t block_launch_deferred_to_numerical(const int* worklist, int* status, hipStream_t st);

// The kernels of pycllp_hip_ldl, pycllp_hip_ldl_solve (modified) and pycllp_hip_forward_backward_ldl, one matrix per workgroup
// on min(B, 4096) workgroups.  On an error *what names the step it came from, in the entry's words.
hipError_t ldl_launch_factor(int n, long B, const double* A, double* L, double* D, int modified, double beta, double delta,
                             hipStream_t st, const char** what);
hipError_t ldl_launch_solve(int n, long B, const double* A, const double* rhs, double* x, int modified, double beta, double delta,
                            hipStream_t st, const char** what);
hipError_t ldl_launch_forward_backward(int n, long B, const double* L, const double* D, const double* b, double* x, hipStream_t st,
                                       const char** what);
#endif
