// ipm_block.hip -- translation unit of the batched LDL' kernels (ldl_batched.inc) behind the ldl_launch_* functions of
// block.h; abi_sparse.hip holds their entries.  Built with the scheduler flag of ipm_dense.hip, the unit these kernels were
// compiled in before.  (The block kernel itself, ipm_block.inc, and deferred_to_numerical_kernel are compiled in ipm_dense.hip:
// see there.)
#include "block.h"
#include "ldl_batched.inc"

hipError_t ldl_launch_factor(int n, long B, const double* A, double* L, double* D, int modified, double beta, double delta,
                             hipStream_t st, const char** what) {
    const int lds = (int)(sizeof(double) * ((size_t)n * (n + 1) + 8));
    *what = "hipFuncSetAttribute(ldl_batched_kernel)";
    const hipError_t e = set_dyn_lds((const void*)ldl_batched_kernel, lds); if (e != hipSuccess) return e;
    const long blocks = B < 4096 ? B : 4096;
    *what = "ldl_batched_kernel launch";
    hipLaunchKernelGGL(ldl_batched_kernel, dim3((unsigned)blocks), dim3(n <= 64 ? 64 : 128), lds, st, n, B, A, L, D, modified, beta,
                       delta);
    return hipGetLastError();
}

hipError_t ldl_launch_solve(int n, long B, const double* A, const double* rhs, double* x, int modified, double beta, double delta,
                            hipStream_t st, const char** what) {
    const int lds = (int)(sizeof(double) * ((size_t)n * (n + 1) + n + 8));
    *what = "hipFuncSetAttribute(ldl_solve_batched_kernel)";
    const hipError_t e = set_dyn_lds((const void*)ldl_solve_batched_kernel, lds); if (e != hipSuccess) return e;
    const long blocks = B < 4096 ? B : 4096;
    *what = "ldl_solve_batched_kernel launch";
    hipLaunchKernelGGL(ldl_solve_batched_kernel, dim3((unsigned)blocks), dim3(n <= 64 ? 64 : 128), lds, st, n, B, A, rhs, x,
                       modified, beta, delta);
    return hipGetLastError();
}

hipError_t ldl_launch_forward_backward(int n, long B, const double* L, const double* D, const double* b, double* x, hipStream_t st,
                                       const char** what) {
    const int lds = (int)(sizeof(double) * ((size_t)n * (n + 1) / 2 + n + 8));
    *what = "hipFuncSetAttribute(forward_backward_ldl_kernel)";
    const hipError_t e = set_dyn_lds((const void*)forward_backward_ldl_kernel, lds); if (e != hipSuccess) return e;
    const long blocks = B < 4096 ? B : 4096;
    *what = "forward_backward_ldl_kernel launch";
    hipLaunchKernelGGL(forward_backward_ldl_kernel, dim3((unsigned)blocks), dim3(n <= 64 ? 64 : 128), lds, st, n, B, L, D, b, x);
    return hipGetLastError();
}
