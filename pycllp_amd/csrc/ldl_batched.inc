// ldl_batched.inc -- stand-alone batched LDL' / modified LDL' of explicit dense symmetric matrices.
//
// Replaces the reference's test kernels `ldl` and `modified_ldl` (pycllp/cl/ldl.cl:28-55, 57-107; numpy
// prototypes pycllp/ldl.py:58-112), which factor one per-work-item matrix each (launched by the reference's
// tests/test_ldl.py:139-193 on 32 matrices of 100 x 100).  Here one matrix is owned by one workgroup: the matrix
// sits in LDS (row stride n+1: column reads are conflict free), thread i owns row i, the sweep is right-looking
// and stores L in place.  Output layout as the reference: L packed lower-triangular with unit diagonal,
// L[i(i+1)/2 + j] (ldl.cl:12-18, per matrix instead of batch-interleaved), D[n].  n <= LDL_MAX_N (block.h).

__device__ __forceinline__ double block_max(double v, double* red, int tid, int nwaves) {
    v = wave_max(v);
    if ((tid & 63) == 0) red[tid >> 6] = v;
    __syncthreads();
    double r = red[0];
    for (int w = 1; w < nwaves; w++) r = fmax(r, red[w]);
    __syncthreads();
    return r;
}

__global__ void __launch_bounds__(128)
ldl_batched_kernel(int n, long B, const double* __restrict__ Ag, double* __restrict__ Lg, double* __restrict__ Dg,
                   int modified, double beta, double delta) {
    extern __shared__ __attribute__((aligned(16))) double lds[];
    const int S = n + 1;
    double* M = lds;                 // n x S
    double* red = lds + n * S;       // per-wave partials
    const int i = threadIdx.x;
    const int nwaves = blockDim.x >> 6;
    const long tri_n = (long)n * (n + 1) / 2;
    for (long mat = blockIdx.x; mat < B; mat += gridDim.x) {
        const double* A = Ag + mat * (long)n * n;
        for (int e = i; e < n * n; e += blockDim.x) M[(e / n) * S + (e % n)] = A[e];
        __syncthreads();
        for (int j = 0; j < n; j++) {
            const double piv = M[j * S + j];
            const double u = (i > j && i < n) ? M[i * S + j] : 0.0;
            double Dj = piv;
            if (modified) {   // Nocedal & Wright alg. 3.4 guard, ldl.cl:98-99
                const double theta = block_max(fabs(u), red, i, nwaves);
                const double tb = theta / beta;
                Dj = fmax(fabs(piv), fmax(tb * tb, delta));
            }
            const double l = u / Dj;
            __syncthreads();                       // column j has been read by everyone
            if (i > j && i < n) M[i * S + j] = l;
            if (i == j) Dg[mat * n + j] = Dj;
            __syncthreads();
            if (i > j && i < n) {
                const double lD = l * Dj;
                for (int k = j + 1; k <= i; k++) M[i * S + k] = fma(-lD, M[k * S + j], M[i * S + k]);
            }
            __syncthreads();
        }
        if (i < n) {
            double* L = Lg + mat * tri_n + (long)i * (i + 1) / 2;
            for (int k = 0; k < i; k++) L[k] = M[i * S + k];
            L[i] = 1.0;
        }
        __syncthreads();
    }
}

// x = A^-1 rhs with the modified LDL' formed on the fly -- pycllp/ldl.py:242-281 forward_backward_modified_ldl (the
// prototype of the OpenCL Newton solve): the forward substitution rides on the factorisation sweep (x_j /= D_j, then
// x_i -= u_ij x_j with the RAW column u, ldl.py:270-273), the backward substitution reuses L.  One matrix per
// workgroup, thread i owns row i.  modified == 0 gives pycllp/ldl.py:202-239 solve_ldl (used for n > 128 never: the
// register kernel of ipm_wreg.hip (ldl_solve_wreg_kernel) serves it; kept as the generic form).
__global__ void __launch_bounds__(128)
ldl_solve_batched_kernel(int n, long B, const double* __restrict__ Ag, const double* __restrict__ rhs,
                         double* __restrict__ xg, int modified, double beta, double delta) {
    extern __shared__ __attribute__((aligned(16))) double lds[];
    const int S = n + 1;
    double* M = lds;
    double* xs = lds + n * S;        // [n]
    double* red = xs + n;
    const int i = threadIdx.x;
    const int nwaves = blockDim.x >> 6;
    for (long mat = blockIdx.x; mat < B; mat += gridDim.x) {
        const double* A = Ag + mat * (long)n * n;
        for (int e = i; e < n * n; e += blockDim.x) M[(e / n) * S + (e % n)] = A[e];
        if (i < n) xs[i] = rhs[mat * n + i];
        __syncthreads();
        for (int j = 0; j < n; j++) {
            const double piv = M[j * S + j];
            const double u = (i > j && i < n) ? M[i * S + j] : 0.0;
            double Dj = piv;
            if (modified) {
                const double theta = block_max(fabs(u), red, i, nwaves);
                const double tb = theta / beta;
                Dj = fmax(fabs(piv), fmax(tb * tb, delta));
            }
            const double xj = xs[j] / Dj;
            const double l = u / Dj;
            __syncthreads();                       // column j and x_j have been read by everyone
            if (i == j) xs[j] = xj;
            if (i > j && i < n) { xs[i] -= u * xj; M[i * S + j] = l; }
            __syncthreads();
            if (i > j && i < n)
                for (int k = j + 1; k <= i; k++) M[i * S + k] = fma(-u, M[k * S + j], M[i * S + k]);
            __syncthreads();
        }
        // backward: x_i -= sum_{k>i} L[k][i] x_k, column oriented (thread i owns x_i)
        for (int k = n - 1; k > 0; k--) {
            const double xk = xs[k];
            if (i < k) xs[i] -= M[k * S + i] * xk;
            __syncthreads();
        }
        if (i < n) xg[mat * n + i] = xs[i];
        __syncthreads();
    }
}

// x = (L D L')^-1 b for given factors -- pycllp/ldl.py:165-180 forward_backward_ldl.  L packed as pycllp_hip_ldl writes it.
__global__ void __launch_bounds__(128)
forward_backward_ldl_kernel(int n, long B, const double* __restrict__ Lg, const double* __restrict__ Dg,
                            const double* __restrict__ bg, double* __restrict__ xg) {
    extern __shared__ __attribute__((aligned(16))) double lds[];
    const long tri_n = (long)n * (n + 1) / 2;
    double* L = lds;                 // packed
    double* xs = lds + tri_n;
    const int i = threadIdx.x;
    for (long mat = blockIdx.x; mat < B; mat += gridDim.x) {
        for (long e = i; e < tri_n; e += blockDim.x) L[e] = Lg[mat * tri_n + e];
        if (i < n) xs[i] = bg[mat * n + i];
        __syncthreads();
        for (int k = 0; k < n - 1; k++) {        // forward: y_i -= L[i][k] y_k
            const double yk = xs[k];
            if (i > k && i < n) xs[i] -= L[(long)i * (i + 1) / 2 + k] * yk;
            __syncthreads();
        }
        if (i < n) xs[i] /= Dg[mat * n + i];
        __syncthreads();
        for (int k = n - 1; k > 0; k--) {        // backward: x_i -= L[k][i] x_k
            const double xk = xs[k];
            if (i < k) xs[i] -= L[(long)k * (k + 1) / 2 + i] * xk;
            __syncthreads();
        }
        if (i < n) xg[mat * n + i] = xs[i];
        __syncthreads();
    }
}
