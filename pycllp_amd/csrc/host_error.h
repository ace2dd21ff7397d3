// The thread's error message (pycllp_hip_last_error): abi_sparse.hip keeps the buffer, every unit that holds entries writes
// it through these.  Host code only.
#pragma once

// message <- "<entry>: <what>"; returns code (a PYCLLP_E_* value)
int pycllp_entry_error(int code, const char* entry, const char* what);
// message <- "<what>: <hipGetErrorString(code)>" for a hipError_t, <what> alone for a PYCLLP_E_* value; returns code
int pycllp_runtime_error(int code, const char* what);
// message <- "<entry>: (m=.., n=..) exceeds the compiled kernels (m<=.., n<=..)" or, with max_m = 0, "<entry>: n=.. exceeds
// the compiled kernel (n<=..)"; returns PYCLLP_E_UNSUPPORTED
int pycllp_exceeds_error(const char* entry, int m, int n, int max_m, int max_n);
// message <- "<entry>: a_cols = .., expected .. (..)": the columns of per-problem dense matrices, `tail` when they come without
// the identity tail; returns PYCLLP_E_BADARG
int pycllp_a_cols_error(const char* entry, long a_cols, int expected, bool tail);
