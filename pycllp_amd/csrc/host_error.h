// The thread's error message (pycllp_hip_last_error) for the units that hold entries of their own: ipm_dense.hip keeps the
// buffer, the others write it through these.  Host code only.
#pragma once

// message <- "<entry>: <what>"; returns code (a PYCLLP_E_* value)
int pycllp_entry_error(int code, const char* entry, const char* what);
// message <- "<what>: <hipGetErrorString(code)>"; returns code (a hipError_t)
int pycllp_runtime_error(int code, const char* what);
