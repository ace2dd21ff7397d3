"""ctypes loader for csrc/libpycllp_hip.so (C ABI: include/pycllp_hip.h).

The library is the product; there is NO fallback.  A missing library raises ``RuntimeError`` at first
use, and the solvers refuse to run without a ROCm device.
"""
import ctypes
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
# PYCLLP_HIP_LIB lets a developer point at a diagnostic build of the SAME library (tools/phase_profile.py)
LIB_PATH = os.environ.get("PYCLLP_HIP_LIB") or os.path.join(_HERE, "csrc", "libpycllp_hip.so")

STATUS_OPTIMAL, STATUS_PRIMAL_INFEASIBLE, STATUS_NUMERICAL, STATUS_DUAL_INFEASIBLE, STATUS_ITERATION_LIMIT = 0, 2, 3, 4, 5
FLAG_WARM_START, FLAG_WAVE_KERNEL, FLAG_FORCE_GUARD_PATH, FLAG_AUTOSCALE, FLAG_NO_SLACK_PATH = 1, 2, 4, 8, 16
FLAG_HSD = 32
FLAG_BLOCK_KERNEL = 64
FLAG_PREDCORR = 128
FLAG_AUTOSCALE_PER_LP = 256
FLAG_GENERIC_SHAPE = 512
FLAG_EXACT_NORMS = 1024
FLAG_PER_LP_FIRST_GRAM = 2048


class Opts(ctypes.Structure):
    """Mirror of ``pycllp_hip_opts``."""
    _fields_ = [("eps", ctypes.c_double), ("delta", ctypes.c_double), ("r", ctypes.c_double),
                ("pivot_floor", ctypes.c_double), ("refine_tol", ctypes.c_double),
                ("max_iter", ctypes.c_int), ("max_refine", ctypes.c_int), ("flags", ctypes.c_int),
                ("reserve_cus", ctypes.c_int)]


_i, _l, _d, _p = ctypes.c_int, ctypes.c_long, ctypes.c_double, ctypes.c_void_p     # _p: a device array, a handle, a stream
_O, _ip, _pp = ctypes.POINTER(Opts), ctypes.POINTER(ctypes.c_int), ctypes.POINTER(ctypes.c_void_p)


def _solve(arrays):
    """handle, B, the device arrays, opts, stream: the solve entries."""
    return [_p, _l] + [_p] * arrays + [_O, _p]


# (symbol, argument types, result type) of every symbol include/pycllp_hip.h declares (tests/test_abi.py checks the two
# stay in sync)
SIGNATURES = (
    ("pycllp_hip_abi_version", [], _i), ("pycllp_hip_last_error", [], ctypes.c_char_p),
    ("pycllp_hip_default_opts", [_O], None),
    ("pycllp_hip_dense_max_rows", [], _i), ("pycllp_hip_dense_max_cols", [], _i),
    ("pycllp_hip_dense_init", [_i, _i, _p, _p, _pp], _i),
    ("pycllp_hip_dense_solve", _solve(9), _i),                  # b, c, x, y, z, pobj, dobj, status, iters
    ("pycllp_hip_dense_solve_bounded", _solve(11), _i),         # b, c, u, x, y, z, s, pobj, dobj, status, iters
    ("pycllp_hip_dense_solve_bounded_hsd", _solve(11), _i),     # as solve_bounded, on the self-dual embedding
    ("pycllp_hip_dense_solve_batch", [_p, _l, _p, _l] + [_p] * 9 + [_O, _p], _i),    # A [B, m, a_cols], a_cols, then as solve
    ("pycllp_hip_dense_solve_batch_bounded", [_p, _l, _p, _l] + [_p] * 11 + [_O, _p], _i),    # ... then as solve_bounded
    ("pycllp_hip_dense_solve_batch_bounded_hsd", [_p, _l, _p, _l] + [_p] * 11 + [_O, _p], _i),    # ... on the self-dual embedding
    ("pycllp_hip_dense_newton", [_p, _l, _p, _p, _p, _p, _p, _d, _p, _p, _O, _p], _i),
    ("pycllp_hip_dense_launch_info", [_p] + [_ip] * 5, _i), ("pycllp_hip_dense_kernel_kind", [_p], _i),
    ("pycllp_hip_dense_variant_info", [_p] + [_ip] * 3, _i), ("pycllp_hip_dense_plan_info", [_p] + [_ip] * 4, _i),
    ("pycllp_hip_dense_full_shape", [_p], _i),
    ("pycllp_hip_dense_free", [_p], None),
    ("pycllp_hip_ldl", [_i, _l, _p, _p, _p, _i, _d, _d, _p], _i),
    ("pycllp_hip_ldl_solve", [_i, _l, _p, _p, _p, _i, _d, _d, _p], _i),
    ("pycllp_hip_forward_backward_ldl", [_i, _l, _p, _p, _p, _p, _p], _i),
    ("pycllp_hip_sparse_max_rows", [], _i), ("pycllp_hip_sparse_max_cols", [], _i),
    ("pycllp_hip_sparse_init", [_i, _i, _i, _p, _p, _p, _p, _pp], _i),
    ("pycllp_hip_sparse_solve", _solve(9), _i),
    ("pycllp_hip_sparse_solve_batch", _solve(10), _i),          # A's values first
    ("pycllp_hip_sparse_solve_bounded", _solve(11), _i),
    ("pycllp_hip_sparse_solve_bounded_hsd", _solve(11), _i),    # as solve_bounded, on the self-dual embedding
    ("pycllp_hip_sparse_solve_batch_bounded", _solve(12), _i),  # A's values first, then as solve_bounded
    ("pycllp_hip_sparse_newton", [_p, _l, _p, _p, _p, _p, _p, _d, _p, _p, _O, _p], _i),
    ("pycllp_hip_sparse_launch_info", [_p] + [_ip] * 4, _i), ("pycllp_hip_sparse_variant_info", [_p] + [_ip] * 2, _i),
    ("pycllp_hip_sparse_plan_info", [_p] + [_ip] * 4, _i),
    ("pycllp_hip_sparse_free", [_p], None),
    # m, n, mk, B, rowmap, nnz, A's CSR (3), a, b, c, l, u, f, then b^, c^, u^, f^, invalid, stream
    ("pycllp_hip_general_to_bounded", [_i, _i, _i, _l, _p, _i] + [_p] * 14 + [_p], _i),
    # m, n, mk, B, rowmap, l, f^, invalid, x^, y^, z^, s^, then x, y, z, s, pobj, dobj, status, iters, stream
    ("pycllp_hip_general_from_bounded", [_i, _i, _i, _l] + [_p] * 16 + [_p], _i),
    # m, n, mk, B, rowmap, nnz, order, indptr, indices, A's values [B, nnz], out_len, gather, a, b, c, l, u, f, then A^ [B, out_len],
    # b^, c^, u^, f^, invalid, stream
    ("pycllp_hip_general_to_bounded_batch", [_i, _i, _i, _l, _p, _i] + [_p] * 4 + [_l] + [_p] * 13 + [_p], _i),
)
EXPORTS = tuple(name for name, _, _ in SIGNATURES)
# Entries that a library built from an earlier commit does not have.  Only a library named by PYCLLP_HIP_LIB (a diagnostic or
# an earlier build, for A/B runs of two builds under one Python tree) may lack them: it loads without them, `has_entry` says so,
# and what they report is then left out, never made up.  The product's own library must have every entry (AttributeError).
LATER_ENTRIES = ("pycllp_hip_dense_full_shape", "pycllp_hip_sparse_solve_bounded_hsd", "pycllp_hip_dense_solve_batch_bounded_hsd")
_absent = set()


def has_entry(name):
    """Whether the loaded library exports ``name`` (False only for a LATER_ENTRIES symbol of a PYCLLP_HIP_LIB library)."""
    lib()
    return name not in _absent

_lib = None


def lib():
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise RuntimeError(
            "pycllp_amd: HIP library %s is missing -- build it with `python -c 'import __graft_entry__ as g; "
            "g.build()'` or `make -C pycllp_amd/csrc` (there is no CPU fallback)" % LIB_PATH)
    L = ctypes.CDLL(LIB_PATH)
    for name, args, res in SIGNATURES:
        if name in LATER_ENTRIES and os.environ.get("PYCLLP_HIP_LIB") and not hasattr(L, name):
            _absent.add(name)
            continue
        f = getattr(L, name)
        f.argtypes, f.restype = args, res
    if L.pycllp_hip_abi_version() != 1:
        raise RuntimeError("pycllp_amd: ABI version mismatch in %s" % LIB_PATH)
    _lib = L
    return L


# The reference caps the refinement of its Newton systems at 5 passes (pycllp/cl/ldl.cl:645), which the plain path keeps.
# The homogeneous self-dual variant is this package's addition and its systems are harder near the end: with a cap of 5
# the degenerate LP 7557 of config 5's share sits at a 1.6e-10 relative gap for 70-150 iterations (oracle: 118 in all,
# the kernels 58-200 depending on rounding), with 10 passes it needs 48 iterations, with 20 passes 39.  No other LP of
# the test workloads uses more than 5.  The choice is made INSIDE the library (pycllp_hip_opts.max_refine = -1 = "auto",
# what pycllp_hip_default_opts returns: 5 on the plain path, 20 with PYCLLP_FLAG_HSD), so a C caller gets it too.
MAX_REFINE_AUTO, HSD_MAX_REFINE = -1, 20


def default_opts(**kw):
    o = Opts()
    lib().pycllp_hip_default_opts(ctypes.byref(o))
    for k, v in kw.items():
        if k not in dict(Opts._fields_):
            raise TypeError("unknown solver option %r" % k)
        setattr(o, k, v)
    return o


def check(rc, what):
    if rc != 0:
        msg = lib().pycllp_hip_last_error().decode("utf-8", "replace")
        if rc == -2:
            raise NotImplementedError("%s: %s" % (what, msg))
        if rc < 0:
            raise ValueError("%s: %s" % (what, msg))
        raise RuntimeError("%s failed (hipError %d): %s" % (what, rc, msg))
