"""CPU: the C-ABI library loads and exports every symbol include/pycllp_hip.h declares (no compute calls)."""
import ctypes
import os
import re

import pytest

from conftest import ROOT
from pycllp_amd import _native


def declared_symbols():
    text = open(os.path.join(ROOT, "include", "pycllp_hip.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return sorted(set(re.findall(r"\b(pycllp_hip_\w+)\s*\(", text)))


def test_header_and_loader_agree():
    assert declared_symbols() == sorted(_native.EXPORTS)


def test_library_exports_every_declared_symbol():
    L = ctypes.CDLL(_native.LIB_PATH)
    for name in declared_symbols():
        assert hasattr(L, name), name


def test_defaults_and_argument_errors_without_gpu():
    L = _native.lib()
    assert L.pycllp_hip_abi_version() == 1
    o = _native.default_opts()
    assert (o.eps, o.delta, o.r, o.pivot_floor, o.refine_tol) == (1e-10, 0.02, 0.9, 1e-6, 1e-11)
    assert (o.max_iter, o.max_refine, o.flags) == (200, -1, 0)     # -1 = PYCLLP_MAX_REFINE_AUTO: 5 plain / 20 HSD, resolved in C
    assert L.pycllp_hip_dense_max_rows() == 256 and L.pycllp_hip_dense_max_cols() == 1280
    h = ctypes.c_void_p()
    # NULL matrix / bad sizes are rejected before any HIP call
    assert L.pycllp_hip_dense_init(3, 3, None, None, ctypes.byref(h)) == -1
    assert L.pycllp_hip_dense_init(0, 3, ctypes.c_void_p(8), None, ctypes.byref(h)) == -1
    assert b"bad argument" in L.pycllp_hip_last_error()
    # sizes outside the compiled kernels -> PYCLLP_E_UNSUPPORTED, surfaced as NotImplementedError
    rc = L.pycllp_hip_dense_init(257, 40, ctypes.c_void_p(8), None, ctypes.byref(h))
    assert rc == -2
    with pytest.raises(NotImplementedError):
        _native.check(rc, "init")
    with pytest.raises(TypeError):
        _native.default_opts(bogus=1)


def test_struct_layout_matches_header():
    assert ctypes.sizeof(_native.Opts) == 5 * 8 + 4 * 4


_BOUNDED = ("b", "c", "u", "x", "y", "z", "s", "pobj", "dobj", "status", "iters")
_GROUP_FLAGS = ("HSD", "PREDCORR", "WARM_START", "WAVE_KERNEL", "NO_SLACK_PATH")
_WAVE_FLAGS = _GROUP_FLAGS + ("BLOCK_KERNEL", "FORCE_GUARD_PATH")
# entry -> (its device arrays in order, the pointers it requires, the flags it rejects, its sentence about them): the strings
# are the library's, byte for byte
RESTRICTED = {
    "pycllp_hip_dense_solve_bounded": (
        _BOUNDED, ("b", "c", "u", "x", "status"), _GROUP_FLAGS,
        b"pycllp_hip_dense_solve_bounded: HSD, PREDCORR, WARM_START, WAVE_KERNEL and NO_SLACK_PATH are not available with "
        b"upper bounds"),
    "pycllp_hip_dense_solve_batch": (
        ("A", "b", "c", "x", "y", "z", "pobj", "dobj", "status", "iters"), ("A", "b", "c", "x", "status"), _GROUP_FLAGS[:4],
        b"pycllp_hip_dense_solve_batch: HSD, PREDCORR, WARM_START and WAVE_KERNEL are not available with per-problem matrices"),
    "pycllp_hip_dense_solve_batch_bounded": (
        ("A",) + _BOUNDED, ("A", "b", "c", "u", "x", "status"), _GROUP_FLAGS,
        b"pycllp_hip_dense_solve_batch_bounded: HSD, PREDCORR, WARM_START, WAVE_KERNEL and NO_SLACK_PATH are not available "
        b"with upper bounds on per-problem matrices"),
    "pycllp_hip_sparse_solve_bounded": (
        _BOUNDED, ("b", "c", "u", "x", "status"), _WAVE_FLAGS,
        b"pycllp_hip_sparse_solve_bounded: HSD, PREDCORR, WARM_START, WAVE_KERNEL, BLOCK_KERNEL, NO_SLACK_PATH and "
        b"FORCE_GUARD_PATH are not available with upper bounds"),
    "pycllp_hip_sparse_solve_batch_bounded": (
        ("Adata",) + _BOUNDED, ("Adata", "b", "c", "u", "x", "status"), _WAVE_FLAGS,
        b"pycllp_hip_sparse_solve_batch_bounded: HSD, PREDCORR, WARM_START, WAVE_KERNEL, BLOCK_KERNEL, NO_SLACK_PATH and "
        b"FORCE_GUARD_PATH are not available with upper bounds on per-problem matrices"),
}


@pytest.mark.parametrize("entry", sorted(RESTRICTED))
def test_restricted_entries_refuse_with_their_own_messages(entry):
    """The argument checks of the entries that take only some flags come before the handle is read (the handle here is 64
    zero bytes) and before any HIP call, and each names its own entry in ``pycllp_hip_last_error()``."""
    L = _native.lib()
    arrays, required, rejected, sentence = RESTRICTED[entry]
    fn = getattr(L, entry)
    fake = ctypes.create_string_buffer(64)
    handle = ctypes.cast(fake, ctypes.c_void_p)
    bad_argument = entry.encode() + b": bad argument"

    def call(h, flags=0, null=None):
        args = [h, 4]
        for name in arrays:
            args.append(None if name == null else ctypes.c_void_p(8))
            if name == "A":
                args.append(5)                                   # a_cols: read only after the checks
        return fn(*args, ctypes.byref(_native.default_opts(flags=flags)), None)

    assert call(None) == -1 and L.pycllp_hip_last_error() == bad_argument
    for name in required:
        assert call(handle, null=name) == -1 and L.pycllp_hip_last_error() == bad_argument, name
    for name in rejected:
        assert call(handle, flags=getattr(_native, "FLAG_" + name)) == -1 and L.pycllp_hip_last_error() == sentence, name
    assert fake.raw == bytes(64)
