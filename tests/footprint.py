"""Where the library's entries write: an arena of guarded arrays around one call of one entry of include/pycllp_hip.h.

All input and output arrays of a call live in ONE ``torch.uint8`` allocation, each between two guard bands of ``GUARD`` bytes
(16 KiB: more than one padded row of the widest kernel, 1 280 columns x 8 B; an overrun that jumps further than one padded
row past an array is out of scope here).  Guard bands and output arrays start out as a sentinel: for f64 a quiet NaN with a
fixed payload (``SENT64``, compared as int64), for i32 a pattern that is no status and no iteration count (``SENT32``).  Two
placements:

  aligned   every array starts at a multiple of 256 B (what the torch allocator gives the plugins)
  natural   every f64 array starts at an address = 8 mod 16, every i32 array at an address = 4 mod 8: the weakest alignment the C
            types allow

An output may be passed as NULL (``null=``): it keeps its place in the arena and the entry gets no pointer to it.  After the call
and a stream sync ``Arena.check()`` asserts -- array name and first offending index in the message --
  (a) every guard band is bit-identical to the sentinel,
  (b) every input array is bit-identical to the copy taken before the call,
  (c) no element of a non-NULL output still holds the sentinel, and every NULL output is still all sentinel.

``call(entry, ...)`` hands the arrays to the library the way ``pycllp_amd.solvers.hip.Handle`` does (tensor views as device
pointers, None as NULL) and returns the entry's return code.  The module works on CPU tensors too: the CPU tests drive it with
Python functions in the entries' place.
"""
import ctypes

import numpy as np
import torch

GUARD = 16 * 1024
SENT64 = 0x7FF85EA7C0DEFACE            # a quiet NaN: exponent all ones, top mantissa bit set, payload 0x5EA7C0DEFACE
SENT32 = -0x5A5AC0DF                   # negative: no status (0..5), no iteration or refinement count
F64, I32 = torch.float64, torch.int32
_SENT64_I = np.array([SENT64], dtype=np.uint64).view(np.int64)[0].item()


class Spec(object):
    """One array of a call: ``role`` 'in' (``data``: numpy, copied in) or 'out' (``shape``; sentinel-filled)."""

    def __init__(self, name, role, dtype, shape=None, data=None):
        assert role in ("in", "out") and dtype in (F64, I32)
        self.name, self.role, self.dtype = name, role, dtype
        if role == "in":
            self.data = np.ascontiguousarray(data, dtype=np.float64 if dtype == F64 else np.int32)
            shape = self.data.shape
        self.shape = tuple(int(v) for v in shape)
        self.nbytes = int(np.prod(self.shape, dtype=np.int64)) * (8 if dtype == F64 else 4)


def inp(name, data, dtype=F64):
    return Spec(name, "in", dtype, data=data)


def out(name, shape, dtype=F64):
    return Spec(name, "out", dtype, shape=shape)


def _start(addr, dtype, placement):
    """The first address >= addr at which an array of ``dtype`` may start under ``placement``."""
    if placement == "aligned":
        return (addr + 255) & ~255
    assert placement == "natural"
    mod, rem = (16, 8) if dtype == F64 else (8, 4)
    return addr + (rem - addr) % mod


class Arena(object):
    def __init__(self, specs, placement, device="cpu", null=()):
        self.specs = list(specs)
        self.placement = placement
        names = [s.name for s in self.specs]
        assert len(set(names)) == len(names)
        self.null = set(null)
        assert self.null <= {s.name for s in self.specs if s.role == "out"}, self.null
        total = sum(s.nbytes + GUARD + 512 for s in self.specs) + GUARD + 512
        self.buf = torch.empty((total + 7) // 8 * 8, dtype=torch.uint8, device=device)
        base = self.buf.data_ptr()
        assert base % 16 == 0
        self.buf.view(torch.int64).fill_(_SENT64_I)
        self.offset, self.views = {}, {}
        cur = base
        for s in self.specs:
            cur = _start(cur + GUARD, s.dtype, placement)
            off = cur - base
            self.offset[s.name] = off
            v = self.buf[off:off + s.nbytes].view(s.dtype).view(s.shape)
            assert v.data_ptr() == cur
            if placement == "aligned":
                assert cur % 256 == 0
            else:
                assert cur % 16 == 8 if s.dtype == F64 else cur % 8 == 4
            if s.role == "in":
                v.copy_(torch.from_numpy(s.data))
            elif s.dtype == I32:
                v.fill_(SENT32)
            self.views[s.name] = v
            cur += s.nbytes
        assert cur - base + GUARD <= self.buf.numel()
        self.image = self.buf.clone()          # guard bands and inputs as they must stay
        self.fixed = torch.ones(self.buf.numel(), dtype=torch.bool, device=device)      # bytes no call may change
        for s in self.specs:
            if s.role == "out":
                self.fixed[self.offset[s.name]:self.offset[s.name] + s.nbytes] = False

    def __getitem__(self, name):
        """The array as the entry gets it: its view, or None for an output passed as NULL."""
        return None if name in self.null else self.views[name]

    def arrays(self):
        return {s.name: self[s.name] for s in self.specs}

    def result(self, name):
        return self.views[name].cpu().numpy().copy()

    def results(self):
        return {s.name: self.result(s.name) for s in self.specs if s.role == "out" and s.name not in self.null}

    def _sentinel_mask(self, s):
        v = self.views[s.name].reshape(-1)
        if s.dtype == F64:
            return v.view(torch.int64) == _SENT64_I
        return v == SENT32

    def check(self, outputs_written=True, untouched=()):
        """(a), (b), (c) of the module docstring.  ``outputs_written=False``: a refused call -- every output, NULL or not, must
        still be all sentinel.  ``untouched``: outputs the header says this call leaves as they were; they must still be all
        sentinel too."""
        if self.buf.is_cuda:
            torch.cuda.synchronize(self.buf.device)
        diff = self.buf != self.image
        if bool((diff & self.fixed).any()):
            self._report(diff.cpu().numpy())
        for s in self.specs:
            if s.role == "in":
                continue
            # (c)
            mask = self._sentinel_mask(s)
            if s.name in self.null or not outputs_written or s.name in untouched:
                if not bool(mask.all()):
                    why = ("passed as NULL" if s.name in self.null else
                           "of a refused call" if not outputs_written else "that the call leaves untouched")
                    raise AssertionError("output %r %s was written at element %d (%s placement)"
                                         % (s.name, why, int(np.flatnonzero(~mask.cpu().numpy())[0]), self.placement))
            elif bool(mask.any()):
                raise AssertionError("output %r not written at element %d (%s placement)"
                                     % (s.name, int(np.flatnonzero(mask.cpu().numpy())[0]), self.placement))

    def _report(self, diff):
        """Raise for the first changed byte outside the outputs: (a) a guard band, (b) an input."""
        size = lambda q: 8 if q.dtype == F64 else 4
        prev = None                 # the array before the band
        prev_end = 0
        for s in self.specs + [None]:
            lo = self.offset[s.name] if s is not None else self.buf.numel()
            bad = np.flatnonzero(diff[prev_end:lo])
            if bad.size:
                first = prev_end + int(bad[0])
                # the band belongs to the nearer array: index in its elements (negative: before its start)
                if s is not None and (prev is None or lo - first <= first - prev_end):
                    owner, idx = s, -((lo - first + size(s) - 1) // size(s))
                else:
                    owner, idx = prev, (first - self.offset[prev.name]) // size(prev)
                raise AssertionError("guard band of %r overwritten at element %d (%s placement, arena byte %d)"
                                     % (owner.name, idx, self.placement, first))
            if s is not None:
                if s.role == "in":
                    bad = np.flatnonzero(diff[lo:lo + s.nbytes])
                    if bad.size:
                        raise AssertionError("input %r changed at element %d (%s placement)"
                                             % (s.name, int(bad[0]) // size(s), self.placement))
                prev, prev_end = s, lo + s.nbytes
        raise AssertionError("arena changed outside its outputs")


class Plain(object):
    """The same arrays as ordinary separate contiguous tensors (the reference call): the interface of ``Arena`` without
    guards; outputs start as the sentinel so that ``check()`` still sees an unwritten element."""

    def __init__(self, specs, device="cpu"):
        self.specs, self.null, self.placement, self.views = list(specs), set(), "separate", {}
        for s in self.specs:
            if s.role == "in":
                self.views[s.name] = torch.from_numpy(s.data).to(device).contiguous()
            elif s.dtype == I32:
                self.views[s.name] = torch.full(s.shape, SENT32, dtype=I32, device=device)
            else:
                self.views[s.name] = torch.full(s.shape, _SENT64_I, dtype=torch.int64, device=device).view(F64)

    __getitem__ = Arena.__getitem__
    arrays = Arena.arrays
    result = Arena.result
    results = Arena.results
    _sentinel_mask = Arena._sentinel_mask

    def check(self, untouched=()):
        if any(v.is_cuda for v in self.views.values()):
            torch.cuda.synchronize()
        for s in self.specs:
            if s.role == "in":
                assert np.array_equal(self.views[s.name].cpu().numpy().view(np.uint8), s.data.view(np.uint8)), \
                    "input %r changed" % s.name
            else:
                mask = self._sentinel_mask(s).cpu().numpy()
                if s.name in untouched:
                    assert mask.all(), "output %r that the call leaves untouched was written at element %d" % (
                        s.name, int(np.flatnonzero(~mask)[0]))
                else:
                    assert not mask.any(), "output %r not written at element %d" % (s.name, int(np.flatnonzero(mask)[0]))


# ---- the entries --------------------------------------------------------------------------------------------------------------
SOLVE_OUT = ("x", "y", "z", "pobj", "dobj", "status", "iters")
BOUNDED_OUT = ("x", "y", "z", "s", "pobj", "dobj", "status", "iters")
# entry -> (library symbol, handle family or None, arrays in the order of the C arguments, outputs that may be NULL)
ENTRIES = {
    "dense_solve": ("pycllp_hip_dense_solve", "dense", ("b", "c") + SOLVE_OUT, ("y", "z", "pobj", "dobj", "iters")),
    "dense_solve_bounded": ("pycllp_hip_dense_solve_bounded", "dense", ("b", "c", "u") + BOUNDED_OUT,
                            ("y", "z", "s", "pobj", "dobj", "iters")),
    "dense_solve_batch": ("pycllp_hip_dense_solve_batch", "dense", ("A", "b", "c") + SOLVE_OUT,
                          ("y", "z", "pobj", "dobj", "iters")),
    "dense_solve_batch_bounded": ("pycllp_hip_dense_solve_batch_bounded", "dense", ("A", "b", "c", "u") + BOUNDED_OUT,
                                  ("y", "z", "s", "pobj", "dobj", "iters")),
    "dense_newton": ("pycllp_hip_dense_newton", "dense", ("x", "z", "y", "b", "c", "dy", "nrefine"), ("nrefine",)),
    "sparse_solve": ("pycllp_hip_sparse_solve", "sparse", ("b", "c") + SOLVE_OUT, ("y", "z", "pobj", "dobj", "iters")),
    "sparse_solve_batch": ("pycllp_hip_sparse_solve_batch", "sparse", ("A", "b", "c") + SOLVE_OUT,
                           ("y", "z", "pobj", "dobj", "iters")),
    "sparse_solve_bounded": ("pycllp_hip_sparse_solve_bounded", "sparse", ("b", "c", "u") + BOUNDED_OUT,
                             ("y", "z", "s", "pobj", "dobj", "iters")),
    "sparse_solve_batch_bounded": ("pycllp_hip_sparse_solve_batch_bounded", "sparse", ("A", "b", "c", "u") + BOUNDED_OUT,
                                   ("y", "z", "s", "pobj", "dobj", "iters")),
    "sparse_newton": ("pycllp_hip_sparse_newton", "sparse", ("x", "z", "y", "b", "c", "dy", "nrefine"), ("nrefine",)),
    "ldl": ("pycllp_hip_ldl", None, ("A", "L", "D"), ()),
    "ldl_solve": ("pycllp_hip_ldl_solve", None, ("A", "rhs", "x"), ()),
    "forward_backward_ldl": ("pycllp_hip_forward_backward_ldl", None, ("L", "D", "b", "x"), ()),
}
OUTPUTS = {"dense_newton": ("dy", "nrefine"), "sparse_newton": ("dy", "nrefine"), "ldl": ("L", "D"), "ldl_solve": ("x",),
           "forward_backward_ldl": ("x",)}
for _e, (_s, _f, _a, _o) in ENTRIES.items():
    OUTPUTS.setdefault(_e, BOUNDED_OUT if "bounded" in _e else SOLVE_OUT)
I32_ARRAYS = ("status", "iters", "nrefine")


def _ptr(t):
    return ctypes.c_void_p(None if t is None else t.data_ptr())


def call(entry, arrays, B, handle=None, opts=None, stream=None, lib=None, **scalars):
    """One call of ``entry`` on ``arrays`` (name -> tensor or None = NULL; an ``Arena``/``Plain`` ``.arrays()``), queued on
    ``stream`` (None: torch's current stream).  ``scalars``: a_cols (dense_solve_batch*), mu (newton), n, modified, beta, delta
    (LDL entries).  Returns the entry's return code; nothing is synchronised."""
    symbol, family, names, _ = ENTRIES[entry]
    if lib is None:
        from pycllp_amd import _native
        lib = _native.lib()
    if stream is None:
        stream = torch.cuda.current_stream()
    st = ctypes.c_void_p(stream.cuda_stream)
    p = [_ptr(arrays[k]) for k in names]
    fn = getattr(lib, symbol)
    if family is None:
        n = int(scalars["n"])
        if entry == "forward_backward_ldl":
            return fn(n, B, *p, st)
        return fn(n, B, *p, int(scalars["modified"]), float(scalars["beta"]), float(scalars["delta"]), st)
    assert handle is not None and handle.family == family, (entry, handle)
    o = ctypes.byref(opts)
    if entry.endswith("newton"):
        return fn(handle, B, *p[:5], float(scalars["mu"]), *p[5:], o, st)
    if entry.startswith("dense_solve_batch"):
        return fn(handle, B, p[0], ctypes.c_long(int(scalars["a_cols"])), *p[1:], o, st)
    return fn(handle, B, *p, o, st)
