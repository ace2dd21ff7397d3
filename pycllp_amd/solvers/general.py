"""HIP solver plugins for ``GeneralLP``:  optimise c'x + f  s.t.  a <= A x <= b,  l <= x <= u.

The LP is brought into the bounded equality form (``GeneralLP.to_bounded_equality_form``: A^ = [+-A | I], 0 <= x^ <= u^) and
solved on the bounded slack-aware lane-group kernel (``pycllp_hip_dense_solve_bounded``, csrc/ipm_group_slot.inc, BD): one row
per kept row of the LP and no row per upper bound.  What that kernel does not serve -- more than 32 kept rows, more than 96
columns, per-problem values of A -- is solved through the reference's conversion ``to_standard_form().to_equality_form()``
(``pycllp/lp.py:725-792``) on ``HipDensePrimalNormalSolver`` and mapped back the same way, so the plugin takes every LP the
library takes.  ``kernel`` tells which path served the last ``solve``: ``'bounded group'`` or ``'expanded'``.

``hip_sparse_general_primal_normal`` is the same plugin on the bounded one-LP-per-wavefront kernel
(``pycllp_hip_sparse_solve_bounded``, csrc/ipm_wreg_bounded.inc): any shared A^ with m' <= 128 kept rows and N <= 512 columns
that a variant of that kernel covers (``kernel == 'bounded wave'``), sparse or dense, the expansion for the rest.

On the native path the batch is converted ON THE DEVICE (``DeviceConversion``: ``pycllp_hip_general_to_bounded`` before the solve,
``pycllp_hip_general_from_bounded`` behind it, csrc/general_form.hip): the host only classifies the rows
(``GeneralLP.bounded_structure``), ``solve(lp)`` uploads a, b, c, l, u and downloads results of the original size, and
``solve_device`` is the same chain on tensors, in the ORIGINAL variables.  Batches with per-problem values of A
(``PerProblemBounded``, the mix-in of ``general_batch`` and ``sparse_general_batch``) go the same way through
``BatchDeviceConversion`` (``pycllp_hip_general_to_bounded_batch``, the same unit), which also writes every LP's matrix in the
layout its solve entry takes; there the chain on tensors is ``solve_device_general``.  Both go through one text,
``_solve_on_device`` and ``_solve_native`` of the shared-A plugin; a plugin states how it launches (``_launch_converted``).
"""
import contextlib
import ctypes
import types

import numpy as np
import torch

from . import BaseGeneralSolver
from .. import _native
from ..lp import GeneralLP, SparseMatrix, bounded_rowmap
from .hip import (DeviceArrays, Handle, HipDensePrimalNormalSolver, _require_gpu, autoscale_wanted, bounded_outputs,
                  plugin_options, solve_opts)

NATIVE_MAX_ROWS, NATIVE_MAX_COLS = 32, 96      # the slack-aware kernels: m' <= 32 rows, n <= 96 original columns
WAVE_MAX_ROWS, WAVE_MAX_COLS = 128, 512        # the bounded wave kernel: m' <= 128 rows, N <= 512 columns of A^
_REJECTED = (_native.FLAG_HSD | _native.FLAG_PREDCORR | _native.FLAG_WARM_START | _native.FLAG_WAVE_KERNEL
             | _native.FLAG_NO_SLACK_PATH)
RESULTS = ("x", "y", "z", "s", "status", "iters", "primal_obj", "dual_obj")


def as_general(lp):
    """This package's ``GeneralLP`` for ``lp`` (duck-typed on ``A, a, b, c, l, u, f``: a reference GeneralLP works too)."""
    if isinstance(lp, GeneralLP):
        return lp
    A = lp.A if isinstance(lp.A, SparseMatrix) else SparseMatrix(matrix=np.asarray(lp.A.todense(), dtype=np.float64))
    return GeneralLP(A, lp.b, lp.c, a=getattr(lp, "a", None), l=getattr(lp, "l", None), u=getattr(lp, "u", None),
                     f=getattr(lp, "f", 0.0))


def subset(glp, idx):
    """The GeneralLP of the problems ``idx`` of ``glp``."""
    A = glp.A
    data = A.data[idx] if A.nproblems > 1 else A.data
    A2 = SparseMatrix(A._rows.copy(), A._cols.copy(), data.copy())
    A2._shape = (glp.nrows, glp.ncols)
    return GeneralLP(A2, glp.b[idx], glp.c[idx], a=glp.a[idx], l=glp.l[idx], u=glp.u[idx], f=glp.f[idx])


def download_bounded(out, blp, bmap, device):
    """The tail of a bounded solve: waits for ``device``, downloads ``out`` (``bounded_outputs``) and maps it back to the
    GeneralLP's variables with ``bmap``; the objectives get the bounded form's ``f``."""
    torch.cuda.synchronize(device)
    r = {k: v.cpu().numpy() for k, v in out.items()}
    xo, yo, zo, so = bmap.general(r["x"], r["y"], r["z"], r["s"])
    f = np.broadcast_to(blp.f, (blp.nproblems,))
    return dict(x=xo, y=yo, z=zo, s=so, status=r["status"], iters=r["iters"], primal_obj=r["pobj"] + f, dual_obj=r["dobj"] + f)


class DeviceConversion(object):
    """The plan of ``GeneralLP.bounded_structure()`` on ``device`` -- the row map and the CSR of the ORIGINAL shared A, terms in
    the order of its coordinate lists -- and the two entries that work by it.  The calls take contiguous float64 CUDA tensors
    and the stream to queue on (None: torch's current stream on ``device``); nothing is synchronised."""
    per_problem = False       # to_bounded takes no Adata in front of a

    def __init__(self, glp, keep, sign, device):
        self.m, self.n, self.mk, self.device = glp.nrows, glp.ncols, len(keep), device
        data, indptr, indices = glp.A.csr_term_order()
        self.nnz = int(data.size)
        self.rowmap, self.data, self.indptr, self.indices = (
            torch.as_tensor(v, device=device) for v in (bounded_rowmap(keep, sign, self.m), data, indptr, indices))

    def _call(self, name, stream, sizes, arrays):
        st = ctypes.c_void_p((stream if stream is not None else torch.cuda.current_stream(self.device)).cuda_stream)
        args = [ctypes.c_void_p(a.data_ptr()) if isinstance(a, torch.Tensor) else a for a in arrays]     # (None: NULL)
        with torch.cuda.device(self.device):
            _native.check(getattr(_native.lib(), name)(*sizes, *args, st), name)

    def _matrix(self, Adata, new, B):
        """(the entry that converts, its matrix arguments between ``nnz`` and ``a``, its matrix outputs in front of b^ by key)."""
        return "pycllp_hip_general_to_bounded", (self.data, self.indptr, self.indices), {}

    def to_bounded(self, stream, a, b, c, l, u, f=None, Adata=None):
        """a, b [B, m], c, l, u [B, n], f [B] (l, f: None = 0) -> dict b [B, m'], c, u [B, N], f [B], invalid [B] (i32)."""
        B, N = int(a.shape[0]), self.n + self.mk
        new = lambda *shape: torch.empty(shape, dtype=torch.float64, device=self.device)     # noqa: E731
        entry, matrix, outputs = self._matrix(Adata, new, B)
        cv = dict(outputs, b=new(B, self.mk), c=new(B, N), u=new(B, N), f=new(B),
                  invalid=torch.empty(B, dtype=torch.int32, device=self.device))
        if B:
            self._call(entry, stream, (self.m, self.n, self.mk, B),
                       (self.rowmap, self.nnz, *matrix, a, b, c, l, u, f, *cv.values()))     # (cv: in the entries' order)
        return cv

    def from_bounded(self, stream, l, f, invalid, out):
        """The outputs ``out`` of a bounded solve (``bounded_outputs``) -> dict of ``RESULTS`` in the GeneralLP's variables plus
        ``invalid``; ``primal_obj``, ``dual_obj``, ``status`` and ``iters`` are ``out``'s own tensors, updated in place."""
        B = int(out["x"].shape[0])
        new = lambda cols: torch.empty((B, cols), dtype=torch.float64, device=self.device)     # noqa: E731
        res = dict(x=new(self.n), y=new(self.m), z=new(self.n), s=new(self.n), status=out["status"], iters=out["iters"],
                   primal_obj=out["pobj"], dual_obj=out["dobj"], invalid=invalid)
        if B:
            self._call("pycllp_hip_general_from_bounded", stream, (self.m, self.n, self.mk, B),
                       (self.rowmap, l, f, invalid, out["x"], out["y"], out["z"], out["s"], res["x"], res["y"], res["z"],
                        res["s"], out["pobj"], out["dobj"], out["status"], out["iters"]))
        return res


class BatchDeviceConversion(DeviceConversion):
    """``DeviceConversion`` for per-problem values of A: the row map, the structure's CSR in term order, the position of its
    terms in the coordinate lists (``SparseMatrix.term_order``) and the gather plan ``gather`` of one LP's matrix output
    (``lp.bounded_gather_dense`` / ``lp.bounded_gather_csr``) on ``device``; ``to_bounded`` takes the values ``[B, nnz]`` in the
    order of the coordinate lists, as ``glp.A.data`` holds them."""
    per_problem = True

    def __init__(self, glp, keep, sign, device, gather):
        super(BatchDeviceConversion, self).__init__(glp, keep, sign, device)
        self.data = None                                      # (no shared values)
        self.out_len = int(gather.size)
        self.order = torch.as_tensor(glp.A.term_order().astype(np.int32), device=device)
        self.gather = torch.as_tensor(np.ascontiguousarray(gather, dtype=np.int32), device=device)

    def _matrix(self, Adata, new, B):
        return ("pycllp_hip_general_to_bounded_batch",
                (self.order, self.indptr, self.indices, Adata, ctypes.c_long(self.out_len), self.gather), dict(A=new(B, self.out_len)))

    def to_bounded(self, stream, Adata, a, b, c, l, u, f=None):
        """Adata [B, nnz], a, b [B, m], c, l, u [B, n], f [B] (l, f: None = 0) -> dict A [B, out_len], b [B, m'], c, u [B, N],
        f [B], invalid [B] (i32)."""
        return super(BatchDeviceConversion, self).to_bounded(stream, a, b, c, l, u, f, Adata)


class HipGeneralPrimalNormalSolver(DeviceArrays, BaseGeneralSolver):
    """``glp.init(s); glp.solve(s)`` on a ``GeneralLP``; results in the ORIGINAL variables: ``x [B, n]``, ``y [B, m]`` (one
    per row of the LP, 0 for a row without bounds), ``z`` / ``s [B, n]`` (duals of x >= l / x <= u), ``status``, ``iters``,
    ``primal_obj``, ``dual_obj`` (f and c'l included)."""
    name = 'hip_general_primal_normal'
    _rejected = _REJECTED
    _rejected_names = "HSD, PREDCORR, WARM_START, WAVE_KERNEL and NO_SLACK_PATH"
    _native_kernel = "bounded group"
    _hsd_entry = True         # the handle has ``solve_bounded_hsd``: solve_device(..., hsd=True) is available
    _hsd_spellings = ("native", "device")      # the values of ``hsd`` that ask for the embedding on this plugin's own kernel
    hsd_device = False        # (``hip_general_batch_primal_normal``'s own option: the same re-solve on per-problem matrices)
    _device_resolved = False  # the last native solve's non-optimal LPs were solved again on the device
    _hsd_refused = None       # the handle whose embedding entry answered PYCLLP_E_UNSUPPORTED: not asked again, nothing gathered

    def __init__(self, device=None, stream=None, autoscale="auto", hsd="auto", predcorr=False, warm_start=False, **options):
        """``hsd='auto'`` (default): the LPs that do not end optimal on the bounded kernel are solved again through the
        expansion on ``HipDensePrimalNormalSolver`` (whose own ``hsd='auto'`` gives infeasible / unbounded LPs the certified
        statuses 2 / 4); ``hsd=False``: the bounded kernel's verdict stands.  ``hsd='native'``
        (``hip_general_primal_normal`` alone): as 'auto', but the LPs that do not end optimal on the bounded kernel are solved
        again ON THE DEVICE, on the bounded kernel's self-dual embedding (``pycllp_hip_dense_solve_bounded_hsd``) with the same
        handle -- no expansion, no second solver, no host conversion; an LP outside the native range (``kernel == 'expanded'``)
        behaves as under 'auto'.  A status-2 LP then carries its certificate in ``y, z, s``, a status-4 LP has ``x = l +`` the
        ray (as ``solve_expanded`` returns it).  ``hsd='device'`` (both shared-A plugins): the same re-solve on the device, on
        the embedding of whichever bounded kernel the plugin runs -- on ``hip_general_primal_normal`` a synonym of 'native', on
        ``hip_sparse_general_primal_normal`` the wave kernel's (``pycllp_hip_sparse_solve_bounded_hsd``), where what the
        embedding returns stands: no expansion at any size.  ``hsd=True``, ``predcorr=True`` and
        ``warm_start=True`` are not available with bounds.  ``autoscale``: as ``HipDensePrimalNormalSolver`` (the 'auto' band
        rule also looks at the finite upper bounds).  Other keyword arguments are fields of ``pycllp_hip_opts``."""
        if not isinstance(hsd, str) and hsd:
            raise ValueError("hsd must be 'auto', False, (the shared-A plugins) 'device' or (hip_general_primal_normal) 'native' "
                             "for %s: the embedding with bounds serves the LPs that do not end optimal, or "
                             "solve_device(..., hsd=True)" % self.name)
        self.hsd_native = isinstance(hsd, str) and hsd in ("native", "device")
        if self.hsd_native:
            if hsd not in self._hsd_spellings:      # (a check of its own: 'native' stays the lane-group plugin's spelling)
                raise ValueError("hsd=%r is not available for %s%s" % (hsd, self.name, " (its kernel has no self-dual embedding)"
                                 if not self._hsd_spellings else ": its spelling there is hsd='device'"))
            hsd = "auto"          # (what the expansion and every other path see)
        if predcorr:
            raise ValueError("predcorr is not available with upper bounds")
        if warm_start:
            raise ValueError("warm_start is not available with upper bounds")
        if int(options.get("flags", 0)) & self._rejected:
            raise ValueError("flags %s are not available with upper bounds" % self._rejected_names)
        self.hsd, self.autoscale, _, _, self.options = plugin_options(options, hsd, autoscale)
        self.device, self.stream = device, stream
        self._handle = None
        self._key = None
        self._conv = None
        self._keepalive = None
        self.kernel = None

    @staticmethod
    def native_fits(glp, blp):
        """``blp``: the bounded form, or its matrix alone (``GeneralLP.bounded_structure``)."""
        return glp.A.nproblems == 1 and 1 <= blp.nrows <= NATIVE_MAX_ROWS and glp.ncols <= NATIVE_MAX_COLS

    @staticmethod
    def _bounded_matrix(Ah):
        """(A^ as the handle of the native kernel takes it -- dense --, a key that tells whether A^ changed)."""
        A = np.ascontiguousarray(Ah.todense(), dtype=np.float64)
        return A, (A.shape, A.tobytes())

    def _ensure_handle(self, glp, Ah, keep, sign):
        """A handle for A^ and the device conversion's plan beside it (both re-made when A, or which rows are kept with which
        sign, changed since the last ones); False if the library declines A^."""
        A, key = self._bounded_matrix(Ah)
        key = (key, keep.tobytes(), sign.tobytes(), glp.A._rows.tobytes(), glp.A._cols.tobytes(), glp.A.data.tobytes())
        if self._handle is not None and self._key == key:
            return True
        self._handle = self._key = self._conv = None
        try:
            self._handle = Handle(A, self.device, self.stream)
        except NotImplementedError:
            return False
        self._conv = DeviceConversion(glp, keep, sign, self.device)
        self._key = key
        return True

    def _on_stream(self):
        """Context in which torch's own work (allocations, the band test) is queued on the stream the entries are given."""
        return torch.cuda.stream(self.stream) if self.stream is not None else contextlib.nullcontext()

    # -- plugin API ------------------------------------------------------------------------------
    def init(self, lp, verbose=0):
        self.device = _require_gpu(self.device)
        glp = as_general(lp)
        glp.check_bounds()
        Ah, keep, sign = glp.bounded_structure()
        if not (self.native_fits(glp, Ah) and self._ensure_handle(glp, Ah, keep, sign)):
            self._handle = self._key = self._conv = None
        self.m, self.n = glp.nrows, glp.ncols

    def solve_device(self, a, b, c, l, u, f=None, hsd=False, **options):
        """Device-resident entry, in the ORIGINAL variables: a, b [B, m], c, l, u [B, n], f [B] (torch CUDA tensors, or numpy
        arrays, which are uploaded; ``l`` and ``f`` may be None = 0) -> dict of CUDA tensors: ``RESULTS`` and ``invalid`` (i32
        [B]: 0, or the check of ``pycllp_hip_general_to_bounded`` the LP failed; such an LP has status 3 and NaN results).
        Conversion, bounded solve and back-conversion are queued on the solver's stream and nothing waits for them; the kernel's
        verdict stands (no look at the data: ``autoscale='auto'``, ``hsd='auto'``, ``hsd='native'`` and ``hsd='device'`` count as
        off).  ``hsd=True`` (the two shared-A plugins): the whole batch runs on the bounded kernel's self-dual embedding
        (``pycllp_hip_dense_solve_bounded_hsd`` / ``pycllp_hip_sparse_solve_bounded_hsd``) in one launch, still without a sync:
        statuses 2 / 4 are certified and come
        with their certificate (``y, z, s`` / ``x = l +`` the ray).  ``options``: fields of ``pycllp_hip_opts`` for this call."""
        if self._handle is None or self._conv is None:
            raise RuntimeError("solve_device() needs init() on an LP the %s kernel serves (after init() the LP takes the "
                               "expansion)" % self._native_kernel)
        if hsd and not self._hsd_entry:
            raise ValueError("hsd=True is not available for %s (its kernel has no self-dual embedding)" % self.name)
        return self._solve_on_device(None, a, b, c, l, u, f, options, hsd=bool(hsd))

    def _solve_on_device(self, Adata, a, b, c, l, u, f, options, hsd=False):
        """The device-resident chain of ``solve_device`` (``Adata`` None) and ``solve_device_general``: upload what is numpy,
        check the shapes against the conversion's plan, convert, launch (``_launch_converted``), convert back; the inputs and
        everything between stay alive until the next call."""
        cv = self._conv
        with self._on_stream():
            mat = () if Adata is None else (self._dev(Adata),)
            a, b, c, u = (self._dev(v) for v in (a, b, c, u))
            l, f = (None if v is None else self._dev(v) for v in (l, f))
            B = int(a.shape[0]) if a.dim() == 2 else -1
            if (any(tuple(v.shape) != (B, cv.nnz) for v in mat) or tuple(a.shape) != (B, cv.m) or tuple(b.shape) != (B, cv.m)
                    or any(tuple(v.shape) != (B, cv.n) for v in (c, u)) or (l is not None and tuple(l.shape) != (B, cv.n))
                    or (f is not None and tuple(f.shape) != (B,))):
                raise ValueError(("Adata must be [B,%d], a and b " % cv.nnz if mat else "a and b must be ")
                                 + "[B,%d], c, l and u [B,%d] and f [B] with equal B" % (cv.m, cv.n))
            bl = cv.to_bounded(self.stream, *mat, a, b, c, l, u, f)
            out = self._launch_converted(bl, B, 0, options, **(dict(hsd=True) if hsd else {}))
            res = cv.from_bounded(self.stream, l, bl["f"], bl["invalid"], out)
        self._keepalive = mat + (a, b, c, l, u, f, bl, out)
        self.kernel = self._native_kernel
        return res

    def _launch_converted(self, bl, B, extra_flags, overrides, hsd=False):
        """The bounded solve of the B LPs that ``to_bounded`` left in ``bl``, queued on the solver's stream -> its outputs
        (``bounded_outputs``); ``hsd``: on the self-dual embedding.  ``NotImplementedError`` where the library declines."""
        cv = self._conv
        o = solve_opts(self.options, extra_flags, **overrides)
        out = bounded_outputs(B, cv.mk, cv.n + cv.mk, self.device)
        if B:
            (self._handle.solve_bounded_hsd if hsd else self._handle.solve_bounded)(self.stream, bl["b"], bl["c"], bl["u"], out, o)
        return out

    def _resolve_native(self, bl, out, extra_flags):
        """hsd='native' / 'device' (and ``hsd_device`` of the batch plugin): the LPs of ``out`` that did not end optimal, solved
        again on the embedding with the same handle -- their b^, c^, u^ (and, with per-problem values, their matrices A^)
        gathered on the device, the results scattered into ``out``.  (The one look at the statuses waits for the first
        launch.)  False where the library declines the embedding for this handle: the answer is the handle's, so it is asked
        once."""
        if self._hsd_refused is not None and self._hsd_refused is self._handle:
            return False
        idx = torch.nonzero(out["status"] != 0).reshape(-1)
        if idx.numel() == 0:
            return True
        sub = {k: bl[k].index_select(0, idx).contiguous() for k in ("A", "b", "c", "u") if k in bl}
        try:
            again = self._launch_converted(sub, int(idx.numel()), extra_flags, {}, hsd=True)
        except NotImplementedError:
            self._hsd_refused = self._handle
            return False                            # (no kernel of this shape: the bounded kernel's verdict stands)
        for k, v in again.items():
            out[k].index_copy_(0, idx, v)
        return True

    def solve(self, lp, verbose=0):
        glp = as_general(lp)
        if glp.nrows != self.m or glp.ncols != self.n:
            raise ValueError("LP shape changed since init(): (%d,%d) vs (%d,%d)" % (glp.nrows, glp.ncols, self.m, self.n))
        glp.check_bounds()
        Ah, keep, sign = glp.bounded_structure()
        res = None
        if self.native_fits(glp, Ah) and self._ensure_handle(glp, Ah, keep, sign):
            res = self._solve_native(glp)
        if res is None:
            self.kernel = "expanded"
            return self._finish(glp, self.solve_expanded(glp), redo=False)
        self.kernel = self._native_kernel
        return self._finish(glp, res)

    def _finish(self, glp, res, redo=True):
        """The tail of ``solve``: with ``hsd='auto'`` the LPs of a native solve that did not end optimal are solved again
        (``_redo`` picks them, ``_solve_again`` solves them), then ``res`` becomes the result attributes."""
        # (hsd='native' / 'device', and hsd_device where the embedding served: done on the device, in _solve_native)
        if redo and self.hsd == "auto" and not self.hsd_native and not (self.hsd_device and self._device_resolved):
            idx = self._redo(glp, np.flatnonzero(res["status"] != 0))
            r2 = self._solve_again(subset(glp, idx)) if idx.size else None
            if r2 is not None:
                for k in RESULTS:
                    res[k][idx] = r2[k]
        for k in RESULTS:
            setattr(self, k, res[k])
        return self.status

    def _redo(self, glp, idx):
        """The LPs among ``idx`` (not optimal on the native kernel) that ``hsd='auto'`` solves again through the expansion."""
        return idx

    def _solve_again(self, glp):
        """``solve_expanded`` for the LPs that ``hsd='auto'`` solves again; None: the kernel's status stands."""
        return self.solve_expanded(glp)

    def launch_info(self):
        """``Handle.launch_info()`` of the native kernel's last launch (None when no handle serves the LP)."""
        return None if self._handle is None else self._handle.launch_info()

    def _solve_native(self, glp):
        """One upload of a, b, c, l, u (and of A.data as it is, where the conversion takes per-problem values); conversion,
        bounded kernel and back-conversion on the device; one download of the results in the GeneralLP's variables.  None if the
        library declines A^ or the handle (PYCLLP_E_UNSUPPORTED).  ``autoscale='auto'`` is decided from the device's b^, c^, u^
        (``autoscale_wanted``: a comparison of maxima, the answer the host's arrays give); the objectives' offset f + c'l is the
        host's sum, so every result carries the bits of the host conversion."""
        cv, B = self._conv, glp.nproblems
        offset = np.broadcast_to(glp.f, (B,)) + (glp.c * glp.l).sum(axis=1)
        host = ((glp.A.data,) if cv.per_problem else ()) + (glp.a, glp.b, glp.c, glp.l, glp.u, offset)
        with self._on_stream():
            *args, fh = (self._dev(np.ascontiguousarray(v)) for v in host)
            bl = cv.to_bounded(self.stream, *args)
            wanted = self.autoscale == "auto" and autoscale_wanted(bl["b"], bl["c"], bl["u"])
            try:
                out = self._launch_converted(bl, B, _native.FLAG_AUTOSCALE if wanted else 0, {})
            except NotImplementedError:
                return None
            self._device_resolved = False
            if self.hsd_native or self.hsd_device:
                self._device_resolved = self._resolve_native(bl, out, _native.FLAG_AUTOSCALE if wanted else 0)
            res = cv.from_bounded(self.stream, args[-2], fh, bl["invalid"], out)      # (args[-2]: l)
            torch.cuda.synchronize(self.device)
            return {k: res[k].cpu().numpy() for k in RESULTS}

    def solve_expanded(self, glp):
        """Solve ``glp`` through ``to_standard_form().to_equality_form()`` on ``HipDensePrimalNormalSolver`` and map the results
        back to the GeneralLP's variables.  The expansion needs every bound finite for all LPs or for none; a batch that mixes
        them (u = +inf for some LPs only) is solved in groups of equal pattern."""
        B, m, n = glp.nproblems, glp.nrows, glp.ncols
        out = dict(x=np.zeros((B, n)), y=np.zeros((B, m)), z=np.zeros((B, n)), s=np.zeros((B, n)),
                   status=np.zeros(B, dtype=np.int32), iters=np.zeros(B, dtype=np.int32),
                   primal_obj=np.zeros(B), dual_obj=np.zeros(B))
        pattern = np.concatenate([np.isfinite(glp.a), np.isfinite(glp.b), np.isfinite(glp.u)], axis=1)
        _, group = np.unique(pattern, axis=0, return_inverse=True)
        for gi in np.unique(group):
            idx = np.flatnonzero(group.reshape(-1) == gi)
            g = glp if idx.size == B else subset(glp, idx)
            keep_lo = np.isfinite(g.a).any(axis=0)
            keep_hi = np.isfinite(g.b).any(axis=0)
            keep_ub = np.isfinite(g.u).any(axis=0)
            eq = g.to_standard_form().to_equality_form()
            solver = HipDensePrimalNormalSolver(device=self.device, stream=self.stream, autoscale=self.autoscale, hsd=self.hsd,
                                                **self.options)
            eq.init(solver)
            eq.solve(solver)
            nlo, nhi = int(keep_lo.sum()), int(keep_hi.sum())
            ye = np.asarray(solver.y)
            y = np.zeros((idx.size, m))
            y[:, keep_lo] -= ye[:, :nlo]
            y[:, keep_hi] += ye[:, nlo:nlo + nhi]
            s = np.zeros((idx.size, n))
            s[:, keep_ub] = ye[:, nlo + nhi:nlo + nhi + int(keep_ub.sum())]
            out["x"][idx] = g.l + np.asarray(solver.x)[:, :n]
            out["y"][idx] = y
            out["z"][idx] = np.asarray(solver.z)[:, :n]
            out["s"][idx] = s
            out["status"][idx] = solver.status
            out["iters"][idx] = solver.iters
            out["primal_obj"][idx] = solver.primal_obj
            out["dual_obj"][idx] = solver.dual_obj
        return out


def expansion_rows(glp):
    """Rows of ``glp.to_standard_form().to_equality_form()`` for the batch: one per finite lower and upper row bound and per
    finite upper column bound in any of its LPs (what ``solve_expanded`` hands to ``HipDensePrimalNormalSolver``)."""
    return int(np.isfinite(glp.a).any(axis=0).sum() + np.isfinite(glp.b).any(axis=0).sum()
               + np.isfinite(glp.u).any(axis=0).sum())


class HipSparseGeneralPrimalNormalSolver(HipGeneralPrimalNormalSolver):
    """``hip_general_primal_normal`` on the bounded one-LP-per-wavefront kernel (``pycllp_hip_sparse_solve_bounded``): the same
    contract, options and results, for bounded forms of up to 128 kept rows and 512 columns, sparse or dense.  ``kernel`` is
    ``'bounded wave'`` or ``'expanded'`` (per-problem values of A, a bounded form no variant of the kernel covers).  With
    ``hsd='auto'`` the LPs that do not end optimal -- NUMERICAL included -- are solved again through the expansion where it
    fits the library (``pycllp_hip_dense_max_rows()`` / ``_max_cols()``); elsewhere the wave kernel's status stands.  With
    ``hsd='device'`` they are solved again on the wave kernel's own self-dual embedding (``pycllp_hip_sparse_solve_bounded_hsd``,
    DESIGN.md section 27) with the same handle, at every size the kernel serves, and what the embedding returns stands;
    ``solve_device(..., hsd=True)`` runs the whole batch there.  ``hsd='native'`` stays the lane-group plugin's spelling."""
    name = 'hip_sparse_general_primal_normal'
    _rejected = _REJECTED | _native.FLAG_BLOCK_KERNEL | _native.FLAG_FORCE_GUARD_PATH | _native.FLAG_EXACT_NORMS | \
        _native.FLAG_PER_LP_FIRST_GRAM
    _rejected_names = "HSD, PREDCORR, WARM_START, WAVE_KERNEL, BLOCK_KERNEL, NO_SLACK_PATH and FORCE_GUARD_PATH"
    _native_kernel = "bounded wave"
    _hsd_entry = True
    _hsd_spellings = ("device",)

    @staticmethod
    def native_fits(glp, blp):
        return glp.A.nproblems == 1 and 1 <= blp.nrows <= WAVE_MAX_ROWS and blp.ncols <= WAVE_MAX_COLS

    @staticmethod
    def _bounded_matrix(Ah):
        A = Ah.tocsr()
        A.sum_duplicates(); A.eliminate_zeros(); A.sort_indices()
        return A, (A.shape, A.data.tobytes(), A.indptr.tobytes(), A.indices.tobytes())

    def _redo(self, glp, idx):
        if idx.size:
            L, rows = _native.lib(), expansion_rows(subset(glp, idx))
            if rows > L.pycllp_hip_dense_max_rows() or glp.ncols + rows > L.pycllp_hip_dense_max_cols():
                return idx[:0]
        return idx


class PerProblemBounded(object):
    """Mix-in in front of one of the two plugins above, for batches with per-problem values of A on a bounded kernel that takes
    them: ``init`` makes the handle from the bounded form (or, where the kernel does not serve it, a delegate: the plugin
    behind the mix-in, with the same options, whose ``kernel`` and results are reported unchanged), ``solve_device`` and
    ``solve`` launch the one entry.  A subclass states ``_delegate_class``, ``native_fits``, ``_make_handle(blp)`` (the
    ``Handle`` of the bounded form; ``NotImplementedError`` where the library declines it), ``_values(blp)`` (the per-problem
    array as the entry takes it, numpy), ``_values_spec(B)`` (the shape that array must have, and the text that says so),
    ``_call(A, b, c, u, out, o)`` (the ``Handle`` call; ``_call_hsd`` where ``_hsd_entry``: the same on the self-dual embedding), ``_gather(glp, keep, sign)`` (the plan of that array as a gather
    from one LP's values, ``lp.bounded_gather_*``; None where it is none) and ``_needs`` (what ``solve_device`` asks of
    ``init``); ``_unchanged``, ``_solve_delegate`` and ``_solve_again`` where it differs.

    The batch is converted ON THE DEVICE (``BatchDeviceConversion``): ``init`` reads the batch-wide structure and LP 0's values
    only, ``solve(lp)`` uploads ``A.data, a, b, c, l, u`` as they are and downloads results of the original size, and
    ``solve_device_general`` is the same chain on tensors.  ``conversion`` says which conversion serves ``solve``: ``'device'``,
    or ``'host'`` (``GeneralLP.to_bounded_equality_form`` and ``_values``) for a structure without a plan; None with a delegate."""
    _changed_what = "%d kept rows (%d at init), %d matrices"
    _hsd_entry = False
    _hsd_spellings = ()

    def __init__(self, *args, **kwargs):
        super(PerProblemBounded, self).__init__(*args, **kwargs)
        self._delegate = None
        self._keepalive = None
        self.mk = None
        self._conv_key = None
        self.conversion = None

    @staticmethod
    def _form(glp):
        """(the shape of the bounded form with LP 0's matrix -- ``A, nrows, ncols``: what ``native_fits``, ``_make_handle`` and
        ``_unchanged`` read of a bounded LP --, keep, sign), from ``check_bounds`` and ``bounded_structure`` alone: the
        ``ValueError``s of ``to_bounded_equality_form`` in their order, no product with l and no ``[B, nnz]`` copy."""
        glp.check_bounds()
        Ah, keep, sign = glp.bounded_structure(problem=0)
        return types.SimpleNamespace(A=Ah, nrows=Ah.nrows, ncols=Ah.ncols), keep, sign

    def _ensure_conversion(self, glp, keep, sign):
        """The device conversion for the structure of ``glp`` and these kept rows and signs: re-made when one of them changed
        since the last one; None where the structure has no gather plan."""
        key = (keep.tobytes(), np.asarray(sign).tobytes(), glp.A._rows.tobytes(), glp.A._cols.tobytes())
        if self._conv_key != key:
            gather = self._gather(glp, keep, sign)
            self._conv = None if gather is None else BatchDeviceConversion(glp, keep, sign, self.device, gather)
            self._conv_key = key
        self.conversion = "host" if self._conv is None else "device"
        return self._conv

    def _make_delegate(self, glp):
        self._handle = None
        self._delegate = self._delegate_class(device=self.device, stream=self.stream, autoscale=self.autoscale, hsd=self.hsd,
                                              **self.options)
        self._delegate.init(glp)

    # -- plugin API ------------------------------------------------------------------------------
    def init(self, lp, verbose=0):
        """Fixes the shape of the bounded form (m' kept rows, N = n + m' columns) and makes the handle from it."""
        self.device = _require_gpu(self.device)
        glp = as_general(lp)
        blp, keep, sign = self._form(glp)
        self.m, self.n, self.mk = glp.nrows, glp.ncols, blp.nrows
        self._handle = self._delegate = self._keepalive = self._conv = self._conv_key = self.conversion = None
        if self.native_fits(glp, blp):
            try:
                self._handle = self._make_handle(blp)
            except NotImplementedError:
                pass
        if self._handle is None:
            self._make_delegate(glp)
        else:
            self._ensure_conversion(glp, keep, sign)

    def solve_device(self, A_dev, b_dev, c_dev, u_dev, hsd=False, **options):
        """Device-resident entry, in the bounded form's variables: the per-problem array (``_values_spec``; the subclass says
        how to make it), b [B, m'], c and u [B, N] (torch CUDA tensors or numpy) -> dict of CUDA tensors (``BOUNDED_RESULTS``).
        Asynchronous on the solver's stream; the kernel's verdict stands (no look at the data: ``autoscale='auto'`` and
        ``hsd='auto'`` count as off).  ``hsd=True`` (``hip_general_batch_primal_normal``): the whole batch runs on the kernel's
        self-dual embedding (``_call_hsd``) in one launch, still without a sync; ``ValueError`` on a plugin without one."""
        self._check_hsd(hsd)
        if self._handle is None:
            raise RuntimeError("solve_device() needs init() on an LP the %s" % self._needs)
        return self._launch(self._dev(A_dev), self._dev(b_dev), self._dev(c_dev), self._dev(u_dev), 0, options, hsd=bool(hsd))

    def _check_hsd(self, hsd):
        if hsd and not self._hsd_entry:
            raise ValueError("hsd=True is not available for %s (its kernel has no self-dual embedding)" % self.name)

    def solve_device_general(self, Adata, a, b, c, l, u, f=None, hsd=False, **options):
        """Device-resident entry, in the ORIGINAL variables: Adata [B, nnz] (every LP's values in the order of the coordinate
        lists given to ``init``), a, b [B, m], c, l, u [B, n], f [B] (torch CUDA tensors, or numpy arrays, which are uploaded;
        ``l`` and ``f`` may be None = 0) -> dict of CUDA tensors: ``RESULTS`` and ``invalid`` (i32 [B]: 0, or the check of
        ``pycllp_hip_general_to_bounded_batch`` the LP failed; such an LP has status 3 and NaN results).  Conversion, bounded
        solve and back-conversion are queued on the solver's stream and nothing waits for them; the kernel's verdict stands (no
        look at the data: ``autoscale='auto'`` and ``hsd='auto'`` count as off).  ``hsd=True``: as ``solve_device``'s, with the
        certificates in the GeneralLP's variables (``y, z, s`` / ``x = l +`` the ray).  ``options``: fields of
        ``pycllp_hip_opts`` for this call."""
        self._check_hsd(hsd)
        if self._handle is None or self._conv is None:
            raise RuntimeError("solve_device_general() needs init() on an LP the %s" % self._needs)
        return self._solve_on_device(Adata, a, b, c, l, u, f, options, hsd=bool(hsd))

    def _launch_converted(self, bl, B, extra_flags, overrides, hsd=False):
        return self._launch(bl["A"].view(self._values_spec(B)[0]), bl["b"], bl["c"], bl["u"], extra_flags, overrides, hsd=hsd)

    def _launch(self, A, b, c, u, extra_flags, overrides, hsd=False):
        B, mk, N = int(b.shape[0]), self.mk, self.n + self.mk
        a_shape, a_text = self._values_spec(B)
        if (b.dim() != 2 or b.shape[1] != mk or tuple(c.shape) != (B, N) or tuple(u.shape) != (B, N)
                or tuple(A.shape) != a_shape):
            raise ValueError("%s, b [B,%d], c and u [B,%d] with equal B; got %r, %r, %r and %r"
                             % (a_text, mk, N, tuple(A.shape), tuple(b.shape), tuple(c.shape), tuple(u.shape)))
        out = bounded_outputs(B, mk, N, self.device)
        o = solve_opts(self.options, extra_flags, **overrides)
        if B:                                   # (an empty tensor has no address to hand over; the entry launches nothing for B = 0)
            (self._call_hsd if hsd else self._call)(A, b, c, u, out, o)
        self._keepalive = (A, b, c, u)
        self.kernel = self._native_kernel
        return out

    def _unchanged(self, glp, blp):
        return self.native_fits(glp, blp) and blp.nrows == self.mk

    def _solve_delegate(self, glp, verbose):
        self._delegate.solve(glp, verbose=verbose)
        self.kernel = self._delegate.kernel

    def solve(self, lp, verbose=0):
        if self._delegate is None and self._handle is None:
            raise RuntimeError("solve() called before init()")
        glp = as_general(lp)
        if glp.nrows != self.m or glp.ncols != self.n:
            raise ValueError("LP shape changed since init(): (%d,%d) vs (%d,%d)" % (glp.nrows, glp.ncols, self.m, self.n))
        res = None
        self._device_resolved = False
        if self._delegate is None:
            form, keep, sign = self._form(glp)
            if not self._unchanged(glp, form):
                raise ValueError("the bounded form changed since init(): " + self._changed_what
                                 % (form.nrows, self.mk, glp.A.nproblems))
            if self._ensure_conversion(glp, keep, sign) is not None:
                res = self._solve_native(glp)
            else:
                res = self._solve_bounded(*glp.to_bounded_equality_form())
            if res is None:                     # the entry answers PYCLLP_E_UNSUPPORTED
                self._make_delegate(glp)
        if res is None:
            self._solve_delegate(glp, verbose)
            return self._finish(glp, {k: getattr(self._delegate, k) for k in RESULTS}, redo=False)
        return self._finish(glp, res)

    def _solve_bounded(self, blp, bmap):
        """``_solve_native`` with the conversion on the host (a structure without a gather plan): one upload, one launch, one download;
        None if the entry declines the handle (PYCLLP_E_UNSUPPORTED)."""
        wanted = self.autoscale == "auto" and autoscale_wanted(blp.b, blp.c, blp.u)
        A, b, c, u = (self._dev(np.ascontiguousarray(v)) for v in (self._values(blp), blp.b, blp.c, blp.u))
        try:
            out = self._launch(A, b, c, u, _native.FLAG_AUTOSCALE if wanted else 0, {})
        except NotImplementedError:
            return None
        return download_bounded(out, blp, bmap, self.device)

    def launch_info(self):
        """``Handle.launch_info()`` of the kernel's last launch; the delegate's where it served the solve."""
        return self._delegate.launch_info() if self._delegate is not None else self._handle.launch_info()
