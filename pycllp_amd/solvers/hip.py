"""HIP host for the batched dense primal-normal interior-point solver.

Mirrors the contract of the reference's OpenCL host ``ClDensePrimalNormalSolver``
(``pycllp/solvers/cl.py:12-124``): the constructor takes optional device handles, ``init(lp)`` captures
the shared constraint matrix once, ``solve(lp)`` consumes the LP's current ``b``/``c`` and leaves
``self.x [nproblems, ncols]`` and ``self.status [nproblems]`` as attributes.  Differences, all
supersets: ``solve`` also returns ``self.status`` (as the reference's CPU solvers do,
``pycllp/solvers/normal_eqns.py:33``) and sets ``y, z, primal_obj, dual_obj, iters``.

PyTorch is plumbing only (device memory, streams); the compute is ``csrc/libpycllp_hip.so``.
"""
import ctypes

import numpy as np
import scipy.sparse as sp
import torch

from . import BaseSolver
from .. import _native


# order of the result arrays inside the one allocation that holds them (HipDensePrimalNormalSolver._buffers)
PACK_ORDER = (("pobj", torch.float64), ("dobj", torch.float64), ("status", torch.int32), ("iters", torch.int32),
              ("y", torch.float64), ("x", torch.float64), ("z", torch.float64))


def pack_layout(B, m, n):
    """(offset, nbytes, dtype, shape) of every result array of a B-LP solve in its packed allocation, 256-byte aligned
    sections; everything up to and including x -- what a result gather ships -- forms a contiguous prefix of
    ``_gather_bytes`` bytes (``pycllp_amd.dist.PackedGather``)."""
    shapes = {"pobj": (B,), "dobj": (B,), "status": (B,), "iters": (B,), "y": (B, m), "x": (B, n), "z": (B, n)}
    layout, off = {}, 0
    for name, dt in PACK_ORDER:
        nb = int(np.prod(shapes[name], dtype=np.int64)) * torch.empty((), dtype=dt).element_size()
        layout[name] = (off, nb, dt, shapes[name])
        off = (off + nb + 255) & ~255
        if name == "x":
            layout["_gather_bytes"] = off
    layout["_total_bytes"] = off
    return layout


def unpack(packed, layout, names=("pobj", "dobj", "status", "iters", "y", "x")):
    """Views of the result arrays inside a packed byte buffer (e.g. one received from another rank)."""
    out = {}
    for name in names:
        off, nb, dt, shape = layout[name]
        out[name] = packed[off:off + nb].view(dt).view(shape)
    return out


# pycllp_hip_sparse_launch_info's `kernel` -> (variant, kernel family): 'wave' = the register-resident one-LP-per-wavefront
# kernel (csrc/wreg_wave.h) on Gram term tables or on a dense image of A, 'block' = the one-LP-per-workgroup kernel of
# csrc/ipm_block.inc (m <= 128), 'big' = the one-LP-per-workgroup kernel for large LPs (csrc/ipm_big.hip: 128 < m <= 256 or
# 512 < n <= 1280), Gram from a term list or on the matrix cores
SPARSE_KERNEL_KINDS = {0: ("block", "block"), 1: ("tables", "wave"), 2: ("dense image", "wave"),
                       3: ("term list", "big"), 4: ("MFMA Gram", "big")}
AUTOSCALE_BAND = (0.1, 10.0)


def autoscale_wanted(b, c, u=None):
    """The ``autoscale='auto'`` rule: True when, for any LP of the batch, max|b| or max|c| lies outside [0.1, 10] -- the
    start x = z = y = 1 and the unit floors of the tolerances (eps (1 + |b|)) are tuned to data of order 1 (DESIGN.md section
    2, scaling caveat: decades away from 1 cost 40-170 iterations and objective accuracy).  numpy arrays or torch tensors.
    ``u`` (optional): upper bounds of a bounded LP; max of the finite positive u of an LP outside the band counts too (an
    LP without one -- no bounds, or only fixed variables -- is left out of that test).  An LP whose max|b| or max|c| is not finite
    (a NaN or an Inf in its data) is left out as well: it ends with PYCLLP_STATUS_NUMERICAL whatever the scaling and must not
    decide the arithmetic of the others."""
    lo, hi = AUTOSCALE_BAND
    if isinstance(u, torch.Tensor):
        if u.numel():
            fin = torch.isfinite(u) & (u > 0)
            mx = torch.where(fin, u.abs(), torch.zeros((), dtype=u.dtype, device=u.device)).amax(dim=-1)
            if bool((fin.any(dim=-1) & ((mx < lo) | (mx > hi))).any()):
                return True
    elif u is not None:
        u = np.asarray(u, dtype=np.float64)
        fin = np.isfinite(u) & (u > 0)
        has = fin.any(axis=-1)
        mx = np.where(fin, np.abs(u), 0.0).max(axis=-1) if u.size else np.zeros(0)
        if (has & ((mx < lo) | (mx > hi))).any():
            return True
    for v in (b, c):
        if isinstance(v, torch.Tensor):
            if v.numel() == 0:
                continue
            mx = v.abs().amax(dim=-1)
            if bool((((mx < lo) | (mx > hi)) & torch.isfinite(mx)).any()):
                return True
        else:
            v = np.asarray(v)
            if v.size == 0:
                continue
            mx = np.abs(v).max(axis=-1)
            if (((mx < lo) | (mx > hi)) & np.isfinite(mx)).any():
                return True
    return False


def autoscale_mask(b, c, u=None):
    """The ``autoscale='per_lp'`` rule, the specification of what the kernels decide under PYCLLP_FLAG_AUTOSCALE_PER_LP: bool
    [B], True where the LP is OUT OF BAND and is solved scaled -- ``autoscale_wanted`` applied to that LP alone.  Out of band:
    max|b|, or max|c| over all n columns, is finite and < 0.1 or > 10 (the edges are in band; b = 0 is out of band), or --
    ``u`` given -- the largest finite positive u of the LP is (an LP without one is left out of that test).  A non-finite
    maximum (a NaN or an Inf in the row) triggers nothing by itself.  b [B, m], c [B, n], u [B, n] (a single LP may come as
    vectors): numpy arrays give a numpy array, torch tensors a tensor on their device; an array without columns says False.
    ``autoscale_wanted(b, c, u) == bool(autoscale_mask(b, c, u).any())``."""
    lo, hi = AUTOSCALE_BAND
    use_torch = any(isinstance(v, torch.Tensor) for v in (b, c, u))

    def rows(v):
        if use_torch:
            v = v if isinstance(v, torch.Tensor) else torch.as_tensor(np.asarray(v, dtype=np.float64))
        else:
            v = np.asarray(v, dtype=np.float64)
        return v.reshape(1, -1) if v.ndim == 1 else v

    def part(v, bounds):
        v = rows(v)
        xp = torch if use_torch else np
        if v.shape[-1] == 0:
            return (torch.zeros(tuple(v.shape[:-1]), dtype=torch.bool, device=v.device) if use_torch
                    else np.zeros(v.shape[:-1], dtype=bool))
        if bounds:
            fin = xp.isfinite(v) & (v > 0)
            mx = xp.where(fin, v, xp.zeros_like(v))
            mx = mx.amax(dim=-1) if use_torch else mx.max(axis=-1)
            return fin.any(-1) & ((mx < lo) | (mx > hi))
        mx = v.abs().amax(dim=-1) if use_torch else np.abs(v).max(axis=-1)
        return ((mx < lo) | (mx > hi)) & xp.isfinite(mx)

    mask = part(b, False)
    if use_torch:
        parts = [part(c, False)] + ([part(u, True)] if u is not None else [])
        for q in parts:
            mask = mask | q.to(mask.device)
        return mask
    mask = mask | part(c, False)
    return mask | part(u, True) if u is not None else mask


def warm_lifted(x, lift=1e-3):
    """The start point ``warm_start=True`` makes of a previous x (or z): max(x, lift * max(1, |x|_inf)) per LP (numpy)."""
    x = np.asarray(x, dtype=np.float64)
    return np.maximum(x, lift * np.maximum(1.0, np.abs(x).max(axis=1, keepdims=True)))


def _require_gpu(device):
    if not torch.cuda.is_available():
        raise RuntimeError("pycllp_amd: no ROCm device visible -- the HIP solvers have no CPU fallback")
    return torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)


def plugin_options(options, hsd="auto", autoscale="auto", predcorr=False, warm_start=False, warm_lift=1e-3):
    """(hsd, autoscale, warm_start, warm_lift, options) of a solver plugin's constructor arguments: ``hsd`` and ``autoscale``
    as True, False or 'auto' (FLAG_HSD / FLAG_AUTOSCALE in ``flags`` switch them on), ``autoscale`` also as 'per_lp'
    (FLAG_AUTOSCALE_PER_LP, likewise: the kernels decide for every LP by itself, ``autoscale_mask``), ``options`` -- fields of
    ``pycllp_hip_opts`` -- with the flags of hsd=True, autoscale=True or 'per_lp' and predcorr merged into ``flags``, names
    validated.  Every launch of a plugin takes its flags from ``options``, so 'per_lp' reaches all of them."""
    if isinstance(hsd, str):
        if hsd != "auto":
            raise ValueError("hsd must be True, False or 'auto'")
    elif isinstance(hsd, (bool, np.bool_, int, np.integer)):
        hsd = bool(hsd)           # 1 / np.bool_(True) mean True (`hsd is True` tests below)
    else:
        raise ValueError("hsd must be True, False or 'auto'")
    if predcorr and hsd is True:
        raise ValueError("predcorr is an option of the reference's path; it cannot be combined with hsd=True")
    if isinstance(autoscale, str):
        if autoscale not in ("auto", "per_lp"):
            raise ValueError("autoscale must be True, False, 'auto' or 'per_lp'")
    else:
        autoscale = bool(autoscale)
    options = dict(options)
    flags = int(options.get("flags", 0))
    if flags & _native.FLAG_AUTOSCALE_PER_LP:
        if flags & _native.FLAG_AUTOSCALE or autoscale is True:
            raise ValueError("autoscale: FLAG_AUTOSCALE (True) and FLAG_AUTOSCALE_PER_LP ('per_lp') exclude each other")
        autoscale = "per_lp"
    elif flags & _native.FLAG_AUTOSCALE:
        if autoscale == "per_lp":
            raise ValueError("autoscale: FLAG_AUTOSCALE (True) and FLAG_AUTOSCALE_PER_LP ('per_lp') exclude each other")
        autoscale = True
    if flags & _native.FLAG_HSD:
        hsd = True
    implied = ((_native.FLAG_PREDCORR if predcorr else 0) | (_native.FLAG_AUTOSCALE if autoscale is True else 0)
               | (_native.FLAG_AUTOSCALE_PER_LP if autoscale == "per_lp" else 0)
               | (_native.FLAG_HSD if hsd is True else 0))
    if implied:
        options["flags"] = flags | implied
    warm_lift = float(warm_lift)
    if not (warm_lift >= 0.0):
        raise ValueError("warm_lift must be >= 0")
    _native.default_opts(**options) if options else None      # validate names early
    return hsd, autoscale, bool(warm_start), warm_lift, options


def solve_opts(options, extra_flags=0, **overrides):
    """The ``_native.Opts`` of one solve: a plugin's ``options`` with ``overrides`` (fields of ``pycllp_hip_opts``) and
    ``extra_flags`` added for this call, range-checked."""
    opts = dict(options, **overrides)
    opts["flags"] = int(opts.get("flags", 0)) | extra_flags
    o = _native.default_opts(**opts)
    if o.max_iter < 1 or o.max_refine < _native.MAX_REFINE_AUTO or not (o.eps > 0):
        raise ValueError("max_iter must be >= 1, max_refine >= 0 (or -1 = auto) and eps > 0")
    return o


RESULTS = ("x", "y", "z", "pobj", "dobj", "status", "iters")       # (also the order of the solve entries' outputs)
BOUNDED_RESULTS = ("x", "y", "z", "s", "pobj", "dobj", "status", "iters")      # ... and of the entries with upper bounds


def bounded_outputs(B, m, N, device):
    """Uninitialised output tensors of a bounded solve of B LPs with m rows and N columns (``BOUNDED_RESULTS``)."""
    shapes = dict(x=(B, N), y=(B, m), z=(B, N), s=(B, N), pobj=(B,), dobj=(B,), status=(B,), iters=(B,))
    return {k: torch.empty(shapes[k], dtype=torch.int32 if k in ("status", "iters") else torch.float64, device=device)
            for k in BOUNDED_RESULTS}


class DeviceArrays(object):
    """Mix-in of the plugins: what they upload goes through ``_dev``."""

    def _dev(self, a):
        """``a`` (torch tensor or numpy) as a contiguous float64 tensor on ``self.device``."""
        if isinstance(a, torch.Tensor):
            return a.to(device=self.device, dtype=torch.float64).contiguous()
        return torch.as_tensor(np.require(a, dtype=np.float64, requirements=["C", "W"]), device=self.device)   # (a read-only array is copied)


class Handle(object):
    """One library handle for a constraint matrix on ``device``: ``pycllp_hip_dense`` for a dense numpy ``A``,
    ``pycllp_hip_sparse`` for a scipy CSR ``A`` (for per-problem values of A: their structure with problem 0's values), freed
    exactly once.  The calls take torch tensors and the stream to queue on (None: torch's current stream on ``device``); an
    answer PYCLLP_E_UNSUPPORTED -- the library declines the matrix or the call -- raises ``NotImplementedError``.  As a
    ctypes argument the object stands for its raw handle."""
    _as_parameter_ = None

    def __init__(self, A, device, stream):
        self.device = device
        if isinstance(A, np.ndarray):
            self.family, sizes, arrays = "dense", A.shape, (np.ascontiguousarray(A, dtype=np.float64),)
        else:
            self.family, sizes = "sparse", A.shape + (int(A.nnz),)
            arrays = (np.ascontiguousarray(A.data, dtype=np.float64), np.ascontiguousarray(A.indptr, dtype=np.int32),
                      np.ascontiguousarray(A.indices, dtype=np.int32))
        arrays = [torch.as_tensor(v, device=device) for v in arrays]
        h = ctypes.c_void_p()
        self._call("init", *sizes, *arrays, self._stream(stream), ctypes.byref(h))    # (synchronises the stream)
        self._as_parameter_ = h

    def _stream(self, stream):
        return ctypes.c_void_p((stream if stream is not None else torch.cuda.current_stream(self.device)).cuda_stream)

    def _call(self, entry, *args):
        name = "pycllp_hip_%s_%s" % (self.family, entry)
        args = [ctypes.c_void_p(a.data_ptr()) if isinstance(a, torch.Tensor) else a for a in args]
        with torch.cuda.device(self.device):
            _native.check(getattr(_native.lib(), name)(*args), name)

    def solve(self, stream, b, c, out, o, values=None):
        """B LPs b [B, m], c [B, n] into ``out`` (the arrays of ``RESULTS``).  ``values`` [B, nnz]: per-problem values of A in
        the CSR order of the handle's matrix (sparse family)."""
        entry, lead = ("solve", ()) if values is None else ("solve_batch", (values,))
        self._call(entry, self, int(b.shape[0]), *lead, b, c, *(out[k] for k in RESULTS), ctypes.byref(o), self._stream(stream))

    def solve_bounded(self, stream, b, c, u, out, o, values=None):
        """B LPs with the upper bounds u [B, n] into ``out`` (x, y, z, s, pobj, dobj, status, iters).  ``values`` [B, nnz]:
        per-problem values of A in the CSR order of the handle's matrix (sparse family)."""
        entry, lead = ("solve_bounded", ()) if values is None else ("solve_batch_bounded", (values,))
        self._call(entry, self, int(b.shape[0]), *lead, b, c, u, *(out[k] for k in BOUNDED_RESULTS), ctypes.byref(o),
                   self._stream(stream))

    def solve_bounded_hsd(self, stream, b, c, u, out, o):
        """``solve_bounded`` on the homogeneous self-dual embedding with bounds (``pycllp_hip_dense_solve_bounded_hsd`` on the
        lane-group kernel, ``pycllp_hip_sparse_solve_bounded_hsd`` on the wave kernel: the handle's family names the entry):
        statuses 2 and 4 come with their certificate in ``out`` (y, z, s / x), 0 and 5 with the solution."""
        self._call("solve_bounded_hsd", self, int(b.shape[0]), b, c, u, *(out[k] for k in BOUNDED_RESULTS), ctypes.byref(o),
                   self._stream(stream))

    def _solve_batch(self, entry, stream, A, vectors, outputs, o):
        """``entry`` of the dense family on per-problem matrices: A must be a contiguous [B, m, a_cols] with the B of b."""
        B = int(vectors[0].shape[0])
        if A.dim() != 3 or A.shape[0] != B or not A.is_contiguous():
            raise ValueError("A must be a contiguous [B, m, a_cols] tensor with the B of b; got %r" % (tuple(A.shape),))
        self._call(entry, self, B, A, ctypes.c_long(int(A.shape[2])), *vectors, *outputs, ctypes.byref(o), self._stream(stream))

    def solve_batch_dense(self, stream, A, b, c, out, o):
        """B LPs with their own dense matrices A [B, m, a_cols] (dense family; a_cols = n - m where the handle's tail is the
        identity and ``o`` does not carry FLAG_NO_SLACK_PATH, else n) into ``out`` (the arrays of ``RESULTS``)."""
        self._solve_batch("solve_batch", stream, A, (b, c), [out[k] for k in RESULTS], o)

    def solve_batch_bounded(self, stream, A, b, c, u, out, o):
        """B LPs with their own dense matrices A [B, m, n - m] (dense family, a handle whose tail is the identity) and the upper
        bounds u [B, n] into ``out`` (x, y, z, s, pobj, dobj, status, iters): on the lane-group kernel, or beyond it (m <= 128,
        n <= 256) on the bounded wave kernel with an image per wave."""
        self._solve_batch("solve_batch_bounded", stream, A, (b, c, u), [out[k] for k in BOUNDED_RESULTS], o)

    def solve_batch_bounded_hsd(self, stream, A, b, c, u, out, o):
        """``solve_batch_bounded`` on the homogeneous self-dual embedding with bounds
        (``pycllp_hip_dense_solve_batch_bounded_hsd``, lane-group kernels only): statuses 2 and 4 come with their certificate in
        ``out`` (y, z, s / x), 0 and 5 with the solution.  ``NotImplementedError`` beyond the lane-group kernels and for a shape
        the kernel does not ship in."""
        self._solve_batch("solve_batch_bounded_hsd", stream, A, (b, c, u), [out[k] for k in BOUNDED_RESULTS], o)

    def plan_batch_bounded(self, stream, a_cols):
        """An empty batch (B = 0) through ``solve_batch_bounded``'s entry with matrices of ``a_cols`` columns: nothing is
        launched, but a handle beyond the lane-group kernels builds the bounded wave kernel's plan now, and
        ``NotImplementedError`` says at once that no shape or LDS plan of it covers the LP."""
        t = torch.zeros(1, dtype=torch.float64, device=self.device)      # (the entry wants u non-NULL whatever B is; nothing is read)
        o = _native.default_opts()
        self._call("solve_batch_bounded", self, 0, t, ctypes.c_long(int(a_cols)), *([t] * 11), ctypes.byref(o), self._stream(stream))

    def newton(self, stream, x, z, y, b, c, mu, dy, nrefine, o):
        self._call("newton", self, int(x.shape[0]), x, z, y, b, c, float(mu), dy, nrefine, ctypes.byref(o), self._stream(stream))

    def launch_info(self):
        """grid / block / LDS bytes of the last launch (dense family: the padded m, n too) and, where one of the kernels of
        ``SPARSE_KERNEL_KINDS`` served it, its ``variant`` and ``kernel``.  The compiled instantiation that served it:
        ``wave_shape`` (MB, NQ) on the wavefront-per-LP kernel, ``group_shape`` (MP, NP) and ``slack`` (1: the slack-aware
        kernel) on the lane-group kernels, ``big_shape`` (WGPC, BNC) and ``factor_in_lds`` (the factor blocks in LDS, else in the
        L2 workspace) on the large-LP kernel; ``a_in_lds`` (A's CSR / CSC copy in LDS, else read through L2) where the block
        kernel served the launch.  Dense family: ``full_shape``, whether a full-shape instantiation of a lane-group kernel served
        it (the LP fills a compiled shape exactly; ``_native.FLAG_GENERIC_SHAPE`` in ``flags`` keeps the generic one; the key
        is absent with a PYCLLP_HIP_LIB library that predates the entry, ``_native.LATER_ENTRIES``)."""
        keys = ("grid", "block", "lds_bytes") + (("m_pad", "n_pad") if self.family == "dense" else ("kernel",))
        vals = [ctypes.c_int() for _ in keys]
        self._call("launch_info", self, *[ctypes.byref(v) for v in vals])
        d = dict(zip(keys, [v.value for v in vals]))
        kind = _native.lib().pycllp_hip_dense_kernel_kind(self) if self.family == "dense" else d["kernel"]
        if kind >= 0:
            d["variant"], d["kernel"] = SPARSE_KERNEL_KINDS[kind]
        shape = [ctypes.c_int() for _ in range(3 if self.family == "dense" else 2)]
        self._call("variant_info", self, *[ctypes.byref(v) for v in shape])
        a, b = shape[0].value, shape[1].value
        if a > 0 and (self.family == "sparse" or shape[2].value < 0):
            d["wave_shape"] = (a, b)
        elif a > 0:
            d["group_shape"], d["slack"] = (a, b), shape[2].value
        if self.family == "dense" and _native.has_entry("pycllp_hip_dense_full_shape"):
            d["full_shape"] = bool(_native.lib().pycllp_hip_dense_full_shape(self))
        plan = [ctypes.c_int() for _ in range(4)]
        self._call("plan_info", self, *[ctypes.byref(v) for v in plan])
        wgpc, bnc, factor, a_lds = [v.value for v in plan]
        if wgpc > 0:
            d["big_shape"], d["factor_in_lds"] = (wgpc, bnc), bool(factor)
        if a_lds >= 0:
            d["a_in_lds"] = bool(a_lds)
        return d

    def free(self):
        h, self._as_parameter_ = self._as_parameter_, None
        if h is not None:
            getattr(_native.lib(), "pycllp_hip_%s_free" % self.family)(h)

    def __del__(self):
        try:
            self.free()
        except Exception:
            pass


class HipDensePrimalNormalSolver(DeviceArrays, BaseSolver):
    """Drop-in for ``cl_dense_primal_normal`` on MI355X.  The LP must be in equality form
    (callers use ``StandardLP.to_equality_form()`` first, as for the OpenCL solver).  Per-problem values of A
    (``lp.A.data [nproblems, nnz]``) are served by the sparse path's per-problem kernel: one structure, values from HBM."""
    name = 'hip_dense_primal_normal'

    def __init__(self, device=None, stream=None, keep_on_device=False, autoscale="auto", hsd="auto", warm_start=False,
                 predcorr=False, warm_lift=1e-3, **options):
        """``hsd=True`` (PYCLLP_FLAG_HSD) solves on the homogeneous self-dual embedding, the model of the reference's
        CPU solver ``pycllp/ipo/hsd.c``: infeasible (status 2) and unbounded (status 4) LPs are then detected reliably,
        after ~12-15 iterations, and ``x`` / ``y, z`` hold the certificate.  ``hsd="auto"`` (default) runs the reference's
        own path (``pycllp/cl/primal_normal.cl:201-284``) and then re-solves, on the embedding, exactly those LPs that did
        not end optimal: an optimal LP gets the drop-in behaviour, every other one a verdict with a certificate instead of
        the outcome of the reference kernel's 10x-growth heuristic (which labels most infeasible LPs "iteration limit").
        ``hsd=False`` is the reference's path alone.
        ``warm_start=True``: repeat solve -- the library's stated purpose (reference ``README.md:5-6``, the intent recorded
        at ``pycllp/cl/primal_normal.cl:213-219``): the solver keeps x, z, y of the previous ``solve()`` on the device and
        starts every LP that was optimal there from its previous point (PYCLLP_FLAG_WARM_START); the others, and a first
        solve or one with a different batch size, start from x = z = y = 1.  The previous optimum sits ON the boundary
        (x_j z_j ~ 1e-10), where an interior-point method restarts badly: measured on 1 %-perturbed data, 12-18 iterations on
        average with tails of 50-100 and about one jammed LP in 300.  ``warm_lift`` (default 1e-3; 0 = the raw point) lifts the
        start into the interior first -- x <- max(x, warm_lift max(1, |x|_inf)), likewise z: 10 iterations on average, at most
        19, no jam (cold: 20-23).
        ``autoscale=True`` (PYCLLP_FLAG_AUTOSCALE, not in the reference) solves every LP with b/max|b| and c/max|c| and
        scales the results back: for b or c orders of magnitude away from 1.  ``autoscale="auto"`` (default) switches it on
        in ``solve(lp)`` for a batch in which some LP has max|b| or max|c| outside [0.1, 10] (``autoscale_wanted``) and
        leaves a batch inside that band -- the reference's test and benchmark regime -- on the reference's arithmetic bit
        for bit; ``solve_device`` (asynchronous, no look at the data) treats "auto" as off.  ``autoscale="per_lp"``
        (PYCLLP_FLAG_AUTOSCALE_PER_LP) leaves the decision to the kernels, LP by LP (``autoscale_mask``): an LP outside the band
        is solved as under ``autoscale=True``, every other one on the reference's arithmetic, bit for bit and whatever else
        is in the batch.  The flag goes with every launch -- ``solve_device`` and the hsd='auto' re-solves included -- and
        ``solve(lp)`` needs no band test: the host pipeline runs once, without the speculative pass of "auto".
        ``predcorr=True`` (PYCLLP_FLAG_PREDCORR, not in the reference's kernel): Mehrotra's predictor-corrector step on the same
        Gram / LDL' machinery -- one factorisation and two solves per iteration, the same optimum in ~27 % fewer iterations at
        the reference's step fraction r = 0.9 and ~45 % fewer at r = 0.99; the default stays the reference's rule.  With the
        default ``hsd="auto"`` the LPs that do not end optimal are still re-solved on the embedding.  Other keyword arguments are
        the fields of ``pycllp_hip_opts`` (eps, delta, r, pivot_floor, refine_tol, max_iter, max_refine, flags)."""
        super(HipDensePrimalNormalSolver, self).__init__()
        self.hsd, self.autoscale, self.warm_start, self.warm_lift, self.options = plugin_options(
            options, hsd, autoscale, predcorr, warm_start, warm_lift)
        self._extra_flags = 0        # flags solve(lp) adds for one call (autoscale='auto')
        self._prev_B = None
        self.device = device
        self.stream = stream
        self.keep_on_device = keep_on_device
        self._handle = None
        self._a_perm = self._a_values = None
        self.buffers = {}

    # -- helpers ---------------------------------------------------------------------------------
    @staticmethod
    def consume(lp):
        """Everything a HIP host reads from an LP object -- the reference's ``EqualityLP`` or this package's -- as plain
        numpy: the attribute surface of ``pycllp/solvers/cl.py:35-39,99,102`` (``nrows, ncols, nproblems, A.todense(), b, c``)
        plus ``f``.  tools/check_reference_boundary.py runs this on reference-built objects."""
        m, n = int(lp.nrows), int(lp.ncols)
        A = lp.A.todense() if hasattr(lp.A, "todense") else lp.A
        A = np.ascontiguousarray(np.asarray(A, dtype=np.float64))
        if A.shape != (m, n):
            raise ValueError("A has shape %r, expected (%d, %d)" % (A.shape, m, n))
        return dict(m=m, n=n, nproblems=int(lp.nproblems), A=A,
                    b=np.ascontiguousarray(np.asarray(lp.b, dtype=np.float64)), c=np.ascontiguousarray(np.asarray(lp.c, dtype=np.float64)),
                    f=np.atleast_1d(np.asarray(getattr(lp, "f", 0.0), dtype=np.float64)))

    def _shared_matrix(self, lp):
        """The shared A as the handle takes it: densified (``pycllp/solvers/cl.py:39``)."""
        return self.consume(lp)["A"]

    def _check_batch(self, b, c):
        if b.ndim != 2 or c.ndim != 2 or b.shape[1] != self.m or c.shape[1] != self.n or b.shape[0] != c.shape[0]:
            raise ValueError("b must be [B,%d] and c [B,%d] with equal B; got %r and %r"
                             % (self.m, self.n, tuple(b.shape), tuple(c.shape)))
        return int(b.shape[0])

    # -- plugin API ------------------------------------------------------------------------------
    def init(self, lp, verbose=0):
        """Upload A once (``pycllp/solvers/cl.py:39,46``)."""
        self.device = _require_gpu(self.device)
        m, n = int(lp.nrows), int(lp.ncols)
        self._a_perm = self._a_values = None
        if getattr(lp.A, "nproblems", 1) > 1:
            # per-problem values on one structure (SparseMatrix.data[nproblems, nnz], pycllp/lp.py:16-54): the structure
            # comes from the coordinate lists, the values of problem 0 only stand in at init
            rows, cols = np.asarray(lp.A._rows), np.asarray(lp.A._cols)
            perm = np.lexsort((cols, rows))
            if perm.size and ((np.diff(rows[perm]) == 0) & (np.diff(cols[perm]) == 0)).any():
                raise ValueError("per-problem A: duplicate (row, column) entries in the structure")
            self._a_perm = perm
            indptr = np.zeros(m + 1, dtype=np.int64)
            np.add.at(indptr, rows + 1, 1)
            A = sp.csr_matrix((np.asarray(lp.A.data[0], dtype=np.float64)[perm], cols[perm], np.cumsum(indptr)), shape=(m, n))
        else:
            A = self._shared_matrix(lp)
        if verbose > 0:
            print("Initializing %s (m=%d, n=%d) on %s" % (type(self).__name__, m, n, self.device))
        self._handle = None          # (the previous handle is freed before the new one is made)
        self._handle = Handle(A, self.device, self.stream)
        self.m, self.n = m, n
        self.buffers = {}

    def _pack_layout(self, B):
        return pack_layout(B, self.m, self.n)

    def _buffers(self, B, slot=0):
        """Output tensors of one solve: views into ONE device allocation (``packed``, bytes), so that a caller who ships
        the results elsewhere -- the multi-GPU gather -- moves a single contiguous buffer (its first ``gather_bytes``
        bytes hold pobj, dobj, status, iters, y, x) instead of six.  ``slot`` selects one of several independent sets so
        that the results of solve k stay alive (e.g. while they are being gathered) during solve k+1."""
        key = "set%d" % slot
        cur = self.buffers.get(key)
        if cur is None or cur["B"] != B:
            layout = self._pack_layout(B)
            packed = torch.empty(max(layout["_total_bytes"], 256), dtype=torch.uint8, device=self.device)
            cur = dict(B=B, packed=packed, layout=layout, gather_bytes=layout["_gather_bytes"])
            cur.update(unpack(packed, layout, names=[n for n, _ in PACK_ORDER]))
            self.buffers[key] = cur
        return cur

    def solve_device(self, b, c, warm_start=False, slot=0, **options):
        """Device-resident entry: b [B,m], c [B,n] (torch CUDA or numpy) -> dict of CUDA tensors.
        Asynchronous on the solver's stream."""
        if self._handle is None:
            raise RuntimeError("solve() called before init()")
        b = self._dev(b); c = self._dev(c)
        buf = self._buffers(self._check_batch(b, c), slot)
        self._launch(b, c, buf, solve_opts(self.options, self._extra_flags | (_native.FLAG_WARM_START if warm_start else 0),
                                           **options))
        self._keepalive = (b, c)
        return buf

    def _launch(self, b, c, out, o, row0=0, values=None):
        """One solve of the LPs b, c into ``out`` on the solver's stream.  Per-problem A: LP k takes row row0 + k of ``values``
        (default ``_a_values``) -- a chunk of the host pipeline starts at its row of the batch."""
        if self._a_perm is not None:
            values = self._a_values if values is None else values
            if values is None or values.shape[0] < row0 + b.shape[0]:
                raise ValueError("per-problem A: no values for this batch (use lp.solve(solver))")
            values = values[row0:row0 + b.shape[0]]
        self._handle.solve(self.stream, b, c, out, o, values)

    # -- host-to-host path -----------------------------------------------------------------------
    PIPELINE_MIN_BATCH = 8192   # below this one upload / launch / download is as fast
    PIPELINE_CHUNKS = 8

    def _host_staging(self, B):
        """Page-locked host images of b, c and of every result, allocated once per batch size (the counterpart of
        the host arrays ``pycllp/solvers/cl.py:40-41`` keeps) plus the two copy streams of the pipeline."""
        st = self.buffers.get("host")
        if st is None or st["B"] != B:
            f64, i32 = torch.float64, torch.int32
            pin = lambda shape, dt: torch.empty(shape, dtype=dt, pin_memory=True)
            st = dict(B=B, b=pin((B, self.m), f64), c=pin((B, self.n), f64),
                      x=pin((B, self.n), f64), z=pin((B, self.n), f64), y=pin((B, self.m), f64),
                      pobj=pin((B,), f64), dobj=pin((B,), f64), status=pin((B,), i32), iters=pin((B,), i32),
                      db=torch.empty((B, self.m), dtype=f64, device=self.device),
                      dc=torch.empty((B, self.n), dtype=f64, device=self.device),
                      s_in=torch.cuda.Stream(self.device), s_out=torch.cuda.Stream(self.device))
            st["hb"], st["hc"] = st["b"].numpy(), st["c"].numpy()
            self.buffers["host"] = st
        return st

    def _solve_host(self, b, c, warm=False):
        """numpy in, numpy out, as a three-stage pipeline over row chunks of the batch: upload chunk k+1, solve
        chunk k and download chunk k-1 run on three HIP streams, so the PCIe time hides behind the kernel.  The
        returned arrays are views of the solver's page-locked buffers and are overwritten by the next solve()
        (the reference's ``self.x`` behaves the same way, ``pycllp/solvers/cl.py:40,119``)."""
        b = np.ascontiguousarray(b, dtype=np.float64); c = np.ascontiguousarray(c, dtype=np.float64)
        B = self._check_batch(b, c)
        st, buf = self._host_staging(B), self._buffers(B, 0)
        nchunk = max(1, min(self.PIPELINE_CHUNKS, B // self.PIPELINE_MIN_BATCH))
        edges = [B * k // nchunk for k in range(nchunk + 1)]
        compute = self.stream if self.stream is not None else torch.cuda.current_stream(self.device)
        o = solve_opts(self.options, _native.FLAG_WARM_START if warm else 0)
        # autoscale='auto' decided on the device (self._extra_flags is None): the chunks are solved WITHOUT the flag while their
        # band tests (two row reductions each, queued behind the chunk's upload) accumulate; if some LP of the batch turns out
        # to lie outside the band -- b or c decades away from 1: LPs that take 40-170 iterations unscaled -- the batch is solved
        # once more with the flag from the data already on the device.  Data inside the band (the common case) keeps the
        # full overlap of staging, upload, solve and download.
        if self._extra_flags is None and warm:
            # (a warm start reads the x, z, y the first pass would overwrite: decide before launching anything)
            self._extra_flags = _native.FLAG_AUTOSCALE if autoscale_wanted(b, c) else 0
        speculative = self._extra_flags is None
        if not speculative:
            o.flags |= self._extra_flags
        lo_band, hi_band = AUTOSCALE_BAND
        tests = []

        def solve_chunks(upload):
            for lo, hi in zip(edges[:-1], edges[1:]):
                if upload:
                    # plain memcpy on this thread: torch's CPU copy_ would wake its whole intra-op thread pool, whose
                    # spin-waiting burns a container's CPU quota and shows up as sporadic ~80 ms stalls
                    np.copyto(st["hb"][lo:hi], b[lo:hi]); np.copyto(st["hc"][lo:hi], c[lo:hi])
                    with torch.cuda.stream(st["s_in"]):
                        st["db"][lo:hi].copy_(st["b"][lo:hi], non_blocking=True)
                        st["dc"][lo:hi].copy_(st["c"][lo:hi], non_blocking=True)
                        compute.wait_event(st["s_in"].record_event())
                        if speculative:
                            for v in (st["db"][lo:hi], st["dc"][lo:hi]):
                                mx = v.abs().amax(dim=-1)
                                tests.append((((mx < lo_band) | (mx > hi_band)) & torch.isfinite(mx)).any())
                part = {k: buf[k][lo:hi] for k in RESULTS}
                self._launch(st["db"][lo:hi], st["dc"][lo:hi], part, o, row0=lo)
                done = compute.record_event()
                with torch.cuda.stream(st["s_out"]):
                    st["s_out"].wait_event(done)
                    for k in RESULTS:
                        st[k][lo:hi].copy_(part[k], non_blocking=True)

        with torch.cuda.device(self.device):
            solve_chunks(upload=True)
            if speculative:
                compute.wait_stream(st["s_in"])          # (the band tests ran there: read them only once they are computed)
                with torch.cuda.stream(compute):
                    self._extra_flags = _native.FLAG_AUTOSCALE if bool(torch.stack(tests).any()) else 0
                if self._extra_flags:                    # (the hsd='auto' re-solve of this call runs with it too)
                    o.flags |= _native.FLAG_AUTOSCALE
                    st["s_out"].synchronize()            # (the first pass's downloads still read the results)
                    solve_chunks(upload=False)
            st["s_out"].synchronize()
        return {k: st[k].numpy() for k in RESULTS}

    def _prepare_warm(self, B):
        """True when this solve may start from the previous solution: same batch size, a previous solve exists.  LPs that
        did not end optimal last time are reset to the cold start x = z = y = 1 (their x, z may hold a certificate)."""
        if not self.warm_start or self._prev_B != B or "set0" not in self.buffers:
            return False
        buf = self.buffers["set0"]
        with self._on_solver_stream():       # the kernel that reads x, z, y is launched on the solver's stream
            bad = buf["status"] != 0
            if bool(bad.any()):
                buf["x"][bad] = 1.0; buf["z"][bad] = 1.0; buf["y"][bad] = 0.0 if self.hsd is True else 1.0
            if self.warm_lift > 0.0:      # off the boundary (see __init__): the same rule as warm_lifted() below
                for k in ("x", "z"):
                    v = buf[k]
                    floor = self.warm_lift * torch.clamp(v.abs().amax(dim=1, keepdim=True), min=1.0)
                    torch.maximum(v, floor, out=v)
        return True

    def _on_solver_stream(self):
        """Context in which torch tensor work is queued on the stream the solve kernels run on (gathers and
        resets issued on torch's current stream raced a kernel launched on a caller-supplied stream)."""
        import contextlib
        return torch.cuda.stream(self.stream) if self.stream is not None else contextlib.nullcontext()

    def _resolve_non_optimal(self, b, c, res):
        """hsd='auto': the LPs that did not end optimal are solved again on the homogeneous self-dual embedding and their
        results replace the first verdict.  ``res``: dict of numpy arrays or CUDA tensors of the first solve."""
        on_device = isinstance(res["status"], torch.Tensor)
        if on_device:
            idx = torch.nonzero(res["status"] != 0).flatten()
            host_idx = idx.cpu().numpy()
        else:
            host_idx = np.flatnonzero(res["status"] != 0)
        if host_idx.size == 0:
            return
        flags = (int(self.options.get("flags", 0)) | _native.FLAG_HSD) & ~(_native.FLAG_WARM_START | _native.FLAG_PREDCORR)
        o = solve_opts(self.options, self._extra_flags, flags=flags)
        with self._on_solver_stream():       # gathers, launch and scatters in ONE stream order
            if not on_device:
                idx = torch.as_tensor(host_idx, device=self.device)
            if isinstance(b, torch.Tensor) or isinstance(c, torch.Tensor):
                b2, c2 = self._dev(b)[idx], self._dev(c)[idx]
            else:
                b2, c2 = self._dev(np.asarray(b)[host_idx]), self._dev(np.asarray(c)[host_idx])
            r2 = self._buffers(host_idx.size, 3)
            self._launch(b2, c2, r2, o, values=None if self._a_values is None else self._a_values[idx])
            if on_device:
                for k in RESULTS:
                    res[k][idx] = r2[k]
            torch.cuda.synchronize(self.device)
        if not on_device:
            for k in RESULTS:
                res[k][host_idx] = r2[k].cpu().numpy()

    def solve(self, lp, verbose=0):
        """Solve every problem of ``lp`` (current ``lp.b``, ``lp.c``, and ``lp.A.data`` for per-problem values of A); results in
        attributes."""
        if int(lp.nrows) != self.m or int(lp.ncols) != self.n:
            raise ValueError("LP shape changed since init(): (%d,%d) vs (%d,%d)" % (lp.nrows, lp.ncols, self.m, self.n))
        if self._handle is None:
            raise RuntimeError("solve() called before init()")
        if self._a_perm is not None:
            data = np.asarray(lp.A.data, dtype=np.float64)
            if data.shape != (int(lp.nproblems), self._a_perm.size):
                raise ValueError("per-problem A: lp.A.data must be [nproblems, nnz] = (%d, %d); got %r"
                                 % (lp.nproblems, self._a_perm.size, data.shape))
            self._a_values = torch.as_tensor(np.ascontiguousarray(data[:, self._a_perm]), device=self.device)
        if verbose > 0:
            print("Solving %d LPs with %s..." % (lp.nproblems, type(self).__name__))
        f = np.asarray(getattr(lp, "f", 0.0), dtype=np.float64)
        B = int(lp.nproblems)
        # autoscale='auto': the band test of the whole batch.  For host arrays headed for the host pipeline it is left to the
        # device (_solve_host: after the upload, two reductions): on 65 536 x (32 + 96) doubles the numpy version of the test
        # took 24 ms of a 9 ms host-to-host solve.
        host_pipeline = (not isinstance(lp.b, torch.Tensor) and not isinstance(lp.c, torch.Tensor) and not self.keep_on_device)
        if self.autoscale == "auto" and host_pipeline and B * (self.m + self.n) >= (1 << 16):
            self._extra_flags = None       # (small batches: the numpy test costs microseconds, the device test ~8 launches)
        else:
            self._extra_flags = _native.FLAG_AUTOSCALE if (self.autoscale == "auto" and autoscale_wanted(lp.b, lp.c)) else 0
        try:
            return self._solve_plugin(lp, f, B, verbose)
        finally:
            self._extra_flags = 0

    def _solve_plugin(self, lp, f, B, verbose):
        warm = self._prepare_warm(B)
        on_host = not isinstance(lp.b, torch.Tensor) and not isinstance(lp.c, torch.Tensor)
        if on_host and not self.keep_on_device:
            res = self._solve_host(lp.b, lp.c, warm)
            if self.hsd == "auto":
                self._resolve_non_optimal(lp.b, lp.c, res)
            self.x, self.y, self.z = res["x"], res["y"], res["z"]
            self.status, self.iters = res["status"], res["iters"]
            # objective offset f is added when reporting (as pycllp/solvers/pathfollowing.py:113-114)
            self.primal_obj, self.dual_obj = res["pobj"] + f, res["dobj"] + f
        else:
            buf = self.solve_device(lp.b, lp.c, warm_start=warm)
            torch.cuda.synchronize(self.device)
            res = {k: buf[k] for k in RESULTS}
            if self.hsd == "auto":
                self._resolve_non_optimal(lp.b, lp.c, res)
            if self.keep_on_device:
                self.x, self.y, self.z = res["x"], res["y"], res["z"]
                self.status, self.iters = res["status"], res["iters"]
                ft = torch.as_tensor(np.broadcast_to(f, (buf["B"],)).copy(), device=self.device)
                self.primal_obj, self.dual_obj = res["pobj"] + ft, res["dobj"] + ft
            else:
                self.x = res["x"].cpu().numpy(); self.y = res["y"].cpu().numpy(); self.z = res["z"].cpu().numpy()
                self.status = res["status"].cpu().numpy(); self.iters = res["iters"].cpu().numpy()
                self.primal_obj = res["pobj"].cpu().numpy() + f
                self.dual_obj = res["dobj"].cpu().numpy() + f
        self._prev_B = B
        if verbose > 0:
            print("Solve complete.")
        return self.status

    def newton_step(self, x, z, y, b, c, mu, **options):
        """Stand-alone Newton step dy for B states: the reference's ``solve_primal_normal`` kernel
        (``pycllp/cl/ldl.cl:602-653``, as launched by its ``tests/test_ldl.py:219-273``), on a sparse shared A its
        ``sparse_solve_primal_normal`` (``ldl.cl:656-712``, as launched by ``tests/test_ldl.py:276-361``)."""
        if self._handle is None:
            raise RuntimeError("newton_step() called before init()")
        if self._a_perm is not None:
            # the handle holds problem 0's values only: a step for LP k > 0 would silently use the wrong matrix
            raise NotImplementedError("newton_step() with per-problem values of A: the stand-alone Newton entry takes one "
                                      "shared matrix (pycllp/cl/ldl.cl:656-712); init a solver per matrix instead")
        x, z, y, b, c = [self._dev(np.atleast_2d(v) if not isinstance(v, torch.Tensor) else v) for v in (x, z, y, b, c)]
        B = int(x.shape[0])
        dy = torch.empty((B, self.m), dtype=torch.float64, device=self.device)
        nref = torch.empty(B, dtype=torch.int32, device=self.device)
        self._handle.newton(self.stream, x, z, y, b, c, mu, dy, nref, _native.default_opts(**dict(self.options, **options)))
        torch.cuda.synchronize(self.device)
        self.nrefine = nref.cpu().numpy()
        return dy.cpu().numpy()

    def launch_info(self):
        """grid / block / LDS bytes of the last solve and, where the sparse path's kernels served it, which one
        (``SPARSE_KERNEL_KINDS``)."""
        return self._handle.launch_info()


class HipSparsePrimalNormalSolver(HipDensePrimalNormalSolver):
    """Drop-in for ``cl_sparse_primal_normal`` (``pycllp/solvers/cl.py:127-278``): shared SPARSE constraint matrix, one LP
    per workgroup, m <= 128 rows and n <= 512 columns (equality form).  Same contract and result attributes as the
    dense solver; ``init`` takes the CSR arrays of ``lp.A`` (the reference builds them from the densified A,
    ``cl.py:175-178``), the transposed copy and the structure of A diag(x/z) A' are derived inside the library."""
    name = 'hip_sparse_primal_normal'

    def _shared_matrix(self, lp):
        if hasattr(lp.A, "tocsr"):
            A = sp.csr_matrix(lp.A.tocsr())
        else:
            A = sp.csr_matrix(np.asarray(lp.A.todense() if hasattr(lp.A, "todense") else lp.A, dtype=np.float64))
        A = sp.csr_matrix(A, shape=(int(lp.nrows), int(lp.ncols)))
        A.sum_duplicates(); A.eliminate_zeros(); A.sort_indices()
        return A
