"""HIP solver plugin for batches in which every LP has its own DENSE constraint matrix.

``lp.A`` is a ``SparseMatrix`` with ``data [nproblems, nnz]`` (one structure, per-problem values).  Up to m = 32 rows and
n = 128 columns of the equality form the values are densified to ``[B, m, a_cols]`` on the host and solved on the lane-group
kernel for per-problem A (``pycllp_hip_dense_solve_batch``, csrc/ipm_group_slot.inc, PA): ``kernel == 'group per-problem'``.
Beyond that a fully dense structure (``fully_dense``) of up to m = 128 rows and n = 256 columns goes through the same entry to the
wavefront-per-LP kernel with a dense image per wave (csrc/ipm_wreg_dapa.hip), where its LDS plan admits the shape:
``kernel == 'wave per-problem'``.  Every other LP goes to ``HipSparsePrimalNormalSolver`` unchanged: ``kernel == 'delegated'``.
"""
import numpy as np
import torch

from . import BaseSolver
from .. import _native
from ..lp import EqualityLP, SparseMatrix
from .hip import (RESULTS, DeviceArrays, Handle, HipSparsePrimalNormalSolver, _require_gpu, autoscale_wanted, plugin_options,
                  solve_opts)

GROUP_MAX_ROWS, GROUP_MAX_COLS = 32, 128      # the lane-group kernels
SLACK_MAX_DENSE_COLS = 96                     # ... and their slack-aware shapes: at most 96 columns before the identity tail
WAVE_MAX_ROWS, WAVE_MAX_COLS = 128, 256       # the wave kernel with an image per wave (WREG_DAPA_SHAPES of csrc/wreg.h)
_REJECTED = _native.FLAG_HSD | _native.FLAG_PREDCORR | _native.FLAG_WARM_START | _native.FLAG_WAVE_KERNEL


def identity_tail(rows, cols, data, m, n):
    """True when the last m columns of every problem's matrix are the identity, judged from the structure: the entries of
    those columns that are non-zero in any problem are exactly the m diagonal ones, and they are 1 in every problem."""
    if n <= m:
        return False
    rows, cols, data = np.asarray(rows), np.asarray(cols), np.atleast_2d(np.asarray(data))
    tail = cols >= n - m
    nz = tail & (data != 0).any(axis=0)
    if int(nz.sum()) != m or not np.array_equal(np.sort(rows[nz]), np.arange(m)):
        return False
    return bool((rows[nz] == cols[nz] - (n - m)).all() and (data[:, nz] == 1.0).all())


def fully_dense(rows, cols, data, m, n):
    """True when the structure is that of a dense matrix: every position of the first nd columns is present exactly once, where
    nd = n - m and the last m columns are the identity (``identity_tail``), or nd = n and there is no such tail."""
    rows, cols = np.asarray(rows, dtype=np.int64), np.asarray(cols, dtype=np.int64)
    if rows.size == 0 or rows.min() < 0 or rows.max() >= m or cols.min() < 0 or cols.max() >= n:
        return False
    nd = n - m if identity_tail(rows, cols, data, m, n) else n
    head = cols < nd
    if nd == n and rows.size != m * n or int(head.sum()) != m * nd:
        return False
    return np.unique(rows[head] * nd + cols[head]).size == m * nd


def densify_batch(rows, cols, data, m, a_cols):
    """``data [B, nnz]`` on the coordinate structure ``rows, cols`` as dense ``[B, m, a_cols]`` (float64, C order): problem
    k's slice is ``todense(k)[:, :a_cols]``.  Entries in columns >= a_cols (an implied identity tail) are left out; entries
    that share a position are summed, as ``todense`` sums them."""
    rows, cols = np.asarray(rows, dtype=np.int64), np.asarray(cols, dtype=np.int64)
    data = np.atleast_2d(np.asarray(data, dtype=np.float64))
    if rows.size and (rows.min() < 0 or rows.max() >= m or cols.min() < 0):
        raise ValueError("structure outside the %d rows of the LP" % m)
    keep = cols < a_cols
    flat = rows[keep] * a_cols + cols[keep]
    out = np.zeros((data.shape[0], m * a_cols), dtype=np.float64)
    if np.unique(flat).size == flat.size:
        out[:, flat] = data[:, keep]
    else:
        np.add.at(out, (slice(None), flat), data[:, keep])
    return out.reshape(data.shape[0], m, a_cols)


class HipDenseBatchPrimalNormalSolver(DeviceArrays, BaseSolver):
    """``lp.init(s); lp.solve(s)`` on an equality-form LP with per-problem values of a dense A; results as the other HIP
    plugins leave them (``x, y, z, status, iters, primal_obj, dual_obj``) and ``kernel``: which path served the last solve."""
    name = 'hip_dense_batch_primal_normal'

    def __init__(self, device=None, stream=None, autoscale="auto", hsd="auto", predcorr=False, warm_start=False, **options):
        """``hsd='auto'`` (default): the LPs that do not end optimal are solved again, as a per-problem subset, on
        ``HipSparsePrimalNormalSolver(hsd=True)``, which gives infeasible / unbounded LPs the certified statuses 2 / 4;
        ``hsd=False``: the kernel's verdict stands.  ``hsd=True``, ``predcorr=True`` and ``warm_start=True`` are not available
        (the kernel has no embedding, no predictor-corrector and no warm start).  ``autoscale``: as
        ``HipDensePrimalNormalSolver``.  Other keyword arguments are fields of ``pycllp_hip_opts``; FLAG_NO_SLACK_PATH in
        ``flags`` keeps an identity tail in the matrices handed to the kernel."""
        if not isinstance(hsd, str) and hsd:
            raise ValueError("hsd must be 'auto' or False for %s (its kernel has no embedding)" % self.name)
        if predcorr:
            raise ValueError("predcorr is not available with per-problem dense matrices")
        if warm_start:
            raise ValueError("warm_start is not available with per-problem dense matrices")
        if int(options.get("flags", 0)) & _REJECTED:
            raise ValueError("flags HSD, PREDCORR, WARM_START and WAVE_KERNEL are not available with per-problem dense matrices")
        self.hsd, self.autoscale, _, _, self.options = plugin_options(options, hsd, autoscale)
        self.device, self.stream = device, stream
        self._handle = self._delegate = None
        self._wave = False
        self.kernel = None
        self.slack = False

    # -- plugin API ------------------------------------------------------------------------------
    def init(self, lp, verbose=0):
        """Fixes the shape, and from the structure whether the last m columns are the identity (then they are implied, and
        only the n - m columns before them are handed to the kernel)."""
        self.device = _require_gpu(self.device)
        m, n = int(lp.nrows), int(lp.ncols)
        self.m, self.n = m, n
        self._handle = self._delegate = None
        self._keepalive = None
        A = lp.A
        group = m <= GROUP_MAX_ROWS and n <= GROUP_MAX_COLS
        self._wave = (not group and m <= WAVE_MAX_ROWS and n <= WAVE_MAX_COLS and isinstance(A, SparseMatrix)
                      and fully_dense(A._rows, A._cols, A.data, m, n))
        if not group and not self._wave:
            return self._delegate_to_sparse(lp, verbose)
        if not isinstance(A, SparseMatrix):
            raise ValueError("%s takes lp.A as a SparseMatrix with data [nproblems, nnz]" % self.name)
        no_slack = bool(int(self.options.get("flags", 0)) & _native.FLAG_NO_SLACK_PATH)
        ident = identity_tail(A._rows, A._cols, A.data, m, n) and (self._wave or n - m <= SLACK_MAX_DENSE_COLS)
        self.slack = ident and not no_slack
        # a handle whose matrix has the identity tail where this batch as a whole has not (problem 0 only, say) would expect
        # the short matrices: the full ones then go with FLAG_NO_SLACK_PATH
        self._flags = 0 if self.slack else _native.FLAG_NO_SLACK_PATH
        self.a_cols = n - m if self.slack else n
        if verbose > 0:
            print("Initializing %s (m=%d, n=%d, a_cols=%d) on %s" % (type(self).__name__, m, n, self.a_cols, self.device))
        self._handle = Handle(np.ascontiguousarray(A.todense(0), dtype=np.float64).reshape(m, n), self.device, self.stream)
        if self._wave:
            # the first launch, of an empty batch: the library builds its LDS plan and declines here where no variant or plan
            # covers the shape -- the solver then delegates from now on
            try:
                empty = lambda *shape: torch.empty(shape, dtype=torch.float64, device=self.device)
                self._launch(empty(0, m, self.a_cols), empty(0, m), empty(0, n), 0, {})
            except NotImplementedError:
                self._handle = None
                self._delegate_to_sparse(lp, verbose)

    def _delegate_to_sparse(self, lp, verbose):
        self._wave = False
        self._delegate = HipSparsePrimalNormalSolver(device=self.device, stream=self.stream, autoscale=self.autoscale,
                                                     hsd=self.hsd, **self.options)
        self._delegate.init(lp, verbose=verbose)

    def solve_device(self, A_dev, b_dev, c_dev, **options):
        """Device-resident entry: A [B, m, a_cols] (``self.a_cols``: n - m where the identity tail is implied, else n),
        b [B, m], c [B, n] (torch CUDA tensors or numpy) -> dict of CUDA tensors (``RESULTS``).  Asynchronous on the solver's
        stream; the kernel's verdict stands (no look at the data: ``autoscale='auto'`` and ``hsd='auto'`` count as off)."""
        if self._handle is None:
            raise RuntimeError("solve_device() needs init() on an LP the lane-group kernel (m <= 32, n <= 128) or the wave "
                               "kernel for per-problem dense matrices serves")
        return self._launch(self._dev(A_dev), self._dev(b_dev), self._dev(c_dev), 0, options)

    def _launch(self, A, b, c, extra_flags, overrides):
        B = int(b.shape[0])
        if (b.dim() != 2 or c.dim() != 2 or b.shape[1] != self.m or tuple(c.shape) != (B, self.n)
                or tuple(A.shape) != (B, self.m, self.a_cols)):
            raise ValueError("A must be [B,%d,%d], b [B,%d] and c [B,%d] with equal B; got %r, %r and %r"
                             % (self.m, self.a_cols, self.m, self.n, tuple(A.shape), tuple(b.shape), tuple(c.shape)))
        f64, i32 = torch.float64, torch.int32
        mk = lambda shape, dt: torch.empty(shape, dtype=dt, device=self.device)
        out = dict(x=mk((B, self.n), f64), y=mk((B, self.m), f64), z=mk((B, self.n), f64), pobj=mk((B,), f64),
                   dobj=mk((B,), f64), status=mk((B,), i32), iters=mk((B,), i32))
        o = solve_opts(self.options, self._flags | extra_flags, **overrides)
        self._handle.solve_batch_dense(self.stream, A, b, c, out, o)
        self._keepalive = (A, b, c)
        self.kernel = "wave per-problem" if self._wave else "group per-problem"
        return out

    def solve(self, lp, verbose=0):
        if self._delegate is None and self._handle is None:
            raise RuntimeError("solve() called before init()")
        if int(lp.nrows) != self.m or int(lp.ncols) != self.n:
            raise ValueError("LP shape changed since init(): (%d,%d) vs (%d,%d)" % (lp.nrows, lp.ncols, self.m, self.n))
        if self._delegate is not None:
            d = self._delegate
            d.solve(lp, verbose=verbose)
            self.kernel = "delegated"
            for k in ("x", "y", "z", "status", "iters", "primal_obj", "dual_obj"):
                setattr(self, k, getattr(d, k))
            return self.status
        B = int(lp.nproblems)
        data = np.asarray(lp.A.data, dtype=np.float64)
        if data.ndim != 2 or data.shape[0] not in (1, B) or data.shape[1] != np.asarray(lp.A._rows).size:
            raise ValueError("lp.A.data must be [nproblems, nnz]; got %r" % (data.shape,))
        if verbose > 0:
            print("Solving %d LPs with %s..." % (B, type(self).__name__))
        b = np.ascontiguousarray(lp.b, dtype=np.float64); c = np.ascontiguousarray(lp.c, dtype=np.float64)
        A = densify_batch(lp.A._rows, lp.A._cols, np.broadcast_to(data, (B, data.shape[1])), self.m, self.a_cols)
        extra = _native.FLAG_AUTOSCALE if (self.autoscale == "auto" and autoscale_wanted(b, c)) else 0
        out = self._launch(self._dev(A), self._dev(b), self._dev(c), extra, {})
        torch.cuda.synchronize(self.device)
        res = {k: out[k].cpu().numpy() for k in RESULTS}
        if self.hsd == "auto":
            self._resolve_non_optimal(lp, data, b, c, res, extra)
        f = np.asarray(getattr(lp, "f", 0.0), dtype=np.float64)
        self.x, self.y, self.z = res["x"], res["y"], res["z"]
        self.status, self.iters = res["status"], res["iters"]
        self.primal_obj, self.dual_obj = res["pobj"] + f, res["dobj"] + f
        if verbose > 0:
            print("Solve complete.")
        return self.status

    def _resolve_non_optimal(self, lp, data, b, c, res, extra_flags):
        """hsd='auto': the LPs that did not end optimal, as a per-problem subset on ``HipSparsePrimalNormalSolver(hsd=True)``;
        their results replace the kernel's verdict, every other LP stays as it is.  A subset the sparse path's per-problem
        kernels decline (too many Gram terms for their tables) is solved LP by LP on the same solver object, each as a shared-A
        problem (the sparse path's handle holds one matrix, so every such LP costs an ``init``)."""
        idx = np.flatnonzero(res["status"] != 0)
        if idx.size == 0:
            return
        flags = (int(self.options.get("flags", 0)) | extra_flags) & ~_native.FLAG_NO_SLACK_PATH
        opts = dict(self.options, flags=flags)
        vals = np.broadcast_to(data, (b.shape[0], data.shape[1]))

        s = HipSparsePrimalNormalSolver(device=self.device, stream=self.stream, hsd=True, autoscale=False, **opts)

        def run(sel):
            A2 = SparseMatrix(np.asarray(lp.A._rows).copy(), np.asarray(lp.A._cols).copy(), vals[sel].copy())
            A2._shape = (self.m, self.n)
            sub = EqualityLP(A2, b[sel], c[sel], 0.0)
            sub.init(s)
            sub.solve(s)
            for k, attr in (("x", "x"), ("y", "y"), ("z", "z"), ("status", "status"), ("iters", "iters"),
                            ("pobj", "primal_obj"), ("dobj", "dual_obj")):
                res[k][sel] = getattr(s, attr)

        try:
            run(idx)
        except NotImplementedError:
            for k in idx:
                run(np.array([k]))

    def launch_info(self):
        """grid / block / LDS bytes, ``group_shape`` (MP, NP) and ``slack`` of the last launch (``Handle.launch_info``) -- on the
        wave kernel ``wave_shape`` (MB, NQ), ``variant`` and ``kernel`` instead; the delegate's where it served the solve."""
        return self._delegate.launch_info() if self._delegate is not None else self._handle.launch_info()
