"""HIP solver plugin for ``GeneralLP`` batches in which every LP has its own DENSE matrix:
optimise c'x + f  s.t.  a <= A_k x <= b,  l <= x <= u,  ``lp.A.data`` of shape ``[nproblems, nnz]``.

The LP is brought into the bounded equality form (``GeneralLP.to_bounded_equality_form``: A^_k = [+-A_k | I], 0 <= x^ <= u^),
the kept rows of every A_k are densified to ``[B, m', n]`` (signs applied, slack columns left out) and the batch is solved on the
lane-group kernel that has both upper bounds and per-slot matrix images (``pycllp_hip_dense_solve_batch_bounded``,
csrc/ipm_group_slot.inc, BD && PA): ``kernel == 'bounded group per-problem'``.  One row per kept row of the LP, no row per upper
bound, and no detour over the sparse path's per-problem kernels, which is where ``hip_general_primal_normal`` sends such a
batch (``'expanded'``).  What the kernel does not serve -- a shared A, more than 32 kept rows, more than 96 columns -- is
handed to a ``HipGeneralPrimalNormalSolver`` with the same options, whose ``kernel`` and results are reported unchanged.
"""
import numpy as np
import torch

from .. import _native
from .dense_batch import densify_batch
from .general import NATIVE_MAX_COLS, NATIVE_MAX_ROWS, RESULTS, HipGeneralPrimalNormalSolver, as_general, subset
from .hip import Handle, _require_gpu, autoscale_wanted, solve_opts

OUTPUTS = ("x", "y", "z", "s", "pobj", "dobj", "status", "iters")      # of the entry, in the bounded form's variables


class HipGeneralBatchPrimalNormalSolver(HipGeneralPrimalNormalSolver):
    """``glp.init(s); glp.solve(s)`` on a ``GeneralLP`` with per-problem values of A; contract, options, rejections and result
    attributes of ``HipGeneralPrimalNormalSolver`` (``x, y, z, s, status, iters, primal_obj, dual_obj`` in the GeneralLP's
    variables).  ``kernel``: ``'bounded group per-problem'``, or the delegate's ``'bounded group'`` / ``'expanded'``.  With
    ``hsd='auto'`` the LPs that do not end optimal on the kernel are solved again through the expansion
    (``solve_expanded``), every other LP keeps its bits; ``hsd=False``: the kernel's verdict stands."""
    name = 'hip_general_batch_primal_normal'
    _native_kernel = "bounded group per-problem"

    def __init__(self, *args, **kwargs):
        super(HipGeneralBatchPrimalNormalSolver, self).__init__(*args, **kwargs)
        self._delegate = None
        self._keepalive = None
        self.mk = None

    @staticmethod
    def native_fits(glp, blp):
        return glp.A.nproblems > 1 and 1 <= blp.nrows <= NATIVE_MAX_ROWS and glp.ncols <= NATIVE_MAX_COLS

    @staticmethod
    def bounded_matrices(blp):
        """``[B, m', n]`` (float64, C order): the kept rows of every LP's matrix with their signs, without the slack columns --
        problem k's slice is ``blp.A.todense(k)[:, :n]``."""
        mk, n = blp.nrows, blp.ncols - blp.nrows
        data = np.asarray(blp.A.data, dtype=np.float64)
        return densify_batch(blp.A._rows, blp.A._cols, np.broadcast_to(data, (blp.nproblems, data.shape[1])), mk, n)

    def _make_delegate(self, glp):
        self._handle = None
        self._delegate = HipGeneralPrimalNormalSolver(device=self.device, stream=self.stream, autoscale=self.autoscale,
                                                      hsd=self.hsd, **self.options)
        self._delegate.init(glp)

    # -- plugin API ------------------------------------------------------------------------------
    def init(self, lp, verbose=0):
        """Fixes the shape of the bounded form (m' kept rows, n columns) and makes the handle from LP 0's ``[A^_0 | I]``."""
        self.device = _require_gpu(self.device)
        glp = as_general(lp)
        blp, _ = glp.to_bounded_equality_form()
        self.m, self.n, self.mk = glp.nrows, glp.ncols, blp.nrows
        self._handle = self._delegate = self._keepalive = None
        if self.native_fits(glp, blp):
            A0 = np.ascontiguousarray(blp.A.todense(0), dtype=np.float64).reshape(blp.nrows, blp.ncols)
            try:
                self._handle = Handle(A0, self.device, self.stream)
            except NotImplementedError:
                pass
        if self._handle is None:
            self._make_delegate(glp)

    def _dev(self, a):
        if isinstance(a, torch.Tensor):
            return a.to(device=self.device, dtype=torch.float64).contiguous()
        return torch.as_tensor(np.require(a, dtype=np.float64, requirements=["C", "W"]), device=self.device)

    def solve_device(self, A_dev, b_dev, c_dev, u_dev, **options):
        """Device-resident entry, in the bounded form's variables: A [B, m', n] (kept rows, signs applied, no slack columns),
        b [B, m'], c and u [B, n + m'] (torch CUDA tensors or numpy) -> dict of CUDA tensors (``OUTPUTS``).  Asynchronous on the
        solver's stream; the kernel's verdict stands (no look at the data: ``autoscale='auto'`` and ``hsd='auto'`` count as
        off)."""
        if self._handle is None:
            raise RuntimeError("solve_device() needs init() on an LP the bounded per-problem kernel serves (per-problem A, "
                               "m' <= 32, n <= 96)")
        return self._launch(self._dev(A_dev), self._dev(b_dev), self._dev(c_dev), self._dev(u_dev), 0, options)

    def _launch(self, A, b, c, u, extra_flags, overrides):
        B, mk, N = int(b.shape[0]), self.mk, self.n + self.mk
        if (b.dim() != 2 or b.shape[1] != mk or tuple(c.shape) != (B, N) or tuple(u.shape) != (B, N)
                or tuple(A.shape) != (B, mk, self.n)):
            raise ValueError("A must be [B,%d,%d], b [B,%d], c and u [B,%d] with equal B; got %r, %r, %r and %r"
                             % (mk, self.n, mk, N, tuple(A.shape), tuple(b.shape), tuple(c.shape), tuple(u.shape)))
        f64, i32 = torch.float64, torch.int32
        mk_ = lambda shape, dt: torch.empty(shape, dtype=dt, device=self.device)
        out = dict(x=mk_((B, N), f64), y=mk_((B, mk), f64), z=mk_((B, N), f64), s=mk_((B, N), f64), pobj=mk_((B,), f64),
                   dobj=mk_((B,), f64), status=mk_((B,), i32), iters=mk_((B,), i32))
        o = solve_opts(self.options, extra_flags, **overrides)
        if B:                                   # (an empty tensor has no address to hand over; the entry launches nothing for B = 0)
            self._handle.solve_batch_bounded(self.stream, A, b, c, u, out, o)
        self._keepalive = (A, b, c, u)
        self.kernel = self._native_kernel
        return out

    def solve(self, lp, verbose=0):
        if self._delegate is None and self._handle is None:
            raise RuntimeError("solve() called before init()")
        glp = as_general(lp)
        if glp.nrows != self.m or glp.ncols != self.n:
            raise ValueError("LP shape changed since init(): (%d,%d) vs (%d,%d)" % (glp.nrows, glp.ncols, self.m, self.n))
        res = None
        if self._delegate is None:
            blp, bmap = glp.to_bounded_equality_form()
            if not self.native_fits(glp, blp) or blp.nrows != self.mk:
                raise ValueError("the bounded form changed since init(): %d kept rows (%d at init), %d matrices"
                                 % (blp.nrows, self.mk, glp.A.nproblems))
            res = self._solve_bounded(blp, bmap)
            if res is None:                     # the entry answers PYCLLP_E_UNSUPPORTED
                self._make_delegate(glp)
        if res is None:
            d = self._delegate
            d.solve(glp, verbose=verbose)
            self.kernel = d.kernel
            for k in RESULTS:
                setattr(self, k, getattr(d, k))
            return self.status
        if self.hsd == "auto":
            idx = np.flatnonzero(res["status"] != 0)
            if idx.size:
                r2 = self.solve_expanded(subset(glp, idx))
                for k in RESULTS:
                    res[k][idx] = r2[k]
        for k in RESULTS:
            setattr(self, k, res[k])
        return self.status

    def _solve_bounded(self, blp, bmap):
        """One upload, one launch, one download; None if the entry declines the handle (PYCLLP_E_UNSUPPORTED)."""
        B = blp.nproblems
        wanted = self.autoscale == "auto" and autoscale_wanted(blp.b, blp.c, blp.u)
        A, b, c, u = (self._dev(np.ascontiguousarray(v)) for v in (self.bounded_matrices(blp), blp.b, blp.c, blp.u))
        try:
            out = self._launch(A, b, c, u, _native.FLAG_AUTOSCALE if wanted else 0, {})
        except NotImplementedError:
            return None
        torch.cuda.synchronize(self.device)
        r = {k: v.cpu().numpy() for k, v in out.items()}
        xo, yo, zo, so = bmap.general(r["x"], r["y"], r["z"], r["s"])
        f = np.broadcast_to(blp.f, (B,))
        return dict(x=xo, y=yo, z=zo, s=so, status=r["status"], iters=r["iters"], primal_obj=r["pobj"] + f, dual_obj=r["dobj"] + f)

    def launch_info(self):
        """``Handle.launch_info()`` of the kernel's last launch; the delegate's where it served the solve."""
        return self._delegate.launch_info() if self._delegate is not None else self._handle.launch_info()
