"""HIP solver plugin for ``GeneralLP`` batches in which every LP has its own values on one SPARSE structure:
optimise c'x + f  s.t.  a <= A_k x <= b,  l <= x <= u,  ``lp.A.data`` of shape ``[nproblems, nnz]``.

The LP is brought into the bounded equality form (``GeneralLP.to_bounded_equality_form``: A^_k = [+-A_k | I], 0 <= x^ <= u^),
the structure of A^ becomes the CSR arrays of a sparse handle, every LP's values are permuted into that order and the batch
is solved on the bounded one-LP-per-wavefront kernel compiled for per-problem values
(``pycllp_hip_sparse_solve_batch_bounded``, csrc/ipm_wreg_bdpa.hip): ``kernel == 'bounded wave per-problem'``.  One row per
kept row of the LP, no row per upper bound: bounded forms of up to 128 kept rows and 512 columns, where
``hip_sparse_general_primal_normal`` sends such a batch through the expansion, which the sparse path's per-problem kernels
take up to 128 rows only.  What the kernel does not serve -- a shared A, m' > 128, N > 512, a structure whose tables do not
fit -- is handed to a ``HipSparseGeneralPrimalNormalSolver`` with the same options, whose ``kernel`` and results are reported
unchanged.
"""
import numpy as np
import scipy.sparse as sp
import torch

from .. import _native
from .general import (RESULTS, WAVE_MAX_COLS, WAVE_MAX_ROWS, HipSparseGeneralPrimalNormalSolver, as_general, expansion_rows,
                      subset)
from .general_batch import OUTPUTS  # noqa: F401  (the keys solve_device returns)
from .hip import Handle, _require_gpu, autoscale_wanted, solve_opts

PA_MAX_ROWS, PA_MAX_COLS = 128, 512      # what the sparse path's per-problem kernels take of an expansion (rows, all columns)


def csr_structure(A):
    """(perm, indptr, indices) of the CSR order of ``A``'s STRUCTURE (a ``SparseMatrix``): from ``(rows, cols)`` alone, never
    from the values, so an entry that is 0 in some LP keeps its slot.  ``A.data[:, perm]`` are the values in that order.
    Duplicate (row, column) entries raise ``ValueError``."""
    rows, cols = np.asarray(A._rows), np.asarray(A._cols)
    perm = np.lexsort((cols, rows))
    if perm.size and ((np.diff(rows[perm]) == 0) & (np.diff(cols[perm]) == 0)).any():
        raise ValueError("per-problem A: duplicate (row, column) entries in the structure")
    counts = np.zeros(A.nrows + 1, dtype=np.int64)
    np.add.at(counts, rows + 1, 1)
    return perm, np.cumsum(counts).astype(np.int32), cols[perm].astype(np.int32)


class HipSparseGeneralBatchPrimalNormalSolver(HipSparseGeneralPrimalNormalSolver):
    """``glp.init(s); glp.solve(s)`` on a ``GeneralLP`` with per-problem values of a sparse A; contract, options, rejections and
    result attributes of ``HipSparseGeneralPrimalNormalSolver``.  ``kernel``: ``'bounded wave per-problem'``, or the delegate's
    ``'bounded wave'`` / ``'expanded'``.  With ``hsd='auto'`` the LPs that do not end optimal on the kernel are solved again
    through the expansion (``solve_expanded``) where the library takes it for per-problem values; elsewhere the kernel's
    status stands, and every other LP keeps its bits."""
    name = 'hip_sparse_general_batch_primal_normal'
    _native_kernel = "bounded wave per-problem"

    def __init__(self, *args, **kwargs):
        super(HipSparseGeneralBatchPrimalNormalSolver, self).__init__(*args, **kwargs)
        self._delegate = None
        self._keepalive = None
        self._perm = None
        self.mk = None

    @staticmethod
    def native_fits(glp, blp):
        return glp.A.nproblems > 1 and 1 <= blp.nrows <= WAVE_MAX_ROWS and blp.ncols <= WAVE_MAX_COLS

    def bounded_values(self, blp):
        """``[B, nnz]`` (float64, C order): every LP's values of A^ in the CSR order of the handle."""
        data = np.asarray(blp.A.data, dtype=np.float64)
        if data.shape != (blp.nproblems, self._perm.size):
            raise ValueError("per-problem A: the bounded form's values must be [nproblems, nnz] = (%d, %d); got %r"
                             % (blp.nproblems, self._perm.size, data.shape))
        return np.ascontiguousarray(data[:, self._perm])

    def _make_delegate(self, glp):
        self._handle = None
        self._delegate = HipSparseGeneralPrimalNormalSolver(device=self.device, stream=self.stream, autoscale=self.autoscale,
                                                            hsd=self.hsd, **self.options)
        self._delegate.init(glp)

    # -- plugin API ------------------------------------------------------------------------------
    def init(self, lp, verbose=0):
        """Fixes the shape of the bounded form (m' kept rows, N columns) and makes the handle from the structure of A^."""
        self.device = _require_gpu(self.device)
        glp = as_general(lp)
        blp, _ = glp.to_bounded_equality_form()
        self.m, self.n, self.mk = glp.nrows, glp.ncols, blp.nrows
        self._handle = self._delegate = self._keepalive = self._perm = None
        if self.native_fits(glp, blp):
            perm, indptr, indices = csr_structure(blp.A)
            A0 = sp.csr_matrix((np.asarray(blp.A.data[0], dtype=np.float64)[perm], indices, indptr), shape=(blp.nrows, blp.ncols))
            try:
                self._handle = Handle(A0, self.device, self.stream)
                self._perm, self._structure = perm, (blp.A._rows.tobytes(), blp.A._cols.tobytes())
            except NotImplementedError:
                pass
        if self._handle is None:
            self._make_delegate(glp)

    def _dev(self, a):
        if isinstance(a, torch.Tensor):
            return a.to(device=self.device, dtype=torch.float64).contiguous()
        return torch.as_tensor(np.require(a, dtype=np.float64, requirements=["C", "W"]), device=self.device)

    def solve_device(self, Adata_dev, b_dev, c_dev, u_dev, **options):
        """Device-resident entry, in the bounded form's variables: Adata [B, nnz] (values of A^ in the handle's CSR order, the
        slack columns' ones among them: ``bounded_values``), b [B, m'], c and u [B, N] (torch CUDA tensors or numpy) -> dict of
        CUDA tensors (``OUTPUTS``).  Asynchronous on the solver's stream; the kernel's verdict stands (no look at the data:
        ``autoscale='auto'`` and ``hsd='auto'`` count as off)."""
        if self._handle is None:
            raise RuntimeError("solve_device() needs init() on an LP the bounded per-problem wave kernel serves (per-problem A, "
                               "m' <= 128, N <= 512)")
        return self._launch(self._dev(Adata_dev), self._dev(b_dev), self._dev(c_dev), self._dev(u_dev), 0, options)

    def _launch(self, A, b, c, u, extra_flags, overrides):
        B, mk, N, nnz = int(b.shape[0]), self.mk, self.n + self.mk, int(self._perm.size)
        if (b.dim() != 2 or b.shape[1] != mk or tuple(c.shape) != (B, N) or tuple(u.shape) != (B, N)
                or tuple(A.shape) != (B, nnz)):
            raise ValueError("Adata must be [B,%d], b [B,%d], c and u [B,%d] with equal B; got %r, %r, %r and %r"
                             % (nnz, mk, N, tuple(A.shape), tuple(b.shape), tuple(c.shape), tuple(u.shape)))
        f64, i32 = torch.float64, torch.int32
        mk_ = lambda shape, dt: torch.empty(shape, dtype=dt, device=self.device)
        out = dict(x=mk_((B, N), f64), y=mk_((B, mk), f64), z=mk_((B, N), f64), s=mk_((B, N), f64), pobj=mk_((B,), f64),
                   dobj=mk_((B,), f64), status=mk_((B,), i32), iters=mk_((B,), i32))
        o = solve_opts(self.options, extra_flags, **overrides)
        if B:                                   # (an empty tensor has no address to hand over; the entry launches nothing for B = 0)
            self._handle.solve_bounded(self.stream, b, c, u, out, o, values=A)
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
            if (not self.native_fits(glp, blp) or blp.nrows != self.mk
                    or (blp.A._rows.tobytes(), blp.A._cols.tobytes()) != self._structure):
                raise ValueError("the bounded form changed since init(): %d kept rows (%d at init), %d matrices, or another "
                                 "structure of A" % (blp.nrows, self.mk, glp.A.nproblems))
            res = self._solve_bounded(blp, bmap)
            if res is None:                     # the entry answers PYCLLP_E_UNSUPPORTED
                self._make_delegate(glp)
        if res is None:
            d = self._delegate
            try:
                d.solve(glp, verbose=verbose)
            finally:
                self.kernel = d.kernel          # (also where the library refuses the delegate's expansion)
            for k in RESULTS:
                setattr(self, k, getattr(d, k))
            return self.status
        if self.hsd == "auto":
            idx = self._redo(glp, np.flatnonzero(res["status"] != 0))
            if idx.size:
                try:
                    r2 = self.solve_expanded(subset(glp, idx))
                except NotImplementedError:     # the library declines the expansion: the kernel's status stands
                    r2 = None
                if r2 is not None:
                    for k in RESULTS:
                        res[k][idx] = r2[k]
        for k in RESULTS:
            setattr(self, k, res[k])
        return self.status

    def _redo(self, glp, idx):
        """The expansion has per-problem values too: the sparse path's per-problem kernels take it up to 128 rows and 512 columns."""
        if idx.size:
            rows = expansion_rows(subset(glp, idx))
            if rows > PA_MAX_ROWS or glp.ncols + rows > PA_MAX_COLS:
                return idx[:0]
        return idx

    def _solve_bounded(self, blp, bmap):
        """One upload, one launch, one download; None if the entry declines the handle (PYCLLP_E_UNSUPPORTED)."""
        B = blp.nproblems
        wanted = self.autoscale == "auto" and autoscale_wanted(blp.b, blp.c, blp.u)
        A, b, c, u = (self._dev(np.ascontiguousarray(v)) for v in (self.bounded_values(blp), blp.b, blp.c, blp.u))
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
