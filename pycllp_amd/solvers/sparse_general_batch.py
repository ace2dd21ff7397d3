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
unchanged.  The machinery is ``general.PerProblemBounded``'s, shared with ``general_batch``; this module states what differs.
"""
import numpy as np
import scipy.sparse as sp

from ..lp import bounded_gather_csr
from .general import (WAVE_MAX_COLS, WAVE_MAX_ROWS, HipSparseGeneralPrimalNormalSolver, PerProblemBounded, expansion_rows,
                      subset)
from .general_batch import OUTPUTS  # noqa: F401  (the keys solve_device returns)
from .hip import Handle

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


class HipSparseGeneralBatchPrimalNormalSolver(PerProblemBounded, HipSparseGeneralPrimalNormalSolver):
    """``glp.init(s); glp.solve(s)`` on a ``GeneralLP`` with per-problem values of a sparse A; contract, options, rejections and
    result attributes of ``HipSparseGeneralPrimalNormalSolver``.  ``kernel``: ``'bounded wave per-problem'``, or the delegate's
    ``'bounded wave'`` / ``'expanded'``.  With ``hsd='auto'`` the LPs that do not end optimal on the kernel are solved again
    through the expansion (``solve_expanded``) where the library takes it for per-problem values; elsewhere the kernel's
    status stands, and every other LP keeps its bits.  ``solve_device`` takes Adata [B, nnz] (values of A^ in the handle's CSR
    order, the slack columns' ones among them: ``bounded_values``); the handle is made from the structure of A^.
    ``solve_device_general`` takes the LPs as they are (``PerProblemBounded``); ``conversion`` is ``'device'``."""
    name = 'hip_sparse_general_batch_primal_normal'
    _native_kernel = "bounded wave per-problem"
    _delegate_class = HipSparseGeneralPrimalNormalSolver
    _needs = "bounded per-problem wave kernel serves (per-problem A, m' <= 128, N <= 512)"
    _changed_what = PerProblemBounded._changed_what + ", or another structure of A"
    _perm = None

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

    _values = bounded_values

    def _gather(self, glp, keep, sign):
        return bounded_gather_csr(glp.A, keep, sign, self._perm)

    def init(self, lp, verbose=0):
        self._perm = None
        super(HipSparseGeneralBatchPrimalNormalSolver, self).init(lp, verbose)

    def _make_handle(self, blp):
        perm, indptr, indices = csr_structure(blp.A)
        A0 = sp.csr_matrix((np.asarray(blp.A.data[0], dtype=np.float64)[perm], indices, indptr), shape=(blp.nrows, blp.ncols))
        h = Handle(A0, self.device, self.stream)
        self._perm, self._structure = perm, (blp.A._rows.tobytes(), blp.A._cols.tobytes())
        return h

    def _values_spec(self, B):
        return (B, int(self._perm.size)), "Adata must be [B,%d]" % self._perm.size

    def _call(self, A, b, c, u, out, o):
        self._handle.solve_bounded(self.stream, b, c, u, out, o, values=A)

    def _unchanged(self, glp, blp):
        return (super(HipSparseGeneralBatchPrimalNormalSolver, self)._unchanged(glp, blp)
                and (blp.A._rows.tobytes(), blp.A._cols.tobytes()) == self._structure)

    def _solve_delegate(self, glp, verbose):
        try:
            self._delegate.solve(glp, verbose=verbose)
        finally:
            self.kernel = self._delegate.kernel          # (also where the library refuses the delegate's expansion)

    def _solve_again(self, glp):
        try:
            return self.solve_expanded(glp)
        except NotImplementedError:     # the library declines the expansion: the kernel's status stands
            return None

    def _redo(self, glp, idx):
        """The expansion has per-problem values too: the sparse path's per-problem kernels take it up to 128 rows and 512 columns."""
        if idx.size:
            rows = expansion_rows(subset(glp, idx))
            if rows > PA_MAX_ROWS or glp.ncols + rows > PA_MAX_COLS:
                return idx[:0]
        return idx
