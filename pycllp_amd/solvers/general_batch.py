"""HIP solver plugin for ``GeneralLP`` batches in which every LP has its own DENSE matrix:
optimise c'x + f  s.t.  a <= A_k x <= b,  l <= x <= u,  ``lp.A.data`` of shape ``[nproblems, nnz]``.

The LP is brought into the bounded equality form (``GeneralLP.to_bounded_equality_form``: A^_k = [+-A_k | I], 0 <= x^ <= u^),
the kept rows of every A_k are densified to ``[B, m', n]`` (signs applied, slack columns left out) and the batch is solved on the
lane-group kernel that has both upper bounds and per-slot matrix images (``pycllp_hip_dense_solve_batch_bounded``,
csrc/ipm_group_slot.inc, BD && PA): ``kernel == 'bounded group per-problem'``.  One row per kept row of the LP, no row per upper
bound, and no detour over the sparse path's per-problem kernels, which is where ``hip_general_primal_normal`` sends such a
batch (``'expanded'``).  What the kernel does not serve -- a shared A, more than 32 kept rows, more than 96 columns -- is
handed to a ``HipGeneralPrimalNormalSolver`` with the same options, whose ``kernel`` and results are reported unchanged.
The machinery is ``general.PerProblemBounded``'s, shared with ``sparse_general_batch``; this module states what differs.
"""
import numpy as np

from .dense_batch import densify_batch
from .general import NATIVE_MAX_COLS, NATIVE_MAX_ROWS, HipGeneralPrimalNormalSolver, PerProblemBounded
from ..lp import bounded_gather_dense
from .hip import BOUNDED_RESULTS, Handle

OUTPUTS = BOUNDED_RESULTS      # of the entry, in the bounded form's variables


class HipGeneralBatchPrimalNormalSolver(PerProblemBounded, HipGeneralPrimalNormalSolver):
    """``glp.init(s); glp.solve(s)`` on a ``GeneralLP`` with per-problem values of A; contract, options, rejections and result
    attributes of ``HipGeneralPrimalNormalSolver`` (``x, y, z, s, status, iters, primal_obj, dual_obj`` in the GeneralLP's
    variables).  ``kernel``: ``'bounded group per-problem'``, or the delegate's ``'bounded group'`` / ``'expanded'``.  With
    ``hsd='auto'`` the LPs that do not end optimal on the kernel are solved again through the expansion
    (``solve_expanded``), every other LP keeps its bits; ``hsd=False``: the kernel's verdict stands.  ``solve_device`` takes
    A [B, m', n] (kept rows, signs applied, no slack columns: ``bounded_matrices``); the handle is made from LP 0's
    ``[A^_0 | I]``.  ``solve_device_general`` takes the LPs as they are (``PerProblemBounded``); ``conversion`` is ``'device'``, or
    ``'host'`` for a structure with duplicate (row, column) entries."""
    name = 'hip_general_batch_primal_normal'
    _native_kernel = "bounded group per-problem"
    _delegate_class = HipGeneralPrimalNormalSolver
    _needs = "bounded per-problem kernel serves (per-problem A, m' <= 32, n <= 96)"

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

    _values = bounded_matrices

    @staticmethod
    def _gather(glp, keep, sign):
        """None for a structure with duplicate (row, column) entries: ``densify_batch`` sums them, a gather cannot."""
        return bounded_gather_dense(glp.A, keep, sign)

    def _make_handle(self, blp):
        A0 = np.ascontiguousarray(blp.A.todense(0), dtype=np.float64).reshape(blp.nrows, blp.ncols)
        return Handle(A0, self.device, self.stream)

    def _values_spec(self, B):
        return (B, self.mk, self.n), "A must be [B,%d,%d]" % (self.mk, self.n)

    def _call(self, A, b, c, u, out, o):
        self._handle.solve_batch_bounded(self.stream, A, b, c, u, out, o)
