"""HIP solver plugin for ``GeneralLP`` batches in which every LP has its own DENSE matrix:
optimise c'x + f  s.t.  a <= A_k x <= b,  l <= x <= u,  ``lp.A.data`` of shape ``[nproblems, nnz]``.

The LP is brought into the bounded equality form (``GeneralLP.to_bounded_equality_form``: A^_k = [+-A_k | I], 0 <= x^ <= u^),
the kept rows of every A_k are densified to ``[B, m', n]`` (signs applied, slack columns left out) and the batch is solved on the
lane-group kernel that has both upper bounds and per-slot matrix images (``pycllp_hip_dense_solve_batch_bounded``,
csrc/ipm_group_slot.inc, BD && PA): ``kernel == 'bounded group per-problem'``.  One row per kept row of the LP, no row per upper
bound, and no detour over the sparse path's per-problem kernels, which is where ``hip_general_primal_normal`` sends such a
batch (``'expanded'``).  What the kernel does not serve -- a shared A, more than 32 kept rows, more than 96 columns -- is
handed to a ``HipGeneralPrimalNormalSolver`` with the same options, whose ``kernel`` and results are reported unchanged.
With ``dense_wave=True`` a batch beyond the lane-group kernels whose structure is fully dense goes through the same entry to the
bounded wavefront-per-LP kernel with a dense image per wave (csrc/ipm_wreg_bddapa.hip): up to 128 kept rows and 256 columns of
the bounded form, where the kernel's LDS plan admits the shape; ``kernel == 'bounded wave per-problem'``.
The machinery is ``general.PerProblemBounded``'s, shared with ``sparse_general_batch``; this module states what differs.
"""
import functools

import numpy as np

from .dense_batch import GROUP_MAX_COLS, GROUP_MAX_ROWS, densify_batch, fully_dense
from .general import (NATIVE_MAX_COLS, NATIVE_MAX_ROWS, HipGeneralPrimalNormalSolver, PerProblemBounded, expansion_rows,
                      subset)
from ..lp import bounded_gather_dense
from .hip import BOUNDED_RESULTS, Handle

OUTPUTS = BOUNDED_RESULTS      # of the entry, in the bounded form's variables
DENSE_WAVE_MAX_ROWS, DENSE_WAVE_MAX_COLS = 128, 256      # the bounded wave kernel with an image per wave (WREG_BDDAPA_SHAPES of csrc/wreg.h): m', N
PA_MAX_ROWS, PA_MAX_COLS = 128, 512      # what the sparse path's per-problem kernels take of an expansion (rows, all columns)


class HipGeneralBatchPrimalNormalSolver(PerProblemBounded, HipGeneralPrimalNormalSolver):
    """``glp.init(s); glp.solve(s)`` on a ``GeneralLP`` with per-problem values of A; contract, options, rejections and result
    attributes of ``HipGeneralPrimalNormalSolver`` (``x, y, z, s, status, iters, primal_obj, dual_obj`` in the GeneralLP's
    variables).  ``kernel``: ``'bounded group per-problem'``, or the delegate's ``'bounded group'`` / ``'expanded'``.  With
    ``hsd='auto'`` the LPs that do not end optimal on the kernel are solved again through the expansion
    (``solve_expanded``), every other LP keeps its bits; ``hsd=False``: the kernel's verdict stands.  ``solve_device`` takes
    A [B, m', n] (kept rows, signs applied, no slack columns: ``bounded_matrices``); the handle is made from LP 0's
    ``[A^_0 | I]``.  ``solve_device_general`` takes the LPs as they are (``PerProblemBounded``); ``conversion`` is ``'device'``, or
    ``'host'`` for a structure with duplicate (row, column) entries.

    ``dense_wave=True`` (default False: the routing above) also takes a batch beyond the lane-group kernels -- up to m' = 128
    kept rows and N = n + m' = 256 columns, the structure of A fully dense -- on the bounded wave kernel with a dense image per
    wave: ``kernel == 'bounded wave per-problem'``, the same three entries.  There ``hsd='auto'`` solves the LPs that do not end
    optimal again only where their expansion fits the sparse path's per-problem kernels (128 rows, 512 columns); elsewhere the
    kernel's status stands.  The option is this plugin's alone: a delegate does not get it.

    ``hsd_device=True`` (default False; needs ``hsd='auto'``): the LPs that do not end optimal on the lane-group kernel are
    solved again ON THE DEVICE, on that kernel's self-dual embedding (``pycllp_hip_dense_solve_batch_bounded_hsd``, DESIGN.md
    section 28) with the same handle -- their rows of A^, b^, c^, u^ gathered on the device, the results scattered back before the
    back-conversion; no expansion, no second solver, no host conversion.  A status-2 LP then carries its certificate in
    ``y, z, s``, a status-4 LP has ``x = l +`` the ray.  Where the library declines the embedding (a ``dense_wave`` handle
    beyond the lane-group kernels) those LPs take the route of ``hsd='auto'``; a delegate does not get the option.
    ``solve_device(..., hsd=True)`` and ``solve_device_general(..., hsd=True)`` run the whole batch on the embedding in one
    launch, with or without ``hsd_device``."""
    name = 'hip_general_batch_primal_normal'
    _native_kernel = "bounded group per-problem"
    _delegate_class = HipGeneralPrimalNormalSolver
    _needs = "bounded per-problem kernel serves (per-problem A, m' <= 32, n <= 96)"
    _wave = False       # the handle is one beyond the lane-group kernels (dense_wave)
    _hsd_entry = True   # the handle has ``solve_batch_bounded_hsd``: solve_device(..., hsd=True) is available

    def __init__(self, *args, dense_wave=False, hsd_device=False, **kwargs):
        if not isinstance(dense_wave, (bool, np.bool_)):
            raise ValueError("dense_wave must be True or False; got %r" % (dense_wave,))
        if not isinstance(hsd_device, (bool, np.bool_)):
            raise ValueError("hsd_device must be True or False; got %r" % (hsd_device,))
        super(HipGeneralBatchPrimalNormalSolver, self).__init__(*args, **kwargs)
        if hsd_device and self.hsd != "auto":
            raise ValueError("hsd_device=True needs hsd='auto': it says where the LPs that do not end optimal are solved again")
        self.hsd_device = bool(hsd_device)
        self.dense_wave = bool(dense_wave)
        if self.dense_wave:
            self.native_fits = functools.partial(type(self).native_fits, dense_wave=True)
            self._needs = ("bounded per-problem kernels serve (per-problem A; m' <= 32, n <= 96, or a fully dense structure "
                           "with m' <= 128, n + m' <= 256)")

    @staticmethod
    def group_fits(glp, blp):
        """The lane-group kernel's range."""
        return glp.A.nproblems > 1 and 1 <= blp.nrows <= NATIVE_MAX_ROWS and glp.ncols <= NATIVE_MAX_COLS

    @staticmethod
    def native_fits(glp, blp, dense_wave=False):
        if HipGeneralBatchPrimalNormalSolver.group_fits(glp, blp):
            return True
        # (m' <= 32 with 96 < n and N <= 128 gets a lane-group handle, which has no bounded kernel for it: not admitted)
        return bool(dense_wave and glp.A.nproblems > 1 and 1 <= blp.nrows <= DENSE_WAVE_MAX_ROWS
                    and blp.ncols <= DENSE_WAVE_MAX_COLS and (blp.nrows > GROUP_MAX_ROWS or blp.ncols > GROUP_MAX_COLS)
                    and fully_dense(blp.A._rows, blp.A._cols, blp.A.data, blp.nrows, blp.ncols))

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
        h = Handle(A0, self.device, self.stream)
        self._wave = blp.nrows > GROUP_MAX_ROWS or blp.ncols > GROUP_MAX_COLS      # a handle beyond the lane-group kernels
        if self._wave:      # an empty batch: the wave kernel's plan is built now, or the library declines the shape now
            try:
                h.plan_batch_bounded(self.stream, blp.ncols - blp.nrows)
            except NotImplementedError:
                h.free()
                raise
        self._native_kernel = "bounded wave per-problem" if self._wave else type(self)._native_kernel
        return h

    def _values_spec(self, B):
        return (B, self.mk, self.n), "A must be [B,%d,%d]" % (self.mk, self.n)

    def _call(self, A, b, c, u, out, o):
        self._handle.solve_batch_bounded(self.stream, A, b, c, u, out, o)

    def _call_hsd(self, A, b, c, u, out, o):
        self._handle.solve_batch_bounded_hsd(self.stream, A, b, c, u, out, o)

    # hsd='auto' on the wave kernel's handle: as sparse_general_batch -- the expansion has per-problem values too
    def _redo(self, glp, idx):
        if self._wave and self._delegate is None and idx.size:
            rows = expansion_rows(subset(glp, idx))
            if rows > PA_MAX_ROWS or glp.ncols + rows > PA_MAX_COLS:
                return idx[:0]
        return idx

    def _solve_again(self, glp):
        if not (self._wave and self._delegate is None):
            return super(HipGeneralBatchPrimalNormalSolver, self)._solve_again(glp)
        try:
            return self.solve_expanded(glp)
        except NotImplementedError:     # the library declines the expansion: the kernel's status stands
            return None
