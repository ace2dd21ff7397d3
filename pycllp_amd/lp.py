"""Problem containers with the attribute surface the reference's solver plugins consume.

The reference's ``pycllp/lp.py`` "stays" (BASELINE.json north_star) but does not travel to the GPU
box, so this module carries a compact, independently written container exposing exactly what a
solver touches (``pycllp/solvers/cl.py:35-39,99,102``): ``nrows, ncols, nproblems, A.todense(), b, c, f``
plus ``init(solver)`` / ``solve(solver)`` (``pycllp/lp.py:531-535``) and ``StandardLP.to_equality_form()``
(``pycllp/lp.py:551-567``).  Broadcasting rules follow ``pycllp/lp.py:338-352``: a 1-D ``b`` is one
problem, a 1-D ``c`` is repeated for every problem, a scalar ``f`` is repeated, and mismatched problem
counts raise ``ValueError``.  A real ``pycllp`` LP object can be passed to the solvers instead: they
duck-type on the attributes above.
"""
import numpy as np
import scipy.sparse as sp


class SparseMatrix(object):
    """One shared sparsity pattern in coordinate form (``pycllp/lp.py:16-54``).

    ``data`` is ``[nproblems, nnz]``: one shared structure, per-problem values (``pycllp/lp.py:16-24``).  The reference's LP
    classes accept a single set of values only (``pycllp/lp.py:335-336``: "can only have a single problem in the current
    implementation"); here ``nproblems`` sets of values are accepted when there is one per problem of the LP, and the HIP
    solvers read them per LP."""

    def __init__(self, rows=None, cols=None, data=None, matrix=None):
        if matrix is not None:
            coo = sp.coo_matrix(matrix)
            self._rows = np.asarray(coo.row, dtype=np.int64)
            self._cols = np.asarray(coo.col, dtype=np.int64)
            self.data = np.asarray(coo.data, dtype=np.float64).reshape(1, -1)
            self._shape = coo.shape
        elif data is not None:
            if not (len(rows) == len(cols) == np.shape(data)[-1]):
                raise ValueError("Arrays rows, cols and data must be the same length.")
            self._rows = np.asarray(rows, dtype=np.int64)
            self._cols = np.asarray(cols, dtype=np.int64)
            self.data = np.atleast_2d(np.asarray(data, dtype=np.float64))
            self._shape = None
        else:
            self._rows = np.zeros(0, dtype=np.int64)
            self._cols = np.zeros(0, dtype=np.int64)
            self.data = np.zeros((1, 0))
            self._shape = None

    @property
    def nrows(self):
        n = int(self._rows.max()) + 1 if self._rows.size else 0
        return max(n, self._shape[0]) if self._shape else n

    @property
    def ncols(self):
        n = int(self._cols.max()) + 1 if self._cols.size else 0
        return max(n, self._shape[1]) if self._shape else n

    @property
    def nnzeros(self):
        return int(self._rows.size)

    @property
    def nproblems(self):
        return int(self.data.shape[0])

    def add_col(self, rows, values):
        """Append a column with the given row entries; returns its index."""
        col = self.ncols
        rows = np.atleast_1d(np.asarray(rows, dtype=np.int64))
        values = np.atleast_1d(np.asarray(values, dtype=np.float64))
        self._rows = np.concatenate([self._rows, rows])
        self._cols = np.concatenate([self._cols, np.full(rows.shape, col, dtype=np.int64)])
        self.data = np.concatenate([self.data, np.tile(values, (self.data.shape[0], 1))], axis=1)
        if self._shape:
            self._shape = (max(self._shape[0], int(rows.max()) + 1), col + 1)
        return col

    def tocoo(self, problem=0):
        return sp.coo_matrix((self.data[problem], (self._rows, self._cols)), shape=(self.nrows, self.ncols))

    def tocsc(self, problem=0):
        return self.tocoo(problem).tocsc()

    def tocsr(self, problem=0):
        return self.tocoo(problem).tocsr()

    def tocsc_arrays(self):
        """(values [nproblems, nnz], row index, column pointer) as ``pycllp/lp.py:289-299``."""
        csc = self.tocsc()
        csc.sort_indices()
        order = np.lexsort((self._rows, self._cols))
        return (np.ascontiguousarray(self.data[:, order]), csc.indices.astype(np.int32),
                csc.indptr.astype(np.int32))

    def todense(self, problem=0):
        return np.asarray(self.tocoo(problem).todense())

    def term_order(self):
        """i64 [nnz]: the position in the coordinate lists of the q-th term of ``csr_term_order`` (a stable sort by row) --
        ``Aorder`` of ``pycllp_hip_general_to_bounded_batch``, which reads per-problem values ``data [B, nnz]`` as they are."""
        return np.argsort(self._rows, kind="stable")

    def csr_term_order(self, problem=0):
        """(data f64 [nnz], indptr i32 [nrows + 1], indices i32 [nnz]): the CSR arrays with the terms of a row in the order of
        the coordinate lists (a stable sort by row; duplicates stay apart) -- the order in which a product with this matrix sums
        them on the host, and what ``pycllp_hip_general_to_bounded`` takes."""
        order = self.term_order()
        indptr = np.concatenate([[0], np.cumsum(np.bincount(self._rows, minlength=self.nrows))])
        return (np.ascontiguousarray(self.data[problem][order], dtype=np.float64), indptr.astype(np.int32),
                self._cols[order].astype(np.int32))


class EqualityLP(object):
    """maximise c'x + f  subject to  A x = b, x >= 0   (``pycllp/lp.py:306-330``)."""

    def __init__(self, A=None, b=None, c=None, f=None):
        if A is None:
            self.A = SparseMatrix()
            self.b = np.zeros((1, 0)); self.c = np.zeros((1, 0)); self.f = np.zeros(1)
            return
        if b is None or c is None or f is None:
            raise ValueError("If A matrix is provided then b, c and f must also be provided.")
        if not isinstance(A, SparseMatrix):
            A = SparseMatrix(matrix=A)
        self.A = A
        self.b = np.array(b, dtype=np.float64)
        if self.b.ndim == 1:
            self.b = self.b.reshape(1, -1)
        nprb = self.b.shape[0]
        if A.nproblems > 1 and A.nproblems != nprb:
            raise ValueError("A matrix holds %d sets of values for %d problems: one shared set or one per problem." % (A.nproblems, nprb))
        self.c = np.array(c, dtype=np.float64)
        if self.c.ndim == 1:
            self.c = np.tile(self.c, (nprb, 1))
        if self.c.shape[0] != nprb:
            raise ValueError("A matrix and c array do not have the same number of problems.")
        self.f = np.full(nprb, float(f)) if np.isscalar(f) else np.array(f, dtype=np.float64)

    nrows = property(lambda self: self.A.nrows)
    ncols = property(lambda self: self.A.ncols)
    nnzeros = property(lambda self: self.A.nnzeros)
    nproblems = property(lambda self: self.b.shape[0])
    m = nrows
    n = ncols

    def add_col(self, rows, values, obj):
        """Append a variable with objective coefficient ``obj`` (scalar or per-problem)."""
        col = self.A.add_col(rows, values)
        o = np.broadcast_to(np.asarray(obj, dtype=np.float64), (self.nproblems,)).reshape(-1, 1)
        self.c = np.concatenate([self.c, o], axis=1)
        return col

    def init(self, solver, verbose=0):
        solver.init(self, verbose=verbose)

    def solve(self, solver, verbose=0):
        return solver.solve(self, verbose=verbose)


class StandardLP(EqualityLP):
    """maximise c'x + f  subject to  A x <= b, x >= 0."""

    def to_equality_form(self):
        """Copy and append one unit slack column (objective 0) per row (``pycllp/lp.py:551-567``)."""
        A = SparseMatrix(self.A._rows.copy(), self.A._cols.copy(), self.A.data.copy())   # per-problem values survive
        A._shape = (self.nrows, self.ncols)
        lp = EqualityLP(A, self.b.copy(), self.c.copy(), self.f.copy())
        for row in range(self.nrows):
            lp.add_col([row], [1.0], 0.0)
        return lp


class GeneralLP(StandardLP):
    """optimise c'x + f  subject to  a <= A x <= b,  l <= x <= u   (``pycllp/lp.py:570-623``; ``a`` defaults to "no lower
    bound on the rows", ``l`` to 0, ``u`` to +inf; 1-D bounds are repeated for every problem)."""

    def __init__(self, A=None, b=None, c=None, a=None, l=None, u=None, f=None):
        super(GeneralLP, self).__init__(A=A, b=b, c=c, f=f)
        if A is None:
            self.a = np.zeros((1, 0)); self.l = np.zeros((1, 0)); self.u = np.zeros((1, 0))
            return
        nprb = self.nproblems

        def rows_of(v, like, default):
            if v is None:
                return np.full(like.shape, default)
            v = np.array(v, dtype=np.float64)
            return np.tile(v, (nprb, 1)) if v.ndim == 1 else v

        self.a = rows_of(a, self.b, -np.inf)      # the reference stores +inf and drops the row again (lp.py:597-599, 511-529)
        self.l = rows_of(l, self.c, 0.0)
        self.u = rows_of(u, self.c, np.inf)

    def to_standard_form(self):
        """The StandardLP  max c'x + f', A' x <= b', x >= 0  with the same optimum (``pycllp/lp.py:725-792``):
        shift x <- x - l, write a <= A x as -A x <= -a, add x <= u - l for the finite upper bounds, and drop every row
        without a finite bound (``remove_unbounded``, ``pycllp/lp.py:511-529``).  A row, or an upper bound, that is finite
        for some problems of the batch and infinite for others raises ``ValueError`` exactly as the reference's
        ``remove_unbounded`` does (``lp.py:518-523``): a stand-in "big" bound would enter the relative tolerances
        (eps * (1 + |b|)) and the autoscale factors of that LP and ruin its solve."""
        if np.isneginf(self.l).any():
            raise ValueError('Lower bounds (l) contains -inf.')
        m, n, B = self.nrows, self.ncols, self.nproblems
        b, a, c, f = self.b.copy(), self.a.copy(), self.c.copy(), self.f.copy()
        l = self.l
        u = self.u - np.where(np.isfinite(self.u), l, 0.0)
        for k in range(B):
            Ak = self.A.tocsr(k if self.A.nproblems > 1 else 0)
            Al = Ak @ l[k]
            b[k] -= Al; a[k] -= Al
            f[k] += c[k] @ l[k]
        keep_lo = np.isfinite(a).any(axis=0)          # rows  -A x <= -a
        keep_hi = np.isfinite(b).any(axis=0)          # rows   A x <=  b
        keep_ub = np.isfinite(u).any(axis=0)          # rows     x <=  u - l
        for what, bound, keep in (("lower row bound a", a, keep_lo), ("row bound b", b, keep_hi), ("upper bound u", u, keep_ub)):
            mixed = keep & ~np.isfinite(bound).all(axis=0)
            if mixed.any():
                raise ValueError("Can not remove unbounded rows. %s of index %d is unbounded for some problems of the batch "
                                 "but not all." % (what, int(np.flatnonzero(mixed)[0])))
        rows, cols, data = [], [], []
        rhs = []
        r0 = 0
        for sign, keep, bound in ((-1.0, keep_lo, -a), (1.0, keep_hi, b)):
            newrow = np.cumsum(keep) - 1 + r0
            sel = keep[self.A._rows]
            rows.append(newrow[self.A._rows[sel]]); cols.append(self.A._cols[sel]); data.append(sign * self.A.data[:, sel])
            rhs.append(bound[:, keep])
            r0 += int(keep.sum())
        ub = np.flatnonzero(keep_ub)
        rows.append(r0 + np.arange(ub.size)); cols.append(ub); data.append(np.ones((self.A.data.shape[0], ub.size)))
        rhs.append(u[:, ub])
        bb = np.concatenate(rhs, axis=1)
        A2 = SparseMatrix(np.concatenate(rows), np.concatenate(cols), np.concatenate(data, axis=1))
        A2._shape = (bb.shape[1], n)
        return StandardLP(A2, bb, c, f)

    def check_bounds(self):
        """The ``ValueError``s of ``to_bounded_equality_form`` about single bounds: l = -inf, u < l, a > b."""
        if np.isneginf(self.l).any():
            raise ValueError('Lower bounds (l) contains -inf.')
        if (self.u < self.l).any():
            raise ValueError('Upper bounds (u) below lower bounds (l).')
        if (np.isfinite(self.a) & (self.a > self.b)).any():
            raise ValueError('Row lower bounds (a) above row upper bounds (b).')

    def bounded_structure(self, problem=None):
        """(A^, keep, sign): the part of ``to_bounded_equality_form`` that is one for the whole batch -- which rows are kept
        (``keep``: their indices; a row without a bound in every LP is dropped), with which sign (``sign``: +1.0 where b is
        finite for every LP, -1.0 where b = +inf and a is finite for every LP; any other mix raises ``ValueError``) and the
        matrix A^ = [+-A | I] as a ``SparseMatrix``.  It reads only which bounds are finite and A: a few reductions and work
        proportional to nnz, no product with l.  ``problem``: A^ with the values of that LP alone (what a handle is made from)
        instead of every LP's -- for per-problem values of A the work stays O(nnz), with no signed ``[B, nnz]`` copy."""
        m, n = self.nrows, self.ncols
        rows, cols, data = self.A._rows, self.A._cols, self.A.data
        if problem is not None and data.shape[0] > 1:
            data = data[problem:problem + 1]
        bfin, afin = np.isfinite(self.b), np.isfinite(self.a)
        plus = bfin.all(axis=0)
        minus = ~bfin.any(axis=0) & afin.all(axis=0)
        drop = ~bfin.any(axis=0) & ~afin.any(axis=0)
        mixed = ~(plus | minus | drop)
        if mixed.any():
            raise ValueError("Can not keep row %d in the bounded form: its bounds a, b are finite for some problems of the batch "
                             "but not all." % int(np.flatnonzero(mixed)[0]))
        keep = np.flatnonzero(plus | minus)
        sign = np.where(plus[keep], 1.0, -1.0)
        mk = keep.size
        newrow = np.full(m, -1, dtype=np.int64)
        newrow[keep] = np.arange(mk)
        sel = newrow[rows] >= 0
        rsign = sign[newrow[rows[sel]]]
        A2 = SparseMatrix(np.concatenate([newrow[rows[sel]], np.arange(mk)]), np.concatenate([cols[sel], n + np.arange(mk)]),
                          np.concatenate([rsign * data[:, sel], np.ones((data.shape[0], mk))], axis=1))
        A2._shape = (mk, n + mk)
        return A2, keep, sign

    def to_bounded_equality_form(self):
        """(``BoundedEqualityLP``, ``BoundedMap``): the LP  max c^'x^ + f^  s.t.  A^ x^ = b^,  0 <= x^ <= u^  with the same
        optimum, for the bounded kernel (``HipGeneralPrimalNormalSolver``).  Unlike ``to_standard_form`` it adds no row per upper
        bound and no second row per ranged or equality row:
          * x = l + x^:  b^ = b - A l,  a^ = a - A l,  f^ = f + c'l;
          * one sign per row for the whole batch: b finite for every LP keeps +A (its slack gets the upper bound b^ - a^, +inf
            where a is not finite, 0 for an equality row); b = +inf and a finite for every LP keeps -A with right-hand side
            -a^ and an unbounded slack; a row without either bound in every LP is dropped; any other mix raises ``ValueError``;
          * A^ = [+-A | I]: one +1 slack column per kept row, slacks last;  u^_j = u_j - l_j for the columns, +inf for none.
        u^ = 0 marks a fixed variable (a column with l == u, the slack of an equality row).  A non-finite ``a`` of either sign
        means "no lower bound" (the reference stores +inf there, this package -inf)."""
        self.check_bounds()
        m, n, B = self.nrows, self.ncols, self.nproblems
        rows, cols, data = self.A._rows, self.A._cols, self.A.data
        l = self.l
        # A l for every LP in one product: per-problem values (data [B, nnz]) or one shared set (data [1, nnz])
        S = sp.csr_matrix((np.ones(rows.size), (np.arange(rows.size), rows)), shape=(rows.size, m))
        Al = np.asarray((S.T @ (data * l[:, cols]).T).T)
        bh, ah = self.b - Al, self.a - Al
        f = self.f + (self.c * l).sum(axis=1)
        A2, keep, sign = self.bounded_structure()
        plus, mk = sign > 0, keep.size
        b2 = np.where(plus, bh[:, keep], -ah[:, keep])
        with np.errstate(invalid="ignore"):
            us = np.where(plus, np.where(np.isfinite(ah[:, keep]), bh[:, keep] - ah[:, keep], np.inf), np.inf)
        u2 = np.concatenate([np.where(np.isfinite(self.u), self.u - l, np.inf), us], axis=1)
        c2 = np.concatenate([self.c, np.zeros((B, mk))], axis=1)
        return BoundedEqualityLP(A2, b2, c2, f, u2), BoundedMap(l.copy(), keep, sign, m)


class BoundedEqualityLP(EqualityLP):
    """maximise c'x + f  subject to  A x = b,  0 <= x <= u   (u [nproblems, ncols]: +inf = no bound, 0 = fixed)."""

    def __init__(self, A=None, b=None, c=None, f=None, u=None):
        super(BoundedEqualityLP, self).__init__(A=A, b=b, c=c, f=f)
        self.u = np.full(self.c.shape, np.inf) if u is None else np.array(u, dtype=np.float64).reshape(self.c.shape)


def bounded_rowmap(keep, sign, m):
    """``keep`` and ``sign`` of ``GeneralLP.bounded_structure()`` as the one array the device conversion takes (i32 [m]): for
    row i of the GeneralLP k + 1 where it is row k of the bounded form with +A, -(k + 1) where with -A, 0 where it is dropped."""
    rowmap = np.zeros(m, dtype=np.int32)
    rowmap[keep] = np.where(np.asarray(sign) > 0, 1, -1) * (np.arange(len(keep)) + 1)
    return rowmap


GATHER_ONE = np.iinfo(np.int32).max      # "this slot holds 1.0" in a gather plan


def bounded_gather_coo(A, keep, sign):
    """The values of ``bounded_structure()``'s A^, entry by entry of its coordinate lists, as a gather from ONE LP's values of
    ``A`` (a ``SparseMatrix``; i32, one per entry of A^): t + 1 for +data[t], -(t + 1) for -data[t], ``GATHER_ONE`` for the 1.0
    of a slack column.  O(nnz): the plans of ``pycllp_hip_general_to_bounded_batch`` are made from it."""
    rows = np.asarray(A._rows)
    rsign = np.zeros(A.nrows, dtype=np.int64)
    rsign[keep] = np.where(np.asarray(sign) > 0, 1, -1)
    t = np.flatnonzero(rsign[rows] != 0)
    return np.concatenate([rsign[rows[t]] * (t + 1), np.full(len(keep), GATHER_ONE)]).astype(np.int32)


def bounded_gather_dense(A, keep, sign):
    """The gather plan (i32 [m' n]) of the dense ``[m', n]`` row-major image of the kept rows of +-A without the slack columns
    (0: the slot holds 0.0) -- ``bounded_matrices`` of ``hip_general_batch_primal_normal`` for one LP.  None where two entries
    of the structure share a (row, column): their sum is no gather."""
    rows, cols, n = np.asarray(A._rows), np.asarray(A._cols), A.ncols
    newrow = np.full(A.nrows, -1, dtype=np.int64)
    newrow[keep] = np.arange(len(keep))
    coo = bounded_gather_coo(A, keep, sign)
    coo = coo[:coo.size - len(keep)]                 # (without the slack columns' ones)
    t = np.abs(coo.astype(np.int64)) - 1
    flat = newrow[rows[t]] * n + cols[t]
    if np.unique(flat).size != flat.size:
        return None
    plan = np.zeros(len(keep) * n, dtype=np.int32)
    plan[flat] = coo
    return plan


def bounded_gather_csr(A, keep, sign, perm):
    """The gather plan (i32 [nnz of A^]) of the values of A^ = [+-A | I] in the CSR order ``perm`` of its structure
    (``sparse_general_batch.csr_structure`` of ``bounded_structure()``'s A^) -- ``bounded_values`` of
    ``hip_sparse_general_batch_primal_normal`` for one LP."""
    return np.ascontiguousarray(bounded_gather_coo(A, keep, sign)[np.asarray(perm)])


class BoundedMap(object):
    """Maps a solution of ``GeneralLP.to_bounded_equality_form()`` back to the GeneralLP's variables and rows."""

    def __init__(self, l, rows, sign, m):
        self.l, self.rows, self.sign, self.m = l, rows, sign, m

    def general(self, x, y, z=None, s=None):
        """(x, y, z, s) of the GeneralLP from x^, y^ (and the duals z^, s^ of x^ >= 0, x^ <= u^): x = l + x^ over the original
        columns, y per original row (sign restored, 0 for a dropped row), z / s the duals of x >= l / x <= u."""
        n = self.l.shape[1]
        x = self.l + np.asarray(x)[:, :n]
        yo = np.zeros((x.shape[0], self.m))
        yo[:, self.rows] = self.sign * np.asarray(y)
        return (x, yo, None if z is None else np.asarray(z)[:, :n].copy(), None if s is None else np.asarray(s)[:, :n].copy())
