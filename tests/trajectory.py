"""Trajectory parity (helpers, no tests): the iterate of a solve kernel after k iterations against the CPU reference's.

Every other comparison of a solve kernel with a reference happens at the converged optimum, and an interior-point method corrects
its own errors on the way there: a Gram product, step length or refinement that is wrong by 1e-10 ends at the same optimum after
the same number of iterations.  After k = 1, 2, 4, 8 iterations the iterate is the same mathematics in another summation order,
reproducible to 1e-14 .. 1e-12, so an error of that size shows.

A CASE is (kernel family, kind, point, mode).  ``reference(id)`` runs the oracle (oracle/port.py; tests/bounded_twin.py for the
bounded kinds) with ``max_iter = k``; ``tolerance(id)`` derives the bound from the reference alone: SPREAD = the largest
deviation, over the LPs of the batch, of the reference's own results on ``NPERM`` seeded row-and-column permutations of the same
LPs, mapped back; tol = max(FACTOR * spread, FLOOR) per k and quantity.  FACTOR = 32 because a kernel differs from the oracle in
more than summation order (FMA contraction, matrix-core accumulation order, A'y and rho carried incrementally, reciprocals by
Newton steps); FLOOR = 1e-13 (about 450 ulp) because a sample of four can land near zero.  ``kernel_results(case)`` runs the
same ladder on the GPU and returns what served each launch."""
import collections
import functools

import numpy as np

import bounded_twin
import test_kernel_variants as tkv
import test_workgroup_kernel_plans as twp
from pycllp_amd import problems
from pycllp_amd.lp import EqualityLP, GeneralLP, SparseMatrix, StandardLP
from test_general_solver import make_general
from test_sparse_general_solver import make_sparse_general

K = (1, 2, 4, 8)
K_SHORT = (1, 4)                      # warm start and autoscale rows
B, B_BIG = 24, 6                      # LPs per case; B_BIG at the large-LP kernel's points and the largest bounded one
NPERM, FACTOR, FLOOR, CEILING = 4, 32.0, 1e-13, 1e-9
WARM, GUARD, AUTOSCALE, NO_SLACK, BLOCK = 1, 4, 8, 16, 64          # PYCLLP_FLAG_*
ORACLE_FLAGS = dict(tkv.ORACLE_FLAGS, guard=0)
QUANTITIES = ("x", "y", "z", "pobj", "dobj")
# At the iteration limit the oracle and most kernels return the objectives of the iterate BEFORE the last step; the per-problem
# dense-A lane-group kernel stores c'x, b'y of the point it stores (tests/test_dense_batch.py test_trajectory).
STORES_ITS_OWN_OBJECTIVES = ("perA",)

# family, kind, point label, mode ('cold', 'warm', 'autoscale', 'degenerate'; the pair rows of tests/pair_cases.py also
# 'warm+autoscale', see ``modes``), the k ladder, input key (see ``inputs``), what
# must serve it (lane groups and wave kernel: the compiled shape; block and large-LP kernel: the case of
# test_workgroup_kernel_plans.py whose plan it is), extra solver flags, explicit margin {k: bound} with its cause
Case = collections.namedtuple("Case", "id family kind point mode ks key where flags margin cause")


# ---- inputs ---------------------------------------------------------------------------------------------------------------
def _frozen(lp):
    for a in (lp.b, lp.c):
        a.setflags(write=False)
    return lp


def head(lp, n):
    """The first n LPs of an EqualityLP batch (per-problem values of A included)."""
    if lp.A.nproblems > 1:
        A = SparseMatrix(np.asarray(lp.A._rows), np.asarray(lp.A._cols), np.asarray(lp.A.data)[:n])
        A._shape = (lp.nrows, lp.ncols)
    else:
        A = lp.A
    return EqualityLP(A, lp.b[:n].copy(), lp.c[:n].copy(), 0.0)


def degenerate(lp):
    """LPs on the matrix of ``lp`` with its last row replaced by row 3 + 1e-6 noise (a sparse A: noise = the row it replaces, so
    the structure is the union of the two), around a strictly feasible primal-dual pair of the new matrix as ``equality_lp``
    builds them: M = A D A' is singular to 1e-12, the pivot floor is active and refinement runs to its cap at every iteration,
    while b stays in the range of A, so x is reproducible."""
    A = np.array(lp.A.todense(), dtype=np.float64)
    nb, (m, N) = lp.nproblems, A.shape
    rs = np.random.RandomState(31)
    A[-1] = A[3] + 1e-6 * (rs.randn(N) if (A != 0).mean() > 0.5 else A[-1])
    x0, y0 = rs.rand(nb, N) + 0.1, rs.randn(nb, m)
    b, c = x0 @ A.T, y0 @ A - (rs.rand(nb, N) + 0.1)
    b /= np.abs(b).max(axis=1, keepdims=True)
    c /= np.abs(c).max(axis=1, keepdims=True)
    return EqualityLP(SparseMatrix(matrix=A), b, c, 0.0)


def bounded_general(key):
    """(the GeneralLP batch of a bounded input key, the point x0 strictly inside [l, u] its row bounds are built around)."""
    what = key[0]
    if what in MORE_BOUNDED:                                 # per-problem matrices (tests/bounded_cases.py): not banded
        return MORE_BOUNDED[what](key)
    if what == "bounded-dense":
        _, mk, n, nb, seed = key
        glp, x0 = make_general(mk, n, nb, seed=seed, mixed_u=True, fixed=2, with_x0=True)
    elif what == "bounded-sparse":
        _, mk, n, nb, density, seed = key
        kinds = tkv.bounded_kinds(mk)
        glp, x0 = make_sparse_general(len(kinds), n, nb, seed, density=density, fixed=2, mixed_u=True, kinds=kinds, with_x0=True)
    elif what == "bounded-image":
        _, mk, n, nb, seed = key
        kinds = tkv.bounded_kinds(mk)
        glp, x0 = make_general(len(kinds), n, nb, seed, kinds=kinds, fixed=2, mixed_u=True, with_x0=True)
    else:
        raise KeyError(key)
    return tkv.banded(glp), x0


def degenerate_bounded(glp, x0, seed=36):
    """The GeneralLP batch ``glp`` (one matrix, or one per LP) with its last kept row replaced by row 3 + 1e-6 noise (a sparse A:
    noise = the row it replaces, as in ``degenerate``; a matrix per LP: its own noise) and both rows made equality rows through
    x0, the interior point the batch is built around: a = b = A x0 there.  Bounds, fixed columns and costs stay.  The slacks of
    the two rows are fixed, so M = A^ D A^' is singular to 1e-12 as in ``degenerate``, and b^ stays in the range of A^.
    Refinement stagnates on such a matrix (an LP spends all its passes or none), at a residual of 1e-9 .. 1e-7 (1 + |b|) that
    the noise decides; ``seed`` is one under which every input of tests/bounded_cases.py has, at every k, an LP below
    1e-8 (1 + |b|), so that refine_tol = 1e-8 is a row of its own (test_bounded_options.py asserts it)."""
    P = glp.A.nproblems
    A = np.stack([np.asarray(glp.A.todense(i) if P > 1 else glp.A.todense(), dtype=np.float64) for i in range(P)])
    kept = np.flatnonzero(np.isfinite(glp.a).any(axis=0) | np.isfinite(glp.b).any(axis=0))
    last = int(kept[-1])
    assert 3 in kept and last > 3
    rs = np.random.RandomState(seed)
    A[:, last] = A[:, 3] + 1e-6 * (rs.randn(P, A.shape[2]) if (A != 0).mean() > 0.5 else A[:, last])
    a, b = glp.a.copy(), glp.b.copy()
    for i in (3, last):
        a[:, i] = b[:, i] = (A[:, i] * x0).sum(axis=1)
    if P > 1:
        m, n = A.shape[1:]
        Asp = SparseMatrix(np.repeat(np.arange(m), n), np.tile(np.arange(n), m), A.reshape(P, -1))
        Asp._shape = (m, n)
    else:
        Asp = SparseMatrix(matrix=A[0])
    return GeneralLP(Asp, b, glp.c.copy(), a=a, l=glp.l.copy(), u=glp.u.copy(), f=np.array(glp.f))


def image_bounded_rows(n, shape):
    """The most kept rows (<= 16 MB) of a dense bounded form with n columns whose image fits beside one wave area of the
    bounded kernel while its term tables do not: the bounded case of a dense-image point 'at its own kept-row count'."""
    return max(mk for mk in range(1, 16 * shape[0] + 1)
               if tkv.image_waves(mk, mk + n, True, shape, True) and tkv.tables_cannot_fit(mk, mk + n, True, shape, True)
               and tkv.first_covering("image", tkv.WAVE_DA_SHAPES, mk, mk + n) == shape)


@functools.lru_cache(maxsize=None)
def inputs(key):
    """The LP batch of an input key (shared by the cases that solve the same LPs; read-only)."""
    what = key[0]
    if what == "standard":                                   # dense standard form m x n -> equality form with identity tail
        _, m, n, nb, seed = key
        A, b, c = problems.random_dense_arrays(m, n, nb, seed=seed)
        return _frozen(StandardLP(SparseMatrix(matrix=A), b, c, 0.0).to_equality_form())
    if what == "equality":                                   # dense equality form without tail
        _, m, N, nb, seed = key
        return _frozen(tkv.equality_lp(m, N, nb, seed))
    if what == "sparse":                                     # sparse standard form, shared or per-problem values
        _, m, n, nb, density, seed, pa = key
        A, b, c = problems.random_sparse_arrays(m, n, nb, density=density, seed=seed)
        if pa:
            rows, cols, data = problems.per_problem_values(A, nb, seed=seed + 2)
            return _frozen(StandardLP(SparseMatrix(rows, cols, data), b, c, 0.0).to_equality_form())
        return _frozen(StandardLP(SparseMatrix(matrix=A), b, c, 0.0).to_equality_form())
    if what == "sparse-equality":                            # sparse equality form without tail
        _, m, N, nb, per_col, seed = key
        return _frozen(twp.sparse_equality_lp(m, N, nb, per_col, seed))
    if what == "variants":                                   # a point of test_kernel_variants.py
        case = key[1]
        lp = tkv.make_case(case)
        if case[2] == "bounded":
            from pycllp_amd.solvers.general import subset
            return subset(lp, np.arange(min(B, lp.nproblems)))
        return _frozen(head(lp, min(B, lp.nproblems)))
    if what == "plans":                                      # a point of test_workgroup_kernel_plans.py
        case = key[1]
        lp = twp.make_case(case)
        return _frozen(head(lp, min(B_BIG if case[0] == "big" else B, lp.nproblems)))
    if what in ("bounded-dense", "bounded-sparse", "bounded-image"):
        return bounded_general(key)[0]
    if what == "degenerate-bounded":
        return degenerate_bounded(*bounded_general(key[1]))
    if what == "degenerate":
        return _frozen(degenerate(inputs(key[1])))
    if what in MORE_INPUTS:                                  # input keys of tests/option_cases.py
        return MORE_INPUTS[what](key)
    if what == "scaled":                                     # the same LPs with b 1e3 and c 1e-2: what autoscale is for
        lp = inputs(key[1])
        return _frozen(EqualityLP(lp.A, lp.b * 1e3, lp.c * 1e-2, 0.0))
    raise KeyError(key)


MORE_INPUTS = {}
MORE_BOUNDED = {}                                            # input keys that ``bounded_general`` takes from elsewhere
Problem = collections.namedtuple("Problem", "A b c u f bmap shared tail")


@functools.lru_cache(maxsize=None)
def problem(key, bounded):
    """The arrays the references take: A [m, N] (or one per LP), b, c, u (bounded), the objective offset and the map back to
    the GeneralLP's variables (bounded); ``tail``: the last m columns of A are the identity."""
    lp = inputs(key)
    if bounded:
        blp, bmap = lp.to_bounded_equality_form()
        shared = blp.A.nproblems == 1
        As = (np.asarray(blp.A.todense(), dtype=np.float64),) if shared else \
            tuple(np.asarray(blp.A.todense(i), dtype=np.float64) for i in range(blp.nproblems))
        return Problem(As, blp.b, blp.c, blp.u, np.broadcast_to(blp.f, (blp.nproblems,)), bmap, shared, True)
    shared = lp.A.nproblems == 1
    As = tuple(np.asarray(lp.A.todense(i), dtype=np.float64) for i in range(lp.nproblems)) if not shared else \
        (np.asarray(lp.A.todense(), dtype=np.float64),)
    m, N = As[0].shape
    tail = N > m and all(np.array_equal(A[:, N - m:], np.eye(m)) for A in As)
    return Problem(As, lp.b, lp.c, None, np.zeros(lp.nproblems), None, shared, tail)


def warm_point(nb, m, N):
    """Seeded x0, z0 in [0.5, 1.5] and y0 ~ N(0, 1)."""
    rs = np.random.RandomState(77)
    return 0.5 + rs.rand(nb, N), rs.randn(nb, m), 0.5 + rs.rand(nb, N)


def modes(case):
    """The start and scaling options of a case: the subset of {'warm', 'autoscale'} its mode names -- one of them, or both
    joined by '+' (tests/pair_cases.py)."""
    return frozenset(case.mode.split("+")) & {"warm", "autoscale"}


def start_point(case, P):
    """x0, y0, z0 of a warm case: ``warm_point``, and under autoscale that point scaled with the data -- x0 max|b_k|,
    y0 max|c_k|, z0 max|c_k| per LP -- so that after the solver's division the start is the well-conditioned ``warm_point``
    itself and the three divisions are what the case tests."""
    nb, (m, N) = P.b.shape[0], P.A[0].shape
    x0, y0, z0 = warm_point(nb, m, N)
    if "autoscale" in modes(case):
        sb, sc = np.abs(P.b).max(axis=1, keepdims=True), np.abs(P.c).max(axis=1, keepdims=True)
        x0, y0, z0 = x0 * sb, y0 * sc, z0 * sc
    return x0, y0, z0


def probe_entry(P):
    """(row, column) of the entry of A the 'must bite' test scales: the last structural entry (before an identity tail) of the
    last row that has one -- the edge of a ragged case.  Entries below 1e-3 max|A| do not count (the noise of a degenerate
    case)."""
    A = P.A[0]
    m, N = A.shape
    nd = N - m if P.tail else N
    for i in range(m - 1, -1, -1):
        nz = np.flatnonzero(np.abs(A[i, :nd]) > 1e-3 * np.abs(A).max())
        if nz.size:
            return i, int(nz[-1])
    raise ValueError("A has no structural entry")


# ---- the reference --------------------------------------------------------------------------------------------------------
def run_reference(case, k, perm=None, r_scale=1.0, a_scale=1.0, start=None, **opts):
    """The reference's results after k iterations: dict(x, y, z[, s], pobj, dobj, status, iters, nrefs, aty; a bounded case: also
    the twin's floored and guard_ratio, aty over the GeneralLP's own columns, a matrix per LP where the case has one).  ``perm``: seed of
    a row-and-column permutation under which the LPs are solved (results mapped back); ``r_scale``: factor on the step
    fraction r; ``a_scale``: factor on ``probe_entry`` of A; ``opts``: further fields of the oracle's options (``r``: the step
    fraction ``r_scale`` multiplies, default 0.9); ``start``: (x0, y0, z0) a warm case starts from in place
    of ``start_point``."""
    from oracle import port
    bounded = case.kind == "bounded"
    P = problem(case.key, bounded)
    m, N = P.A[0].shape
    nb = P.b.shape[0]
    opts = dict(opts)
    r_frac = opts.pop("r", 0.9) * r_scale
    rows, cols = np.arange(m), np.arange(N)
    if perm is not None:
        rs = np.random.RandomState(1000 + perm)
        rows, cols = rs.permutation(m), rs.permutation(N)
        if case.mode == "degenerate":
            # The order of elimination decides which of the two near-dependent rows meets the pivot floor, and the floored factor
            # is the factor of another matrix: the reference under a row permutation is another computation (its x moves by
            # 1e-9 .. 1e-5), not the same one in another summation order.  A kernel eliminates in the oracle's row order, so only
            # the columns -- the summation order of the Gram product, of A x and of A'y -- are permuted.
            rows = np.arange(m)
    As = [A.copy() for A in P.A]
    if a_scale != 1.0:
        i, j = probe_entry(P)
        for A in As:
            A[i, j] *= a_scale
    As = [np.ascontiguousarray(A[rows][:, cols]) for A in As]
    b, c = P.b[:, rows], P.c[:, cols]
    if bounded:
        u = P.u[:, cols]
        if P.shared:
            r = bounded_twin.solve(As[0], b, c, u, max_iter=k, r=r_frac, **opts)
        else:
            each = [bounded_twin.solve(As[i], b[i:i + 1], c[i:i + 1], u[i:i + 1], max_iter=k, r=r_frac, **opts) for i in range(nb)]
            r = {q: np.concatenate([e[q] for e in each]) for q in each[0]}
    else:
        flags = ORACLE_FLAGS[case.kind] | (AUTOSCALE if "autoscale" in modes(case) else 0)
        x0, y0, z0 = (start_point(case, P) if start is None else start) if "warm" in modes(case) else (None,) * 3
        start = {}
        if x0 is not None:
            start, flags = dict(x0=x0[:, cols], y0=y0[:, rows], z0=z0[:, cols]), flags | WARM
        opts = dict(opts, max_iter=k, r=r_frac, flags=flags)
        if P.shared:
            r = port.dense_solve(As[0], b, c, nthreads=8, **start, **opts)
        else:
            each = [port.dense_solve(As[i], b[i:i + 1], c[i:i + 1], **{q: v[i:i + 1] for q, v in start.items()}, **opts)
                    for i in range(nb)]
            r = {q: np.concatenate([e[q] for e in each]) for q in each[0]}
    out = dict(status=r["status"], iters=r["iters"], nrefs=r["nrefs"], pobj=r["pobj"] + P.f, dobj=r["dobj"] + P.f)
    inv_r, inv_c = np.argsort(rows), np.argsort(cols)
    for q in ("x", "z", "s"):
        if q in r:
            out[q] = r[q][:, inv_c]
    out["y"] = r["y"][:, inv_r]
    out["aty"] = a_transpose_y(P, out["y"])
    if case.family in STORES_ITS_OWN_OBJECTIVES:
        out["pobj"], out["dobj"] = (P.c * out["x"]).sum(axis=1), (P.b * out["y"]).sum(axis=1)
    if bounded:
        # A^'y^ over the GeneralLP's own columns: over a slack column it is y^ itself, which a degenerate case does not determine
        out["aty"] = out["aty"][:, :P.bmap.l.shape[1]]
        out["floored"], out["guard_ratio"] = r["floored"], r["guard_ratio"]
        out["x"], out["y"], out["z"], out["s"] = P.bmap.general(out["x"], out["y"], out["z"], out["s"])
    return out


def a_transpose_y(P, y):
    return np.stack([P.A[0 if P.shared else i].T @ y[i] for i in range(y.shape[0])])


def quantities(case):
    if case.mode == "degenerate":
        # y along the near-dependent direction is not determined (spread ~ 1e-7)
        return ("x", "z", "s", "aty") if case.kind == "bounded" else ("x", "z", "aty")
    return QUANTITIES + (("s",) if case.kind == "bounded" else ())


def deviation(a, ref):
    """Per LP: max|a - ref| / max|ref| of a vector (max|ref| = 0: absolute), |a - ref| / (1 + |ref|) of an objective."""
    a, ref = np.asarray(a, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    if ref.ndim == 1:
        return np.abs(a - ref) / (1.0 + np.abs(ref))
    scale = np.abs(ref).max(axis=1)
    return np.abs(a - ref).max(axis=1) / np.where(scale > 0, scale, 1.0)


def option_key(opts):
    """Solver options as the hashable the caches below take."""
    return tuple(sorted(dict(opts).items()))


@functools.lru_cache(maxsize=None)
def _reference_at(cid, k, opts):
    out = run_reference(BY_ID[cid], k, **dict(opts))
    for a in out.values():
        a.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def _spread_at(cid, k, opts):
    case = BY_ID[cid]
    ref = _reference_at(cid, k, opts)
    runs = [run_reference(case, k, perm=p, **dict(opts)) for p in range(NPERM)]
    return {q: max(float(deviation(r[q], ref[q]).max()) for r in runs) for q in quantities(case)}


def reference(cid, opts=(), ks=None):
    """{k: the reference's results} of a case under the options ``opts`` (``option_key``), each computed once (read-only);
    ``ks``: the iteration counts, default the case's ladder."""
    return {k: _reference_at(cid, k, opts) for k in (BY_ID[cid].ks if ks is None else ks)}


def spread(cid, opts=(), ks=None):
    """{k: {quantity: largest deviation of the reference under NPERM permutations, over the LPs of the batch}}"""
    return {k: _spread_at(cid, k, opts) for k in (BY_ID[cid].ks if ks is None else ks)}


def tolerance(cid, opts=(), ks=None):
    """{k: {quantity: bound}}: max(FACTOR spread, FLOOR), or the case's explicit margin (never above CEILING)."""
    case = BY_ID[cid]
    out = {}
    for k, sp in spread(cid, opts, ks).items():
        out[k] = {q: max(FACTOR * v, FLOOR) for q, v in sp.items()}
        if case.margin and k in case.margin:
            assert case.cause and case.margin[k] <= CEILING
            out[k] = {q: max(t, case.margin[k]) for q, t in out[k].items()}
    return out


# ---- the GPU --------------------------------------------------------------------------------------------------------------
# family of a bounded case -> (the plugin that solves it, the ``kernel`` it must report); 'perA-*': a matrix per LP
BOUNDED_PLUGINS = {"slack": ("hip_general_primal_normal", "bounded group"),
                   "tables": ("hip_sparse_general_primal_normal", "bounded wave"),
                   "image": ("hip_sparse_general_primal_normal", "bounded wave"),
                   "perA-group": ("hip_general_batch_primal_normal", "bounded group per-problem"),
                   "perA-wave": ("hip_sparse_general_batch_primal_normal", "bounded wave per-problem")}


def assert_served(case, info, lp, solver):
    if case.kind == "bounded":
        assert solver.kernel == BOUNDED_PLUGINS[case.family][1], solver.kernel
    if case.family.startswith("perA-"):                      # the compiled shape: lane groups (MP, NP), wave kernel (MB, NQ)
        assert info.get("group_shape" if case.family == "perA-group" else "wave_shape") == case.where, info
    elif case.where is None:                                # the block kernel by flag, whatever its plan
        assert info.get("kernel") == "block" and "wave_shape" not in info, info
    elif case.family in ("block", "big"):
        twp.assert_served_by(info, case.where, lp, grid=lp.nproblems)
    else:
        tkv.assert_served_by(info, (case.family, case.where))


def solver_options(case):
    kind = case.kind
    return dict(hsd=kind.endswith("hsd"), predcorr=kind.endswith("pc"), autoscale="autoscale" in modes(case),
                **({"flags": case.flags} if case.flags else {}))


def kernel_results(case, ks=None, seen=None, **opts):
    """{k: results of the kernel after k iterations} in the layout of ``run_reference``; every launch asserts what served it.
    ``ks``: the iteration limits (default the case's ladder); ``seen``: a list that receives ``launch_info()`` of every launch;
    ``opts``: further fields of ``pycllp_hip_opts``."""
    import torch
    from pycllp_amd.solvers import solver_registry
    lp = inputs(case.key)
    ks = case.ks if ks is None else ks
    out = {}
    if case.kind == "bounded":
        P = problem(case.key, True)
        name = BOUNDED_PLUGINS[case.family][0]
        n = P.bmap.l.shape[1]
        for k in ks:
            s = solver_registry[name](device="cuda:0", hsd=False, autoscale=False, max_iter=k,
                                      **dict({"flags": case.flags} if case.flags else {}, **opts))
            lp.init(s)
            lp.solve(s)
            assert_served(case, s.launch_info(), lp, s)
            if seen is not None:
                seen.append(s.launch_info())
            out[k] = dict(x=s.x, y=s.y, z=s.z, s=s.s, pobj=s.primal_obj, dobj=s.dual_obj, status=s.status, iters=s.iters)
            out[k]["aty"] = a_transpose_y(P, P.bmap.sign * np.asarray(s.y)[:, P.bmap.rows])[:, :n]
        return out
    P = problem(case.key, False)
    dense = case.family in ("slack", "group") or (case.family == "big" and case.where[2] == "mfma")
    name = "hip_dense_primal_normal" if dense else "hip_sparse_primal_normal"
    s = solver_registry[name](device="cuda:0", max_iter=1, **solver_options(case))
    lp.init(s)
    if not P.shared:
        lp.solve(s)                                        # uploads the per-problem values of A (one iteration)
    warm = "warm" in modes(case)
    for k in ks:
        if warm:
            if "set0" not in s.buffers:
                s.solve_device(lp.b, lp.c, max_iter=1)     # allocates the result buffers a warm start reads
            for q, v in zip(("x", "y", "z"), start_point(case, P)):
                s.buffers["set0"][q].copy_(torch.as_tensor(v, device="cuda:0"))
        g = s.solve_device(lp.b, lp.c, warm_start=warm, max_iter=k, **opts)
        torch.cuda.synchronize()
        assert_served(case, s.launch_info(), lp, s)
        if seen is not None:
            seen.append(s.launch_info())
        out[k] = {q: g[q].cpu().numpy() for q in ("x", "y", "z", "pobj", "dobj", "status", "iters")}
        out[k]["aty"] = a_transpose_y(P, out[k]["y"])
    return out


def measured(case, got):
    """{k: {quantity: the kernel's largest deviation from the reference over the LPs}}; 'c'x' -- whether the kernel's pobj is
    c'x of the x it returns (deviation of the two)."""
    ref = reference(case.id)
    P = problem(case.key, case.kind == "bounded")
    out = {}
    for k in case.ks:
        out[k] = {q: float(deviation(got[k][q], ref[k][q]).max()) for q in quantities(case)}
        if case.kind != "bounded":
            out[k]["pobj-c'x"] = float(deviation(got[k]["pobj"], (P.c * got[k]["x"]).sum(axis=1)).max())
    return out


def assert_on_trajectory(case, got):
    ref, tol = reference(case.id), tolerance(case.id)
    dev = measured(case, got)
    for k in case.ks:
        print("%s k=%d %s" % (case.id, k, "  ".join("%s %.1e (tol %.1e)" % (q, dev[k][q], tol[k][q]) for q in quantities(case))))
    for k in case.ks:
        for side in (got[k], ref[k]):
            assert (side["status"] == 5).all() and (side["iters"] == k).all(), (k, side["status"], side["iters"])
        for q in quantities(case):
            d = deviation(got[k][q], ref[k][q])
            assert d.shape == (ref[k]["status"].size,)                       # every LP of the batch
            assert d.max() <= tol[k][q], "%s after %d iterations: %s off by %.2e on LP %d (bound %.2e)" % (
                case.id, k, q, d.max(), int(d.argmax()), tol[k][q])


# ---- the case table -------------------------------------------------------------------------------------------------------
def _plans_case(family, where, gram, kind, point):
    for c in twp.CASES:
        if c[:5] == (family, where, gram, kind, point):
            return c
    raise KeyError((family, where, gram, kind, point))


def smallest_big_points():
    """{(gram, factor_in_lds): (cell, point)}: of the large-LP kernel's cells, per Gram path and factor storage the point with
    the smallest m^2 N that has a column to spare per row (N >= 2 m; a nearly square LP is decided within the first
    iterations)."""
    out = {}
    for gram in twp.GRAMS:
        for factor in ("W", "L"):
            pts = [c for c in twp.CASES if c[0] == "big" and c[2] == gram and c[1][0] == factor and c[3] == "plain"
                   and c[6] >= 2 * c[5]]
            c = min(pts, key=lambda c: (c[5] * c[5] * c[6], c[6]))
            out[(gram, factor == "L")] = (c[1], c[4])
    return out


# Cases whose ladder stops at k = 4: at k = 8 the reference's own spread has grown so far that one entry of A off by 1e-8 (or the
# step fraction off by 1e-9) no longer moves x by twice the tolerance -- the comparison would not bite there
# (test_tolerance_bites), so the k is dropped rather than the perturbation shrunk.  The predictor-corrector ladders of the
# degenerate cases stop there too: at k = 8 their spread times FACTOR passes CEILING.
STOPS_AT_4 = ("tables-40x90-plain", "tables-33x193-pa-hsd", "big-mfma-W3x3-97x513-hsd", "big-mfma-W3x3-97x513-pc",
              "big-mfma-L3x3-8x513-pc", "group-32x96-pc-degenerate", "image-40x100-pc-degenerate",
              "big-mfma-L3x3-8x513-pc-degenerate")


def build_cases():
    cases = []

    def add(family, kind, point, key, where, mode="cold", ks=K, flags=0, margin=None, cause=""):
        cid = "-".join([family, point, kind] + ([mode] if mode != "cold" else []))
        if cid in STOPS_AT_4:
            ks = tuple(k for k in ks if k <= 4)
        cases.append(Case(cid, family, kind, point, mode, ks, key, where, flags, margin, cause))

    def extras(family, point, key, where, flags=0, autoscale_kinds=("plain", "hsd")):
        add(family, "plain", point, key, where, mode="warm", ks=K_SHORT, flags=flags)
        for kind in autoscale_kinds:
            add(family, kind, point, ("scaled", key), where, mode="autoscale", ks=K_SHORT, flags=flags)

    cover = tkv.first_covering
    # lane groups, slack-aware: standard form m x n
    for m, n in ((32, 64), (16, 32), (20, 30)):
        key, where = ("standard", m, n, B, 100 * m + n), cover("slack", tkv.GROUP_SHAPES, m, m + n)
        for kind in ("plain", "hsd", "pc"):
            add("slack", kind, "%dx%d" % (m, n), key, where)
        if (m, n) == (32, 64):
            add("slack", "guard", "32x64", key, where, flags=GUARD)                  # PYCLLP_FLAG_FORCE_GUARD_PATH
            add("slack", "bounded", "24x30", ("bounded-dense", 24, 30, B, 2430), cover("slack", tkv.GROUP_SHAPES, 24, 54))
            extras("slack", "32x64", key, where)
    # lane groups, general kernels: no identity tail
    for m, N in ((32, 96), (17, 33)):
        key, where = ("equality", m, N, B, 100 * m + N), cover("group", tkv.GROUP_SHAPES, m, N)
        for kind in ("plain", "hsd", "pc"):
            add("group", kind, "%dx%d" % (m, N), key, where, flags=NO_SLACK)
        if (m, N) == (32, 96):
            extras("group", "32x96", key, where, flags=NO_SLACK)
            add("group", "plain", "32x96", ("degenerate", key), where, mode="degenerate", flags=NO_SLACK)
            add("group", "pc", "32x96", ("degenerate", key), where, mode="degenerate", flags=NO_SLACK)
    # wave kernel, term tables: the ragged point of shape (3, 4); 40 x 90 at density 0.1
    ragged = [c for c in tkv.CASES if c[0] == "tables" and c[1] == (3, 4) and c[3] == "ragged"]
    for kind in ("plain", "hsd", "pc", "pa", "pa-hsd", "pa-pc", "bounded"):
        c = next(c for c in ragged if c[2] == kind)
        add("tables", kind, "%dx%d" % (c[4], c[5]), ("variants", c), (3, 4))
        if kind == "bounded":
            key = ("bounded-sparse", 40, 90, B, 0.1, 4090)
        else:
            key = ("sparse", 40, 90, B, 0.1, 5, kind.startswith("pa"))
        add("tables", kind, "40x90", key, cover("tables", tkv.WAVE_TAB_SHAPES, 40, 130))
    key, where = ("sparse", 40, 90, B, 0.1, 5, False), cover("tables", tkv.WAVE_TAB_SHAPES, 40, 130)
    extras("tables", "40x90", key, where)
    key, where = ("sparse-equality", 40, 90, B, 3, 4091), cover("tables", tkv.WAVE_TAB_SHAPES, 40, 90)
    for kind in ("plain", "pc"):
        add("tables", kind, "40x90-no-tail", ("degenerate", key), where, mode="degenerate")
    add("block", "plain", "40x90-no-tail", ("degenerate", key), None, mode="degenerate", flags=BLOCK)
    # wave kernel, dense image: 100 x 80 standard, 40 x 100 equality without tail
    key, where = ("standard", 100, 80, B, 10080), cover("image", tkv.WAVE_DA_SHAPES, 100, 180)
    for kind in ("plain", "hsd", "pc"):
        add("image", kind, "100x80", key, where)
    mk = image_bounded_rows(80, where)
    add("image", "bounded", "%dx80" % mk, ("bounded-image", mk, 80, B_BIG, 10080), where)   # (the numpy twin costs ~ m^3 per LP)
    extras("image", "100x80", key, where)
    key, where = ("equality", 40, 100, B, 40100), cover("image", tkv.WAVE_DA_SHAPES, 40, 100)
    for kind in ("plain", "hsd", "pc"):
        add("image", kind, "40x100", key, where)
    for kind in ("plain", "pc"):
        add("image", kind, "40x100", ("degenerate", key), where, mode="degenerate")
    # block kernel: the smallest point of each LDS plan
    for plan, kinds in (("lds-paired", ("plain", "hsd", "pa", "pa-hsd")), ("l2", ("plain", "hsd"))):
        for kind in kinds:
            c = _plans_case("block", plan, None, kind, "ragged")
            add("block", kind, "%s-%dx%d" % (plan, c[5], c[6]), ("plans", c), c, flags=BLOCK if plan != "l2" else 0)
        c = _plans_case("block", plan, None, "plain", "ragged")
        extras("block", "%s-%dx%d" % (plan, c[5], c[6]), ("plans", c), c, flags=BLOCK if plan != "l2" else 0)
    # large-LP kernel: the smallest point per Gram path and factor storage
    for (gram, in_lds), (cell, point) in sorted(smallest_big_points().items()):
        for kind in ("plain", "hsd", "pc"):
            c = _plans_case("big", cell, gram, kind, point)
            add("big", kind, "%s-%s-%dx%d" % (gram, twp.cell_name(cell), c[5], c[6]), ("plans", c), c)
        if in_lds:
            c = _plans_case("big", cell, gram, "plain", point)
            extras("big", "%s-%s-%dx%d" % (gram, twp.cell_name(cell), c[5], c[6]), ("plans", c), c)
        if gram == "mfma" and in_lds and twp.big_form(c) == "equality":          # (built without a tail: the degenerate case too)
            for kind in ("plain", "pc"):
                c = _plans_case("big", cell, gram, kind, point)
                add("big", kind, "%s-%s-%dx%d" % (gram, twp.cell_name(cell), c[5], c[6]), ("degenerate", ("plans", c)), c,
                    mode="degenerate")
    return cases


CASES = build_cases()
BY_ID = {c.id: c for c in CASES}
assert len(BY_ID) == len(CASES)


def register(case):
    """Make a case that is no row of ``CASES`` (tests/option_cases.py) known to ``reference``, ``spread`` and ``tolerance``."""
    assert BY_ID.setdefault(case.id, case) == case, case.id
    return case
