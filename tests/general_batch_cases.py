"""Helpers of tests/test_general_batch.py (no tests): GeneralLP batches in which every LP has its own dense matrix, the bounded
twin run LP by LP with that LP's own matrix, the project's parity bounds, and the trajectory references with their tolerances
(the rule of tests/trajectory.py)."""
import functools

import numpy as np

import bounded_twin
from pycllp_amd.lp import GeneralLP, SparseMatrix
from test_general_solver import NATIVE_SIZES, SHAPES, make_general

GROUP_SHAPES = list(SHAPES)
B_EVERY = 37
OUTPUTS = ("x", "y", "z", "s", "pobj", "dobj", "status", "iters")
SMALLEST = dict(NATIVE_SIZES)                                          # shape -> (m', n): the smallest sizes of the bounded tests
FULL = {s: (s[0], s[1] - s[0]) for s in GROUP_SHAPES}                  # no pad row, no pad column, every lane carries a row


def kinds(mk):
    return ["le"] + [("eq", "rng", "le", "ge")[i % 4] for i in range(mk - 1)]


def first_covering(mk, n):
    """The slack-aware shape that serves a bounded form of mk kept rows and n columns before the slacks."""
    for s in GROUP_SHAPES:
        if mk <= s[0] and n <= s[1] - s[0]:
            return s
    return None


@functools.lru_cache(maxsize=None)
def make(mk, n, B=B_EVERY, seed=None, with_x0=False):
    """The batch of a test (shared, read-only): mk kept rows, n columns, every LP with its own matrix.  ``with_x0``: (the
    batch, the interior point its row bounds are built around)."""
    seed = 300 + sum(first_covering(mk, n)) if seed is None else seed
    glp, x0 = make_general(mk, n, B, seed, per_problem_A=True, fixed=1, mixed_u=True, kinds=kinds(mk), with_x0=True)
    for a in (glp.a, glp.b, glp.c, glp.l, glp.u, glp.A.data, x0):
        a.setflags(write=False)
    return (glp, x0) if with_x0 else glp


def scaled_rows(glp, factor):
    """The same LPs with LP k's matrix and row bounds times factor[k] (> 0): other values of A_k, the same optimum."""
    fk = np.asarray(factor, dtype=np.float64)[:, None]
    A = SparseMatrix(np.asarray(glp.A._rows).copy(), np.asarray(glp.A._cols).copy(), np.asarray(glp.A.data) * fk)
    A._shape = (glp.nrows, glp.ncols)
    return GeneralLP(A, glp.b * fk, glp.c.copy(), a=glp.a * fk, l=glp.l.copy(), u=glp.u.copy(), f=glp.f.copy())


def scaled_data(glp, sb, sc):
    """b, a, l, u times sb and c times sc: what autoscale is for."""
    A = SparseMatrix(np.asarray(glp.A._rows).copy(), np.asarray(glp.A._cols).copy(), np.asarray(glp.A.data).copy())
    A._shape = (glp.nrows, glp.ncols)
    return GeneralLP(A, glp.b * sb, glp.c * sc, a=glp.a * sb, l=glp.l * sb, u=glp.u * sb, f=glp.f * sb * sc)


def twin_each(blp, idx=None, **opts):
    """bounded_twin.solve LP by LP, each with its own matrix A^_k: dict of stacked results (``OUTPUTS``, in the bounded form's
    variables, f not added) for the LPs ``idx`` (default all)."""
    idx = range(blp.nproblems) if idx is None else idx
    each = [bounded_twin.solve(blp.A.todense(k), blp.b[k:k + 1], blp.c[k:k + 1], blp.u[k:k + 1], **opts) for k in idx]
    return {q: np.concatenate([e[q] for e in each]) for q in OUTPUTS}


def general_results(bmap, blp, r, idx=None):
    """Results in the bounded form's variables (of the LPs ``idx``) as the plugin reports them: x, y, z, s in the GeneralLP's
    variables, objectives with f."""
    idx = np.arange(blp.nproblems) if idx is None else np.asarray(idx)
    n = bmap.l.shape[1]
    y = np.zeros((idx.size, bmap.m))
    y[:, bmap.rows] = bmap.sign * r["y"]
    f = np.broadcast_to(blp.f, (blp.nproblems,))[idx]
    return dict(x=bmap.l[idx] + r["x"][:, :n], y=y, z=r["z"][:, :n], s=r["s"][:, :n], pobj=r["pobj"] + f, dobj=r["dobj"] + f,
                status=r["status"], iters=r["iters"])


def plugin_results(s):
    return dict(x=s.x, y=s.y, z=s.z, s=s.s, pobj=s.primal_obj, dobj=s.dual_obj, status=s.status, iters=s.iters)


def rel(a, b):
    return np.abs(np.asarray(a) - b) / np.maximum(1.0, np.abs(b))


def assert_parity(got, ref, idx=None, optimal=True):
    """The project's parity bounds: status equal (and 0), iterations within 1, objectives 1e-9 relative, x at rtol 1e-5 /
    atol 1e-7.  ``got``: results of all LPs, ``ref``: of the LPs ``idx``."""
    idx = np.arange(len(ref["status"])) if idx is None else np.asarray(idx)
    assert np.array_equal(got["status"][idx], ref["status"]), (got["status"][idx], ref["status"])
    if optimal:
        assert (ref["status"] == 0).all(), ref["status"]
    assert np.abs(got["iters"][idx].astype(int) - ref["iters"]).max() <= 1
    assert rel(got["pobj"][idx], ref["pobj"]).max() < 1e-9 and rel(got["dobj"][idx], ref["dobj"]).max() < 1e-9
    np.testing.assert_allclose(got["x"][idx], ref["x"], rtol=1e-5, atol=1e-7)


def residuals(glp, r):
    """(primal, dual, bound, gap) per LP from the returned vectors alone, each relative to 1 + the norm of its data: the
    violation of a <= A x <= b, |A'y - z + s - c|, the violation of l <= x <= u, |pobj - dobj|."""
    A = np.stack([glp.A.todense(k) for k in range(glp.nproblems)])
    ax = np.einsum("kij,kj->ki", A, r["x"])
    fin = lambda v: np.where(np.isfinite(v), v, 0.0)
    nb = 1 + np.maximum(np.linalg.norm(fin(glp.a), axis=1), np.linalg.norm(fin(glp.b), axis=1))
    primal = np.linalg.norm(np.maximum(np.maximum(ax - glp.b, glp.a - ax), 0.0), axis=1) / nb
    dual = np.linalg.norm(np.einsum("kij,ki->kj", A, r["y"]) - r["z"] + r["s"] - glp.c, axis=1) / (1 + np.linalg.norm(glp.c, axis=1))
    bound = np.linalg.norm(np.maximum(np.maximum(r["x"] - glp.u, glp.l - r["x"]), 0.0), axis=1) / (1 + np.linalg.norm(fin(glp.u), axis=1))
    gap = np.abs(r["pobj"] - r["dobj"]) / np.maximum(1.0, np.abs(r["pobj"]))
    return primal, dual, bound, gap


# ---- trajectory: the twin after k iterations, its spread under permutations, the tolerance ---------------------------------
TRAJECTORY_POINTS = {"16-row": (12, 16), "32-row": (24, 40)}          # (m', n)
B_TRAJ = 12
TRAJ_QUANTITIES = ("x", "y", "z", "s", "pobj", "dobj")


def trajectory_lp(point, with_x0=False):
    mk, n = TRAJECTORY_POINTS[point]
    return make(mk, n, B_TRAJ, 7000 + mk, with_x0)


def _run_reference(blp, k, perm=None):
    """The twin's results (bounded form's variables) after k iterations, LP by LP; ``perm``: seed of a row-and-column
    permutation under which every LP is solved (results mapped back)."""
    m, N = blp.nrows, blp.ncols
    rows, cols = np.arange(m), np.arange(N)
    if perm is not None:
        rs = np.random.RandomState(1000 + perm)
        rows, cols = rs.permutation(m), rs.permutation(N)
    inv_r, inv_c = np.argsort(rows), np.argsort(cols)
    out = {q: [] for q in OUTPUTS}
    for i in range(blp.nproblems):
        A = np.ascontiguousarray(blp.A.todense(i)[rows][:, cols])
        r = bounded_twin.solve(A, blp.b[i:i + 1, rows], blp.c[i:i + 1, cols], blp.u[i:i + 1, cols], max_iter=k)
        for q in ("x", "z", "s"):
            out[q].append(r[q][0][inv_c])
        out["y"].append(r["y"][0][inv_r])
        for q in ("pobj", "dobj", "status", "iters"):
            out[q].append(r[q][0])
    return {q: np.asarray(v) for q, v in out.items()}


@functools.lru_cache(maxsize=None)
def trajectory_reference(point, k):
    return _run_reference(trajectory_lp(point).to_bounded_equality_form()[0], k)


@functools.lru_cache(maxsize=None)
def trajectory_tolerance(point, k):
    """{quantity: max(FACTOR x the twin's own spread under NPERM seeded permutations, FLOOR)}, never above CEILING."""
    import trajectory as tj
    blp = trajectory_lp(point).to_bounded_equality_form()[0]
    ref = trajectory_reference(point, k)
    runs = [_run_reference(blp, k, perm=p) for p in range(tj.NPERM)]
    tol = {}
    for q in TRAJ_QUANTITIES:
        spread = max(float(tj.deviation(r[q], ref[q]).max()) for r in runs)
        tol[q] = min(max(tj.FACTOR * spread, tj.FLOOR), tj.CEILING)
    return tol

