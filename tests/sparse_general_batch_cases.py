"""Helpers of tests/test_sparse_general_batch.py (no tests): GeneralLP batches in which every LP has its own values on one sparse
structure, at the five test points of the bounded wave kernel for per-problem A, the bounded twin run LP
by LP with that LP's own matrix, and the trajectory references with their tolerances (the rule of tests/trajectory.py, as
general_batch_cases.trajectory_tolerance applies it)."""
import functools

import numpy as np

import general_batch_cases as gbc
from pycllp_amd.lp import GeneralLP, SparseMatrix
from test_general_solver import make_general
from test_sparse_general_solver import make_sparse_general

B_EVERY = 37
# point -> (m' kept rows, n columns, density of A (None: dense, make_general's per-problem matrices), the (MB, NQ) that serves it,
#           LPs the twin solves at that point)
POINTS = {
    "P1": (12, 20, None, (1, 4), 16),       # one block, no off-diagonal block
    "P2": (40, 120, 0.08, (3, 4), 12),      # several blocks, one m-register
    "P3": (72, 200, 0.05, (5, 6), 8),       # two m-vector registers per lane
    "P4": (96, 288, 0.03, (6, 6), 8),       # README's workload
    "P5": (128, 384, 0.02, (8, 8), 6),      # the cap
}


def per_problem(base, seed, kinds, fixed):
    """``base`` (a shared sparse A) with every LP's values times U[0.75, 1.25) on the same structure, and the row bounds
    rebuilt around an interior point with that LP's own matrix."""
    rng = np.random.default_rng(seed)
    B, m, n = base.nproblems, base.nrows, base.ncols
    rows, cols = np.asarray(base.A._rows), np.asarray(base.A._cols)
    data = np.asarray(base.A.data[0]) * rng.uniform(0.75, 1.25, (B, rows.size))
    x0 = base.l + rng.uniform(0.2, 0.8, (B, n)) * np.where(np.isfinite(base.u), base.u - base.l, 1.0)
    x0[:, :fixed] = base.l[:, :fixed]
    Ax = np.zeros((B, m))
    for k in range(B):
        np.add.at(Ax[k], rows, data[k] * x0[k, cols])
    a, b = np.full((B, m), -np.inf), np.full((B, m), np.inf)
    for i, kind in enumerate(kinds):
        if kind == "eq":
            a[:, i] = b[:, i] = Ax[:, i]
        elif kind == "rng":
            a[:, i] = Ax[:, i] - rng.uniform(0.1, 1, B); b[:, i] = Ax[:, i] + rng.uniform(0.1, 1, B)
        elif kind == "le":
            b[:, i] = Ax[:, i] + rng.uniform(0.1, 1, B)
        elif kind == "ge":
            a[:, i] = Ax[:, i] - rng.uniform(0.1, 1, B)
    A = SparseMatrix(rows.copy(), cols.copy(), data)
    A._shape = (m, n)
    return GeneralLP(A, b, base.c, a=a, l=base.l, u=base.u, f=base.f)


@functools.lru_cache(maxsize=None)
def make(point, B=B_EVERY, seed=None, with_x0=False):
    """The batch of a test (shared, read-only): ``gbc.kinds`` rows (none dropped), two fixed columns, u with +inf, finite and 0.
    ``with_x0`` (a dense point): (the batch, the interior point its row bounds are built around)."""
    mk, n, density, _, _ = POINTS[point]
    seed = 500 + mk if seed is None else seed
    x0 = None
    if density is None:
        glp, x0 = make_general(mk, n, B, seed, per_problem_A=True, fixed=2, mixed_u=True, kinds=gbc.kinds(mk), with_x0=True)
    else:
        base = make_sparse_general(mk, n, B, seed, density, fixed=2, mixed_u=True, kinds=gbc.kinds(mk))
        glp = per_problem(base, seed + 1, gbc.kinds(mk), 2)
    for v in (glp.a, glp.b, glp.c, glp.l, glp.u, glp.A.data):
        v.setflags(write=False)
    if with_x0:
        assert x0 is not None, point
        return glp, x0
    return glp


def sample(point, B):
    """The LPs the twin solves at ``point``: evenly spaced over the batch."""
    k = min(POINTS[point][4], B)
    return np.unique(np.linspace(0, B - 1, k).astype(int))


@functools.lru_cache(maxsize=None)
def twin(point, B=B_EVERY, seed=None):
    """(idx, the twin's results in the GeneralLP's variables) for the sampled LPs of ``make(point, B, seed)``."""
    glp = make(point, B, seed)
    idx = sample(point, B)
    blp, bmap = glp.to_bounded_equality_form()
    return idx, gbc.general_results(bmap, blp, gbc.twin_each(blp, idx), idx)


def in_band(glp):
    """The same LPs with row 0 (positive coefficients, the largest |b|) divided by 20: data inside the autoscale band."""
    data, b, a = np.array(glp.A.data), glp.b.copy(), glp.a.copy()
    r0 = np.asarray(glp.A._rows) == 0
    data[:, r0] /= 20; b[:, 0] /= 20; a[:, 0] /= 20
    A = SparseMatrix(np.asarray(glp.A._rows).copy(), np.asarray(glp.A._cols).copy(), data)
    A._shape = (glp.nrows, glp.ncols)
    return GeneralLP(A, b, glp.c.copy(), a=a, l=glp.l.copy(), u=glp.u.copy(), f=glp.f.copy())


# ---- trajectory: the twin after k iterations, its spread under permutations, the tolerance ---------------------------------
TRAJECTORY_POINTS = ("P1", "P3")
B_TRAJ = 12
TRAJ_QUANTITIES = gbc.TRAJ_QUANTITIES


def trajectory_lp(point, with_x0=False):
    return make(point, B_TRAJ, 7100 + POINTS[point][0], with_x0)


@functools.lru_cache(maxsize=None)
def trajectory_reference(point, k):
    return gbc._run_reference(trajectory_lp(point).to_bounded_equality_form()[0], k)


@functools.lru_cache(maxsize=None)
def trajectory_tolerance(point, k):
    """{quantity: max(FACTOR x the twin's own spread under NPERM seeded permutations, FLOOR)}, never above CEILING."""
    import trajectory as tj
    blp = trajectory_lp(point).to_bounded_equality_form()[0]
    ref = trajectory_reference(point, k)
    runs = [gbc._run_reference(blp, k, perm=p) for p in range(tj.NPERM)]
    tol = {}
    for q in TRAJ_QUANTITIES:
        spread = max(float(tj.deviation(r[q], ref[q]).max()) for r in runs)
        tol[q] = min(max(tj.FACTOR * spread, tj.FLOOR), tj.CEILING)
    return tol
