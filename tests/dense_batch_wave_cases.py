"""Helpers of tests/test_dense_batch_wave.py (no tests): the plan rule of the wave kernel for per-problem dense matrices
(csrc/ipm_wreg.hip wreg_plan_create_dense_pa) restated, the points at which every instantiated shape is run, and the
trajectory reference of its one trajectory point (the rule of tests/trajectory.py, as dense_batch_cases applies it)."""
import functools

import numpy as np

import dense_batch_cases as dbc

MAX_LDS = 160 * 1024
# the dense-image shapes of csrc/wreg.h: every (MB, NQ) the shared-A kernel has, and those compiled for per-problem matrices
WAVE_DA_SHAPES = [(1, 4), (2, 4), (3, 4), (4, 2), (4, 4), (5, 4), (6, 4), (7, 4), (8, 4), (8, 6)]
WAVE_DAPA_SHAPES = WAVE_DA_SHAPES[:-1]         # (8, 6) does not stay free of scratch: left out (DESIGN.md sections 10, 24)


def first_covering(shapes, m, n):
    for s in shapes:
        if m <= 16 * s[0] and n <= 64 * s[1]:
            return s
    return None


def wave_doubles(mb, nq):
    """LDS doubles of one wave's area without the image (wreg.h WGeo::WAVE_D)."""
    return max(192 * nq, 768) + 272 + 64 * nq + 5 * 16 * mb + 144 * mb


def plan(m, n, tail, shapes=WAVE_DAPA_SHAPES):
    """(shape, bytes per wave, waves per workgroup) of an (m, n) equality form with (``tail``) or without an implied identity
    tail; waves 0: refused, not even one wave fits.  None: no shape covers (m, n)."""
    shape = first_covering(shapes, m, n)
    if shape is None:
        return None
    nd = n - m if tail else n
    rows, stride = (m + 7) // 8 * 8, (max(nd, 1) + 15) // 16 * 16 + 1
    per_wave = 8 * (wave_doubles(*shape) + rows * stride)
    return shape, per_wave, max([w for w in (1, 2, 3, 4) if w * per_wave <= MAX_LDS], default=0)


def doubled(shape, per_wave, waves):
    """ipm_wreg.hip solve_grid: two workgroups per compute unit for the m <= 64 shapes at four waves and half the LDS."""
    return shape[0] <= 4 and waves == 4 and 2 * waves * per_wave <= MAX_LDS


# shape -> ((m, n, tail) ragged, (m, n, tail) full): ragged = one live row in the last 16-row block and one live column in the
# last 64-column register where the route (beyond m = 32, n = 128) and the LDS allow it, else the nearest point; full = the
# largest the LDS plan admits; tail / no tail alternate over the shapes where both forms fit
POINTS = {
    (1, 4): ((3, 129, False), (16, 256, True)),
    (2, 4): ((17, 132, True), (32, 256, False)),
    (3, 4): ((33, 38, True), (48, 256, False)),
    (4, 2): ((49, 54, False), (64, 128, True)),
    (4, 4): ((49, 193, True), (64, 256, False)),
    (5, 4): ((65, 70, False), (80, 256, True)),
    (6, 4): ((81, 86, True), (96, 256, True)),
    (7, 4): ((97, 102, False), (112, 256, True)),
    (8, 4): ((113, 118, True), (128, 256, True)),
}
EVERY = [(shape, which) for shape in WAVE_DAPA_SHAPES for which in (0, 1)]


def every_id(case):
    shape, which = case
    m, n, tail = POINTS[shape][which]
    return "%dx%d-%s-%dx%d-%s" % (shape + ("full" if which else "ragged", m, n, "tail" if tail else "general"))


@functools.lru_cache(maxsize=None)
def batch(m, n, tail, B=dbc.B_EVERY):
    return dbc.make(m, n, tail, B=B)


@functools.lru_cache(maxsize=None)
def oracle(m, n, tail, B=dbc.B_EVERY):
    return dbc.oracle_each(batch(m, n, tail, B))


# ---- trajectory: (40, 40 + 40) with the tail --------------------------------------------------------------------------------
TRAJECTORY_POINT = (40, 80, True)


@functools.lru_cache(maxsize=None)
def trajectory_lp():
    m, n, tail = TRAJECTORY_POINT
    return dbc.make(m, n, tail, B=dbc.B_TRAJ, seed=7000 + m)


def _run_reference(lp, k, perm=None):
    """dense_batch_cases._run_reference with the oracle's OWN objectives: at the iteration limit the wave kernels return, as the
    oracle does, the objectives of the iterate before the last step (tests/trajectory.py), not those of the point they store."""
    from oracle import port
    m, N = lp.nrows, lp.ncols
    rows, cols = np.arange(m), np.arange(N)
    if perm is not None:
        rs = np.random.RandomState(1000 + perm)
        rows, cols = rs.permutation(m), rs.permutation(N)
    inv_r, inv_c = np.argsort(rows), np.argsort(cols)
    out = {q: [] for q in ("x", "y", "z", "pobj", "dobj", "status", "iters")}
    for i in range(lp.nproblems):
        A = np.ascontiguousarray(lp.A.todense(i)[rows][:, cols])
        r = port.dense_solve(A, lp.b[i:i + 1, rows], lp.c[i:i + 1, cols], max_iter=k)
        out["x"].append(r["x"][0][inv_c]); out["y"].append(r["y"][0][inv_r]); out["z"].append(r["z"][0][inv_c])
        for q in ("pobj", "dobj", "status", "iters"):
            out[q].append(r[q][0])
    return {q: np.asarray(v) for q, v in out.items()}


@functools.lru_cache(maxsize=None)
def trajectory_reference(k):
    return _run_reference(trajectory_lp(), k)


@functools.lru_cache(maxsize=None)
def trajectory_tolerance(k):
    """dense_batch_cases.trajectory_tolerance at this module's point: {quantity: max(FACTOR x the oracle's own spread under
    NPERM seeded permutations, FLOOR)}, never above CEILING."""
    import trajectory as tj
    ref = trajectory_reference(k)
    runs = [_run_reference(trajectory_lp(), k, perm=p) for p in range(tj.NPERM)]
    tol = {}
    for q in tj.QUANTITIES:
        spread = max(float(tj.deviation(r[q], ref[q]).max()) for r in runs)
        tol[q] = min(max(tj.FACTOR * spread, tj.FLOOR), tj.CEILING)
    return tol
