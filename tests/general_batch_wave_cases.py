"""Helpers of tests/test_general_batch_wave.py (no tests): the plan rule of the bounded wave kernel for per-problem dense
matrices (csrc/wreg_plan.h, WPLAN_BOUNDED_DENSE_PA) restated, the points at which every instantiated shape is run, the batches
and their twin results (tests/bounded_twin.solve LP by LP, each with its own matrix), and the trajectory reference of the one
trajectory point with its tolerance (the rule of general_batch_cases.trajectory_tolerance)."""
import functools

import numpy as np
import scipy.sparse as sp

import dense_batch_wave_cases as dwc
import general_batch_cases as gbc
from test_general_solver import make_general

MAX_LDS = dwc.MAX_LDS
PLAN_KIND = 8                                   # pycllp_hip_debug_plan: wreg_plan_create_bounded_dense_pa
# WREG_BDDAPA_SHAPES of csrc/wreg.h: every (MB, NQ) compiled for upper bounds on per-problem dense matrices
WAVE_BDDAPA_SHAPES = [(1, 4), (2, 4), (3, 4), (4, 2), (4, 4), (5, 4), (6, 4), (7, 4), (8, 4)]
B_EVERY = gbc.B_EVERY                           # 37 LPs on two workgroups: every wave takes several


def plan(mk, N, max_lds=MAX_LDS):
    """(shape, bytes per wave, waves per workgroup) of a bounded form of mk kept rows and N columns, the last mk the identity:
    the first covering shape; the wave area, the image (rows rounded up to 8, nd = N - mk columns rounded up to 16, plus 1) and
    t and s (2 x 64 NQ) per wave; as many waves, 4 down to 1, as fit.  None: no shape covers, or not even one wave fits."""
    shape = dwc.first_covering(WAVE_BDDAPA_SHAPES, mk, N)
    if shape is None:
        return None
    rows, stride = (mk + 7) // 8 * 8, (max(N - mk, 1) + 15) // 16 * 16 + 1
    per_wave = 8 * (dwc.wave_doubles(*shape) + rows * stride + 2 * 64 * shape[1])
    waves = max([w for w in (1, 2, 3, 4) if w * per_wave <= max_lds], default=0)
    return (shape, per_wave, waves) if waves else None


# the issue's table: (m', N) -> (shape, bytes per wave, waves)
TABLE = {(10, 160): ((1, 4), 36864, 4), (33, 38): ((3, 4), 25280, 4), (48, 176): ((3, 4), 69376, 2),
         (64, 128): ((4, 2), 51840, 3), (100, 180): ((7, 4), 94400, 1), (128, 256): ((8, 4), 160896, 1)}


def form_matrix(mk, N, seed=0):
    """A dense [A | I] of the bounded form's shape as scipy CSR (what the handle's plan is built from)."""
    A = np.random.RandomState(seed).uniform(0.5, 1.5, (mk, N))
    A[:, N - mk:] = np.eye(mk)
    return sp.csr_matrix(A)


# shape -> ((m', N) ragged, (m', N) full).  ragged: one live row in the last 16-row block and one live column in the last
# 64-column register (never N <= 128 with m' <= 32: that is a lane-group handle); full: the shape's corner.
POINTS = {
    (1, 4): ((1, 193), (16, 256)),
    (2, 4): ((17, 193), (32, 256)),
    (3, 4): ((33, 193), (48, 256)),
    (4, 2): ((49, 65), (64, 128)),
    (4, 4): ((49, 193), (64, 256)),
    (5, 4): ((65, 193), (80, 256)),
    (6, 4): ((81, 193), (96, 256)),
    (7, 4): ((97, 193), (112, 256)),
    (8, 4): ((113, 193), (128, 256)),
}
EVERY = [(shape, which) for shape in WAVE_BDDAPA_SHAPES for which in (0, 1)]


def every_id(case):
    shape, which = case
    return "%dx%d-%s-%dx%d" % (shape + ("full" if which else "ragged",) + POINTS[shape][which])


@functools.lru_cache(maxsize=None)
def make(mk, N, B=B_EVERY, seed=None):
    """The batch of a test (shared, read-only): a bounded form of mk kept rows and N = n + mk columns, every LP with its own
    dense matrix, mixed row kinds, finite, infinite and zero upper bounds."""
    seed = 500 + mk + N if seed is None else seed
    glp = make_general(mk, N - mk, B, seed, per_problem_A=True, fixed=1, mixed_u=True, kinds=gbc.kinds(mk))
    for a in (glp.a, glp.b, glp.c, glp.l, glp.u, glp.A.data):
        a.setflags(write=False)
    return glp


@functools.lru_cache(maxsize=None)
def twin(mk, N, B=B_EVERY, seed=None):
    """The twin's results for ``make``'s batch in the GeneralLP's variables (computed once, shared, read-only)."""
    return twin_of(make(mk, N, B, seed))


def twin_of(glp, idx=None, **opts):
    blp, bmap = glp.to_bounded_equality_form()
    return gbc.general_results(bmap, blp, gbc.twin_each(blp, idx, **opts), idx)


# ---- trajectory: one (3, 4) point --------------------------------------------------------------------------------------------
TRAJECTORY_POINT = (40, 140)                    # (m', N)


def trajectory_lp():
    return make(TRAJECTORY_POINT[0], TRAJECTORY_POINT[1], gbc.B_TRAJ, 7000 + TRAJECTORY_POINT[0])


@functools.lru_cache(maxsize=None)
def trajectory_reference(k):
    return gbc._run_reference(trajectory_lp().to_bounded_equality_form()[0], k)


@functools.lru_cache(maxsize=None)
def trajectory_tolerance(k):
    """general_batch_cases.trajectory_tolerance at this module's point: {quantity: max(FACTOR x the twin's own spread under
    NPERM seeded permutations, FLOOR)}, never above CEILING."""
    import trajectory as tj
    blp = trajectory_lp().to_bounded_equality_form()[0]
    ref = trajectory_reference(k)
    runs = [gbc._run_reference(blp, k, perm=p) for p in range(tj.NPERM)]
    tol = {}
    for q in gbc.TRAJ_QUANTITIES:
        spread = max(float(tj.deviation(r[q], ref[q]).max()) for r in runs)
        tol[q] = min(max(tj.FACTOR * spread, tj.FLOOR), tj.CEILING)
    return tol
