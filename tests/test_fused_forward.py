"""The forward substitution that the LDL' sweep of the lane-group kernels carries along (csrc/ipm_group.inc,
GWave::factor_dpp_fwd) and the column-by-column stores of L: every call site, at the shapes and options where the carried
right-hand side, the hand-over between the two DPP rows or the store addresses can go wrong, against the CPU references with the
tolerances of test_gram_tiles.py (status equal and 0, iterations +-1, objectives 1e-9 relative, x at rtol 1e-5).

A batch of 6 000 LPs is more than one LP per wavefront of the launch and no multiple of the slots: waves start with all lane
groups live, and at the tail some run with a lane group idle.

Two checks are bit for bit: the same batch in reversed order, and the same batch with PYCLLP_FLAG_FORCE_GUARD_PATH, which drops the
carried forward half and runs the unfused substitution on the guarded factor.  The guarded factorisation is the sweep's arithmetic
wherever the guard does not bite (and where it bites, both runs take it), and the two runs were bit-identical before the sweep
carried anything (checked on the parent commit with this test), so the assertion pins the carried forward half against
GWave::forward inside one build."""
import functools

import numpy as np
import pytest

import bounded_twin
import dense_batch_cases as dbc
from conftest import rel_err
from pycllp_amd import problems
from pycllp_amd.lp import SparseMatrix, StandardLP
from pycllp_amd.solvers import solver_registry
from test_general_solver import make_general
from test_hip_parity import oracle_on
from test_kernel_variants import banded, equality_lp

pytestmark = pytest.mark.gpu
B = 6000
FORCE_GUARD, HSD, PREDCORR = 4, 32, 128        # PYCLLP_FLAG_FORCE_GUARD_PATH; the oracle's flags of the two variants
TIGHT = 1e-15                                  # refine_tol that the residual of a Newton step rarely meets (default 1e-11)
BITWISE = ("status", "iters", "primal_obj", "dual_obj", "x", "y", "z")


@functools.lru_cache(maxsize=None)
def standard(m, n):
    A, b, c = problems.random_dense_arrays(m, n, B, seed=100 * m + n)
    lp = StandardLP(SparseMatrix(matrix=A), b, c, 0.0).to_equality_form()
    for a in (lp.b, lp.c):
        a.setflags(write=False)
    return lp


@functools.lru_cache(maxsize=None)
def equality():
    return equality_lp(32, 96, B, seed=3296)


@functools.lru_cache(maxsize=None)
def reference(key, flags, refine_tol=None):
    """The oracle's solve of a batch, computed once and shared (read-only)."""
    lp = equality() if key == "equality" else standard(*key)
    opts = {} if refine_tol is None else dict(refine_tol=refine_tol)
    r = oracle_on(lp, auto=False, flags=flags, **opts)
    for a in r.values():
        a.setflags(write=False)
    return r


@functools.lru_cache(maxsize=None)
def solved(key, **opts):
    """The kernel's solve of a batch, shared by the tests that compare it with something else."""
    return solve(equality() if key == "equality" else standard(*key), **opts)


def solve(lp, b=None, c=None, **opts):
    s = solver_registry["hip_dense_primal_normal"](device="cuda:0", autoscale=False, **opts)
    if b is not None:
        lp = type(lp)(lp.A, b, c, 0.0)
    lp.init(s)
    lp.solve(s)
    return s


def assert_all_groups_live(info, shape, slack):
    assert info["group_shape"] == shape and info["slack"] == slack, info
    assert B > info["grid"] * (info["block"] // 64), info      # more LPs than wavefronts: second lane groups start live


def assert_matches(s, r):
    np.testing.assert_array_equal(s.status, r["status"])
    assert (s.status == 0).all()
    assert np.abs(s.iters.astype(int) - r["iters"]).max() <= 1
    assert rel_err(s.primal_obj, r["pobj"]).max() <= 1e-9 and rel_err(s.dual_obj, r["dobj"]).max() <= 1e-9
    np.testing.assert_allclose(s.x, r["x"], rtol=1e-5, atol=1e-6)


PC_OPTS = dict(predcorr=True, hsd=False)

CASES = [
    # id, batch, instantiation (MP, NP), slack-aware, solver options, oracle flags
    ("32x64-both-dpp-rows", (32, 64), (32, 96), 1, {}, 0),
    ("20x30-padded-rows", (20, 30), (32, 64), 1, {}, 0),                       # identity rows carry a zero right-hand side
    ("17x20-one-live-bottom-row", (17, 20), (32, 64), 1, {}, 0),
    ("16x32-one-dpp-row", (16, 32), (16, 48), 1, {}, 0),
    ("12x20-one-dpp-row-padded", (12, 20), (16, 48), 1, {}, 0),
    ("equality-32x96-no-identity-tail", "equality", (32, 96), 0, {}, 0),       # ROWB = false addresses
    ("32x96-on-32x128", (32, 96), (32, 128), 1, {}, 0),                        # COLB = false addresses: the plain sweep
    # predictor-corrector: the slack-aware (32, 96) kernel keeps the plain sweep (column stores only); every other shape carries
    # the predictor's solve and runs the corrector's unfused on the same factor
    ("32x64-predcorr-plain-sweep", (32, 64), (32, 96), 1, PC_OPTS, PREDCORR),
    ("20x30-predcorr-carried-predictor", (20, 30), (32, 64), 1, PC_OPTS, PREDCORR),
    ("16x32-predcorr-carried-predictor", (16, 32), (16, 48), 1, PC_OPTS, PREDCORR),
    ("12x20-predcorr-carried-predictor", (12, 20), (16, 48), 1, PC_OPTS, PREDCORR),
    ("equality-32x96-predcorr-carried-predictor", "equality", (32, 96), 0, PC_OPTS, PREDCORR),
    ("32x64-hsd-two-right-hand-sides", (32, 64), (32, 96), 1, dict(hsd=True), HSD),
    ("20x30-hsd-padded-rows", (20, 30), (32, 64), 1, dict(hsd=True), HSD),
    ("32x64-forced-guard-path", (32, 64), (32, 96), 1, dict(flags=FORCE_GUARD), 0),    # the carried result dropped
]


@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_carried_forward_solve_matches_the_oracle(case):
    _, key, shape, slack, opts, flags = case
    s = solved(key, **opts)
    assert_all_groups_live(s.launch_info(), shape, slack)
    assert_matches(s, reference(key, flags))


def test_refinement_solves_follow_the_carried_one():
    """A tight refine_tol: every iteration's first solve is carried, the refinement solves behind it run unfused on the same L.
    (The oracle alone solves every LP of this batch to status 0 at this refine_tol, with 11 to 39 refinement passes per LP.)"""
    r = reference((32, 64), 0, TIGHT)
    assert (r["status"] == 0).all() and r["nrefs"].min() > 0
    s = solve(standard(32, 64), refine_tol=TIGHT)
    assert_all_groups_live(s.launch_info(), (32, 96), 1)
    assert_matches(s, r)


def test_bounded_general_lp():
    """The slot-body call site of the bounded kernel: the GeneralLP of test_gram_tiles_bounded_general_lp, 24 kept rows."""
    glp = banded(make_general(24, 30, B, seed=2430, mixed_u=True, fixed=2))
    s = solver_registry["hip_general_primal_normal"](device="cuda:0", hsd=False)
    glp.init(s)
    glp.solve(s)
    assert s.kernel == "bounded group"
    info = s.launch_info()
    assert info["group_shape"][0] == 32 and B > info["grid"] * (info["block"] // 64), info
    assert (s.status == 0).all(), np.unique(s.status, return_counts=True)
    blp, _ = glp.to_bounded_equality_form()
    sel = np.r_[0:B:24, B - 6:B]                             # every 24th LP and the tail
    tw = bounded_twin.solve(blp.A.todense(), blp.b[sel], blp.c[sel], blp.u[sel])
    assert (tw["status"] == 0).all()
    assert np.abs(s.iters[sel] - tw["iters"]).max() <= 1, (s.iters[sel], tw["iters"])
    assert rel_err(s.primal_obj[sel], tw["pobj"] + blp.f[sel]).max() <= 1e-9
    assert rel_err(s.dual_obj[sel], tw["dobj"] + blp.f[sel]).max() <= 1e-9
    np.testing.assert_allclose(s.x[sel], glp.l[sel] + tw["x"][:, :glp.ncols], rtol=1e-5, atol=1e-6)


def test_per_problem_dense_matrices():
    """The slot-body call site of the per-problem-A kernel, (32, 96) slack-aware; the oracle LP by LP on every 24th LP and the
    tail."""
    lp = dbc.standard_batch(24, 40, B, seed=2440)
    s = solver_registry["hip_dense_batch_primal_normal"](device="cuda:0", hsd=False, autoscale=False)
    lp.init(s)
    lp.solve(s)
    info = s.launch_info()
    assert s.kernel == "group per-problem" and info["group_shape"] == (32, 96) and info["slack"] == 1, info
    assert B > info["grid"] * (info["block"] // 64), info
    assert (s.status == 0).all()
    sel = np.r_[0:B:24, B - 6:B]
    got = dict(x=s.x, y=s.y, z=s.z, pobj=s.primal_obj, dobj=s.dual_obj, status=s.status, iters=s.iters)
    dbc.assert_matches_oracle(got, dbc.oracle_each(lp, sel), sel)


def test_result_is_independent_of_lane_group_and_neighbour():
    """The same batch in forward and reversed order: carried and skipped lanes meet other neighbours, and every LP must come
    back bit for bit the same."""
    lp = standard(32, 64)
    fwd = solved((32, 64))
    rev = solve(lp, np.ascontiguousarray(lp.b[::-1]), np.ascontiguousarray(lp.c[::-1]))
    for name in BITWISE:
        np.testing.assert_array_equal(getattr(fwd, name), getattr(rev, name)[::-1], err_msg=name)


@pytest.mark.parametrize("key,opts", [((32, 64), {}), ((20, 30), {}), ((12, 20), {}), ((32, 64), dict(hsd=True)),
                                      ((20, 30), PC_OPTS), ((12, 20), PC_OPTS), ("equality", PC_OPTS)],
                         ids=["32x64", "20x30", "12x20", "32x64-hsd", "20x30-predcorr", "12x20-predcorr", "equality-32x96-predcorr"])
def test_carried_forward_half_equals_the_unfused_one(key, opts):
    """With and without PYCLLP_FLAG_FORCE_GUARD_PATH, bit for bit (see the module docstring)."""
    fused = solved(key, **opts)
    plain = solved(key, flags=FORCE_GUARD, **opts)
    for name in BITWISE:
        np.testing.assert_array_equal(getattr(fused, name), getattr(plain, name), err_msg=name)
