"""The Gram product of the 32-row lane-group kernels on 4x4x4 matrix-core tiles (csrc/ipm_group.inc, GWave::gram_one): every
kernel that takes it, at the shapes where its tile schedule, its operand reads and its stores can go wrong, against the CPU
references with the tolerances of test_kernel_variants.py (status equal, objectives 1e-9 relative, iterations +-1).

A batch of 6 000 LPs is more than one LP per wavefront of the launch, so waves start with two live lane groups, and no multiple
of the slots, so that at the tail some waves run with their second group idle (its Gram product is skipped)."""
import functools

import numpy as np
import pytest

import bounded_twin
from conftest import rel_err
from pycllp_amd import problems
from pycllp_amd.lp import SparseMatrix, StandardLP
from pycllp_amd.solvers import solver_registry
from test_general_solver import check_kkt, make_general
from test_hip_parity import oracle_on
from test_kernel_variants import banded, equality_lp

pytestmark = pytest.mark.gpu
B = 6000
FORCE_GUARD, HSD, PREDCORR = 4, 32, 128        # PYCLLP_FLAG_FORCE_GUARD_PATH; the oracle's flags of the two variants


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
def reference(key, flags):
    """The oracle's solve of a batch, computed once and shared (read-only)."""
    lp = equality() if key == "equality" else standard(*key)
    r = oracle_on(lp, auto=False, flags=flags)
    for a in r.values():
        a.setflags(write=False)
    return r


def solve(lp, b=None, c=None, **opts):
    s = solver_registry["hip_dense_primal_normal"](device="cuda:0", autoscale=False, **opts)
    if b is not None:
        lp = type(lp)(lp.A, b, c, 0.0)
    lp.init(s)
    lp.solve(s)
    return s


def assert_two_groups_live(info, shape, slack):
    assert info["group_shape"] == shape and info["slack"] == slack, info
    assert B > info["grid"] * (info["block"] // 64), info      # more LPs than wavefronts: second lane groups start live


def assert_matches(s, r):
    np.testing.assert_array_equal(s.status, r["status"])
    assert (s.status == 0).all()
    assert np.abs(s.iters.astype(int) - r["iters"]).max() <= 1
    assert rel_err(s.primal_obj, r["pobj"]).max() <= 1e-9 and rel_err(s.dual_obj, r["dobj"]).max() <= 1e-9
    np.testing.assert_allclose(s.x, r["x"], rtol=1e-5, atol=1e-6)


CASES = [
    # id, batch, instantiation (MP, NP), slack-aware, solver options, oracle flags
    ("32x64", (32, 64), (32, 96), 1, {}, 0),
    ("20x30-padded-rows-and-columns", (20, 30), (32, 64), 1, {}, 0),           # zero rows of A, the identity fix-up
    ("equality-32x96-no-identity-tail", "equality", (32, 96), 0, {}, 0),
    ("32x96-longest-k-loop", (32, 96), (32, 128), 1, {}, 0),
    ("32x64-hsd", (32, 64), (32, 96), 1, dict(hsd=True), HSD),
    ("32x64-predcorr", (32, 64), (32, 96), 1, dict(predcorr=True, hsd=False), PREDCORR),
    ("32x64-guarded-cold-path", (32, 64), (32, 96), 1, dict(flags=FORCE_GUARD), 0),   # reads the raw lower triangle from the slab
]


@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_gram_tiles_match_the_oracle(case):
    _, key, shape, slack, opts, flags = case
    lp = equality() if key == "equality" else standard(*key)
    s = solve(lp, **opts)
    assert_two_groups_live(s.launch_info(), shape, slack)
    assert_matches(s, reference(key, flags))


def test_gram_tiles_bounded_general_lp():
    """The bounded kernel takes the same member: a GeneralLP with ranged rows and upper bounds, 24 kept rows."""
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

    class Some:                      # the optimality conditions on every 16th LP (check_kkt is a Python loop)
        pass
    sub, some = np.arange(0, B, 16), Some()
    some.x, some.y, some.z, some.s = s.x[sub], s.y[sub], s.z[sub], s.s[sub]
    check_kkt(type(glp)(glp.A, glp.b[sub], glp.c[sub], a=glp.a[sub], l=glp.l[sub], u=glp.u[sub], f=glp.f[sub]), some)


def test_gram_product_is_independent_of_lane_group_and_neighbour():
    """The same batch in forward and reversed order: every LP meets another lane group, another wave and another neighbour,
    and must come back bit for bit the same."""
    lp = standard(32, 64)
    fwd = solve(lp)
    rev = solve(lp, np.ascontiguousarray(lp.b[::-1]), np.ascontiguousarray(lp.c[::-1]))
    assert_two_groups_live(fwd.launch_info(), (32, 96), 1)
    for name in ("status", "iters", "primal_obj", "dual_obj", "x", "y", "z"):
        np.testing.assert_array_equal(getattr(fwd, name), getattr(rev, name)[::-1], err_msg=name)
