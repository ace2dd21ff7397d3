"""The hot LDL' sweep of ipm_group_kernel decides "would the Nocedal-Wright guard have bitten?" from the pivots -- a group
whose pivots are all > 0 did not meet it (csrc/ipm_group.inc, GWave::factor_sweep) -- and no longer from a running maximum of
u^2 / D.  A redo taken where nothing bit runs the guarded factorisation, which is the sweep's arithmetic there, so the verdict
itself never shows in a result: every solve here must equal, bit for bit, the same solve under PYCLLP_FLAG_FORCE_GUARD_PATH,
which takes the guarded path in every iteration.  Shapes: the full-shape (32, 96) kernel, a generic 32-row kernel with padded
rows, four groups per wave with and without padding (the predictor-corrector kernels keep the running maximum: no case), a
batch of one LP and one of slots + 1 LPs (idle lane groups), and matrices with a duplicated and a zero row (M singular to
rounding: pivots of either sign and exact zeros), those also against the oracle's status and iteration count (+-1, the
tolerance of test_fused_forward.py).  The mixed-sign LPs of tests/golden/status_cases.npz do not fit: on the plain path most of
them diverge to the iteration limit, and there the forced guard path already leaves the hot sweep's trajectory in the parent
(status 3 after 125-190 iterations against status 5 after 200 on the first two shapes, measured with the parent's library),
and the 10x-growth exit is not the oracle's.  Against the PARENT's library those LPs and the singular batches are compared by
tools/dev/outputs_vs_parent.py, byte for byte (profiles/guard_sign/outputs_vs_parent.txt)."""
import functools

import numpy as np
import pytest

from pycllp_amd import problems
from pycllp_amd.lp import EqualityLP, SparseMatrix, StandardLP
from pycllp_amd.solvers import solver_registry
from test_hip_parity import oracle_on

pytestmark = pytest.mark.gpu
FORCE_GUARD = 4                                # PYCLLP_FLAG_FORCE_GUARD_PATH
BITWISE = ("status", "iters", "primal_obj", "dual_obj", "x", "y", "z")


def solve(lp, **opts):
    s = solver_registry["hip_dense_primal_normal"](device="cuda:0", autoscale=False, hsd=False, **opts)
    lp.init(s)
    lp.solve(s)
    return s


@functools.lru_cache(maxsize=None)
def standard(m, n, B):
    A, b, c = problems.random_dense_arrays(m, n, B, seed=1000 * m + n)
    return StandardLP(SparseMatrix(matrix=A), b, c, 0.0).to_equality_form()


def assert_same_bits(a, b):
    for name in BITWISE:
        np.testing.assert_array_equal(getattr(a, name), getattr(b, name), err_msg=name)


def slots(info):
    return info["grid"] * (info["block"] // 64) * (64 // info["group_shape"][0])


CASES = [
    # id, (m, n) of the StandardLP, LPs, instantiation, solver options
    ("32x64-full-shape", (32, 64), 192, (32, 96), {}),
    ("20x30-padded-rows", (20, 30), 192, (32, 64), {}),
    ("16x32-four-groups", (16, 32), 256, (16, 48), {}),
    ("10x20-four-groups-padded", (10, 20), 256, (16, 48), {}),
    ("32x64-one-lp", (32, 64), 1, (32, 96), {}),
    ("16x32-one-lp", (16, 32), 1, (16, 48), {}),
]


@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_default_solve_equals_the_forced_guard_path(case):
    _, (m, n), B, shape, opts = case
    lp = standard(m, n, B)
    hot = solve(lp, **opts)
    info = hot.launch_info()
    assert info["group_shape"] == shape and info["slack"] == 1, info
    assert (hot.status == 0).all()
    assert_same_bits(hot, solve(lp, flags=FORCE_GUARD, **opts))


@pytest.mark.parametrize("m,n", [(32, 64), (16, 32)])
def test_one_lp_more_than_the_launch_has_slots(m, n):
    """Every slot of the launch gets an LP and one LP is left for the queue: at the tail every lane group but one is idle."""
    full = 5999
    for _ in range(4):                        # the plan's waves per workgroup grow with the batch: walk to the fixed point
        lp = standard(m, n, full + 1)
        hot = solve(lp)
        if slots(hot.launch_info()) == full:
            break
        full = slots(hot.launch_info())
    assert slots(hot.launch_info()) == full == lp.nproblems - 1, (hot.launch_info(), full)
    assert (hot.status == 0).all()
    assert_same_bits(hot, solve(lp, flags=FORCE_GUARD))


def singular_lp(m, N, B, seed):
    """An EqualityLP without identity tail whose last row repeats row 3 and whose row m // 2 is zero, around a strictly
    feasible primal-dual pair (as test_kernel_variants.equality_lp): b repeats and vanishes with the rows, so every LP is
    feasible, and M = A D A' has an exact zero row and a pivot that is pure rounding."""
    rs = np.random.RandomState(seed)
    A = rs.randn(m, N) / np.sqrt(N)
    A[-1] = A[3]
    A[m // 2] = 0.0
    x0, y0 = rs.rand(B, N) + 0.1, rs.randn(B, m)
    b, c = x0 @ A.T, y0 @ A - (rs.rand(B, N) + 0.1)
    b /= np.abs(b).max(axis=1, keepdims=True)
    c /= np.abs(c).max(axis=1, keepdims=True)
    return EqualityLP(SparseMatrix(matrix=A), b, c, 0.0)


@pytest.mark.parametrize("m,N,shape", [(32, 96, (32, 96)), (24, 60, (32, 64)), (12, 40, (16, 48))],
                         ids=["32x96", "24x60-padded", "12x40-four-groups"])
def test_duplicated_and_zero_row(m, N, shape):
    lp = singular_lp(m, N, 64, seed=100 * m + N)
    hot = solve(lp)
    info = hot.launch_info()
    assert info["group_shape"] == shape and info["slack"] == 0, info
    assert_same_bits(hot, solve(lp, flags=FORCE_GUARD))
    r = oracle_on(lp, auto=False)
    print("status kernel %s oracle %s, iterations apart at most %d" % (np.unique(hot.status, return_counts=True),
          np.unique(r["status"], return_counts=True), np.abs(hot.iters.astype(int) - r["iters"]).max()))
    np.testing.assert_array_equal(hot.status, r["status"])
    assert np.abs(hot.iters.astype(int) - r["iters"]).max() <= 1
