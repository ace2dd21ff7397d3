"""The self-swap helpers of csrc/wave_common.h (self_swap16 / self_swap32 behind top_row_d, bottom_row_d, both_rows_d,
row_pair_sum, row_pair_max, quad_sum, quad_sum2) hand the lane swap two 64-bit copies of the value instead of its halves twice.
That is data movement only, and test_lane_swaps.py pins every call site of the dense shared-A kernels.  The header is shared:
the bounded and the per-problem-A lane-group kernels are rebuilt through it too.  One small batch each, on a shape with both
16-lane rows of a group (32 rows) and on one with a single row (16 rows, where only quad_sum2 swaps), against their CPU twins
with the tolerances of test_lane_swaps.py."""
import numpy as np
import pytest

import bounded_twin
import dense_batch_cases as dbc
from conftest import rel_err
from pycllp_amd.solvers import solver_registry
from test_general_solver import make_general
from test_kernel_variants import banded

pytestmark = pytest.mark.gpu
NLP = 96


@pytest.mark.parametrize("rows,cols,mp", [(24, 30, 32), (12, 20, 16)], ids=["24-kept-rows-on-32", "12-kept-rows-on-16"])
def test_bounded_kernel_against_its_twin(rows, cols, mp):
    glp = banded(make_general(rows, cols, NLP, seed=100 * rows + cols, mixed_u=True, fixed=2))
    s = solver_registry["hip_general_primal_normal"](device="cuda:0", hsd=False)
    glp.init(s)
    glp.solve(s)
    assert s.kernel == "bounded group" and s.launch_info()["group_shape"][0] == mp, s.launch_info()
    assert (s.status == 0).all(), np.unique(s.status, return_counts=True)
    blp, _ = glp.to_bounded_equality_form()
    tw = bounded_twin.solve(blp.A.todense(), blp.b, blp.c, blp.u)
    assert (tw["status"] == 0).all()
    assert np.abs(s.iters - tw["iters"]).max() <= 1, (s.iters, tw["iters"])
    assert rel_err(s.primal_obj, tw["pobj"] + blp.f).max() <= 1e-9
    assert rel_err(s.dual_obj, tw["dobj"] + blp.f).max() <= 1e-9
    np.testing.assert_allclose(s.x, glp.l + tw["x"][:, :glp.ncols], rtol=1e-5, atol=1e-6)


@pytest.mark.parametrize("rows,cols,mp", [(24, 30, 32), (12, 20, 16)], ids=["24x30-on-32-rows", "12x20-on-16-rows"])
def test_per_problem_kernel_against_the_oracle(rows, cols, mp):
    lp = dbc.standard_batch(rows, cols, NLP, seed=100 * rows + cols)
    s = solver_registry["hip_dense_batch_primal_normal"](device="cuda:0", hsd=False, autoscale=False)
    lp.init(s)
    lp.solve(s)
    info = s.launch_info()
    assert s.kernel == "group per-problem" and info["group_shape"][0] == mp and info["slack"] == 1, info
    assert (s.status == 0).all()
    sel = np.arange(NLP)
    got = dict(x=s.x, y=s.y, z=s.z, pobj=s.primal_obj, dobj=s.dual_obj, status=s.status, iters=s.iters)
    dbc.assert_matches_oracle(got, dbc.oracle_each(lp, sel), sel)
