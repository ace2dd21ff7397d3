"""The split LDL' sweep of the 32-row lane-group kernels (csrc/ipm_group.inc: GWave::factor_sweep with SP, load_row_for_sweep,
merge_through_slab; csrc/wave_common.h: both_rows_d, ror8_top_d, chain_half_neg).  During columns 0 .. 15 the top 16-lane row of a
group updates columns 16 .. 23 of the bottom-right block for the bottom row: top lane t holds them for row R = 16 + (t ^ 8), reads
them from that row of the slab and hands them back through it behind column 15.

Against the CPU references with the tolerances of test_fused_forward.py (status equal and 0, iterations +-1, objectives 1e-9
relative, x at rtol 1e-5), at the row counts around the seams of that map: m = 17 (one live bottom row, which top lane 8 serves),
24 and 25 (the last live row on either side of R's fold at t = 8), 32 (none padded) and 20; the padded rows are identity rows that
the top lanes read through the substituted row.  Then every other kernel that takes the split: the address form without identity
tail, the (32, 128) shapes, HSD, predictor-corrector, the bounded and the per-problem-A slot body.

Bit for bit inside one build: PYCLLP_FLAG_FORCE_GUARD_PATH replaces the sweep's factor by the guarded one, which never runs the
sweep and is the same arithmetic wherever the guard does not bite; the two runs were bit-identical before the split.  And an LP's
result does not depend on its lane group or its neighbours: the reversed batch, and three LPs against the head of the large
batch.

The batches, the oracle's results and the kernel's solves that test_fused_forward.py also uses are its cached ones."""
import numpy as np
import pytest

import bounded_twin
import dense_batch_cases as dbc
from conftest import rel_err
from pycllp_amd.solvers import solver_registry
from test_fused_forward import (B, BITWISE, FORCE_GUARD, HSD, PC_OPTS, PREDCORR, assert_all_groups_live, assert_matches,
                                reference, solve, solved, standard)
from test_general_solver import make_general
from test_kernel_variants import banded

pytestmark = pytest.mark.gpu

CASES = [
    # id, batch, instantiation (MP, NP), slack-aware, solver options, oracle flags
    ("17x30-one-live-bottom-row", (17, 30), (32, 64), 1, {}, 0),
    ("24x64-fold-of-the-rotation", (24, 64), (32, 96), 1, {}, 0),
    ("25x30-first-row-past-the-fold", (25, 30), (32, 64), 1, {}, 0),
    ("32x64-no-padded-row", (32, 64), (32, 96), 1, {}, 0),
    ("20x30-padded-rows", (20, 30), (32, 64), 1, {}, 0),
    ("equality-32x96-no-identity-tail", "equality", (32, 96), 0, {}, 0),       # ROWB = false: the row addresses formed at the load
    ("32x96-on-32x128", (32, 96), (32, 128), 1, {}, 0),                        # COLB = false: L stored after the sweep
    ("32x64-hsd", (32, 64), (32, 96), 1, dict(hsd=True), HSD),
    ("20x30-hsd-padded-rows", (20, 30), (32, 64), 1, dict(hsd=True), HSD),
    ("32x96-hsd-on-32x128", (32, 96), (32, 128), 1, dict(hsd=True), HSD),      # the split without the carried solves, two ...
    ("32x96-predcorr-on-32x128", (32, 96), (32, 128), 1, PC_OPTS, PREDCORR),   # ... and one kernel more that store L behind the sweep
    ("20x30-predcorr", (20, 30), (32, 64), 1, PC_OPTS, PREDCORR),
    ("equality-32x96-predcorr", "equality", (32, 96), 0, PC_OPTS, PREDCORR),
]


@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_matches_the_oracle(case):
    _, key, shape, slack, opts, flags = case
    s = solved(key, **opts)
    assert_all_groups_live(s.launch_info(), shape, slack)
    assert_matches(s, reference(key, flags))


def test_bounded_general_lp():
    """The slot body in the bounded kernel at (32, 64): a GeneralLP with 24 kept rows, against the bounded twin on every 24th LP
    and the tail."""
    glp = banded(make_general(24, 30, B, seed=2430, mixed_u=True, fixed=2))
    s = solver_registry["hip_general_primal_normal"](device="cuda:0", hsd=False)
    glp.init(s)
    glp.solve(s)
    assert s.kernel == "bounded group"
    info = s.launch_info()
    assert info["group_shape"][0] == 32 and B > info["grid"] * (info["block"] // 64), info
    assert (s.status == 0).all(), np.unique(s.status, return_counts=True)
    blp, _ = glp.to_bounded_equality_form()
    sel = np.r_[0:B:24, B - 6:B]
    tw = bounded_twin.solve(blp.A.todense(), blp.b[sel], blp.c[sel], blp.u[sel])
    assert (tw["status"] == 0).all()
    assert np.abs(s.iters[sel] - tw["iters"]).max() <= 1, (s.iters[sel], tw["iters"])
    assert rel_err(s.primal_obj[sel], tw["pobj"] + blp.f[sel]).max() <= 1e-9
    assert rel_err(s.dual_obj[sel], tw["dobj"] + blp.f[sel]).max() <= 1e-9
    np.testing.assert_allclose(s.x[sel], glp.l[sel] + tw["x"][:, :glp.ncols], rtol=1e-5, atol=1e-6)


def test_per_problem_dense_matrices():
    """The slot body in the per-problem-A kernel at (32, 96) slack-aware, 24 kept rows; the oracle LP by LP on every 24th LP and
    the tail."""
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


@pytest.mark.parametrize("key", [(32, 64), (20, 30)], ids=["32x64", "20x30"])
def test_split_sweep_equals_the_guarded_factor(key):
    """With and without PYCLLP_FLAG_FORCE_GUARD_PATH, bit for bit (see the module docstring)."""
    swept = solved(key)
    guarded = solved(key, flags=FORCE_GUARD)
    for name in BITWISE:
        np.testing.assert_array_equal(getattr(swept, name), getattr(guarded, name), err_msg=name)


@pytest.mark.parametrize("key", [(32, 64), (17, 30)], ids=["32x64", "17x30"])
def test_reversed_batch_bit_for_bit(key):
    """Every LP changes lane group and wave: the rows a top lane reads and writes for its bottom lane are those of its own group."""
    lp = standard(*key)
    fwd = solved(key)
    rev = solve(lp, np.ascontiguousarray(lp.b[::-1]), np.ascontiguousarray(lp.c[::-1]))
    for name in BITWISE:
        np.testing.assert_array_equal(getattr(fwd, name), getattr(rev, name)[::-1], err_msg=name)


@pytest.mark.parametrize("key", [(32, 64), (25, 30)], ids=["32x64", "25x30"])
def test_three_lps_bit_for_bit(key):
    """A batch of 3 LPs: the second lane group of a wave is never live and idle groups run along from the start.  The same three
    LPs as the head of the large batch."""
    lp = standard(*key)
    big = solved(key)
    few = solve(lp, np.ascontiguousarray(lp.b[:3]), np.ascontiguousarray(lp.c[:3]))
    assert few.launch_info()["group_shape"][0] == 32
    for name in BITWISE:
        np.testing.assert_array_equal(getattr(few, name), getattr(big, name)[:3], err_msg=name)
