"""The cross-row exchanges of the lane-group kernels on lane swaps (csrc/wave_common.h: quad_sum2, top_row_d, bottom_row_d,
row_pair_sum, row_pair_max; csrc/ipm_group.inc: GWave::gram_one's A x / A (d t) sums, the hand-over between the two 16-lane rows
of a 32-lane group in forward(), backward() and the carrying sweep, the last stage of grp_sum / grp_max, and A'u with u broadcast
from registers in At_times / At_times2): every call site at the smallest shape where it can go wrong, against the CPU
references with the tolerances of test_gram_tiles.py and test_fused_forward.py (status equal and 0, iterations +-1, objectives 1e-9
relative, x at rtol 1e-5).

A lane swap moves active lanes only, and what it returns depends on the lane's 16-lane row.  So besides the shapes (both rows of
a group, padded rows, four groups per wave at MP = 16, the (32, 128) shapes whose forward substitution is never carried) two
checks are bit for bit: the batch in reversed order, where every LP changes lane group and wave, and a batch of 3 LPs, where lane
groups are idle from the start and the second group of a wave is never live, against the same LPs inside the large batch.

The batches, the oracle's results and the kernel's solves that test_fused_forward.py also uses are its cached ones: computed once
per session."""
import functools

import numpy as np
import pytest

import autoscale_cases as ac
import bounded_twin
import dense_batch_cases as dbc
from conftest import rel_err
from pycllp_amd.solvers import solver_registry
from test_fused_forward import (B, BITWISE, FORCE_GUARD, HSD, PC_OPTS, PREDCORR, TIGHT, assert_all_groups_live, assert_matches,
                                reference, solve, solved, standard)
from test_general_solver import make_general
from test_hip_parity import oracle_on
from test_kernel_variants import banded

pytestmark = pytest.mark.gpu
AUTOSCALE = 8                                  # PYCLLP_FLAG_AUTOSCALE

CASES = [
    # id, batch, instantiation (MP, NP), slack-aware, solver options, oracle flags
    ("32x64-headline", (32, 64), (32, 96), 1, {}, 0),
    ("20x30-padded-rows-and-columns", (20, 30), (32, 64), 1, {}, 0),
    ("equality-32x96-no-identity-tail", "equality", (32, 96), 0, {}, 0),
    ("32x96-on-32x128-unfused-forward", (32, 96), (32, 128), 1, {}, 0),
    ("16x32-four-groups-per-wave", (16, 32), (16, 48), 1, {}, 0),
    ("12x20-four-groups-per-wave-padded", (12, 20), (16, 48), 1, {}, 0),
    ("32x64-hsd", (32, 64), (32, 96), 1, dict(hsd=True), HSD),
    ("32x64-predcorr", (32, 64), (32, 96), 1, PC_OPTS, PREDCORR),              # the corrector runs the whole fwd_back
    ("32x64-forced-guard-path", (32, 64), (32, 96), 1, dict(flags=FORCE_GUARD), 0),
]


@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_matches_the_oracle(case):
    _, key, shape, slack, opts, flags = case
    s = solved(key, **opts)
    assert_all_groups_live(s.launch_info(), shape, slack)
    assert_matches(s, reference(key, flags))


def test_refinement_solves():
    """refine_tol = 1e-15: every LP runs refinement passes, each a whole unfused fwd_back on the iteration's factor."""
    r = reference((32, 64), 0, TIGHT)
    assert (r["status"] == 0).all() and r["nrefs"].min() > 0
    s = solved((32, 64), refine_tol=TIGHT)
    assert_all_groups_live(s.launch_info(), (32, 96), 1)
    assert_matches(s, r)


@functools.lru_cache(maxsize=None)
def out_of_band():
    """standard(32, 64) with every 97th LP scaled out of band (b x 1e3, c x 1e-2): finalize() rescales those under a per-group
    condition, next to groups that it leaves alone."""
    lp = ac.mixed_equality(standard(32, 64), np.arange(5, B, 97))
    for a in (lp.b, lp.c):
        a.setflags(write=False)
    return lp


def test_autoscale_with_out_of_band_lps():
    lp = out_of_band()
    assert 0 < ac.mask_of(dict(b=lp.b, c=lp.c)).sum() < B
    r = oracle_on(lp, auto=False, flags=AUTOSCALE)
    s = solver_registry["hip_dense_primal_normal"](device="cuda:0", autoscale=True)
    lp.init(s)
    lp.solve(s)
    assert_all_groups_live(s.launch_info(), (32, 96), 1)
    assert_matches(s, r)


def test_bounded_general_lp():
    """The slot body's call site in the bounded kernel: a GeneralLP with 24 kept rows, against the bounded twin on every 24th LP
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
    """The slot body's call site in the per-problem-A kernel at (32, 64) slack-aware; the oracle LP by LP on every 24th LP and the
    tail."""
    lp = dbc.standard_batch(24, 30, B, seed=2430)
    s = solver_registry["hip_dense_batch_primal_normal"](device="cuda:0", hsd=False, autoscale=False)
    lp.init(s)
    lp.solve(s)
    info = s.launch_info()
    assert s.kernel == "group per-problem" and info["group_shape"] == (32, 64) and info["slack"] == 1, info
    assert B > info["grid"] * (info["block"] // 64), info
    assert (s.status == 0).all()
    sel = np.r_[0:B:24, B - 6:B]
    got = dict(x=s.x, y=s.y, z=s.z, pobj=s.primal_obj, dobj=s.dual_obj, status=s.status, iters=s.iters)
    dbc.assert_matches_oracle(got, dbc.oracle_each(lp, sel), sel)


@pytest.mark.parametrize("key,opts", [((32, 64), {}), ((12, 20), {}), ((32, 64), dict(hsd=True))], ids=["32x64", "12x20", "32x64-hsd"])
def test_reversed_batch_bit_for_bit(key, opts):
    """Every LP changes lane group and wave (at MP = 32 also the half of the wave): a sum that differed between the 16-lane rows
    would show."""
    lp = standard(*key)
    fwd = solved(key, **opts)
    rev = solve(lp, np.ascontiguousarray(lp.b[::-1]), np.ascontiguousarray(lp.c[::-1]), **opts)
    for name in BITWISE:
        np.testing.assert_array_equal(getattr(fwd, name), getattr(rev, name)[::-1], err_msg=name)


@pytest.mark.parametrize("key", [(32, 64), (12, 20)], ids=["32x64", "12x20"])
def test_three_lps_bit_for_bit(key):
    """A batch of 3 LPs: no wave ever has a second live lane group, idle groups run along from the start.  The same three LPs as
    the head of the large batch."""
    lp = standard(*key)
    big = solved(key)
    few = solve(lp, np.ascontiguousarray(lp.b[:3]), np.ascontiguousarray(lp.c[:3]))
    info = few.launch_info()
    assert info["group_shape"][0] == (32 if key[0] > 16 else 16), info
    for name in BITWISE:
        np.testing.assert_array_equal(getattr(few, name), getattr(big, name)[:3], err_msg=name)
