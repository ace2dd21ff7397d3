"""Trajectory parity: x, y, z and the objectives of every solve kernel after k = 1, 2, 4, 8 iterations against the CPU references,
within a tolerance derived from the references alone (tests/trajectory.py).  One case per arithmetic path, at the smallest shape
that reaches it; warm start and autoscale rows per family; a degenerate case that keeps refinement at its cap and the pivot floor
active.

CPU: the table holds what it claims, the references stay at the iteration limit for every LP and k, and the tolerance bites --
a step fraction off by 1e-9 or one entry of A off by 1e-8 moves the reference by more than twice the tolerance, while the
converged comparison of test_kernel_variants.py accepts the former.  GPU: every case asserts what served it, then every LP."""
import types

import numpy as np
import pytest

import scipy.sparse as sp

import test_kernel_variants as tkv
import test_workgroup_kernel_plans as twp
import trajectory as tj
from conftest import rel_err

IDS = [c.id for c in tj.CASES]

# what the table must hold: family -> point -> kinds (cold start); the warm start / autoscale rows; the degenerate cases
TABLE = {
    "slack": {"32x64": {"plain", "hsd", "pc", "guard"}, "24x30": {"bounded"}, "16x32": {"plain", "hsd", "pc"},
              "20x30": {"plain", "hsd", "pc"}},
    "group": {"32x96": {"plain", "hsd", "pc"}, "17x33": {"plain", "hsd", "pc"}},
    "tables": {"33x193": {"plain", "hsd", "pc", "pa", "pa-hsd", "pa-pc", "bounded"},
               "40x90": {"plain", "hsd", "pc", "pa", "pa-hsd", "pa-pc", "bounded"}},
    "image": {"100x80": {"plain", "hsd", "pc"}, "40x100": {"plain", "hsd", "pc"}},          # + bounded at its own row count
    "block": {"lds-paired-97x257": {"plain", "hsd", "pa", "pa-hsd"}, "l2-121x257": {"plain", "hsd"}},
    "big": None,                                                                            # four points x plain, hsd, pc
}
EXTRA_ROWS = {("warm", "plain"), ("autoscale", "plain"), ("autoscale", "hsd")}
DEGENERATE = {("group", "plain"), ("group", "pc"), ("tables", "plain"), ("tables", "pc"), ("image", "plain"), ("image", "pc"),
              ("block", "plain"), ("big", "plain"), ("big", "pc")}


def of_mode(mode):
    return [c for c in tj.CASES if c.mode == mode]


# ---- CPU ------------------------------------------------------------------------------------------------------------------
def test_table_holds_every_family_and_kind():
    cold = of_mode("cold")
    for family, points in TABLE.items():
        have = {}
        for c in cold:
            if c.family == family:
                have.setdefault(c.point, set()).add(c.kind)
        if family == "big":
            assert len(have) == 4 and all(kinds == {"plain", "hsd", "pc"} for kinds in have.values()), have
            grams = {(c.where[2], c.where[1][0]) for c in cold if c.family == "big"}
            assert grams == {(g, f) for g in twp.GRAMS for f in ("W", "L")}
            continue
        if family == "image":
            bounded = [p for p, kinds in have.items() if kinds == {"bounded"}]
            assert len(bounded) == 1 and bounded[0] == "%dx80" % tj.image_bounded_rows(80, (7, 4))
            del have[bounded[0]]
        assert have == points, (family, have)
    for family in TABLE:
        rows = {(c.mode, c.kind) for c in tj.CASES if c.family == family and c.mode in ("warm", "autoscale")}
        assert rows == EXTRA_ROWS, (family, rows)
        assert all(c.ks == tj.K_SHORT for c in tj.CASES if c.mode in ("warm", "autoscale"))
    assert {(c.family, c.kind) for c in of_mode("degenerate")} == DEGENERATE
    assert all(c.ks == (tj.K[:3] if c.id in tj.STOPS_AT_4 else tj.K) for c in cold + of_mode("degenerate"))
    assert set(tj.STOPS_AT_4) <= set(IDS)
    assert not any(c.kind == "bounded" for c in tj.CASES if c.mode != "cold")           # the bounded entries refuse both flags
    for c in tj.CASES:
        small = c.family == "big" or (c.family, c.kind) == ("image", "bounded")
        assert tj.inputs(c.key).nproblems == (tj.B_BIG if small else 13 if c.family == "block" and c.where else tj.B), c.id


def assert_point_is_served_first(c):
    """The point of case ``c`` is first covered by the shape, or has the plan, that ``c.where`` names."""
    bounded = c.kind == "bounded"
    P = tj.problem(c.key, bounded)
    m, N = P.A[0].shape
    A = sp.csr_matrix(P.A[0])
    if c.family in ("slack", "group"):
        assert P.tail == (c.family == "slack") and (c.flags & tj.NO_SLACK) == (0 if P.tail else tj.NO_SLACK), c.id
        assert tkv.first_covering(c.family, tkv.GROUP_SHAPES, m, N) == c.where, c.id
    elif c.family == "tables":
        assert tkv.first_covering("tables", tkv.WAVE_TAB_SHAPES, m, N) == c.where, c.id
        assert not tkv.tables_cannot_fit(m, N, P.tail, c.where, bounded) or A.nnz < 0.25 * m * N, c.id
    elif c.family == "image":
        assert tkv.first_covering("image", tkv.WAVE_DA_SHAPES, m, N) == c.where, c.id
        assert tkv.image_waves(m, N, P.tail, c.where, bounded) >= 1 and tkv.tables_cannot_fit(m, N, P.tail, c.where, bounded)
    elif c.family == "block" and c.where is not None:
        plan = twp.block_plan(m, N, A.nnz, pa=c.kind.startswith("pa"))
        assert plan[0] == c.where[1] and (m, N) == c.where[5:7], c.id
        assert plan[1] == (c.where[1] != "l2")                                       # a_in_lds 1 and 0
        assert (c.flags == tj.BLOCK) or twp.default_is_block(m, N), c.id
    elif c.family == "block":
        assert c.flags == tj.BLOCK and m <= twp.BLK_MAX_M and N <= twp.BLK_MAX_N
    else:
        cell, gram = c.where[1], c.where[2]
        assert twp.reachable(m, N) and twp.big_plan((m + 15) // 16, N)[0] == cell, c.id
        assert twp.gram_is_dense(A, P.tail) == (gram == "mfma"), c.id


def test_every_point_is_served_first_by_the_shape_or_plan_named():
    for c in tj.CASES:
        assert_point_is_served_first(c)
    # 32 x 64 runs on the (32, 96) kernel (4x4x4 tiles), 20 x 30 on padded rows and columns
    where = {c.point: c.where for c in tj.CASES if c.family == "slack" and c.kind == "plain" and c.mode == "cold"}
    assert where == {"32x64": (32, 96), "16x32": (16, 48), "20x30": (32, 64)}


def test_degenerate_inputs_have_no_identity_tail():
    for c in of_mode("degenerate"):
        P = tj.problem(c.key, False)
        assert not P.tail and P.shared, c.id
        A = P.A[0]
        assert 0 < np.abs(A[-1] - A[3]).max() <= 1e-5, c.id


@pytest.mark.parametrize("cid", IDS)
def test_reference_stays_at_the_iteration_limit_for_every_lp(cid):
    case = tj.BY_ID[cid]
    ref = tj.reference(cid)
    n = tj.inputs(case.key).nproblems
    for k in case.ks:
        assert ref[k]["status"].shape == (n,) and (ref[k]["status"] == 5).all(), (k, ref[k]["status"])
        assert (ref[k]["iters"] == k).all()
        for q in tj.quantities(case):
            assert np.isfinite(ref[k][q]).all() and len(ref[k][q]) == n


def converged(case, **kw):
    """The reference at convergence as the object ``assert_matches`` takes."""
    r = tj.run_reference(case, 200, **kw)
    return types.SimpleNamespace(primal_obj=r["pobj"], dual_obj=r["dobj"], **r)


@pytest.mark.parametrize("cid", IDS)
def test_tolerance_bites(cid):
    """A step fraction r (1 + 1e-9) moves x by more than twice the tolerance at every k -- and passes the converged comparison;
    one entry of A scaled by (1 + 1e-8) does so too.  Both on at least one LP of the batch: an LP that takes the full step
    (theta = 1) does not feel r at all."""
    case = tj.BY_ID[cid]
    ref, tol = tj.reference(cid), tj.tolerance(cid)
    for k in case.ks:
        assert tol[k]["x"] <= tj.CEILING
        d = tj.deviation(tj.run_reference(case, k, r_scale=1.0 + 1e-9)["x"], ref[k]["x"])
        assert d.max() > 2 * tol[k]["x"], (k, d.max(), tol[k]["x"])
        d = tj.deviation(tj.run_reference(case, k, a_scale=1.0 + 1e-8)["x"], ref[k]["x"])
        assert d.max() > 2 * tol[k]["x"], (k, d.max(), tol[k]["x"])
    if case.mode == "degenerate":
        return
    # the gap this file closes: the same perturbation passes the comparison at convergence
    s, r = converged(case, r_scale=1.0 + 1e-9), converged(case)
    if case.kind == "bounded":
        assert (s.status == 0).all() and (r.status == 0).all()
        assert np.abs(s.iters - r.iters).max() <= 1
        assert rel_err(s.primal_obj, r.primal_obj).max() <= 1e-9 and rel_err(s.dual_obj, r.dual_obj).max() <= 1e-9
        np.testing.assert_allclose(s.x, r.x, rtol=1e-5, atol=1e-6)
    else:
        tkv.assert_matches(s, dict(status=r.status, iters=r.iters, pobj=r.pobj, dobj=r.dobj, x=r.x), tj.inputs(case.key))


@pytest.mark.parametrize("cid", [c.id for c in of_mode("degenerate")])
def test_degenerate_case_exercises_refinement_and_the_pivot_floor(cid):
    case = tj.BY_ID[cid]
    ref, tol = tj.reference(cid), tj.tolerance(cid)
    n = tj.inputs(case.key).nproblems
    for k in case.ks:
        assert (ref[k]["nrefs"] == 5 * k).sum() >= n / 2, (k, ref[k]["nrefs"])            # refinement at its cap of 5 passes
        for opts in (dict(max_refine=0), dict(pivot_floor=1e-4)):
            d = tj.deviation(tj.run_reference(case, k, **opts)["x"], ref[k]["x"])
            assert d.max() > 2 * tol[k]["x"], (k, opts, d.max(), tol[k]["x"])


# ---- GPU ------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("cid", IDS)
def test_kernel_walks_the_reference_trajectory(cid):
    case = tj.BY_ID[cid]
    tj.assert_on_trajectory(case, tj.kernel_results(case))
