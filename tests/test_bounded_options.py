"""The five bounded kernels -- lane groups with shared and per-problem A, the wave kernel on term tables, on the dense image and
with per-problem A -- under refinement, the pivot floor and the forced guard, against the CPU twin at the same options
(tests/bounded_cases.py; tolerances by the rule of tests/trajectory.py under the row's options, nothing from the kernel).

CPU: the degenerate inputs are degenerate LP by LP, keep one pivot per factorisation at the floor and refinement at its cap, and
stay clear of the guard's term, so that every LP must end at the iteration limit on the wave kernels too; every option row moves
the twin by more than twice its tolerance; refine_tol = 1e-8 is neither the default nor 'no refinement'.  GPU: every row asserts
what served the launch, then every LP.  The per-problem dense-image wave kernel (not bounded, against the oracle) has its delta, r
and stopping rows here too: no path of tests/option_cases.py reaches it.

The GPU tests append their measured deviations to the file PYCLLP_TRAJECTORY_REPORT names
(profiles/bounded_options/deviations.txt)."""
import numpy as np
import pytest

import bounded_cases as bc
import dense_batch_wave_cases as wc
import general_batch_cases as gbc
import option_cases as oc
import sparse_general_batch_cases as sgc
import trajectory as tj

ROWS = {r.id: r for r in bc.option_rows() + bc.image_per_problem_rows()}
IMAGE = bc.image_per_problem_case()
GUARD_ROWS = {r.id: r for r in bc.guard_rows()}
DEGENERATE = {c.id: c for c in bc.degenerate_cases()}
PER_PROBLEM = {c.id: c for c in bc.per_problem_cases()}
STOPPING = dict(PER_PROBLEM, **{IMAGE.id: IMAGE})


def kernel_results(case, ks, **opts):
    return (bc.image_per_problem_results if case is IMAGE else tj.kernel_results)(case, ks, **opts)


# ---- CPU ------------------------------------------------------------------------------------------------------------------
def test_table_holds_the_five_kernels():
    assert [c.family for c in bc.degenerate_cases()] == ["slack", "tables", "image", "perA-group", "perA-wave"]
    assert all(c.kind == "bounded" and c.mode == "degenerate" and c.ks == (1, 2, 4) for c in bc.degenerate_cases())
    assert [c.id for c in bc.shared_cases()] == ["slack-24x30-bounded", "tables-40x90-bounded",
                                                 "image-%dx80-bounded" % tj.image_bounded_rows(80, (7, 4))]
    group, wave = bc.per_problem_cases()
    assert tj.inputs(group.key) is gbc.trajectory_lp("16-row") and group.where == (16, 32)
    assert tj.inputs(wave.key) is sgc.trajectory_lp("P1") and wave.where == sgc.POINTS["P1"][3]
    for c in bc.degenerate_cases():
        assert tj.inputs(c.key).nproblems == tj.inputs(c.key[1]).nproblems in (tj.B, tj.B_BIG, gbc.B_TRAJ)
        assert tj.quantities(c) == ("x", "z", "s", "aty")
    names = lambda cid: sorted(r.id.rsplit(":", 1)[1] for r in bc.option_rows() if r.case.id == cid)
    for cid in DEGENERATE:
        assert names(cid) == ["default", "max_refine", "pivot_floor", "refine_tol"]
    for cid in PER_PROBLEM:
        assert names(cid) == ["delta", "r"]
    assert len(bc.option_rows()) == 4 * 5 + 2 * 2 and all(len(bc.row_ks(r)) >= 2 for r in ROWS.values())
    lp = tj.inputs(IMAGE.key)
    assert lp is wc.trajectory_lp() and lp.A.nproblems == lp.nproblems and IMAGE.kind == "plain" and IMAGE.flags == 0
    assert [r.id for r in bc.image_per_problem_rows()] == ["%s:delta" % IMAGE.id, "%s:r" % IMAGE.id]
    assert dict(ROWS["%s:refine_tol" % next(iter(DEGENERATE))].opts) == dict(refine_tol=1e-8)
    guard = [r.case for r in bc.guard_rows()]
    assert [(c.family, c.mode, c.ks) for c in guard] == [("slack", "cold", tj.K), ("perA-group", "cold", tj.K),
                                                         ("slack", "degenerate", bc.KS), ("perA-group", "degenerate", bc.KS)]
    for c in guard:
        plain = bc.unforced(c)
        assert c.flags == tj.GUARD and plain.flags == 0 and c._replace(id=plain.id, flags=0) == plain


@pytest.mark.parametrize("cid", list(DEGENERATE))
def test_degenerate_input_is_the_bounded_input_with_a_near_duplicate_row(cid):
    """Row 3 and the last kept row are equality rows through one interior point and differ by 1e-6, in every LP's own matrix;
    everything else -- the other rows, the column bounds with their fixed columns and missing upper bounds, the costs -- is the
    well-conditioned input's."""
    lp, src = tj.inputs(DEGENERATE[cid].key), tj.inputs(DEGENERATE[cid].key[1])
    P = tj.problem(DEGENERATE[cid].key, True)
    keep = P.bmap.rows
    last, n = int(keep[-1]), lp.ncols
    assert P.tail and P.shared == (lp.A.nproblems == 1) and len(P.A) == (1 if P.shared else lp.nproblems)
    for i in (3, last):
        assert np.array_equal(lp.a[:, i], lp.b[:, i]) and np.isfinite(lp.b[:, i]).all()
    others = np.setdiff1d(np.arange(lp.nrows), [3, last])
    for q in ("c", "l", "u", "f"):
        assert np.array_equal(getattr(lp, q), getattr(src, q)), q
    assert np.array_equal(lp.a[:, others], src.a[:, others]) and np.array_equal(lp.b[:, others], src.b[:, others])
    assert (lp.u == lp.l).any() and np.isinf(lp.u).any() and np.isfinite(lp.u).any()
    k3, kl = int(np.flatnonzero(keep == 3)[0]), len(keep) - 1
    for A in P.A:
        assert 0 < np.abs(A[kl, :n] - A[k3, :n]).max() <= 1e-5
    assert (P.u[:, n + k3] == 0).all() and (P.u[:, n + kl] == 0).all()                  # both slacks fixed
    assert P.shared or not np.array_equal(P.A[0][kl, :n] - P.A[0][k3, :n], P.A[1][kl, :n] - P.A[1][k3, :n])


@pytest.mark.parametrize("cid", list(DEGENERATE))
def test_degenerate_input_keeps_the_floor_and_refinement_busy_and_the_guard_quiet(cid):
    """Per LP and iteration one pivot at least meets the floor; at the default options refinement spends its 5 passes per
    iteration on half of the LPs at least; and the guard's own term stays below 0.9 of the pivot under every option of the
    rows, which is what lets the GPU tests demand status 5 from the wave kernels (their exit 'the guard would have bitten')."""
    n = tj.inputs(DEGENERATE[cid].key).nproblems
    for k in bc.KS:
        ref = tj.reference(cid, (), (k,))[k]
        assert ref["floored"].shape == (n,) and (ref["floored"] >= k).all(), (k, ref["floored"])
        assert (ref["nrefs"] == 5 * k).sum() >= n / 2, (k, ref["nrefs"])
        for _, opts, _ in bc.ON_DEGENERATE:
            ref = tj.reference(cid, bc.KEY(opts), (k,))[k]
            assert (ref["guard_ratio"] <= bc.GUARD_RATIO).all(), (k, opts, ref["guard_ratio"])
            assert (ref["nrefs"] <= opts.get("max_refine", 5) * k).all()


@pytest.mark.parametrize("rid", list(ROWS))
def test_row_stays_at_the_iteration_limit_and_bites(rid):
    """For every k kept: the twin at the row's options has status 5 after exactly k iterations for every LP, a tolerance that
    respects the ceiling, and differs from the twin at the row's base by more than twice the tolerance -- a kernel that did not
    read the option would fail the row.  The refine_tol rows differ as much from the twin without refinement."""
    row = ROWS[rid]
    case, ks = row.case, bc.row_ks(row)
    ref, tol = (f(case.id, row.opts, ks) for f in (tj.reference, tj.tolerance))
    n = tj.inputs(case.key).nproblems
    for k in ks:
        assert ref[k]["status"].shape == (n,) and (ref[k]["status"] == 5).all() and (ref[k]["iters"] == k).all(), k
        for q in tj.quantities(case):
            assert np.isfinite(ref[k][q]).all() and tj.FLOOR <= tol[k][q] <= tj.CEILING, (k, q, tol[k][q])
        moved, bound = oc.bite(row, k)
        assert moved > 2 * bound, (k, moved, bound)
        if rid.endswith(":refine_tol"):
            moved, bound = oc.bite(row._replace(base=bc.NO_REFINEMENT), k)
            assert moved > 2 * bound, (k, moved, bound)


def test_dropped_points_do_not_bite():
    for (rid, k), reason in bc.dropped().items():
        moved, bound = oc.bite(ROWS[rid], k)
        assert reason and moved <= 2 * bound, (rid, k, moved, bound)


@pytest.mark.parametrize("rid", list(GUARD_ROWS))
def test_guard_row_has_a_reference_the_guard_does_not_decide(rid):
    """The twin's factor is the guarded one.  Its term stays below the pivot on every LP of the forced rows, so the forced and
    the unforced launch are held to one reference; the bound is the unforced case's."""
    row = GUARD_ROWS[rid]
    case, ks = row.case, bc.row_ks(row)
    ref, tol = tj.reference(case.id, row.opts, ks), tj.tolerance(case.id, row.opts, ks)
    plain = tj.reference(bc.unforced(case).id, row.opts, ks)
    for k in ks:
        assert (ref[k]["status"] == 5).all() and (ref[k]["iters"] == k).all() and (ref[k]["guard_ratio"] < 1).all()
        for q in tj.quantities(case):
            assert np.array_equal(ref[k][q], plain[k][q]) and tj.FLOOR <= tol[k][q] <= tj.CEILING, (k, q, tol[k][q])


@pytest.mark.parametrize("cid", list(STOPPING))
def test_stopping_row_ends_early_and_decisively(cid):
    st = oc.stopping(cid)
    n = tj.inputs(STOPPING[cid].key).nproblems
    assert st.ref["status"].shape == (n,) and (st.ref["status"] == 0).all() and (st.default["status"] == 0).all()
    assert (st.ref["iters"] <= st.default["iters"] - 3).all(), (st.ref["iters"], st.default["iters"])
    assert st.default["iters"].max() < oc.CAP
    assert 4 * st.decisive.sum() >= 3 * n, (st.decisive.sum(), n)
    assert all(tj.FLOOR <= t <= tj.CEILING for t in st.tol.values())


# ---- GPU ------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("rid", list(ROWS))
def test_kernel_follows_the_twin_under_the_option(rid):
    row = ROWS[rid]
    ks = bc.row_ks(row)
    oc.assert_on_row(row, kernel_results(row.case, ks, **dict(row.opts)), ks)


@pytest.mark.gpu
@pytest.mark.parametrize("rid", list(GUARD_ROWS))
def test_forced_guard_follows_the_twin(rid):
    """The guarded factor on the lane-group kernels, k by k.  Whether it gives the bits of the unforced launch goes into the
    report and is not asserted: where the guard does not bite both are factors of one matrix, not one instruction sequence."""
    row = GUARD_ROWS[rid]
    ks = bc.row_ks(row)
    got = tj.kernel_results(row.case, ks)
    plain = tj.kernel_results(bc.unforced(row.case), ks)
    same = bc.same_bits(got, plain, ks, tj.quantities(row.case))
    oc.report(["%s forced launch %s the unforced one" % (rid, "has the bits of" if same else "differs in bits from")])
    oc.assert_on_row(row, got, ks)


@pytest.mark.gpu
@pytest.mark.parametrize("cid", list(STOPPING))
def test_kernel_stops_with_the_twin_at_eps(cid):
    case = STOPPING[cid]
    got = kernel_results(case, (oc.CAP,), eps=oc.EPS)[oc.CAP]
    oc.assert_stops_with_the_reference(case, got)
