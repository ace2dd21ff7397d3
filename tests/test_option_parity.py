"""Option parity: every numerical field of ``pycllp_hip_opts`` -- eps, delta, r, pivot_floor, refine_tol, max_iter, max_refine --
at a non-default value on every arithmetic path, against the CPU references at the same value (tests/option_cases.py; tolerances
by the rule of tests/trajectory.py under the row's options, nothing from the kernel).

CPU: the table holds exactly the paths of ``trajectory.CASES`` and ``dense_batch_cases.TRAJECTORY_POINTS``; every row keeps the
reference at the iteration limit and MOVES it by more than twice the tolerance (a kernel that ignored the option would fail the
row); the points left out do not; predictor-corrector does not read delta; the stopping rows end early and decisively; the
Newton rows move A'dy and have a reproducible pass count.  GPU: every row asserts what served the launch, then every LP.

The GPU tests append their measured deviations to the file PYCLLP_TRAJECTORY_REPORT names
(profiles/option_parity/deviations.txt)."""
import numpy as np
import pytest

import dense_batch_cases as dbc
import option_cases as oc
import trajectory as tj

ROWS = {r.id: r for r in oc.iterate_rows()}
PATHS = {c.id: c for c in oc.paths()}
NEWTON = {c.id: c for c in oc.newton_cases()}
NEWTON_IDS = ["%s:%s" % (cid, name) for cid in NEWTON for name, _ in oc.NEWTON_ROWS]


# ---- CPU ------------------------------------------------------------------------------------------------------------------
def test_table_holds_exactly_the_paths():
    """One path per (family, kind) of the cold cases, per LDS plan of the block kernel and per (Gram path, factor storage) of
    the large-LP kernel, each at the smallest m^2 N among its points; the per-problem kernel on both its tables."""
    cold = [c for c in tj.CASES if c.mode == "cold"]

    def size(c):
        m, N = tj.problem(c.key, c.kind == "bounded").A[0].shape
        return m * m * N

    want = {}
    for c in cold:
        cell = c.where[1] if c.family == "block" else (c.where[2], c.where[1][0]) if c.family == "big" else None
        k = (c.family, c.kind, cell)
        if k not in want or size(c) < size(want[k]):
            want[k] = c
    have = [c for c in oc.paths() if c.family != "perA"]
    assert sorted(c.id for c in have) == sorted(c.id for c in want.values())
    assert {(c.family, c.kind) for c in have} == {(c.family, c.kind) for c in cold}
    assert {c.where[1] for c in have if c.family == "block"} == {"lds-paired", "l2"}
    assert len({(c.where[2], c.where[1][0]) for c in have if c.family == "big"}) == 4
    per = [c for c in oc.paths() if c.family == "perA"]
    m, n, slack = min(dbc.TRAJECTORY_POINTS.values(), key=lambda p: p[0] * p[0] * p[1])
    assert sorted((c.where[1], c.flags) for c in per) == [(0, tj.NO_SLACK), (1, 0)]
    for c in per:
        lp = tj.inputs(c.key)
        assert (lp.nrows, lp.ncols, lp.nproblems) == (m, n, dbc.B_TRAJ) and lp.A.nproblems == dbc.B_TRAJ
        assert c.where[0] == dbc.first_covering(m, n, bool(c.where[1]))
    for c in oc.paths():
        small = c.family == "big" or (c.family, c.kind) == ("image", "bounded")
        nb = dbc.B_TRAJ if c.family == "perA" else tj.B_BIG if small else 13 if c.family == "block" else tj.B
        assert tj.inputs(oc.stop_case(c).key).nproblems == tj.inputs(c.key).nproblems == nb, c.id


def test_rows_cover_every_option_on_the_paths_that_read_it():
    rows = oc.iterate_rows()
    on = lambda name: {r.case.id for r in rows if r.id.endswith(":" + name)}
    assert on("r") == set(PATHS)
    assert on("delta") == {cid for cid, c in PATHS.items() if not c.kind.endswith("pc")}
    degenerate = {c.id for c in tj.CASES if c.mode == "degenerate"}
    assert {c.kind for c in tj.CASES if c.mode == "degenerate"} == {"plain", "pc"}
    per = [r.case for r in rows if r.case.family == "perA" and r.case.mode == "degenerate"]
    assert len({c.id for c in per}) == 1 and per[0].where[1] == 0 and not tj.problem(per[0].key, False).tail
    for name in ("max_refine", "refine_tol", "pivot_floor"):
        assert {cid for cid in on(name) if not cid.endswith("hsd-degenerate")} >= degenerate | {per[0].id}
    hsd = oc.hsd_degenerate_cases()
    assert [c.family for c in hsd] == ["group", "tables", "image", "block", "big"] and all(c.kind == "hsd" for c in hsd)
    big = hsd[-1]
    assert big.where[2] == "mfma" and big.where[1][0] == "L"
    for name in ("base", "max_refine0", "max_refine2", "refine_tol"):
        assert on(name) >= {c.id for c in hsd}
    for r in rows:
        if r.id.endswith("hsd-degenerate:base"):
            assert dict(r.opts) == dict(pivot_floor=1e-3) and dict(r.base) == dict(pivot_floor=1e-6)
        elif r.case.id.endswith("hsd-degenerate"):
            assert dict(r.base) == dict(pivot_floor=1e-3) and len(r.opts) == 2 and dict(r.opts)["pivot_floor"] == 1e-3
        else:
            assert len(r.opts) == 1 and r.base == ()
        assert set(oc.row_ks(r)) <= set(oc.KS) and oc.row_ks(r)                          # (a row left with no k raises)


def test_per_problem_degenerate_batch_is_degenerate_lp_by_lp():
    case = next(r.case for r in oc.iterate_rows() if r.case.family == "perA" and r.case.mode == "degenerate")
    P = tj.problem(case.key, False)
    assert not P.shared and not P.tail and len(P.A) == dbc.B_TRAJ
    for A in P.A:
        assert 0 < np.abs(A[-1] - A[3]).max() <= 1e-5
    assert not np.array_equal(P.A[0], P.A[1])


@pytest.mark.parametrize("rid", list(ROWS))
def test_row_stays_at_the_iteration_limit_and_bites(rid):
    """For every k kept: the reference at the row's options has status 5 after exactly k iterations for every LP, a tolerance
    that respects the ceiling, and differs from the reference at the row's base by more than twice the tolerance on at least
    one LP -- a kernel that did not read the option would fail the row."""
    row = ROWS[rid]
    case, ks = row.case, oc.row_ks(row)
    ref, tol, spread = (f(case.id, row.opts, ks) for f in (tj.reference, tj.tolerance, tj.spread))
    n = tj.inputs(case.key).nproblems
    for k in ks:
        assert ref[k]["status"].shape == (n,) and (ref[k]["status"] == 5).all() and (ref[k]["iters"] == k).all(), k
        for q in tj.quantities(case):
            assert np.isfinite(ref[k][q]).all() and tol[k][q] <= tj.CEILING, (k, q, tol[k][q])
        moved, bound = oc.bite(row, k)
        assert moved > 2 * bound, (k, moved, bound)
        if rid.endswith("hsd-degenerate:base"):
            # refinement at the AUTO cap of the HSD kernels (20 passes per iteration), and a reproducible reference
            assert (ref[k]["nrefs"] == 20 * k).sum() >= n / 2, (k, ref[k]["nrefs"])
            assert max(spread[k].values()) < tj.CEILING / tj.FACTOR


def test_dropped_points_do_not_bite():
    for (rid, k), reason in oc.dropped().items():
        moved, bound = oc.bite(ROWS[rid], k)
        assert reason and moved <= 2 * bound, (rid, k, moved, bound)
    assert {rid for rid, k in oc.dropped() if k == 1 and rid.endswith(":delta")} == {
        "%s:delta" % cid for cid, c in PATHS.items() if c.kind.endswith("hsd")}


def test_pc_does_not_read_delta():
    """A fact of the algorithm, recorded: Mehrotra's rule sets the centring itself, so delta moves the reference by exactly 0."""
    rows = oc.pc_delta_rows()
    assert {r.case.id for r in rows} == {cid for cid, c in PATHS.items() if c.kind.endswith("pc")} and rows
    for row in rows:
        for k in oc.KS:
            ref, base = (tj.reference(row.case.id, o, (k,))[k] for o in (row.opts, row.base))
            for q in tj.quantities(row.case):
                assert np.array_equal(ref[q], base[q]), (row.id, k, q)


@pytest.mark.parametrize("pid", list(PATHS))
def test_stopping_row_ends_early_and_decisively(pid):
    case = oc.stop_case(PATHS[pid])
    st = oc.stopping(case.id)
    n = tj.inputs(case.key).nproblems
    assert st.ref["status"].shape == (n,) and (st.ref["status"] == 0).all() and (st.default["status"] == 0).all()
    assert (st.ref["iters"] <= st.default["iters"] - 3).all(), (st.ref["iters"], st.default["iters"])
    assert st.default["iters"].max() < oc.CAP
    assert 4 * st.decisive.sum() >= 3 * n, (st.decisive.sum(), n)
    assert all(tj.FLOOR <= t <= tj.CEILING for t in st.tol.values())


@pytest.mark.parametrize("cid", list(NEWTON))
def test_newton_rows_move_the_step_and_count_reproducibly(cid):
    P = tj.problem(NEWTON[cid].key, False)
    assert P.shared and not P.tail and 0 < np.abs(P.A[0][-1] - P.A[0][3]).max() <= 1e-5
    base = oc.newton(cid, oc.KEY({}))
    for name, opts in oc.NEWTON_ROWS:
        nw = oc.newton(cid, oc.KEY(opts))
        assert nw.ref["aty"].shape == (oc.NEWTON_SYSTEMS, P.A[0].shape[1]) and np.isfinite(nw.ref["aty"]).all()
        assert nw.tol <= tj.CEILING and 4 * nw.stable.sum() >= 3 * oc.NEWTON_SYSTEMS, (name, nw.tol, nw.stable)
        if "max_refine" in opts:
            assert (nw.ref["nrefine"] <= opts["max_refine"]).all()
        if opts:
            moved = float(tj.deviation(nw.ref["aty"], base.ref["aty"]).max())
            assert moved > 2 * nw.tol, (name, moved, nw.tol)
    assert (base.ref["nrefine"] == 5).sum() >= oc.NEWTON_SYSTEMS / 2                      # refinement at its default cap


def test_families_named():
    assert {c.family for c in NEWTON.values()} == set(oc.NEWTON_FAMILIES) and len(NEWTON) == len(oc.NEWTON_FAMILIES)
    assert NEWTON["block-40x90-no-tail-plain-degenerate"].flags == tj.BLOCK


# ---- GPU ------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("rid", list(ROWS))
def test_kernel_follows_the_reference_under_the_option(rid):
    row = ROWS[rid]
    oc.assert_on_row(row, oc.kernel_results(row.case, oc.row_ks(row), **dict(row.opts)))


@pytest.mark.gpu
@pytest.mark.parametrize("pid", list(PATHS))
def test_kernel_stops_with_the_reference_at_eps(pid):
    case = oc.stop_case(PATHS[pid])
    got = oc.kernel_results(case, (oc.CAP,), eps=oc.EPS)[oc.CAP]
    oc.assert_stops_with_the_reference(case, got)


@pytest.mark.gpu
@pytest.mark.parametrize("nid", NEWTON_IDS)
def test_newton_entry_under_the_option(nid):
    cid, name = nid.rsplit(":", 1)
    opts = dict(oc.NEWTON_ROWS)[name]
    case, nw = NEWTON[cid], oc.newton(cid, oc.KEY(opts))
    dy, nrefine = oc.newton_kernel(case, **opts)
    A = tj.problem(case.key, False).A[0]
    dev = tj.deviation(dy @ A, nw.ref["aty"])
    oc.report(["%s:newton:%s A'dy %.1e (tol %.1e)  nrefine %s (oracle %s, compared on %d of %d)" % (
        cid, name, dev.max(), nw.tol, nrefine.tolist(), nw.ref["nrefine"].tolist(), nw.stable.sum(), nw.stable.size)])
    assert dev.shape == (oc.NEWTON_SYSTEMS,) and dev.max() <= nw.tol, (dev.max(), nw.tol)
    assert np.array_equal(nrefine[nw.stable], nw.ref["nrefine"][nw.stable]), (nrefine, nw.ref["nrefine"], nw.stable)
