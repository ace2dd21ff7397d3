"""Option pairs: warm start on the embedding, warm start under autoscale (the three divisions of the incoming x, y, z), either with
predictor-corrector, all of them on per-problem values of A, and PYCLLP_FLAG_FORCE_GUARD_PATH with each -- after k = 1, 2, 4, 8
iterations against the CPU references under the same flags and start (tests/pair_cases.py on the machinery of
tests/trajectory.py: the same tolerance rule, nothing from the kernel).

CPU: the table holds exactly its rows; the references stay at the iteration limit; the bound bites (r, one entry of A); the PAIR
bites -- the reference with one option of the pair taken away, or started as a kernel that skipped a division would start, is
off by more than twice the bound at every k; the scaled start is what it claims.  GPU: every row asserts what served it (a
deferred row: that the block kernel did), then every LP, quantity and k; then the same row to convergence; and warm starts with
each option through the plugins' ``lp.solve()``.

FORCE_GUARD_PATH | PREDCORR on the wave kernel is pinned as include/pycllp_hip.h states it: the block kernel finishes the
deferred LPs on the reference's plain rule -- the rows assert the plain reference's iterates and not the predictor-corrector's.

The GPU tests append their measured deviations to the file PYCLLP_TRAJECTORY_REPORT names
(profiles/option_pairs/deviations.txt)."""
import numpy as np
import pytest

import pair_cases as pc
import test_kernel_variants as tkv
import test_trajectory_parity as ttp
import trajectory as tj
from conftest import rel_err

ROWS = {r.case.id: r for r in pc.rows()}
IDS = list(ROWS)


# ---- CPU ------------------------------------------------------------------------------------------------------------------
def test_table_holds_exactly_the_pair_rows():
    have = {}
    for r in ROWS.values():
        c = r.case
        have.setdefault((r.serve, tuple(sorted(tj.modes(c))), r.pair[len(tj.modes(c)):]), set()).add((c.family, c.point))
    eight = {("slack", "32x64"), ("group", "32x96"), ("tables", "40x90"), ("image", "100x80"), ("block", "lds-paired-97x257"),
             ("block", "l2-121x257"), ("big", "mfma-L3x3-8x513"), ("big", "terms-L3x3-1x513")}
    six = eight - {("block", "lds-paired-97x257"), ("block", "l2-121x257")}
    tables, lds = {("tables", "40x90")}, {("block", "lds-paired-97x257")}
    inside = {("slack", "32x64"), ("big", "mfma-L3x3-8x513")}
    w, a, wa = ("warm",), ("autoscale",), ("autoscale", "warm")
    want = {
        ("kernel", w, ("hsd",)): eight, ("kernel", w, ("pa", "hsd")): tables | lds,
        ("kernel", w, ("pc",)): six, ("kernel", w, ("pa", "pc")): tables, ("kernel", w, ("pa",)): tables | lds,
        ("kernel", a, ("pc",)): six,
        ("kernel", a, ("pa",)): tables | lds, ("kernel", a, ("pa", "hsd")): tables | lds, ("kernel", a, ("pa", "pc")): tables,
        ("kernel", wa, ()): eight, ("kernel", wa, ("hsd",)): eight, ("kernel", wa, ("pc",)): six, ("kernel", wa, ("pa",)): tables | lds,
        ("guard", (), ("hsd", "guard")): inside, ("guard", (), ("pc", "guard")): inside, ("guard", w, ("guard",)): inside,
        ("guard", a, ("guard",)): inside, ("guard", wa, ("guard",)): inside,
        ("deferred", (), ("guard",)): tables, ("deferred", (), ("hsd", "guard")): tables, ("deferred", w, ("guard",)): tables,
        ("deferred", a, ("guard",)): tables, ("deferred", w, ("hsd", "guard")): tables, ("deferred", wa, ("guard",)): tables,
        ("deferred", (), ("pa", "guard")): tables, ("deferred", w, ("pa", "guard")): tables,
        ("pc-deferred", (), ("pc", "guard")): tables | {("image", "100x80")},
    }
    assert have == want
    assert len(ROWS) == sum(len(v) for v in want.values()) == 74
    for r in ROWS.values():
        c = r.case
        assert c.id not in {x.id for x in tj.CASES} and c.margin is None
        assert c.ks == tuple(k for k in tj.K if k <= pc.STOPS.get(c.id, (8,))[0]) and len(c.ks) >= 3, c.id
        assert bool(c.flags & tj.GUARD) == (r.serve != "kernel") and bool(c.flags & pc.PREDCORR) == (r.serve == "pc-deferred"), c.id
        assert (c.key[0] == "scaled") == ("autoscale" in tj.modes(c)), c.id
        assert tj.problem(c.key, False).shared != ("pa" in r.pair), c.id
        assert c.kind == ("plain" if r.serve == "pc-deferred" else "-".join(o for o in r.pair if o in ("pa", "hsd", "pc")) or "plain")
        n = tj.inputs(c.key).nproblems
        assert n == (tj.B_BIG if c.family == "big" else 13 if c.family == "block" else tj.B), c.id
        if r.serve in ("deferred", "pc-deferred"):                  # the wave kernel, with a block kernel behind it
            assert c.family in ("tables", "image") and not (c.flags & tj.BLOCK)
            m, N = tj.problem(c.key, False).A[0].shape
            assert m <= ttp.twp.BLK_MAX_M and N <= ttp.twp.BLK_MAX_N
        assert pc.fakes(r) or r.pair in (("guard",), ("pa", "guard")), c.id


@pytest.mark.parametrize("cid", IDS)
def test_point_is_served_first_by_the_shape_or_plan_named(cid):
    ttp.assert_point_is_served_first(ROWS[cid].case)


@pytest.mark.parametrize("cid", IDS)
def test_reference_stays_at_the_iteration_limit_for_every_lp(cid):
    case = ROWS[cid].case
    ref, tol = tj.reference(cid), tj.tolerance(cid)
    n = tj.inputs(case.key).nproblems
    for k in case.ks:
        assert ref[k]["status"].shape == (n,) and (ref[k]["status"] == 5).all(), (k, ref[k]["status"])
        assert (ref[k]["iters"] == k).all()
        for q in tj.quantities(case):
            assert np.isfinite(ref[k][q]).all() and len(ref[k][q]) == n
            assert tol[k][q] <= tj.CEILING, (k, q, tol[k][q])


@pytest.mark.parametrize("cid", IDS)
def test_tolerance_bites(cid):
    """As test_trajectory_parity.test_tolerance_bites: r (1 + 1e-9), and one entry of A times (1 + 1e-8), move the reference's x
    by more than twice the bound at every k kept."""
    case = ROWS[cid].case
    ref, tol = tj.reference(cid), tj.tolerance(cid)
    for k in case.ks:
        for what in (dict(r_scale=1.0 + 1e-9), dict(a_scale=1.0 + 1e-8)):
            d = pc.moved(case, k, ref[k], **what)
            assert d > 2 * tol[k]["x"], (k, what, d, tol[k]["x"])


@pytest.mark.parametrize("cid", IDS)
def test_pair_bites(cid):
    """Every fake of ``pair_cases.fakes`` -- a kernel that ignored one option of the pair, or skipped a division of the warm
    start under autoscale -- is off by more than twice the bound in x at every k kept: it would fail the row."""
    row = ROWS[cid]
    ref, tol = tj.reference(cid), tj.tolerance(cid)
    names = [f[0] for f in pc.fakes(row)]
    if {"warm", "autoscale"} <= set(row.pair):
        assert {"no warm", "no autoscale", "none divided", "y undivided", "x undivided"} <= set(names)
    if row.serve == "pc-deferred":
        assert names == ["pc"]
    else:
        assert set(names) >= {"no " + o for o in row.pair if o in ("warm", "autoscale", "hsd", "pc")}, names
    for fake in pc.fakes(row):
        name, q = fake[0], fake[3]
        assert q == ("y" if name == "y undivided" else "x")
        for k in row.case.ks:
            d = pc.fake_moved(fake, k, ref[k])
            assert d > 2 * tol[k][q], (name, k, q, d, tol[k][q])
            if q == "y":
                # a fact of the algorithm, recorded: x and z do not depend on the y the solve starts from
                for other in ("x", "z"):
                    d = pc.fake_moved(fake, k, ref[k], other)
                    assert d <= tol[k][other], (name, k, other, d, tol[k][other])


def test_ladders_stop_only_where_stated():
    """Each dropped k of ``pair_cases.STOPS`` is still one at which the row would be no test: the bound passes CEILING, or one
    of the 'must bite' perturbations no longer moves x by twice the bound."""
    for cid, (last, reason) in pc.STOPS.items():
        row = ROWS[cid]
        case = row.case
        assert reason and last in tj.K[:-1]
        for k in (k for k in tj.K if k > last):
            ref, tol = tj.reference(cid, (), (k,))[k], tj.tolerance(cid, (), (k,))[k]
            bites = [pc.moved(case, k, ref, r_scale=1.0 + 1e-9), pc.moved(case, k, ref, a_scale=1.0 + 1e-8)]
            bites += [pc.fake_moved(f, k, ref) / tol[f[3]] * tol["x"] for f in pc.fakes(row)]
            assert max(tol.values()) > tj.CEILING or min(bites) <= 2 * tol["x"], (cid, k)


def test_scaled_warm_point_is_the_warm_point_after_the_division():
    for r in ROWS.values():
        case = r.case
        if not {"warm", "autoscale"} <= tj.modes(case):
            continue
        P = tj.problem(case.key, False)
        base = tj.problem(case.key[1], False)
        assert np.array_equal(P.b, base.b * 1e3) and np.array_equal(P.c, base.c * 1e-2)
        sb, sc = np.abs(P.b).max(axis=1, keepdims=True), np.abs(P.c).max(axis=1, keepdims=True)
        assert sb.min() > 10 and sc.max() < 0.1                                          # (far enough for a missing division to show)
        for got, scale, want in zip(tj.start_point(case, P), (sb, sc, sc), tj.warm_point(P.b.shape[0], *P.A[0].shape)):
            assert got.shape == want.shape and (np.abs(got / scale - want) <= np.spacing(np.abs(want))).all(), case.id
        # and the rows that are warm only start from the point itself
        plain = tj.start_point(case._replace(mode="warm"), P)
        assert all(np.array_equal(a, b) for a, b in zip(plain, tj.warm_point(P.b.shape[0], *P.A[0].shape)))


# ---- GPU ------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("cid", IDS)
def test_kernel_walks_the_reference_trajectory_under_the_pair(cid):
    row = ROWS[cid]
    pc.assert_on_trajectory(row, pc.kernel_results(row))


@pytest.mark.gpu
@pytest.mark.parametrize("cid", IDS)
def test_pair_converges_like_the_reference(cid):
    pc.assert_converges_like_the_reference(ROWS[cid])


PLUGINS = [("hip_dense_primal_normal", 16, 32), ("hip_sparse_primal_normal", 40, 90)]
PLUGIN_OPTIONS = {"hsd": (dict(hsd=True), 32), "pc": (dict(predcorr=True, hsd=False), 128), "autoscale": (dict(autoscale=True), 8)}


@pytest.mark.gpu
@pytest.mark.parametrize("option", list(PLUGIN_OPTIONS))
@pytest.mark.parametrize("name,m,n", PLUGINS, ids=[p[0] for p in PLUGINS])
def test_repeat_solve_warm_start_with_the_option_through_the_plugin_api(name, m, n, option):
    """``warm_start=True`` with hsd, predcorr or autoscale through ``lp.solve()`` twice (the second time on data varied by 1 %):
    the second solve ends optimal everywhere, at the cold reference's objectives, and matches the oracle under the same flags
    from the same lifted start."""
    from oracle import port
    from pycllp_amd import problems
    from pycllp_amd.lp import SparseMatrix, StandardLP
    from pycllp_amd.solvers import solver_registry
    from pycllp_amd.solvers.hip import warm_lifted
    kw, flags = PLUGIN_OPTIONS[option]
    rs = np.random.RandomState(3)
    if name.startswith("hip_dense"):
        A, b, c = problems.random_dense_arrays(m, n, tj.B, seed=6)
    else:
        A, b, c = problems.random_sparse_arrays(m, n, tj.B, density=0.1, seed=6)
    lp = StandardLP(SparseMatrix(matrix=A), b, c, 0.0).to_equality_form()
    s = solver_registry[name](device="cuda:0", warm_start=True, **kw)
    lp.init(s)
    lp.solve(s)                                                  # first solve: cold by definition
    assert (s.status == 0).all(), s.status
    x0, y0, z0 = s.x.copy(), s.y.copy(), s.z.copy()
    lp.b[:] = lp.b * (1.0 + 0.01 * rs.rand(*lp.b.shape))
    lp.c[:, :n] = lp.c[:, :n] * (1.0 + 0.01 * rs.rand(tj.B, n))
    lp.solve(s)
    Ad = np.asarray(lp.A.todense(), dtype=np.float64)
    cold = port.dense_solve(Ad, lp.b, lp.c, nthreads=8, flags=flags)
    r = port.dense_solve(Ad, lp.b, lp.c, nthreads=8, x0=warm_lifted(x0), y0=y0, z0=warm_lifted(z0), flags=flags | tj.WARM)
    print("%s %s: iters kernel %s oracle %s cold %s" % (name, option, s.iters.tolist(), r["iters"].tolist(), cold["iters"].tolist()))
    assert (s.status == 0).all() and (cold["status"] == 0).all(), (s.status, cold["status"])
    assert rel_err(s.primal_obj, cold["pobj"]).max() <= 1e-8 and rel_err(s.dual_obj, cold["dobj"]).max() <= 1e-8
    tkv.assert_matches(s, r, lp)
