"""Option parity (helpers, no tests): every numerical field of ``pycllp_hip_opts`` at a non-default value, per arithmetic path,
against the CPU references at the same value.

A PATH is one (family, kind) of ``trajectory.CASES`` in mode 'cold' at its smallest point (smallest m^2 N; the block kernel keeps
its two LDS plans, the large-LP kernel its four (Gram path, factor storage) points), plus the per-problem dense-A lane-group
kernel on both its tables.  A ROW is (case, options, base options): the kernel is compared with the reference at ``options``;
``base`` is the reference the option must move (the CPU 'must bite' check).  Tolerances are those of trajectory.py, recomputed
under the row's options: max(FACTOR x spread of the reference under NPERM permutations, FLOOR), never above CEILING.

  iterate rows   k = 1, 2, 4: delta = 0.1 and r = 0.5 on every path; max_refine = 1, refine_tol = 1e-6, pivot_floor = 1e-3 on the
                 degenerate cases (where refinement and the pivot floor act); the HSD kernels on the degenerate inputs at
                 pivot_floor = 1e-3 (the base row: refinement at the AUTO cap of 20) and one more option each from there
  stopping rows  eps = 1e-4 at convergence on every path: status, iteration count and the optimum
  Newton rows    the stand-alone Newton entries on the degenerate matrices: A'dy and the refinement pass count"""
import collections
import functools
import os

import numpy as np

import dense_batch_cases as dbc
import test_workgroup_kernel_plans as twp
import trajectory as tj

KS = (1, 2, 4)
KEY = tj.option_key
Row = collections.namedtuple("Row", "id case opts base")

# ---- inputs that trajectory.py does not have -------------------------------------------------------------------------------
def redrawn(key):
    """('redrawn', key, seed): the LPs of ``key`` (one shared matrix) with b and c drawn again, by the recipe of
    test_workgroup_kernel_plans.py: b, c ~ U[0.5, 1.5) on an identity tail (A >= 0), else around a strictly feasible
    primal-dual pair with max-norm 1.  The matrix, and with it the kernel and plan that serve the LPs, stays."""
    from pycllp_amd.lp import EqualityLP
    lp, P = tj.inputs(key[1]), tj.problem(key[1], False)
    A, nb = P.A[0], lp.nproblems
    m, N = A.shape
    assert P.shared and (not P.tail or A.min() >= 0)
    rs = np.random.RandomState(key[2])
    if P.tail:
        b, c = 0.5 + rs.rand(nb, m), np.hstack([0.5 + rs.rand(nb, N - m), np.zeros((nb, m))])
    else:
        x0, y0 = rs.rand(nb, N) + 0.1, rs.randn(nb, m)
        b, c = x0 @ A.T, y0 @ A - (rs.rand(nb, N) + 0.1)
        b /= np.abs(b).max(axis=1, keepdims=True)
        c /= np.abs(c).max(axis=1, keepdims=True)
    return tj._frozen(EqualityLP(lp.A, b, c, 0.0))


def _dense_batch_seeded(key):
    m, n, slack = dbc.TRAJECTORY_POINTS[key[1]]
    return dbc.make(m, n, slack, B=dbc.B_TRAJ, seed=key[2])


tj.MORE_INPUTS.update({
    "dense-batch": lambda key: dbc.trajectory_lp(key[1]),             # a trajectory point of dense_batch_cases.py: a matrix per LP
    "dense-batch-seed": _dense_batch_seeded,                          # the same point from another seed
    "degenerate-each": lambda key: dbc.degenerate_batch(*key[1:]),    # trajectory.degenerate LP by LP, without a tail
    "redrawn": redrawn,
})


# ---- paths ------------------------------------------------------------------------------------------------------------------
def _size(case):
    m, N = tj.problem(case.key, case.kind == "bounded").A[0].shape
    return m * m * N


def _cell(case):
    """What distinguishes the points of one (family, kind) that are paths of their own."""
    if case.family == "block":
        return case.where[1]                                  # the LDS plan
    if case.family == "big":
        return (case.where[2], case.where[1][0])              # Gram path, factor storage
    return None


def per_problem_cases():
    """The per-problem dense-A lane-group kernel at the smallest trajectory point of dense_batch_cases.py, on the slack-aware
    table and (PYCLLP_FLAG_NO_SLACK_PATH) on the general one; and a degenerate batch of its own on the general table."""
    point = min(dbc.TRAJECTORY_POINTS, key=lambda p: dbc.TRAJECTORY_POINTS[p][0] ** 2 * dbc.TRAJECTORY_POINTS[p][1])
    m, n, slack = dbc.TRAJECTORY_POINTS[point]
    assert slack
    out = []
    for table, flags in (("slack", 0), ("general", tj.NO_SLACK)):
        where = (dbc.first_covering(m, n, table == "slack"), 1 if table == "slack" else 0)
        out.append(tj.Case("perA-%dx%d-plain-%s" % (m, n, table), "perA", "plain", "%dx%d-%s" % (m, n, table), "cold", KS,
                           ("dense-batch", point), where, flags, None, ""))
    where = (dbc.first_covering(m, n, False), 0)
    out.append(tj.Case("perA-%dx%d-plain-degenerate" % (m, n), "perA", "plain", "%dx%d" % (m, n), "degenerate", KS,
                       ("degenerate-each", m, n, dbc.B_TRAJ, 7100 + m), where, 0, None, ""))
    return out


@functools.lru_cache(maxsize=None)
def paths():
    groups = collections.OrderedDict()
    for c in tj.CASES:
        if c.mode == "cold":
            groups.setdefault((c.family, c.kind, _cell(c)), []).append(c)
    out = [min(g, key=_size) for g in groups.values()]
    out += [tj.register(c) for c in per_problem_cases() if c.mode == "cold"]
    return tuple(out)


def hsd_degenerate_cases():
    """The HSD kernel of the group, tables, image, block and large-LP (MFMA Gram, factor in LDS) families on the degenerate
    inputs of ``trajectory.CASES`` (the smallest of each family)."""
    out = []
    for family in ("group", "tables", "image", "block", "big"):
        pts = [c for c in tj.CASES if c.mode == "degenerate" and c.family == family and c.kind == "plain"]
        c = min(pts, key=_size)
        if family == "big":
            assert c.where[2] == "mfma" and c.where[1][0] == "L", c.id
            where = tj._plans_case("big", c.where[1], "mfma", "hsd", c.where[4])
        else:
            where = c.where
        out.append(tj.register(c._replace(id="-".join([family, c.point, "hsd", "degenerate"]), kind="hsd", ks=KS, where=where)))
    return out


# ---- iterate rows -----------------------------------------------------------------------------------------------------------
ON_EVERY_PATH = (("delta", dict(delta=0.1)), ("r", dict(r=0.5)))
ON_DEGENERATE = (("max_refine", dict(max_refine=1)), ("refine_tol", dict(refine_tol=1e-6)), ("pivot_floor", dict(pivot_floor=1e-3)))
HSD_BASE = dict(pivot_floor=1e-3)
ON_HSD_DEGENERATE = (("max_refine0", dict(max_refine=0)), ("max_refine2", dict(max_refine=2)), ("refine_tol", dict(refine_tol=1e-6)))
HSD_BASE_AGAINST = dict(pivot_floor=1e-6)      # what the base row itself must differ from (the default floor is not reproducible)


@functools.lru_cache(maxsize=None)
def iterate_rows():
    rows = []
    for c in paths():
        for name, opts in ON_EVERY_PATH:
            if name == "delta" and c.kind.endswith("pc"):
                continue                                     # predictor-corrector does not read delta (test_pc_does_not_read_delta)
            rows.append(Row("%s:%s" % (c.id, name), c, KEY(opts), KEY({})))
    degenerate = [c for c in tj.CASES if c.mode == "degenerate"] + [tj.register(c) for c in per_problem_cases()
                                                                     if c.mode == "degenerate"]
    for c in degenerate:
        for name, opts in ON_DEGENERATE:
            rows.append(Row("%s:%s" % (c.id, name), c, KEY(opts), KEY({})))
    for c in hsd_degenerate_cases():
        rows.append(Row("%s:base" % c.id, c, KEY(HSD_BASE), KEY(HSD_BASE_AGAINST)))
        for name, opts in ON_HSD_DEGENERATE:
            rows.append(Row("%s:%s" % (c.id, name), c, KEY(dict(HSD_BASE, **opts)), KEY(HSD_BASE)))
    assert len({r.id for r in rows}) == len(rows) and {rid for rid, _ in dropped()} <= {r.id for r in rows}
    return tuple(rows)


def pc_delta_rows():
    """The rows that are not there: delta on the predictor-corrector paths (CPU only: the reference moves by exactly 0)."""
    return [Row("%s:delta" % c.id, c, KEY(dict(delta=0.1)), KEY({})) for c in paths() if c.kind.endswith("pc")]


# A (row, k) at which the option does not move the reference's x by twice the tolerance is no test of the option and is left out
# of the row's ladder, with its reason (test_dropped_points_do_not_bite asserts that each is still true).
FIRST_HSD_STEP = ("the first HSD step does not feel delta: at x = z = tau = kappa = 1 every complementarity product equals mu, so "
                  "delta mu / x - z = -(1 - delta) and the whole right-hand side is eta = 1 - delta times a vector without delta; "
                  "the direction scales by eta and the step length r / max ratio takes the factor back")
RESIDUAL_ABOVE_BOTH = ("at k = 1 the refinement residual of the large-LP input stays above 1e-6 (1 + |b|) through all 20 passes, so "
                       "refine_tol = 1e-6 ends refinement where 1e-11 does (nrefs = 20 either way) and x moves by exactly 0")


@functools.lru_cache(maxsize=None)
def dropped():
    """{(row id, k): reason}"""
    out = {("%s:delta" % c.id, 1): FIRST_HSD_STEP for c in paths() if c.kind.endswith("hsd")}
    out.update({("%s:refine_tol" % c.id, 1): RESIDUAL_ABOVE_BOTH for c in hsd_degenerate_cases() if c.family == "big"})
    return out


def row_ks(row):
    ks = tuple(k for k in KS if k in row.case.ks and (row.id, k) not in dropped())
    if not ks:
        raise ValueError("row %s is left with no k" % row.id)
    return ks


def bite(row, k):
    """(largest deviation in x of the reference at the row's options from the reference at its base, the tolerance in x)."""
    ref = tj.reference(row.case.id, row.opts, (k,))[k]
    base = tj.reference(row.case.id, row.base, (k,))[k]
    return float(tj.deviation(ref["x"], base["x"]).max()), tj.tolerance(row.case.id, row.opts, (k,))[k]["x"]


# ---- the GPU side -----------------------------------------------------------------------------------------------------------
def assert_served(case, info, lp, solver):
    if case.family == "perA":
        assert solver.kernel == "group per-problem", solver.kernel
        assert info.get("group_shape") == case.where[0] and info.get("slack") == case.where[1], info
    else:
        tj.assert_served(case, info, lp, solver)


def kernel_results(case, ks, **opts):
    """``trajectory.kernel_results`` under the options ``opts``; the per-problem dense-A kernel through its own plugin."""
    if case.family != "perA":
        return tj.kernel_results(case, ks, **opts)
    import torch
    from pycllp_amd.solvers import solver_registry
    from pycllp_amd.solvers.dense_batch import densify_batch
    lp = tj.inputs(case.key)
    P = tj.problem(case.key, False)
    s = solver_registry["hip_dense_batch_primal_normal"](device="cuda:0", hsd=False, autoscale=False,
                                                         **({"flags": case.flags} if case.flags else {}))
    lp.init(s)
    A = densify_batch(lp.A._rows, lp.A._cols, lp.A.data, lp.nrows, s.a_cols)
    out = {}
    for k in ks:
        g = s.solve_device(A, lp.b, lp.c, max_iter=k, **opts)
        torch.cuda.synchronize()
        assert_served(case, s.launch_info(), lp, s)
        out[k] = {q: g[q].cpu().numpy() for q in ("x", "y", "z", "pobj", "dobj", "status", "iters")}
        out[k]["aty"] = tj.a_transpose_y(P, out[k]["y"])
    return out


def report(lines):
    """Print the measured deviations and append them to the file PYCLLP_TRAJECTORY_REPORT names
    (profiles/option_parity/deviations.txt)."""
    for line in lines:
        print(line)
    path = os.environ.get("PYCLLP_TRAJECTORY_REPORT")
    if path:
        with open(path, "a") as f:
            f.write("\n".join(lines) + "\n")


def assert_on_row(row, got, ks=None):
    """Every LP of the batch, every quantity of the case and every k of the row (``ks``: default ``row_ks``) against the
    reference at the row's options."""
    case, ks = row.case, row_ks(row) if ks is None else ks
    ref, tol = tj.reference(case.id, row.opts, ks), tj.tolerance(case.id, row.opts, ks)
    n = ref[ks[0]]["status"].size
    dev = {k: {q: tj.deviation(got[k][q], ref[k][q]) for q in tj.quantities(case)} for k in ks}
    report(["%s k=%d %s" % (row.id, k, "  ".join("%s %.1e (tol %.1e)" % (q, dev[k][q].max(), tol[k][q]) for q in tj.quantities(case)))
            for k in ks])
    for k in ks:
        for side in (got[k], ref[k]):
            assert (side["status"] == 5).all() and (side["iters"] == k).all(), (k, side["status"], side["iters"])
        for q in tj.quantities(case):
            d = dev[k][q]
            assert d.shape == (n,) and tol[k][q] <= tj.CEILING
            assert d.max() <= tol[k][q], "%s after %d iterations: %s off by %.2e on LP %d (bound %.2e)" % (
                row.id, k, q, d.max(), int(d.argmax()), tol[k][q])


# ---- stopping rows ----------------------------------------------------------------------------------------------------------
EPS, CAP = 1e-4, 200
STOP_QUANTITIES = ("x", "pobj", "dobj")
Stopping = collections.namedtuple("Stopping", "ref default decisive tol")


# Paths whose own LPs are decisive (see ``stopping``) on fewer than 3/4 of the batch: the stopping row solves LPs from another
# seed on the same matrix (``redrawn``), the per-problem kernel a batch from another seed.
STOP_SEEDS = {"big-terms-W3x3-97x513-plain": 1, "big-terms-L3x3-1x513-plain": 1, "perA-12x32-plain-slack": 7412,
              "perA-12x32-plain-general": 7412}


def stop_case(path):
    """The case a path's stopping row solves: the path itself, or the same path on the LPs of ``STOP_SEEDS``."""
    seed = STOP_SEEDS.get(path.id)
    if seed is None:
        return path
    key = ("dense-batch-seed", path.key[1], seed) if path.family == "perA" else ("redrawn", path.key, seed)
    return tj.register(path._replace(id="%s-seed%d" % (path.id, seed), key=key))


@functools.lru_cache(maxsize=None)
def stopping(cid):
    """The reference of a path at eps = 1e-4 under the cap of 200 iterations, at the default eps, the LPs that are DECISIVE
    (the same iteration count at eps / 1.1, eps and 1.1 eps) and the tolerance of x and the objectives on those: the rule of
    trajectory.py on the reference's spread at that eps, at convergence."""
    case = tj.BY_ID[cid]
    ref = tj.reference(cid, KEY(dict(eps=EPS)), (CAP,))[CAP]
    default = tj.reference(cid, KEY({}), (CAP,))[CAP]
    decisive = np.ones(ref["iters"].size, dtype=bool)
    for e in (EPS / 1.1, EPS * 1.1):
        decisive &= tj.run_reference(case, CAP, eps=e)["iters"] == ref["iters"]
    runs = [tj.run_reference(case, CAP, perm=p, eps=EPS) for p in range(tj.NPERM)]
    tol = {}
    for q in STOP_QUANTITIES:
        spread = max(float(tj.deviation(r[q], ref[q])[decisive].max()) for r in runs)
        tol[q] = min(max(tj.FACTOR * spread, tj.FLOOR), tj.CEILING)
    return Stopping(ref, default, decisive, tol)


def assert_stops_with_the_reference(case, got):
    st = stopping(case.id)
    ref, dec = st.ref, st.decisive
    off = np.abs(got["iters"].astype(int) - ref["iters"])
    dev = {q: tj.deviation(got[q], ref[q]) for q in STOP_QUANTITIES}
    report(["%s:eps iters off by <= %d (decisive: %d of %d LPs, off by %d) %s" % (
        case.id, off.max(), dec.sum(), dec.size, off[dec].max(),
        "  ".join("%s %.1e (tol %.1e)" % (q, dev[q][dec].max(), st.tol[q]) for q in STOP_QUANTITIES))])
    assert (got["status"] == 0).all(), got["status"]
    assert (off[dec] == 0).all() and off.max() <= 1, (got["iters"], ref["iters"], dec)
    for q in STOP_QUANTITIES:
        assert dev[q][dec].max() <= st.tol[q], "%s at eps = %g: %s off by %.2e (bound %.2e)" % (
            case.id, EPS, q, dev[q][dec].max(), st.tol[q])


# ---- Newton rows ------------------------------------------------------------------------------------------------------------
NEWTON_SYSTEMS = 8
NEWTON_ROWS = (("default", {}), ("max_refine0", dict(max_refine=0)), ("max_refine2", dict(max_refine=2)),
               ("pivot_floor", dict(pivot_floor=1e-3)))
NEWTON_FAMILIES = ("group", "tables", "image", "block", "big")      # pycllp_hip_dense_newton: group and big; sparse: the others


def newton_cases():
    """One degenerate matrix per Newton kernel: the plain degenerate case of each family."""
    return [min((c for c in tj.CASES if c.mode == "degenerate" and c.family == f and c.kind == "plain"), key=_size)
            for f in NEWTON_FAMILIES]


@functools.lru_cache(maxsize=None)
def newton_state(cid):
    """(A, x, z, y, b, c) of the 8 systems: x, z ~ U[0.5, 1.5], y ~ N(0, 1); b, c of the case's LPs (in turn); mu = 1."""
    P = tj.problem(tj.BY_ID[cid].key, False)
    m, N = P.A[0].shape
    rs = np.random.RandomState(4242)
    x, z, y = 0.5 + rs.rand(NEWTON_SYSTEMS, N), 0.5 + rs.rand(NEWTON_SYSTEMS, N), rs.randn(NEWTON_SYSTEMS, m)
    idx = np.arange(NEWTON_SYSTEMS) % P.b.shape[0]
    return P.A[0], x, z, y, np.ascontiguousarray(P.b[idx]), np.ascontiguousarray(P.c[idx])


def _newton_run(cid, opts, perm=None):
    from oracle import port
    A, x, z, y, b, c = newton_state(cid)
    cols = np.arange(A.shape[1]) if perm is None else np.random.RandomState(1000 + perm).permutation(A.shape[1])
    Ap = np.ascontiguousarray(A[:, cols])                     # columns only: see trajectory.run_reference on degenerate cases
    each = [port.solve_primal_normal(Ap, x[i, cols], z[i, cols], y[i], b[i], c[i, cols], 1.0, passes=True, **dict(opts))
            for i in range(NEWTON_SYSTEMS)]
    dy = np.stack([e[0] for e in each])
    return dict(dy=dy, aty=dy @ A, nrefine=np.array([e[1] for e in each], dtype=np.int32))


Newton = collections.namedtuple("Newton", "ref tol stable")


@functools.lru_cache(maxsize=None)
def newton(cid, opts):
    """The oracle's step under ``opts``, the tolerance of A'dy (the rule of trajectory.py on the spread under NPERM column
    permutations) and the systems whose pass count is the same under all of them."""
    ref = _newton_run(cid, opts)
    runs = [_newton_run(cid, opts, perm=p) for p in range(tj.NPERM)]
    spread = max(float(tj.deviation(r["aty"], ref["aty"]).max()) for r in runs)
    stable = np.all([r["nrefine"] == ref["nrefine"] for r in runs], axis=0)
    return Newton(ref, max(tj.FACTOR * spread, tj.FLOOR), stable)


def newton_kernel(case, **opts):
    """(dy, nrefine) of the kernel's stand-alone Newton entry on the states of ``newton_state``; asserts what served it."""
    from pycllp_amd.solvers import solver_registry
    lp = tj.inputs(case.key)
    _, x, z, y, b, c = newton_state(case.id)
    dense = case.family in ("group", "big")
    s = solver_registry["hip_dense_primal_normal" if dense else "hip_sparse_primal_normal"](
        device="cuda:0", hsd=False, autoscale=False, **({"flags": case.flags} if case.flags else {}))
    lp.init(s)
    dy = s.newton_step(x, z, y, b, c, 1.0, **opts)
    info = s.launch_info()
    if case.family == "big":
        twp.assert_served_by(info, case.where, lp, grid=NEWTON_SYSTEMS)
    else:
        tj.assert_served(case, info, lp, s)
    return dy, s.nrefine
