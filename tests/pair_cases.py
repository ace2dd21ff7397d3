"""Option pairs (helpers, no tests): warm start, autoscale, HSD, predictor-corrector, per-problem A and the forced guard path two
(or three) at a time, on the trajectory machinery of tests/trajectory.py -- the same references, tolerance rule and 'served by'
assertions as its one-flag rows.

A ROW is a ``trajectory.Case`` (registered, so ``reference``, ``spread`` and ``tolerance`` know it) plus what the row is about:
``pair`` -- the options it combines -- and ``serve``:

  'kernel'       the kernel of the point runs the whole solve
  'guard'        PYCLLP_FLAG_FORCE_GUARD_PATH on a kernel that has the guarded factorisation inside (lane groups, large-LP kernel)
  'deferred'     the flag on the wave kernel: every LP is handed to the block kernel, which restarts it from the caller's arrays
  'pc-deferred'  the same under PYCLLP_FLAG_PREDCORR: the block kernel has no predictor-corrector step and finishes the LPs on
                 the reference's plain rule (include/pycllp_hip.h); the row's reference is the PLAIN one

Every row starts from the cold row of ``trajectory.CASES`` with the same (family, point, kind): its inputs, what serves it and
its flags.  Rows under autoscale solve the ('scaled', key) inputs (b x 1e3, c x 1e-2); rows that are also warm start from
``trajectory.start_point``: ``warm_point`` scaled with the data.  The reference of a guard row is the oracle without the flag (an
inactive guard changes nothing but rounding)."""
import collections
import functools
import types

import numpy as np

import option_cases as oc
import test_kernel_variants as tkv
import trajectory as tj

PREDCORR = 128                                               # PYCLLP_FLAG_PREDCORR
Row = collections.namedtuple("Row", "case pair serve")

POINTS = collections.OrderedDict([                           # the points of trajectory.build_cases' extras()
    ("slack", ("slack", "32x64")), ("group", ("group", "32x96")), ("tables", ("tables", "40x90")), ("image", ("image", "100x80")),
    ("block-lds", ("block", "lds-paired-97x257")), ("block-l2", ("block", "l2-121x257")),
    ("big-mfma", ("big", "mfma-L3x3-8x513")), ("big-terms", ("big", "terms-L3x3-1x513"))])
ALL = tuple(POINTS)
HAVE_PC = ("slack", "group", "tables", "image", "big-mfma", "big-terms")          # (the block kernel refuses PC)
BOTH = ("warm", "autoscale")

# (options of the start and scaling, kind) -> the points; per-problem A on the tables and the block kernel's lds-paired plan
TABLE = [
    (("warm",), "hsd", ALL), (("warm",), "pa-hsd", ("tables", "block-lds")),
    (("warm",), "pc", HAVE_PC), (("warm",), "pa-pc", ("tables",)),
    (("warm",), "pa", ("tables", "block-lds")),
    (("autoscale",), "pc", HAVE_PC),
    (("autoscale",), "pa", ("tables", "block-lds")), (("autoscale",), "pa-hsd", ("tables", "block-lds")),
    (("autoscale",), "pa-pc", ("tables",)),
    (BOTH, "plain", ALL), (BOTH, "hsd", ALL), (BOTH, "pc", HAVE_PC), (BOTH, "pa", ("tables", "block-lds")),
]
# PYCLLP_FLAG_FORCE_GUARD_PATH: (options, kind) on the kernels with the guard inside, and on the wave kernel (every LP deferred)
GUARD_IN_KERNEL = ("slack", "big-mfma")
GUARD_ROWS = [((), "hsd"), ((), "pc"), (("warm",), "plain"), (("autoscale",), "plain"), (BOTH, "plain")]
DEFERRED_ROWS = [((), "plain"), ((), "hsd"), (("warm",), "plain"), (("autoscale",), "plain"), (("warm",), "hsd"), (BOTH, "plain"),
                 ((), "pa"), (("warm",), "pa")]
PC_DEFERRED = ("tables", "image")

# Rows whose ladder stops before k = 8, with the reason (test_option_pairs.py asserts that each is still true): the rule of
# trajectory.STOPS_AT_4 -- where FACTOR x the reference's own spread passes CEILING, or a perturbation of the 'must bite' tests no
# longer moves x by twice the tolerance, the k is dropped rather than the bound widened or the perturbation shrunk.
A_ENTRY = "at k = 8 one entry of A times (1 + 1e-8) no longer moves x by twice the bound"
STOPS = {cid: (4, A_ENTRY) for cid in (
    "tables-40x90-pa-warm", "tables-40x90-pa-autoscale", "tables-40x90-plain-warm+autoscale", "tables-40x90-pa-warm+autoscale",
    "big-mfma-L3x3-8x513-pc-autoscale", "big-mfma-L3x3-8x513-pc-guard", "tables-40x90-plain-deferred",
    "tables-40x90-plain-warm+autoscale-deferred", "tables-40x90-pa-warm-deferred", "tables-40x90-pc-deferred")}


def base_case(point, kind):
    family, label = POINTS[point]
    return tj.BY_ID["%s-%s-%s" % (family, label, kind)]


def _row(point, kind, options, serve="kernel"):
    base = base_case(point, "plain" if serve == "pc-deferred" else kind)
    assert base.mode == "cold" and base.ks in (tj.K, tj.K[:3]), base.id
    mode = "+".join(o for o in BOTH if o in options) or "cold"
    tag = {"kernel": [], "guard": ["guard"], "deferred": ["deferred"], "pc-deferred": ["deferred"]}[serve]
    family, label = POINTS[point]
    cid = "-".join([family, label, kind] + ([mode] if mode != "cold" else []) + tag)
    flags = base.flags | (tj.GUARD if serve != "kernel" else 0) | (PREDCORR if serve == "pc-deferred" else 0)
    ks = tuple(k for k in tj.K if k <= STOPS.get(cid, (tj.K[-1],))[0])
    key = ("scaled", base.key) if "autoscale" in options else base.key
    case = tj.register(tj.Case(cid, family, base.kind, label, mode, ks, key, base.where, flags, None, ""))
    pair = tuple(options) + (tuple(kind.split("-")) if kind != "plain" else ()) + (("guard",) if serve != "kernel" else ())
    return Row(case, pair, serve)


@functools.lru_cache(maxsize=None)
def rows():
    out = [_row(p, kind, options) for options, kind, points in TABLE for p in points]
    out += [_row(p, kind, options, "guard") for p in GUARD_IN_KERNEL for options, kind in GUARD_ROWS]
    out += [_row("tables", kind, options, "deferred") for options, kind in DEFERRED_ROWS]
    out += [_row(p, "pc", (), "pc-deferred") for p in PC_DEFERRED]
    assert len({r.case.id for r in out}) == len(out) and set(STOPS) <= {r.case.id for r in out}
    return tuple(out)


# ---- the fakes: what a kernel that dropped half of the pair would compute -----------------------------------------------------
LESS = {"hsd": "plain", "pc": "plain", "pa-hsd": "pa", "pa-pc": "pa"}


def fakes(row):
    """[(name, case, start, quantity)]: the reference run that emulates a kernel which dropped half of the pair, and the
    quantity in which it must be off by more than twice the bound.  The case with one option taken away ('no warm', 'no
    autoscale', 'no hsd', 'no pc'), from the start ``trajectory.start_point`` gives that case.  For warm + autoscale also the
    starts of a kernel that divided none of x, y, z, or all but y, or all but x: those handed over times their scale once
    more.  'y undivided' shows in y and ONLY there: x and z of these methods do not depend on the y they start from (the normal
    equations give y + dy, dx and dz without it; y enters its own update alone, with weight 1 - theta per iteration) -- asserted
    in test_option_pairs.py.  'pa' and the guard cannot be taken away on the reference's side (the data are per-problem; the
    reference has no guard).  A 'pc-deferred' row: the predictor-corrector reference, which the results must NOT be."""
    case = row.case
    if row.serve == "pc-deferred":
        return [("pc", case._replace(kind="pc"), None, "x")]
    out = []
    for o in BOTH:
        if o in row.pair:
            rest = "+".join(q for q in BOTH if q in row.pair and q != o) or "cold"
            out.append(("no " + o, case._replace(mode=rest), None, "x"))
    if case.kind in LESS and case.kind.split("-")[-1] in row.pair:
        out.append(("no " + case.kind.split("-")[-1], case._replace(kind=LESS[case.kind]), None, "x"))
    if set(BOTH) <= set(row.pair):
        P = tj.problem(case.key, False)
        sb, sc = np.abs(P.b).max(axis=1, keepdims=True), np.abs(P.c).max(axis=1, keepdims=True)
        x0, y0, z0 = tj.start_point(case, P)
        out += [("none divided", case, (x0 * sb, y0 * sc, z0 * sc), "x"), ("y undivided", case, (x0, y0 * sc, z0), "y"),
                ("x undivided", case, (x0 * sb, y0, z0), "x")]
    return out


def moved(case, k, ref, quantity="x", **kw):
    """Largest deviation in ``quantity`` of ``run_reference(case, k, **kw)`` from ``ref`` over the LPs; a non-finite result
    counts as moved."""
    d = tj.deviation(tj.run_reference(case, k, **kw)[quantity], ref[quantity])
    return float(np.where(np.isfinite(d), d, np.inf).max())


def fake_moved(fake, k, ref, quantity=None):
    _, case, start, q = fake
    return moved(case, k, ref, quantity or q, **({} if start is None else dict(start=start)))


# ---- the GPU side -------------------------------------------------------------------------------------------------------------
BITS = ("x", "y", "z", "pobj", "dobj", "status", "iters")


def launch_options(row):
    """Further fields of ``pycllp_hip_opts``: a deferred warm row leaves one compute unit to the solve, so that its batch is at
    least twice as long as the wave kernel's grid has wavefronts and LPs deferred late still find their start untouched."""
    if row.serve == "deferred" and "warm" in row.pair:
        import torch
        return dict(reserve_cus=torch.cuda.get_device_properties(0).multi_processor_count - 1)
    return {}


def kernel_results(row, ks=None):
    """``trajectory.kernel_results`` of the row; every launch asserts what served it.  A deferred row also asserts that the
    block kernel served its LPs: ``launch_info()`` reports the wave kernel's launch (asserted), so the results must carry the
    bits of a PYCLLP_FLAG_BLOCK_KERNEL launch with the same options (a 'pc-deferred' row: without PREDCORR, which that launch
    refuses) and not those of the launch without the guard flag."""
    case, opts = row.case, launch_options(row)
    ks = case.ks if ks is None else ks
    seen = []
    got = tj.kernel_results(case, ks, seen=seen, **opts)
    if row.serve in ("deferred", "pc-deferred"):
        if opts:
            n = tj.inputs(case.key).nproblems
            for info in seen:
                assert 2 * info["grid"] * (info["block"] // 64) <= n, (info, n)
        block = tj.kernel_results(case._replace(flags=(case.flags | tj.BLOCK) & ~PREDCORR, where=None), ks, **opts)
        wave = tj.kernel_results(case._replace(flags=case.flags & ~tj.GUARD), ks, **opts)
        for k in ks:
            for q in BITS:
                assert np.array_equal(got[k][q].view(np.uint8), block[k][q].view(np.uint8)), \
                    "%s k=%d: %s does not carry the block kernel's bits" % (case.id, k, q)
            assert not np.array_equal(got[k]["x"], wave[k]["x"]), "%s k=%d: x carries the wave kernel's bits" % (case.id, k)
    return got


def assert_on_trajectory(row, got):
    """Every LP, quantity and k against the row's reference; the deviations go to the report of ``option_cases.report``."""
    case = row.case
    dev, tol = tj.measured(case, got), tj.tolerance(case.id)
    oc.report(["%s k=%d %s" % (case.id, k, "  ".join("%s %.1e (tol %.1e)" % (q, dev[k][q], tol[k][q]) for q in tj.quantities(case)))
               for k in case.ks])
    tj.assert_on_trajectory(case, got)
    if row.serve == "pc-deferred":
        (_, pc, _, _), = fakes(row)
        for k in case.ks:
            d = tj.deviation(got[k]["x"], tj.run_reference(pc, k)["x"]).max()
            assert d > 2 * tol[k]["x"], "%s k=%d: x is within %.2e of the predictor-corrector reference" % (case.id, k, d)


def default_max_iter():
    from oracle import port
    return port.default_opts().max_iter


def assert_converges_like_the_reference(row):
    """At the default iteration limit: the project's bar at convergence (``test_kernel_variants.assert_matches``) against the
    reference under the same flags and start -- the exit store, with its scale-back, which the status-5 store does not reach."""
    case, limit = row.case, default_max_iter()
    r = tj.run_reference(case, limit)
    g = tj.kernel_results(case, (limit,), **launch_options(row))[limit]
    oc.report(["%s converged: status %s  iters kernel %s reference %s" % (
        case.id, np.unique(g["status"]).tolist(), g["iters"].tolist(), r["iters"].tolist())])
    s = types.SimpleNamespace(primal_obj=g["pobj"], dual_obj=g["dobj"], **g)
    tkv.assert_matches(s, r, tj.inputs(case.key))
