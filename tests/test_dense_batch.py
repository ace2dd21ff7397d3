"""Per-problem DENSE matrices on the lane-group kernel (pycllp_hip_dense_solve_batch, csrc/ipm_group_slot.inc, PA) and its plugin
hip_dense_batch_primal_normal.  The reference of every comparison is oracle.port.dense_solve run LP by LP with that LP's own
matrix; bounds are the project's: status equal and 0, iterations within 1, objectives 1e-9 relative, x at rtol 1e-5 / atol 1e-7.

test_trajectory appends its measured deviations to the file PYCLLP_TRAJECTORY_REPORT names (profiles/perA_group/trajectory.txt)."""
import os
import re

import numpy as np
import pytest

import dense_batch_cases as dbc
from conftest import ROOT, rel_err
from pycllp_amd import _native
from pycllp_amd.lp import SparseMatrix, StandardLP
from pycllp_amd.solvers import solver_registry
from pycllp_amd.solvers.dense_batch import HipDenseBatchPrimalNormalSolver, densify_batch, identity_tail

NAME = "hip_dense_batch_primal_normal"
KEYS = ("x", "y", "z", "pobj", "dobj", "status", "iters")


# ---- CPU ------------------------------------------------------------------------------------------------------------------
def test_symbol_is_declared_and_exported():
    header = open(os.path.join(ROOT, "include", "pycllp_hip.h")).read()
    assert re.search(r"\bint\s+pycllp_hip_dense_solve_batch\s*\(", header)
    assert "pycllp_hip_dense_solve_batch" in _native.EXPORTS
    sig = dict((n, (a, r)) for n, a, r in _native.SIGNATURES)["pycllp_hip_dense_solve_batch"]
    assert len(sig[0]) == 15                                  # handle, B, A, a_cols, nine arrays... opts, stream


def test_plugin_is_registered():
    assert solver_registry[NAME] is HipDenseBatchPrimalNormalSolver


@pytest.mark.parametrize("kw", [dict(hsd=True), dict(predcorr=True), dict(warm_start=True), dict(flags=_native.FLAG_HSD),
                                dict(flags=_native.FLAG_PREDCORR), dict(flags=_native.FLAG_WARM_START),
                                dict(flags=_native.FLAG_WAVE_KERNEL)])
def test_constructor_rejects(kw):
    with pytest.raises(ValueError):
        solver_registry[NAME](**kw)


def test_constructor_accepts_the_options_that_apply():
    s = solver_registry[NAME](hsd=False, autoscale=True, flags=_native.FLAG_FORCE_GUARD_PATH | _native.FLAG_NO_SLACK_PATH,
                              max_iter=50)
    assert s.options["flags"] & _native.FLAG_AUTOSCALE and s.hsd is False
    assert solver_registry[NAME]().hsd == "auto"


def test_entry_checks_its_arguments_before_any_device_call():
    L = _native.lib()
    buf = np.zeros(64)
    fake = buf.ctypes.data                  # never dereferenced: the flag check comes before the handle is read
    o = _native.default_opts()
    args = lambda h, B, flags: (h, B, 8, 5, 8, 8, 8, 8, 8, 8, 8, 8, 8, _opts(o, flags), None)
    assert L.pycllp_hip_dense_solve_batch(*args(None, 1, 0)) == -1
    assert L.pycllp_hip_dense_solve_batch(*args(fake, -1, 0)) == -1
    for flag in (_native.FLAG_HSD, _native.FLAG_PREDCORR, _native.FLAG_WARM_START, _native.FLAG_WAVE_KERNEL):
        assert L.pycllp_hip_dense_solve_batch(*args(fake, 1, flag)) == -1
        assert b"not available" in L.pycllp_hip_last_error()


def _opts(o, flags):
    import ctypes
    o.flags = flags
    return ctypes.byref(o)


def test_densification_reproduces_todense():
    rs = np.random.RandomState(3)
    m, n, B = 7, 11, 5
    keep = rs.rand(m * n) < 0.6                              # a structure with holes, in shuffled coordinate order
    rows, cols = np.divmod(np.flatnonzero(keep), n)
    order = rs.permutation(rows.size)
    rows, cols = rows[order], cols[order]
    A = SparseMatrix(rows, cols, rs.randn(B, rows.size))
    A._shape = (m, n)
    full = densify_batch(A._rows, A._cols, A.data, m, n)
    assert full.shape == (B, m, n) and full.flags["C_CONTIGUOUS"]
    for k in range(B):
        assert np.array_equal(full[k], A.todense(k))
    lp = dbc.make(5, 5 + 9, True, B=4)                       # identity tail: the short form leaves it out
    assert identity_tail(lp.A._rows, lp.A._cols, lp.A.data, 5, 14)
    short = densify_batch(lp.A._rows, lp.A._cols, lp.A.data, 5, 9)
    for k in range(4):
        assert np.array_equal(short[k], lp.A.todense(k)[:, :9]) and np.array_equal(lp.A.todense(k)[:, 9:], np.eye(5))
    dup = densify_batch([0, 0, 1], [1, 1, 0], [[1.0, 2.0, 4.0]], 2, 2)      # shared positions are summed, as todense sums them
    assert np.array_equal(dup[0], [[0.0, 3.0], [4.0, 0.0]])
    assert not identity_tail(*_structure(dbc.make(4, 9, False, B=3)), 4, 9)


def _structure(lp):
    return lp.A._rows, lp.A._cols, lp.A.data


def test_kernel_shape_list_matches_the_dense_kernels():
    csrc = os.path.join(ROOT, "pycllp_amd", "csrc")
    src = {f: open(os.path.join(csrc, f)).read() for f in sorted(os.listdir(csrc)) if f.endswith((".hip", ".h", ".inc"))}
    a = re.search(r"#else\s*\n#define GROUP_SHAPES\(X\)(.*)", src["group_pa.h"]).group(1)
    shapes = lambda t: [tuple(map(int, s)) for s in re.findall(r"X\((\d+),\s*(\d+)\)", t)]
    assert shapes(a) == dbc.GROUP_SHAPES
    # the one list: no translation unit keeps a copy of its own, and all three expand this one
    defined = {f: set(re.findall(r"#define\s+(GROUP_\w*SHAPES)\b", t)) for f, t in src.items()}
    assert {f: d for f, d in defined.items() if d} == {"group_pa.h": {"GROUP_SHAPES"}}
    for f in ("ipm_dense.hip", "ipm_group_pa.hip", "ipm_group_pabd.hip"):
        assert '#include "group_pa.h"' in src[f] and "GROUP_SHAPES(" in src[f], f


def test_init_needs_a_gpu():
    import torch
    if torch.cuda.is_available():
        pytest.skip("a ROCm device is visible")
    with pytest.raises(RuntimeError, match="no ROCm device"):
        dbc.make(3, 8, True, B=2).init(solver_registry[NAME]())


# ---- GPU ------------------------------------------------------------------------------------------------------------------
def solve(lp, **kw):
    s = solver_registry[NAME](device="cuda:0", **dict(dict(hsd=False, autoscale=False), **kw))
    lp.init(s)
    lp.solve(s)
    return s, dict(x=s.x, y=s.y, z=s.z, pobj=s.primal_obj, dobj=s.dual_obj, status=s.status, iters=s.iters)


EVERY = [(shape, slack, which) for shape in dbc.GROUP_SHAPES for slack in (True, False) for which in (0, 1)]


@pytest.mark.gpu
@pytest.mark.parametrize("shape,slack,which", EVERY,
                         ids=["%dx%d-%s-%s" % (s + ("slack" if sl else "general", "full" if w else "smallest")) for s, sl, w in EVERY])
def test_every_instantiation(shape, slack, which):
    m, n = dbc.smallest_and_full(shape, slack)[which]
    assert dbc.first_covering(m, n, slack) == shape
    lp = dbc.make(m, n, slack)
    s, got = solve(lp)
    info = s.launch_info()
    assert s.kernel == "group per-problem" and s.slack == slack
    assert info.get("group_shape") == shape and info.get("slack") == (1 if slack else 0), info
    dbc.assert_matches_oracle(got, dbc.oracle_each(lp))


@pytest.mark.gpu
def test_slot_refill():
    """Every slot takes several LPs in turn: a stale image, stale column sums or pad entries written by a previous LP would
    show in the LPs that entered refilled slots (the highest indices among them)."""
    import torch
    m, nd = 20, 40                                            # (32, 96) slack-aware: 12 pad rows, 24 pad columns
    ncu = torch.cuda.get_device_properties(0).multi_processor_count
    B = 320
    lp = dbc.standard_batch(m, nd, B, seed=99, scale=True)
    s, got = solve(lp, reserve_cus=ncu - 4)
    info = s.launch_info()
    assert info["group_shape"] == (32, 96) and info["slack"] == 1
    slots = info["grid"] * (info["block"] // 64) * (64 // info["group_shape"][0])
    assert B >= 3 * slots, (B, slots, info)
    assert (got["status"] == 0).all()
    A = dbc.matrices(lp)
    nb, nc = 1 + np.linalg.norm(lp.b, axis=1), 1 + np.linalg.norm(lp.c, axis=1)
    assert (np.linalg.norm(lp.b - np.einsum("kij,kj->ki", A, got["x"]), axis=1) / nb).max() < 1e-8
    assert (np.linalg.norm(lp.c - np.einsum("kij,ki->kj", A, got["y"]) + got["z"], axis=1) / nc).max() < 1e-8
    assert (np.abs(got["pobj"] - got["dobj"]) / np.maximum(1.0, np.abs(got["pobj"]))).max() < 1e-8
    sample = np.unique(np.r_[np.random.RandomState(5).choice(B - 64, 192, replace=False), np.arange(B - 64, B)])
    assert sample.size >= 256
    dbc.assert_matches_oracle(got, dbc.oracle_each(lp, sample), sample)


@pytest.mark.gpu
def test_values_matter_and_order_does_not():
    import torch
    from oracle import port
    from pycllp_amd.solvers.hip import Handle, solve_opts
    lp = dbc.make(24, 24 + 40, True, B=96, seed=11)
    s, got = solve(lp)
    assert (got["status"] == 0).all()
    other = port.dense_solve(lp.A.todense(1), lp.b[:1], lp.c[:1])
    assert abs(got["pobj"][0] - other["pobj"][0]) > 1e-6
    perm = np.random.RandomState(8).permutation(lp.nproblems)
    _, gp = solve(dbc.reorder(lp, perm))
    for k in KEYS:
        assert np.array_equal(gp[k], got[k][perm]), k
    # every matrix equal: the shared-A kernel on the same handle
    dev = torch.device("cuda:0")
    A0 = lp.A.todense(0)
    h = Handle(np.ascontiguousarray(A0), dev, None)
    B, m, n = lp.nproblems, lp.nrows, lp.ncols
    t = lambda a: torch.as_tensor(np.ascontiguousarray(a), device=dev)
    b, c = t(lp.b), t(lp.c)
    mk = lambda: dict(x=torch.empty((B, n), dtype=torch.float64, device=dev), y=torch.empty((B, m), dtype=torch.float64, device=dev),
                      z=torch.empty((B, n), dtype=torch.float64, device=dev), pobj=torch.empty(B, dtype=torch.float64, device=dev),
                      dobj=torch.empty(B, dtype=torch.float64, device=dev), status=torch.empty(B, dtype=torch.int32, device=dev),
                      iters=torch.empty(B, dtype=torch.int32, device=dev))
    shared, batch = mk(), mk()
    o = solve_opts({})
    h.solve(None, b, c, shared, o)
    h.solve_batch_dense(None, t(np.broadcast_to(A0[:, :n - m], (B, m, n - m))), b, c, batch, o)
    torch.cuda.synchronize()
    assert h.launch_info()["group_shape"] == dbc.first_covering(m, n, True) == (32, 96)
    sh, ba = ({k: v.cpu().numpy() for k, v in r.items()} for r in (shared, batch))
    assert np.array_equal(sh["status"], ba["status"]) and (ba["status"] == 0).all()
    assert np.abs(sh["iters"].astype(int) - ba["iters"]).max() <= 1
    assert rel_err(ba["pobj"], sh["pobj"]).max() < 1e-9 and rel_err(ba["dobj"], sh["dobj"]).max() < 1e-9


@pytest.mark.gpu
def test_guard_path_and_no_slack_path_agree():
    lp = dbc.make(20, 20 + 30, True, B=40, seed=21)
    _, got = solve(lp)
    dbc.assert_matches_oracle(got, dbc.oracle_each(lp))
    for flag in (_native.FLAG_FORCE_GUARD_PATH, _native.FLAG_NO_SLACK_PATH):
        s2, g2 = solve(lp, flags=flag)
        assert s2.launch_info()["slack"] == (0 if flag == _native.FLAG_NO_SLACK_PATH else 1)
        assert np.array_equal(g2["status"], got["status"]) and np.abs(g2["iters"].astype(int) - got["iters"]).max() <= 1
        assert rel_err(g2["pobj"], got["pobj"]).max() < 1e-9 and rel_err(g2["dobj"], got["dobj"]).max() < 1e-9
        np.testing.assert_allclose(g2["x"], got["x"], rtol=1e-5, atol=1e-7)


@pytest.mark.gpu
def test_autoscale():
    lp = dbc.standard_batch(20, 30, 40, seed=22, b_scale=1e-3, c_scale=1e2)
    for kw in (dict(autoscale=True), dict(autoscale="auto")):
        _, got = solve(lp, **kw)
        dbc.assert_matches_oracle(got, dbc.oracle_each(lp, flags=8))


@pytest.mark.gpu
@pytest.mark.parametrize("B", [0, 1, 2, 63])
def test_batch_sizes(B):
    full = dbc.make(10, 10 + 12, True, B=63, seed=23)
    lp = dbc.reorder(full, np.arange(B))
    s = solver_registry[NAME](device="cuda:0", hsd=False, autoscale=False)
    full.init(s)
    A = densify_batch(lp.A._rows, lp.A._cols, lp.A.data, 10, 12) if B else np.zeros((0, 10, 12))
    out = s.solve_device(A, lp.b.reshape(B, 10), lp.c.reshape(B, 22))
    got = {k: out[k].cpu().numpy() for k in KEYS}
    assert got["x"].shape == (B, 22)
    if B:
        dbc.assert_matches_oracle(got, dbc.oracle_each(lp))


@pytest.mark.gpu
@pytest.mark.parametrize("point", sorted(dbc.TRAJECTORY_POINTS))
def test_trajectory(point):
    """x, y, z and the objectives of every LP after k = 1, 2, 4, 8 iterations against the oracle at the same k (deviation and
    tolerance of tests/trajectory.py).  The kernel stores the objectives of the point it stores: the reference's are c'x, b'y
    of the oracle's x, y."""
    import trajectory as tj
    lp = dbc.trajectory_lp(point)
    s = solver_registry[NAME](device="cuda:0", hsd=False, autoscale=False)
    lp.init(s)
    A = densify_batch(lp.A._rows, lp.A._cols, lp.A.data, lp.nrows, lp.ncols - lp.nrows)
    lines = []
    for k in tj.K:
        out = s.solve_device(A, lp.b, lp.c, max_iter=k)
        got = {q: out[q].cpu().numpy() for q in KEYS}
        ref, tol = dbc.trajectory_reference(point, k), dbc.trajectory_tolerance(point, k)
        dev = {q: tj.deviation(got[q], ref[q]) for q in tj.QUANTITIES}
        lines.append("%s k=%d %s" % (point, k, "  ".join("%s %.1e (tol %.1e)" % (q, dev[q].max(), tol[q]) for q in tj.QUANTITIES)))
        print(lines[-1])
        for side in (got, ref):
            assert (side["status"] == 5).all() and (side["iters"] == k).all(), (k, side["status"], side["iters"])
        for q in tj.QUANTITIES:
            assert dev[q].shape == (lp.nproblems,)
            assert dev[q].max() <= tol[q], "%s after %d iterations: %s off by %.2e on LP %d (bound %.2e)" % (
                point, k, q, dev[q].max(), int(dev[q].argmax()), tol[q])
    report = os.environ.get("PYCLLP_TRAJECTORY_REPORT")
    if report:
        with open(report, "a") as f:
            f.write("\n".join(lines) + "\n")


@pytest.mark.gpu
def test_plugin_on_a_fully_dense_structure():
    m, n, B = 24, 40, 48
    rs = np.random.RandomState(2)
    rows, cols = dbc.dense_structure(m, n)
    lp = StandardLP(SparseMatrix(rows, cols, 0.1 + rs.rand(B, m * n)), 0.5 + rs.rand(B, m), 0.5 + rs.rand(B, n), 0.0).to_equality_form()
    s = solver_registry[NAME](device="cuda:0")
    lp.init(s)
    st = lp.solve(s)
    assert s.kernel == "group per-problem" and (st == 0).all()
    got = dict(x=s.x, y=s.y, z=s.z, pobj=s.primal_obj, dobj=s.dual_obj, status=s.status, iters=s.iters)
    dbc.assert_matches_oracle(got, dbc.oracle_each(lp))
    A = densify_batch(lp.A._rows, lp.A._cols, lp.A.data, m, n)
    out = s.solve_device(A, lp.b, lp.c)
    for k in KEYS:
        assert np.array_equal(out[k].cpu().numpy(), got[k]), k


@pytest.mark.gpu
def test_plugin_delegates_beyond_the_lane_group_kernels():
    from pycllp_amd import problems
    A, b, c = problems.random_sparse_arrays(40, 60, 24, density=0.2, seed=4)
    rows, cols, data = problems.per_problem_values(A, 24, seed=9)
    lp = StandardLP(SparseMatrix(rows, cols, data), b, c, 0.0).to_equality_form()
    s = solver_registry[NAME](device="cuda:0")
    lp.init(s)
    st = lp.solve(s).copy()
    assert s.kernel == "delegated" and (st == 0).all()
    po, x, it = s.primal_obj.copy(), s.x.copy(), s.iters.copy()
    r = solver_registry["hip_sparse_primal_normal"](device="cuda:0")
    lp.init(r)
    lp.solve(r)
    assert np.array_equal(r.status, st) and np.array_equal(r.iters, it)
    assert np.array_equal(r.primal_obj, po) and np.array_equal(r.x, x)


@pytest.mark.gpu
def test_plugin_resolves_an_infeasible_lp():
    m, nd, B, bad = 12, 20, 30, 17
    base = dbc.standard_batch(m, nd, B, seed=31)
    b = base.b.copy()
    b[bad] = -b[bad]                                          # A > 0, x >= 0, A x <= b < 0: infeasible
    lp = dbc.reorder(base, np.arange(B))
    lp.b = b
    _, raw = solve(lp)                                        # hsd=False: the kernel's verdict
    assert raw["status"][bad] != 0 and (np.delete(raw["status"], bad) == 0).all()
    s, got = solve(lp, hsd="auto")
    assert got["status"][bad] == 2
    rest = np.delete(np.arange(B), bad)
    for k in KEYS:
        assert np.array_equal(got[k][rest], raw[k][rest]), k


@pytest.mark.gpu
def test_plugin_resolves_lp_by_lp_where_the_sparse_path_declines_the_subset(monkeypatch):
    """hsd='auto' when the sparse path's per-problem kernels decline the subset of non-optimal LPs: each is solved as a
    shared-A problem of its own on one solver object."""
    from pycllp_amd.solvers import dense_batch
    made = []

    class Declining(dense_batch.HipSparsePrimalNormalSolver):
        name = None

        def __init__(self, *a, **kw):
            super(Declining, self).__init__(*a, **kw)
            made.append(self)

        def init(self, lp, verbose=0):
            if lp.A.nproblems > 1:
                raise NotImplementedError("declined")
            return super(Declining, self).init(lp, verbose=verbose)

    monkeypatch.setattr(dense_batch, "HipSparsePrimalNormalSolver", Declining)
    m, nd, B, bad = 12, 20, 30, (5, 17)
    base = dbc.standard_batch(m, nd, B, seed=31)
    lp = dbc.reorder(base, np.arange(B))
    lp.b[list(bad)] *= -1.0
    _, raw = solve(lp)
    s, got = solve(lp, hsd="auto")
    assert len(made) == 1
    assert (got["status"][list(bad)] == 2).all()
    rest = np.delete(np.arange(B), bad)
    for k in KEYS:
        assert np.array_equal(got[k][rest], raw[k][rest]), k
