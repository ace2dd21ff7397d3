"""Upper bounds on per-problem DENSE matrices: the lane-group kernel ipm_bounded_pa_kernel (csrc/ipm_group_slot.inc, BD && PA),
its entry pycllp_hip_dense_solve_batch_bounded and the plugin hip_general_batch_primal_normal.  The reference of every numerical
comparison is tests/bounded_twin.solve run LP by LP with that LP's own matrix; bounds are the project's: status equal and 0,
iterations within 1, objectives 1e-9 relative, x at rtol 1e-5 / atol 1e-7; HiGHS at 1e-8 on a sample.

test_trajectory appends its measured deviations to the file PYCLLP_TRAJECTORY_REPORT names (profiles/bounded_perA/trajectory.txt)."""
import ctypes
import os
import re

import numpy as np
import pytest

import general_batch_cases as gbc
from conftest import ROOT
from pycllp_amd import _native
from pycllp_amd.lp import GeneralLP
from pycllp_amd.solvers import solver_registry
from pycllp_amd.solvers.general import subset
from test_general_solver import check_kkt, highs_general, make_general

NAME = "hip_general_batch_primal_normal"
ENTRY = "pycllp_hip_dense_solve_batch_bounded"
KEYS = gbc.OUTPUTS
REJECTED_FLAGS = (_native.FLAG_HSD, _native.FLAG_PREDCORR, _native.FLAG_WARM_START, _native.FLAG_WAVE_KERNEL,
                  _native.FLAG_NO_SLACK_PATH)


# ---- CPU ------------------------------------------------------------------------------------------------------------------
def test_symbol_is_declared_and_exported():
    header = open(os.path.join(ROOT, "include", "pycllp_hip.h")).read()
    assert re.search(r"\bint\s+%s\s*\(" % ENTRY, header)
    assert ENTRY in _native.EXPORTS
    sig = dict((n, (a, r)) for n, a, r in _native.SIGNATURES)[ENTRY]
    assert len(sig[0]) == 17                                  # handle, B, A, a_cols, b, c, u, eight outputs, opts, stream
    assert hasattr(_native.lib(), ENTRY)


def test_plugin_is_registered():
    from pycllp_amd.solvers import HipGeneralBatchPrimalNormalSolver
    assert solver_registry[NAME] is HipGeneralBatchPrimalNormalSolver


@pytest.mark.parametrize("kw", [dict(hsd=True), dict(predcorr=True), dict(warm_start=True)]
                         + [dict(flags=f) for f in REJECTED_FLAGS], ids=str)
def test_constructor_rejects(kw):
    with pytest.raises(ValueError):
        solver_registry[NAME](**kw)


def test_constructor_accepts_the_options_that_apply():
    s = solver_registry[NAME](hsd=False, autoscale=True, flags=_native.FLAG_FORCE_GUARD_PATH, max_iter=50)
    assert s.options["flags"] & _native.FLAG_AUTOSCALE and s.options["flags"] & _native.FLAG_FORCE_GUARD_PATH and s.hsd is False
    assert solver_registry[NAME]().hsd == "auto"


def _entry_args(h, B, u, flags):
    o = _native.default_opts(flags=flags)
    return (h, B, 8, 5, 8, 8, u, 8, 8, 8, 8, 8, 8, 8, 8, ctypes.byref(o), None)


def test_entry_checks_its_arguments_before_any_device_call():
    f = getattr(_native.lib(), ENTRY)
    buf = np.zeros(64)
    fake = buf.ctypes.data                  # never dereferenced: every argument check comes before the handle is read
    assert f(*_entry_args(None, 1, 8, 0)) == -1
    assert f(*_entry_args(fake, -1, 8, 0)) == -1
    assert f(*_entry_args(fake, 1, None, 0)) == -1
    for flag in REJECTED_FLAGS:
        assert f(*_entry_args(fake, 1, 8, flag)) == -1
        assert b"not available" in _native.lib().pycllp_hip_last_error()


def test_kernel_shape_list_matches_the_dense_kernels():
    csrc = os.path.join(ROOT, "pycllp_amd", "csrc")
    src = {f: open(os.path.join(csrc, f)).read() for f in sorted(os.listdir(csrc)) if f.endswith((".hip", ".h", ".inc"))}
    a = re.search(r"#else\s*\n#define GROUP_SHAPES\(X\)(.*)", src["group_pa.h"]).group(1)
    shapes = lambda t: [tuple(map(int, s)) for s in re.findall(r"X\((\d+),\s*(\d+)\)", t)]
    assert shapes(a) == gbc.GROUP_SHAPES
    for dev, only in (("PYCLLP_DEV_ONLY_3296", (32, 96)), ("PYCLLP_DEV_ONLY_1648", (16, 48))):     # the development subsets too
        pick = re.search(r"defined\(%s\).*\n#define GROUP_SHAPES\(X\)(.*)" % dev, src["group_pa.h"]).group(1)
        assert shapes(pick) == [only] and only in gbc.GROUP_SHAPES
    # the one list: it is defined in group_pa.h alone (three times: the default and the two subsets), so no unit has a copy
    defines = {f: re.findall(r"#define\s+(GROUP_\w*SHAPES)\b", t) for f, t in src.items()}
    assert {f: d for f, d in defines.items() if d} == {"group_pa.h": ["GROUP_SHAPES"] * 3}
    assert "GROUP_SHAPES(" in src["ipm_group_pabd.hip"] and '#include "group_pa.h"' in src["ipm_group_pabd.hip"]


def test_densification_keeps_signs_and_drops_rows():
    """'ge' rows enter with sign -1, a 'free' row is dropped, the slack columns are left out."""
    kinds = ["le", "free", "ge", "eq", "rng", "ge", "free", "le"]
    glp = make_general(8, 7, 5, seed=41, per_problem_A=True, fixed=1, mixed_u=True, kinds=kinds)
    blp, bmap = glp.to_bounded_equality_form()
    assert blp.nrows == 6 and list(bmap.sign) == [1.0, -1.0, 1.0, 1.0, -1.0, 1.0]
    A = solver_registry[NAME].bounded_matrices(blp)
    assert A.shape == (5, 6, 7) and A.flags["C_CONTIGUOUS"] and A.dtype == np.float64
    for k in range(5):
        assert np.array_equal(A[k], blp.A.todense(k)[:, :7])
        assert np.array_equal(blp.A.todense(k)[:, 7:], np.eye(6))
        assert np.array_equal(A[k], bmap.sign[:, None] * glp.A.todense(k)[bmap.rows])


def test_twin_lp_by_lp_matches_highs():
    glp = gbc.make(12, 20, 6, 11)
    blp, bmap = glp.to_bounded_equality_form()
    r = gbc.general_results(bmap, blp, gbc.twin_each(blp))
    assert (r["status"] == 0).all(), r["status"]
    for k in range(glp.nproblems):
        ref, _ = highs_general(glp, k)
        assert gbc.rel(r["pobj"][k], ref) <= 1e-8 and gbc.rel(r["dobj"][k], ref) <= 1e-8


def test_init_needs_a_gpu(monkeypatch):
    import torch
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)
    with pytest.raises(RuntimeError, match="no ROCm device"):
        gbc.make(12, 20, 6, 11).init(solver_registry[NAME]())


# ---- GPU ------------------------------------------------------------------------------------------------------------------
def solve(glp, **kw):
    s = solver_registry[NAME](device="cuda:0", **dict(dict(hsd=False, autoscale=False), **kw))
    glp.init(s)
    glp.solve(s)
    return s, gbc.plugin_results(s)


def twin(glp, idx=None, **opts):
    blp, bmap = glp.to_bounded_equality_form()
    return gbc.general_results(bmap, blp, gbc.twin_each(blp, idx, **opts), idx)


EVERY = [(shape, which) for shape in gbc.GROUP_SHAPES for which in ("smallest", "full")]


@pytest.mark.gpu
@pytest.mark.parametrize("shape,which", EVERY, ids=["%dx%d-%s" % (s + (w,)) for s, w in EVERY])
def test_every_instantiation(shape, which):
    mk, n = (gbc.SMALLEST if which == "smallest" else gbc.FULL)[shape]
    assert gbc.first_covering(mk, n) == shape
    glp = gbc.make(mk, n)
    s, got = solve(glp)
    info = s.launch_info()
    assert s.kernel == "bounded group per-problem"
    assert info.get("group_shape") == shape and info.get("slack") == 1, info
    gbc.assert_parity(got, twin(glp))
    for k in range(0, glp.nproblems, 6):
        ref, _ = highs_general(glp, k)
        assert gbc.rel(got["pobj"][k], ref) <= 1e-8 and gbc.rel(got["dobj"][k], ref) <= 1e-8, k
    check_kkt(glp, s)


@pytest.mark.gpu
def test_slot_refill():
    """Every slot takes several LPs in turn: a stale image, stale column sums, pad entries written by a previous LP or bounds
    of the previous LP would show in the LPs that entered refilled slots (the highest indices among them)."""
    import torch
    ncu = torch.cuda.get_device_properties(0).multi_processor_count
    B = 160
    base = gbc.make(20, 40, B, 99)                             # (32, 96): 12 pad rows, 24 pad columns
    glp = gbc.scaled_rows(base, 0.5 + 1.5 * np.random.RandomState(98).rand(B))
    s, got = solve(glp, reserve_cus=ncu - 4)
    info = s.launch_info()
    assert s.kernel == "bounded group per-problem" and info["group_shape"] == (32, 96) and info["slack"] == 1
    slots = info["grid"] * (info["block"] // 64) * (64 // info["group_shape"][0])
    assert B >= 3 * slots, (B, slots, info)
    assert (got["status"] == 0).all(), np.unique(got["status"], return_counts=True)
    for name, res in zip(("primal", "dual", "bound", "gap"), gbc.residuals(glp, got)):
        assert res.max() < 1e-8, (name, res.max(), int(res.argmax()))
    sample = np.unique(np.r_[np.random.RandomState(5).choice(B - 64, 64, replace=False), np.arange(B - 64, B)])
    assert sample.size == 128
    gbc.assert_parity(got, twin(glp, sample), sample)


@pytest.mark.gpu
def test_values_matter_and_order_does_not():
    import torch
    import bounded_twin
    from pycllp_amd.solvers.hip import Handle, solve_opts
    glp = gbc.make(24, 40, 96, 11)
    s, got = solve(glp)
    assert (got["status"] == 0).all()
    blp, _ = glp.to_bounded_equality_form()
    other = bounded_twin.solve(blp.A.todense(1), blp.b[:1], blp.c[:1], blp.u[:1])
    assert abs(got["pobj"][0] - (other["pobj"][0] + blp.f[0])) > 1e-6
    perm = np.random.RandomState(8).permutation(glp.nproblems)
    _, gp = solve(subset(glp, perm))
    for k in KEYS:
        assert np.array_equal(gp[k], got[k][perm]), k
    # every matrix equal (LPs built around one shared matrix): the shared-A bounded kernel on the same handle
    blp, _ = make_general(24, 40, 96, seed=12, fixed=1, mixed_u=True, kinds=gbc.kinds(24)).to_bounded_equality_form()
    dev = torch.device("cuda:0")
    A0 = np.ascontiguousarray(blp.A.todense())
    h = Handle(A0, dev, None)
    B, mk, N = blp.nproblems, blp.nrows, blp.ncols
    t = lambda a: torch.as_tensor(np.ascontiguousarray(a), device=dev)
    b, c, u = t(blp.b), t(blp.c), t(blp.u)
    f64 = lambda *shape: torch.empty(shape, dtype=torch.float64, device=dev)
    i32 = lambda *shape: torch.empty(shape, dtype=torch.int32, device=dev)
    mko = lambda: dict(x=f64(B, N), y=f64(B, mk), z=f64(B, N), s=f64(B, N), pobj=f64(B), dobj=f64(B), status=i32(B), iters=i32(B))
    shared, batch = mko(), mko()
    o = solve_opts({})
    h.solve_bounded(None, b, c, u, shared, o)
    torch.cuda.synchronize()
    assert h.launch_info()["group_shape"] == (32, 96)
    h.solve_batch_bounded(None, t(np.broadcast_to(A0[:, :N - mk], (B, mk, N - mk))), b, c, u, batch, o)
    torch.cuda.synchronize()
    assert h.launch_info()["group_shape"] == gbc.first_covering(mk, N - mk) == (32, 96)
    sh, ba = ({k: v.cpu().numpy() for k, v in r.items()} for r in (shared, batch))
    print("all matrices equal: bit-exact with the shared-A bounded kernel: %s"
          % {k: bool(np.array_equal(sh[k], ba[k])) for k in KEYS})
    assert np.array_equal(sh["status"], ba["status"]) and (ba["status"] == 0).all()
    assert np.abs(sh["iters"].astype(int) - ba["iters"]).max() <= 1
    assert gbc.rel(ba["pobj"], sh["pobj"]).max() < 1e-9 and gbc.rel(ba["dobj"], sh["dobj"]).max() < 1e-9


@pytest.mark.gpu
def test_guard_path_agrees():
    glp = gbc.make(20, 30, 40, 21)
    _, got = solve(glp)
    gbc.assert_parity(got, twin(glp))
    s2, g2 = solve(glp, flags=_native.FLAG_FORCE_GUARD_PATH)
    assert s2.kernel == "bounded group per-problem" and s2.launch_info()["slack"] == 1
    gbc.assert_parity(g2, got)


@pytest.mark.gpu
def test_autoscale():
    glp = gbc.scaled_data(gbc.make(20, 30, 40, 22), 1e-3, 1e2)
    ref = twin(glp, autoscale=True)
    for kw in (dict(autoscale=True), dict(autoscale="auto")):
        s, got = solve(glp, **kw)
        assert s.kernel == "bounded group per-problem"
        gbc.assert_parity(got, ref)


@pytest.mark.gpu
@pytest.mark.parametrize("B", [0, 1, 2, 63])
def test_batch_sizes(B):
    full = gbc.make(10, 12, 63, 23)
    blp, _ = subset(full, np.arange(max(B, 1))).to_bounded_equality_form()
    s = solver_registry[NAME](device="cuda:0", hsd=False, autoscale=False)
    full.init(s)
    A = s.bounded_matrices(blp)[:B]
    out = s.solve_device(A, blp.b[:B], blp.c[:B], blp.u[:B])
    got = {k: out[k].cpu().numpy() for k in KEYS}
    assert got["x"].shape == (B, 22) and got["s"].shape == (B, 22) and got["y"].shape == (B, 10)
    if B:
        assert s.launch_info()["group_shape"] == (16, 32)
        gbc.assert_parity(got, gbc.twin_each(blp))


@pytest.mark.gpu
@pytest.mark.parametrize("point", sorted(gbc.TRAJECTORY_POINTS))
def test_trajectory(point):
    """x, y, z, s and the objectives of every LP (bounded form's variables) after k = 1, 2, 4, 8 iterations against the twin at
    the same k, LP by LP with that LP's matrix (deviation and tolerance of tests/trajectory.py)."""
    import trajectory as tj
    glp = gbc.trajectory_lp(point)
    blp, _ = glp.to_bounded_equality_form()
    s = solver_registry[NAME](device="cuda:0", hsd=False, autoscale=False)
    glp.init(s)
    A = s.bounded_matrices(blp)
    lines = []
    for k in tj.K:
        out = s.solve_device(A, blp.b, blp.c, blp.u, max_iter=k)
        got = {q: out[q].cpu().numpy() for q in KEYS}
        ref, tol = gbc.trajectory_reference(point, k), gbc.trajectory_tolerance(point, k)
        dev = {q: tj.deviation(got[q], ref[q]) for q in gbc.TRAJ_QUANTITIES}
        lines.append("%s k=%d %s" % (point, k, "  ".join("%s %.1e (tol %.1e)" % (q, dev[q].max(), tol[q]) for q in gbc.TRAJ_QUANTITIES)))
        print(lines[-1])
        for side in (got, ref):
            assert (side["status"] == 5).all() and (side["iters"] == k).all(), (k, side["status"], side["iters"])
        for q in gbc.TRAJ_QUANTITIES:
            assert dev[q].shape == (glp.nproblems,)
            assert dev[q].max() <= tol[q], "%s after %d iterations: %s off by %.2e on LP %d (bound %.2e)" % (
                point, k, q, dev[q].max(), int(dev[q].argmax()), tol[q])
    report = os.environ.get("PYCLLP_TRAJECTORY_REPORT")
    if report:
        with open(report, "a") as f:
            f.write("\n".join(lines) + "\n")


@pytest.mark.gpu
def test_plugin_resolves_an_infeasible_lp():
    B, bad = 30, 17
    base = gbc.make(12, 20, B, 31)
    b = base.b.copy()
    b[bad, 0] = base.A.todense(bad)[0] @ base.l[bad] - 1.0      # row 0 (positive coefficients) below what x >= l allows
    glp = GeneralLP(base.A, b, base.c, a=base.a, l=base.l, u=base.u, f=base.f)
    _, raw = solve(glp)                                        # hsd=False: the kernel's verdict
    assert raw["status"][bad] != 0 and (np.delete(raw["status"], bad) == 0).all(), raw["status"]
    s, got = solve(glp, hsd="auto")
    assert s.kernel == "bounded group per-problem" and got["status"][bad] == 2
    rest = np.delete(np.arange(B), bad)
    for k in KEYS:
        assert np.array_equal(got[k][rest], raw[k][rest]), k


@pytest.mark.gpu
def test_plugin_delegates_outside_the_native_range():
    glp = make_general(20, 30, 64, seed=12)                    # shared A: the shared-A bounded kernel
    s, got = solve(glp, hsd="auto", autoscale="auto")
    r = solver_registry["hip_general_primal_normal"](device="cuda:0")
    glp.init(r)
    glp.solve(r)
    assert s.kernel == r.kernel == "bounded group"
    for k, v in gbc.plugin_results(r).items():
        assert np.array_equal(got[k], v), k
    glp = make_general(40, 30, 24, seed=9, per_problem_A=True)  # 40 kept rows: beyond the kernel
    s, got = solve(glp, hsd="auto", autoscale="auto")
    assert s.kernel == "expanded" and (got["status"] == 0).all()
    refs = np.array([highs_general(glp, k)[0] for k in range(glp.nproblems)])
    assert gbc.rel(got["pobj"], refs).max() <= 1e-8
    with pytest.raises(RuntimeError, match="solve_device"):
        s.solve_device(np.zeros((1, 40, 30)), np.zeros((1, 40)), np.zeros((1, 70)), np.zeros((1, 70)))


@pytest.mark.gpu
def test_entry_declines_what_it_cannot_serve():
    import torch
    L = _native.lib()
    f = getattr(L, ENTRY)
    rs = np.random.default_rng(0)
    o = _native.default_opts()
    for tail, a_cols, rc, text in ((False, 8, -2, b"[A_dense | I]"), (True, 8, -1, b"expected 4"), (True, 3, -1, b"expected 4")):
        A = rs.uniform(-1, 1, (4, 8))
        if tail:
            A[:, 4:] = np.eye(4)
        Ad = torch.tensor(A, dtype=torch.float64, device="cuda:0")
        h = ctypes.c_void_p()
        _native.check(L.pycllp_hip_dense_init(4, 8, ctypes.c_void_p(Ad.data_ptr()), None, ctypes.byref(h)), "init")
        try:
            p = ctypes.c_void_p(Ad.data_ptr())
            assert f(h, 1, p, a_cols, p, p, p, p, p, p, p, p, p, p, p, ctypes.byref(o), None) == rc
            assert text in L.pycllp_hip_last_error(), L.pycllp_hip_last_error()
        finally:
            L.pycllp_hip_dense_free(h)
