"""Upper bounds on per-problem SPARSE matrices: the wave kernel ipm_wreg_bounded_pa_kernel (csrc/ipm_wreg_bounded.inc compiled by
ipm_wreg_bdpa.hip), its entry pycllp_hip_sparse_solve_batch_bounded and the plugin hip_sparse_general_batch_primal_normal
(DESIGN.md section 18).  The reference of every numerical comparison is tests/bounded_twin.solve run LP by LP with that LP's own
matrix (general_batch_cases.twin_each); bounds are the project's (gbc.assert_parity): status equal and 0, iterations within 1,
objectives 1e-9 relative, x at rtol 1e-5 / atol 1e-7; HiGHS at 1e-8 for the twin itself.

test_trajectory appends its measured deviations to the file PYCLLP_TRAJECTORY_REPORT names
(profiles/bounded_wave_perA/trajectory.txt)."""
import ctypes
import os
import re

import numpy as np
import pytest

import general_batch_cases as gbc
import sparse_general_batch_cases as sgc
from conftest import ROOT
from pycllp_amd import _native
from pycllp_amd.lp import GeneralLP, SparseMatrix
from pycllp_amd.solvers import solver_registry
from pycllp_amd.solvers.general import subset
from test_general_solver import check_kkt, highs_general, make_general
from test_sparse_general_solver import certificate_lps, make_sparse_general

NAME = "hip_sparse_general_batch_primal_normal"
ENTRY = "pycllp_hip_sparse_solve_batch_bounded"
KERNEL = "bounded wave per-problem"
KEYS = gbc.OUTPUTS
REJECTED_FLAGS = (_native.FLAG_HSD, _native.FLAG_PREDCORR, _native.FLAG_WARM_START, _native.FLAG_WAVE_KERNEL,
                  _native.FLAG_BLOCK_KERNEL, _native.FLAG_NO_SLACK_PATH, _native.FLAG_FORCE_GUARD_PATH)


# ---- CPU ------------------------------------------------------------------------------------------------------------------
def test_symbol_is_declared_and_exported():
    header = open(os.path.join(ROOT, "include", "pycllp_hip.h")).read()
    assert re.search(r"\bint\s+%s\s*\(" % ENTRY, header)
    assert ENTRY in _native.EXPORTS
    sig = dict((n, (a, r)) for n, a, r in _native.SIGNATURES)[ENTRY]
    assert len(sig[0]) == 16                                  # handle, B, Adata, b, c, u, eight outputs, opts, stream
    assert hasattr(_native.lib(), ENTRY)


def test_plugin_is_registered():
    from pycllp_amd.solvers import HipSparseGeneralBatchPrimalNormalSolver
    assert solver_registry[NAME] is HipSparseGeneralBatchPrimalNormalSolver
    assert HipSparseGeneralBatchPrimalNormalSolver.name == NAME


@pytest.mark.parametrize("kw", [dict(hsd=True), dict(hsd="yes"), dict(predcorr=True), dict(warm_start=True),
                                dict(autoscale="sometimes")] + [dict(flags=f) for f in REJECTED_FLAGS], ids=str)
def test_constructor_rejects_what_the_sparse_general_plugin_rejects(kw):
    for name in (NAME, "hip_sparse_general_primal_normal"):
        with pytest.raises(ValueError):
            solver_registry[name](**kw)


def test_constructor_accepts_what_the_sparse_general_plugin_accepts():
    for name in (NAME, "hip_sparse_general_primal_normal"):
        with pytest.raises(TypeError):
            solver_registry[name](bogus=1)
        s = solver_registry[name](hsd=False, autoscale=True, max_iter=50)
        assert s.options["flags"] & _native.FLAG_AUTOSCALE and s.hsd is False and s.options["max_iter"] == 50
        assert solver_registry[name]().hsd == "auto"


def test_entry_checks_its_arguments_before_any_device_call():
    L = _native.lib()
    f = getattr(L, ENTRY)
    o = _native.default_opts()
    fake = ctypes.cast(ctypes.create_string_buffer(64), ctypes.c_void_p)   # never read: the checks precede the use of the handle
    p = ctypes.c_void_p(8)
    args = lambda h, B, A, uu, oo: (h, B, A, p, p, uu, p, p, p, p, p, p, p, p, ctypes.byref(oo), None)   # noqa: E731
    for bad in (args(None, 4, p, p, o), args(fake, 4, None, p, o), args(fake, 4, p, None, o), args(fake, -1, p, p, o)):
        assert f(*bad) == -1
        assert b"bad argument" in L.pycllp_hip_last_error()
    for flag in REJECTED_FLAGS:
        ob = _native.default_opts(flags=flag | _native.FLAG_AUTOSCALE)
        assert f(*args(fake, 4, p, p, ob)) == -1, flag
        assert b"not available with upper bounds" in L.pycllp_hip_last_error(), flag


def _with_explicit_zero(glp):
    """The same batch with LP 0's first two off-slack values set to 0: the structure keeps their slots."""
    data = np.array(glp.A.data)
    data[0, :2] = 0.0
    A = SparseMatrix(np.asarray(glp.A._rows).copy(), np.asarray(glp.A._cols).copy(), data)
    A._shape = (glp.nrows, glp.ncols)
    return GeneralLP(A, glp.b, glp.c, a=glp.a, l=glp.l, u=glp.u, f=glp.f)


@pytest.mark.parametrize("case", ["P1", "P2", "P2-zero"])
def test_csr_permutation_reproduces_every_matrix(case):
    import scipy.sparse as sp
    from pycllp_amd.solvers.sparse_general_batch import csr_structure
    glp = sgc.make(case[:2], 5)
    if case.endswith("zero"):
        glp = _with_explicit_zero(glp)
        assert (np.asarray(glp.A.data[0]) == 0).sum() == 2
    blp, _ = glp.to_bounded_equality_form()
    perm, indptr, indices = csr_structure(blp.A)
    assert perm.size == blp.A.nnzeros == indptr[-1] and indptr.size == blp.nrows + 1
    assert all((np.diff(indices[indptr[i]:indptr[i + 1]].astype(int)) > 0).all() for i in range(blp.nrows))      # CSR order
    s = solver_registry[NAME]()
    s._perm = perm
    vals = s.bounded_values(blp)
    assert vals.shape == (5, perm.size) and vals.flags["C_CONTIGUOUS"] and vals.dtype == np.float64
    for k in range(5):
        A = sp.csr_matrix((vals[k], indices, indptr), shape=(blp.nrows, blp.ncols))
        assert A.nnz == perm.size                             # LP 0's zeros keep their slots
        assert np.array_equal(A.toarray(), blp.A.todense(k)), k
        assert np.array_equal(blp.A.todense(k)[:, glp.ncols:], np.eye(blp.nrows))      # the slack columns' ones are stored


def test_duplicate_entries_raise():
    from pycllp_amd.solvers.sparse_general_batch import csr_structure
    A = SparseMatrix([0, 0, 1], [1, 1, 0], np.ones((2, 3)))
    with pytest.raises(ValueError, match="duplicate"):
        csr_structure(A)


def test_native_range():
    S = solver_registry[NAME]
    for point, (mk, n, _, _, _) in sgc.POINTS.items():
        glp = sgc.make(point, 3)
        blp, _ = glp.to_bounded_equality_form()
        assert (blp.nrows, blp.ncols) == (mk, n + mk) and glp.nrows == mk        # no row is dropped
        assert np.isinf(blp.u).any() and (blp.u == 0).any() and (np.isfinite(blp.u) & (blp.u > 0)).any()
        assert S.native_fits(glp, blp), point
    shared = make_sparse_general(40, 120, 3, seed=1, density=0.08, mixed_u=True, kinds=gbc.kinds(40))
    assert not S.native_fits(shared, shared.to_bounded_equality_form()[0])
    g129 = make_general(129, 20, 2, seed=3, per_problem_A=True, kinds=["le"] * 129)
    assert not S.native_fits(g129, g129.to_bounded_equality_form()[0])
    g513 = make_general(12, 501, 2, seed=4, per_problem_A=True, kinds=["le"] * 12)       # N = 501 + 12
    b513 = g513.to_bounded_equality_form()[0]
    assert b513.ncols == 513 and not S.native_fits(g513, b513)
    g512 = make_general(12, 500, 2, seed=4, per_problem_A=True, kinds=["le"] * 12)
    assert S.native_fits(g512, g512.to_bounded_equality_form()[0])


@pytest.mark.parametrize("point", ["P1", "P2"])
def test_twin_lp_by_lp_matches_highs(point):
    glp = sgc.make(point, 6, 11)
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
        sgc.make("P1", 6, 11).init(solver_registry[NAME]())


# ---- GPU ------------------------------------------------------------------------------------------------------------------
def solve(glp, name=NAME, **kw):
    s = solver_registry[name](device="cuda:0", **dict(dict(hsd=False, autoscale=False), **kw))
    glp.init(s)
    glp.solve(s)
    return s, gbc.plugin_results(s)


def twin(glp, idx=None, **opts):
    blp, bmap = glp.to_bounded_equality_form()
    return gbc.general_results(bmap, blp, gbc.twin_each(blp, idx, **opts), idx)


def check_point(point):
    glp = sgc.make(point)
    s, got = solve(glp)
    info = s.launch_info()
    print(point, info)
    assert s.kernel == KERNEL
    assert (info["variant"], info["kernel"]) == ("tables", "wave"), info      # launch_info: kernel 1
    assert info.get("wave_shape") == sgc.POINTS[point][3], info
    assert 64 <= info["block"] <= 256 and info["block"] % 64 == 0
    idx, ref = sgc.twin(point)
    gbc.assert_parity(got, ref, idx)
    assert (got["status"] == 0).all(), np.unique(got["status"], return_counts=True)
    check_kkt(glp, s)
    return glp, s, info


@pytest.mark.gpu
@pytest.mark.parametrize("point", ["P1", "P2", "P3", "P4"])
def test_every_point(point):
    glp, s, info = check_point(point)
    if point == "P4":
        # the gap this kernel closes: the shared-A plugin sends the batch to the expansion, which the library refuses
        r = solver_registry["hip_sparse_general_primal_normal"](device="cuda:0", hsd=False, autoscale=False)
        glp.init(r)
        with pytest.raises(NotImplementedError):
            glp.solve(r)
        assert r.kernel == "expanded"
        assert info["block"] < 256, info                       # fewer than 4 waves per workgroup


@pytest.mark.gpu
def test_the_cap():
    """P5 (m' = 128, N = 512): the plan fits with fewer waves per workgroup (DESIGN.md section 18 states how many)."""
    check_point("P5")


@pytest.mark.gpu
def test_wave_refill():
    """More LPs than the launch has waves (at most 256 x 4 x 2): every wave takes a second LP, with its own values, t and s."""
    from pycllp_amd.solvers.hip import autoscale_wanted
    B = 3000
    glp = sgc.in_band(sgc.make("P1", B, 77))
    blp, _ = glp.to_bounded_equality_form()
    assert not autoscale_wanted(blp.b, blp.c, blp.u)           # in-band data: the same scaling alone and in the batch
    s, got = solve(glp, autoscale="auto")
    info = s.launch_info()
    assert s.kernel == KERNEL and B > info["grid"] * (info["block"] // 64), info
    assert (got["status"] == 0).all(), np.unique(got["status"], return_counts=True)
    idx = np.linspace(0, B - 1, 64).astype(int)
    gbc.assert_parity(got, twin(glp, idx), idx)
    for j in (0, 1777, B - 1):
        one = subset(glp, np.array([j]))
        # (a batch of one has a shared A for the plugins: the entry itself, through solve_device)
        b1, _ = one.to_bounded_equality_form()
        assert not autoscale_wanted(b1.b, b1.c, b1.u)
        out = s.solve_device(s.bounded_values(blp)[j:j + 1], blp.b[j:j + 1], blp.c[j:j + 1], blp.u[j:j + 1])
        bmap = glp.to_bounded_equality_form()[1]
        r1 = {k: v.cpu().numpy() for k, v in out.items()}
        alone = gbc.general_results(bmap, blp, r1, [j])
        for k in KEYS:
            assert np.array_equal(alone[k][0], got[k][j]), (j, k)


@pytest.mark.gpu
def test_values_matter_and_order_does_not():
    """Row scaling: "the same x to 1e-7" is the project's bound on x (atol 1e-7 with rtol 1e-5, as the same check of
    tests/test_dense_batch.py).  With rtol = 0 the reference itself misses 1e-7 on this batch: the twin's x of the scaled and
    the unscaled LPs differ by up to 2.51e-7 (5 entries of LPs 2 and 47, x about 0.8), because the scaling moves the stop
    tests (eps (1 + |b|)) and with them the iteration count (LP 1: 22 -> 24); the kernel shows the same 2.51e-7."""
    import torch
    from pycllp_amd.solvers.hip import Handle, solve_opts
    glp = sgc.make("P2", 48, 13)
    s, got = solve(glp)
    assert s.kernel == KERNEL and (got["status"] == 0).all()
    f = (0.5 + 1.5 * np.random.RandomState(7).rand(glp.nproblems))[:, None]      # per-LP factors in [0.5, 2]
    s2, g2 = solve(gbc.scaled_rows(glp, f[:, 0]))
    assert s2.kernel == KERNEL and (g2["status"] == 0).all()
    print("scaled rows: max |dx| %.2e, max |dy| %.2e" % (np.abs(g2["x"] - got["x"]).max(), np.abs(g2["y"] * f - got["y"]).max()))
    np.testing.assert_allclose(g2["x"], got["x"], rtol=1e-5, atol=1e-7)
    np.testing.assert_allclose(g2["y"] * f, got["y"], rtol=1e-6, atol=1e-7)
    perm = np.random.RandomState(8).permutation(glp.nproblems)
    _, gp = solve(subset(glp, perm))
    for k in KEYS:
        assert np.array_equal(gp[k], got[k][perm]), k
    # every matrix equal (LPs built around one shared matrix): the shared-A bounded wave kernel on the same handle
    shared_lp = make_sparse_general(40, 120, 48, seed=14, density=0.08, fixed=2, mixed_u=True, kinds=gbc.kinds(40))
    blp, _ = shared_lp.to_bounded_equality_form()
    dev = torch.device("cuda:0")
    A0 = blp.A.tocsr()
    A0.sum_duplicates(); A0.sort_indices()
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
    assert h.launch_info()["wave_shape"] == (3, 4)
    h.solve_bounded(None, b, c, u, batch, o, values=t(np.broadcast_to(A0.data, (B, A0.nnz))))
    torch.cuda.synchronize()
    assert h.launch_info()["wave_shape"] == (3, 4)
    sh, ba = ({k: v.cpu().numpy() for k, v in r.items()} for r in (shared, batch))
    print("all matrices equal: bit-exact with the shared-A bounded wave kernel: %s"
          % {k: bool(np.array_equal(sh[k], ba[k])) for k in KEYS})
    assert (sh["status"] == 0).all()
    gbc.assert_parity(ba, sh)


@pytest.mark.gpu
@pytest.mark.parametrize("sb,sc", [(1e3, 1e-3), (1e-3, 1e3)])
def test_autoscale(sb, sc):
    glp = gbc.scaled_data(sgc.make("P2", 24, 15), sb, sc)
    idx = sgc.sample("P2", 24)
    ref = twin(glp, idx, autoscale=True)
    for kw in (dict(autoscale=True), dict(autoscale="auto")):
        s, got = solve(glp, **kw)
        assert s.kernel == KERNEL
        gbc.assert_parity(got, ref, idx)
    check_kkt(glp, s)


@pytest.mark.gpu
@pytest.mark.parametrize("B", [0, 1, 2, 63])
def test_batch_sizes(B):
    full = sgc.make("P1", 63, 23)
    blp, _ = full.to_bounded_equality_form()
    s = solver_registry[NAME](device="cuda:0", hsd=False, autoscale=False)
    full.init(s)
    out = s.solve_device(s.bounded_values(blp)[:B], blp.b[:B], blp.c[:B], blp.u[:B])
    got = {k: out[k].cpu().numpy() for k in KEYS}
    assert got["x"].shape == (B, 32) and got["s"].shape == (B, 32) and got["y"].shape == (B, 12)
    if B:
        assert s.launch_info()["wave_shape"] == (1, 4)
        idx = np.unique(np.linspace(0, B - 1, min(B, 8)).astype(int))
        gbc.assert_parity(got, gbc.twin_each(blp, idx), idx)


@pytest.mark.gpu
@pytest.mark.parametrize("point", sgc.TRAJECTORY_POINTS)
def test_trajectory(point):
    """x, y, z, s and the objectives of every LP (bounded form's variables) after k = 1, 2, 4, 8 iterations against the twin at
    the same k, LP by LP with that LP's matrix (deviation and tolerance of tests/trajectory.py)."""
    import trajectory as tj
    glp = sgc.trajectory_lp(point)
    blp, _ = glp.to_bounded_equality_form()
    s = solver_registry[NAME](device="cuda:0", hsd=False, autoscale=False)
    glp.init(s)
    A = s.bounded_values(blp)
    lines = []
    for k in tj.K:
        out = s.solve_device(A, blp.b, blp.c, blp.u, max_iter=k)
        got = {q: out[q].cpu().numpy() for q in KEYS}
        ref, tol = sgc.trajectory_reference(point, k), sgc.trajectory_tolerance(point, k)
        dev = {q: tj.deviation(got[q], ref[q]) for q in sgc.TRAJ_QUANTITIES}
        lines.append("%s k=%d %s" % (point, k, "  ".join("%s %.1e (tol %.1e)" % (q, dev[q].max(), tol[q]) for q in sgc.TRAJ_QUANTITIES)))
        print(lines[-1])
        for side in (got, ref):
            assert (side["status"] == 5).all() and (side["iters"] == k).all(), (k, side["status"], side["iters"])
        for q in sgc.TRAJ_QUANTITIES:
            assert dev[q].shape == (glp.nproblems,)
            assert dev[q].max() <= tol[q], "%s after %d iterations: %s off by %.2e on LP %d (bound %.2e)" % (
                point, k, q, dev[q].max(), int(dev[q].argmax()), tol[q])
    report = os.environ.get("PYCLLP_TRAJECTORY_REPORT")
    if report:
        with open(report, "a") as f:
            f.write("\n".join(lines) + "\n")


def certificate_batch():
    """``certificate_lps`` (feasible, infeasible, unbounded) with per-problem values: LP k's matrix times (1 + k / 8)."""
    g = certificate_lps()
    rows, cols = np.asarray(g.A._rows), np.asarray(g.A._cols)
    fk = 1.0 + np.arange(3)[:, None] / 8.0
    A = SparseMatrix(rows.copy(), cols.copy(), np.asarray(g.A.data[0]) * fk)
    A._shape = (g.nrows, g.ncols)
    return GeneralLP(A, g.b * fk, g.c, u=g.u, f=0.0)


@pytest.mark.gpu
def test_plugin_resolves_an_infeasible_lp():
    glp = certificate_batch()
    s, raw = solve(glp)                                        # hsd=False: the kernel's verdict
    assert s.kernel == KERNEL
    assert raw["status"][0] == 0 and raw["status"][1] != 0 and raw["status"][2] != 0, raw["status"]
    s, got = solve(glp, hsd="auto")
    assert s.kernel == KERNEL and list(got["status"]) == [0, 2, 4]
    for k in KEYS:
        assert np.array_equal(got[k][0], raw[k][0]), k
    assert gbc.rel(got["pobj"][0], highs_general(glp, 0)[0]) <= 1e-8


@pytest.mark.gpu
def test_plugin_delegates_outside_the_native_range():
    glp = make_sparse_general(40, 120, 32, seed=12, density=0.08, fixed=2, mixed_u=True)       # shared A
    s, got = solve(glp, hsd="auto", autoscale="auto")
    r, ref = solve(glp, "hip_sparse_general_primal_normal", hsd="auto", autoscale="auto")
    assert s.kernel == r.kernel == "bounded wave"
    for k, v in ref.items():
        assert np.array_equal(got[k], v), k
    glp = make_general(130, 20, 4, seed=9, per_problem_A=True, kinds=["le"] * 130)             # m' = 130: beyond the kernel
    s = solver_registry[NAME](device="cuda:0", hsd="auto", autoscale="auto")
    r = solver_registry["hip_sparse_general_primal_normal"](device="cuda:0", hsd="auto", autoscale="auto")
    outcome = []
    for sol in (s, r):
        glp.init(sol)
        try:
            glp.solve(sol)
            outcome.append(("solved", sol.kernel, sol.status.tolist(), sol.primal_obj.tolist()))
        except NotImplementedError:
            outcome.append(("refused", sol.kernel))
    assert outcome[0] == outcome[1] and outcome[0][1] == "expanded", outcome
    with pytest.raises(RuntimeError, match="solve_device"):
        s.solve_device(np.zeros((1, 5)), np.zeros((1, 130)), np.zeros((1, 150)), np.zeros((1, 150)))


@pytest.mark.gpu
def test_entry_declines_what_it_cannot_serve():
    import scipy.sparse as sp
    import torch
    from pycllp_amd.solvers.hip import Handle, solve_opts
    dev = torch.device("cuda:0")
    rs = np.random.default_rng(0)
    o = solve_opts({})
    # (a large-LP handle, m > 128; a dense 48 x 128 structure [A | I], whose term tables do not fit the LDS)
    for m, n, text in ((130, 150, "stops at m = 128"), (48, 128 + 48, "no variant")):
        A = np.hstack([rs.uniform(0.1, 1, (m, n - m)), np.eye(m)])
        h = Handle(sp.csr_matrix(A), dev, None)
        nnz = int((A != 0).sum())
        z = lambda *shape: torch.zeros(shape, dtype=torch.float64, device=dev)
        out = dict(x=z(1, n), y=z(1, m), z=z(1, n), s=z(1, n), pobj=z(1), dobj=z(1),
                   status=torch.zeros(1, dtype=torch.int32, device=dev), iters=torch.zeros(1, dtype=torch.int32, device=dev))
        with pytest.raises(NotImplementedError, match=text):
            h.solve_bounded(None, z(1, m), z(1, n), z(1, n), out, o, values=z(1, nnz))
    # the plugin hands such a batch to its delegate
    glp = make_general(48, 128, 4, seed=5, per_problem_A=True, kinds=gbc.kinds(48), fixed=2, mixed_u=True)
    s = solver_registry[NAME](device="cuda:0", hsd=False, autoscale=False)
    glp.init(s)
    try:
        glp.solve(s)
    except NotImplementedError:
        pass                                                   # the expansion (m = 208 rows) is beyond the per-problem kernels
    assert s.kernel == "expanded" and s._delegate is not None
