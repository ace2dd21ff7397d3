"""GeneralLP on the bounded kernel: the bounded equality form (CPU), its CPU twin (CPU), the C ABI entry (CPU) and the
solver plugin ``hip_general_primal_normal`` (GPU) against the twin, HiGHS and the expansion path."""
import ctypes

import numpy as np
import pytest
from scipy.optimize import linprog

from conftest import golden
from pycllp_amd import _native
from pycllp_amd.lp import GeneralLP, SparseMatrix
import bounded_twin

SHAPES = [(16, 32), (16, 48), (16, 64), (32, 64), (32, 96), (32, 128)]   # the slack-aware kernels (MP, NP)


def make_general(m, n, B, seed, per_problem_A=False, mixed_u=False, kinds=None, fixed=0, with_x0=False):
    """A feasible, bounded GeneralLP batch: rows by kind -- 'eq' (a == b), 'rng' (a < b), 'le' (b only), 'ge' (a only), 'free'
    (dropped) -- around a point x0 inside [l, u]; row 0 is a '<=' row with positive coefficients, which bounds x >= l.
    ``with_x0``: return (the batch, x0)."""
    rng = np.random.default_rng(seed)
    P = B if per_problem_A else 1
    A = rng.uniform(-1, 1, (P, m, n))
    A[:, 0, :] = rng.uniform(0.1, 1, (P, n))
    if kinds is None:
        kinds = ["le"] + [("eq", "rng", "le", "ge")[i % 4] for i in range(m - 1)]
    l = rng.uniform(0, 0.5, (B, n))
    u = l + rng.uniform(0.5, 2, (B, n))
    if mixed_u:
        u[: B // 2, n - 3:] = np.inf      # the last columns have no bound in half of the LPs
    x0 = l + rng.uniform(0.2, 0.8, (B, n)) * np.where(np.isfinite(u), u - l, 1.0)
    if fixed:
        u[:, :fixed] = l[:, :fixed]
        x0[:, :fixed] = l[:, :fixed]
    Ax = np.einsum("bij,bj->bi", A, x0) if P > 1 else x0 @ A[0].T
    a = np.full((B, m), -np.inf); b = np.full((B, m), np.inf)
    for i, k in enumerate(kinds):
        if k == "eq":
            a[:, i] = b[:, i] = Ax[:, i]
        elif k == "rng":
            a[:, i] = Ax[:, i] - rng.uniform(0.1, 1, B); b[:, i] = Ax[:, i] + rng.uniform(0.1, 1, B)
        elif k == "le":
            b[:, i] = Ax[:, i] + rng.uniform(0.1, 1, B)
        elif k == "ge":
            a[:, i] = Ax[:, i] - rng.uniform(0.1, 1, B)
    c = rng.uniform(-1, 1, (B, n))
    if P > 1:
        Asp = SparseMatrix(np.repeat(np.arange(m), n), np.tile(np.arange(n), m), A.reshape(P, -1))
        Asp._shape = (m, n)
    else:
        Asp = SparseMatrix(matrix=A[0])
    glp = GeneralLP(Asp, b, c, a=a, l=l, u=u, f=rng.uniform(-1, 1, B))
    return (glp, x0) if with_x0 else glp


def highs_general(glp, k):
    """HiGHS optimum (maximisation, f included) of problem k of a GeneralLP."""
    A = glp.A.todense(k if glp.A.nproblems > 1 else 0)
    a, b = glp.a[k], glp.b[k]
    hi, lo = np.isfinite(b), np.isfinite(a)
    A_ub = np.vstack([A[hi], -A[lo]]); b_ub = np.concatenate([b[hi], -a[lo]])
    bounds = [(glp.l[k, j], None if not np.isfinite(glp.u[k, j]) else glp.u[k, j]) for j in range(glp.ncols)]
    r = linprog(-glp.c[k], A_ub=A_ub if len(b_ub) else None, b_ub=b_ub if len(b_ub) else None, bounds=bounds, method="highs")
    assert r.status == 0, r.message
    return -r.fun + glp.f[k], r.x


def highs_bounded(blp, k):
    A = blp.A.todense(k if blp.A.nproblems > 1 else 0)
    bounds = [(0, None if not np.isfinite(v) else v) for v in blp.u[k]]
    r = linprog(-blp.c[k], A_eq=A, b_eq=blp.b[k], bounds=bounds, method="highs")
    assert r.status == 0, r.message
    return -r.fun + blp.f[k], r.x


# ---- CPU: the bounded equality form ----------------------------------------------------------------------------------------
CASES = [dict(m=6, n=5, B=4, seed=1),
         dict(m=8, n=7, B=3, seed=2, fixed=2),
         dict(m=7, n=6, B=4, seed=3, mixed_u=True),
         dict(m=6, n=6, B=3, seed=4, per_problem_A=True),
         dict(m=9, n=5, B=3, seed=5, kinds=["le", "free", "ge", "eq", "rng", "free", "ge", "ge", "eq"]),
         dict(m=5, n=8, B=2, seed=6, kinds=["le", "ge", "ge", "ge", "free"], fixed=1)]


@pytest.mark.parametrize("case", CASES, ids=lambda c: "seed%d" % c["seed"])
def test_bounded_form_keeps_the_optimum(case):
    glp = make_general(**case)
    blp, bmap = glp.to_bounded_equality_form()
    assert blp.nrows == sum(1 for k in (case.get("kinds") or ["x"] * case["m"]) if k != "free")
    assert blp.ncols == glp.ncols + blp.nrows
    for k in range(glp.nproblems):
        ref, _ = highs_general(glp, k)
        obj, xh = highs_bounded(blp, k)
        xs = np.zeros((glp.nproblems, blp.ncols)); xs[k] = xh
        x = bmap.general(xs, np.zeros((glp.nproblems, blp.nrows)))[0][k]
        assert abs(obj - ref) <= 1e-9 * max(1.0, abs(ref))
        assert abs(glp.c[k] @ x + glp.f[k] - ref) <= 1e-9 * max(1.0, abs(ref))


def test_bounded_form_golden_fixtures():
    g = golden("general_lp.npz")
    for key in [str(k) for k in g["keys"]]:
        A = g[key + "_A"]
        glp = GeneralLP(SparseMatrix(matrix=A), g[key + "_b"], g[key + "_c"], a=g[key + "_a"], l=g[key + "_l"], f=0.0)
        blp, _ = glp.to_bounded_equality_form()
        # the golden standard form of the same LP (to_standard_form, as the reference computes it)
        std_obj = -linprog(-g[key + "_std_c"][0], A_ub=g[key + "_std_A"], b_ub=g[key + "_std_b"][0], method="highs").fun \
            + g[key + "_std_f"][0]
        obj, _ = highs_bounded(blp, 0)
        assert abs(obj - std_obj) <= 1e-9 * max(1.0, abs(std_obj)), key


def test_bounded_form_errors():
    A = SparseMatrix(matrix=np.array([[1.0, 1.0], [1.0, -1.0]]))
    with pytest.raises(ValueError, match="-inf"):
        GeneralLP(A, [1.0, 1.0], [1.0, 1.0], l=[-np.inf, 0.0], f=0.0).to_bounded_equality_form()
    with pytest.raises(ValueError, match="below"):
        GeneralLP(A, [1.0, 1.0], [1.0, 1.0], l=[1.0, 0.0], u=[0.5, 1.0], f=0.0).to_bounded_equality_form()
    with pytest.raises(ValueError, match="above"):
        GeneralLP(A, [1.0, 1.0], [1.0, 1.0], a=[2.0, -np.inf], f=0.0).to_bounded_equality_form()
    with pytest.raises(ValueError, match="Can not keep row 1"):
        GeneralLP(A, [[1.0, 1.0], [1.0, np.inf]], [1.0, 1.0], f=0.0).to_bounded_equality_form()
    # +inf and -inf both mean "no lower bound"; the reference stores +inf
    for noa in (np.inf, -np.inf):
        blp, bmap = GeneralLP(A, [1.0, np.inf], [1.0, 1.0], a=[noa, 0.5], f=0.0).to_bounded_equality_form()
        assert list(bmap.sign) == [1.0, -1.0] and np.isinf(blp.u[0, 2]) and np.isinf(blp.u[0, 3])


def test_twin_matches_highs():
    glp = make_general(12, 20, 6, seed=11, fixed=2, mixed_u=True)
    blp, _ = glp.to_bounded_equality_form()
    r = bounded_twin.solve(blp.A.todense(), blp.b, blp.c, blp.u)
    assert (r["status"] == 0).all(), r["status"]
    for k in range(glp.nproblems):
        ref, _ = highs_bounded(blp, k)
        assert abs(r["pobj"][k] + blp.f[k] - ref) <= 1e-8 * max(1.0, abs(ref))
        assert abs(r["dobj"][k] + blp.f[k] - ref) <= 1e-8 * max(1.0, abs(ref))


def test_bounded_abi_rejections_without_gpu():
    L = _native.lib()
    assert hasattr(L, "pycllp_hip_dense_solve_bounded")
    o = _native.default_opts()
    fake = ctypes.create_string_buffer(64)     # never read: every argument check precedes the use of the handle
    u = ctypes.c_void_p(8)
    args = lambda h, uu, oo: (h, 4, u, u, uu, u, u, u, u, u, u, u, u, ctypes.byref(oo), None)   # noqa: E731
    assert L.pycllp_hip_dense_solve_bounded(*args(None, u, o)) == -1
    assert L.pycllp_hip_dense_solve_bounded(*args(ctypes.cast(fake, ctypes.c_void_p), None, o)) == -1
    for flag in (_native.FLAG_HSD, _native.FLAG_PREDCORR, _native.FLAG_WARM_START, _native.FLAG_WAVE_KERNEL,
                 _native.FLAG_NO_SLACK_PATH):
        ob = _native.default_opts(flags=flag)
        assert L.pycllp_hip_dense_solve_bounded(*args(ctypes.cast(fake, ctypes.c_void_p), u, ob)) == -1
        assert b"not available with upper bounds" in L.pycllp_hip_last_error()


def test_solver_option_errors():
    from pycllp_amd.solvers import HipGeneralPrimalNormalSolver
    for kw in (dict(hsd=True), dict(predcorr=True), dict(warm_start=True), dict(flags=_native.FLAG_HSD)):
        with pytest.raises(ValueError):
            HipGeneralPrimalNormalSolver(**kw)


# ---- GPU: the solver plugin ------------------------------------------------------------------------------------------------
# (m', n) per slack-aware kernel: the first kernel whose shape covers the bounded form is the one that serves it
NATIVE_SIZES = {(16, 32): (12, 16), (16, 48): (14, 30), (16, 64): (16, 44), (32, 64): (24, 32), (32, 96): (24, 64),
                (32, 128): (30, 90)}


def gpu_solver(**kw):
    from pycllp_amd.solvers import HipGeneralPrimalNormalSolver
    return HipGeneralPrimalNormalSolver(device="cuda:0", **kw)


def run(glp, **kw):
    s = gpu_solver(**kw)
    glp.init(s)
    glp.solve(s)
    return s


def check_kkt(glp, s, tol=1e-6):
    """Optimality of (x, y, z, s) for  max c'x + f, a <= A x <= b, l <= x <= u  from the returned vectors alone."""
    for k in range(glp.nproblems):
        A = glp.A.todense(k if glp.A.nproblems > 1 else 0)
        x, y, z, sv = s.x[k], s.y[k], s.z[k], s.s[k]
        scale = 1 + np.abs(glp.c[k]).max() + np.abs(y).max()
        ax = A @ x
        a, b, l, u = glp.a[k], glp.b[k], glp.l[k], glp.u[k]
        xs = 1 + np.abs(x).max()
        assert (x >= l - tol * xs).all() and (x <= u + tol * xs).all(), k
        assert (ax <= b + tol * xs * (1 + np.abs(b[np.isfinite(b)]).max(initial=0))).all(), k
        assert (ax >= a - tol * xs * (1 + np.abs(a[np.isfinite(a)]).max(initial=0))).all(), k
        assert np.abs(A.T @ y - z + sv - glp.c[k]).max() <= tol * scale, k
        assert z.min() >= -tol * scale and sv.min() >= -tol * scale, k
        assert np.abs(z * (x - l)).max() <= tol * scale * xs, k
        fin = np.isfinite(u)
        assert np.abs(sv[fin] * (u[fin] - x[fin])).max(initial=0) <= tol * scale * xs, k
        assert (sv[~fin] == 0).all(), k
        with np.errstate(invalid="ignore"):
            gap = np.where(y > 0, y * (b - ax), np.where(y < 0, -y * (ax - a), 0.0))
        assert np.abs(np.nan_to_num(gap, nan=np.inf)).max(initial=0) <= tol * scale * xs, k


def rel(a, b):
    return np.abs(a - b) / np.maximum(1.0, np.abs(b))


@pytest.mark.gpu
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "%dx%d" % s)
def test_native_shape_matches_twin_highs_and_expansion(shape):
    mk, n = NATIVE_SIZES[shape]
    B = 4500                 # more LPs than the launch has slots (at most 256 CUs x 4 waves x 4 lane groups): slots refill
    kinds = ["le"] + [("eq", "rng", "le", "ge")[i % 4] for i in range(mk - 1)]
    glp = make_general(mk, n, B, seed=100 + shape[1] + shape[0], kinds=kinds, fixed=1, mixed_u=True)
    s = run(glp)
    assert s.kernel == "bounded group"
    assert (s.status == 0).all(), np.unique(s.status, return_counts=True)
    blp, _ = glp.to_bounded_equality_form()
    assert blp.nrows == mk
    from pycllp_amd.solvers.hip import autoscale_wanted
    tw = bounded_twin.solve(blp.A.todense(), blp.b, blp.c, blp.u, autoscale=autoscale_wanted(blp.b, blp.c, blp.u))
    assert (tw["status"] == 0).all()
    assert rel(s.primal_obj, tw["pobj"] + blp.f).max() <= 1e-9
    assert np.abs(s.iters - tw["iters"]).max() <= 1, np.abs(s.iters - tw["iters"]).max()
    for k in range(0, B, B // 24):
        ref, _ = highs_general(glp, k)
        assert rel(s.primal_obj[k], ref) <= 1e-8 and rel(s.dual_obj[k], ref) <= 1e-8, k
    ex = gpu_solver().solve_expanded(glp)
    assert (ex["status"] == 0).all()
    assert rel(s.primal_obj, ex["primal_obj"]).max() <= 1e-8
    check_kkt(glp, s)


@pytest.mark.gpu
def test_autoscale_and_guard_path():
    base = make_general(20, 40, 300, seed=7, fixed=2)
    refs = np.array([highs_general(base, k)[0] for k in range(0, 300, 10)])
    for sb, scc in ((1e3, 1e-3), (1e-3, 1e3)):
        glp = GeneralLP(SparseMatrix(matrix=base.A.todense()), base.b * sb, base.c * scc, a=base.a * sb, l=base.l * sb,
                        u=base.u * sb, f=base.f * sb * scc)
        s = run(glp)                                   # autoscale='auto' switches itself on
        assert s.kernel == "bounded group" and (s.status == 0).all()
        assert rel(s.primal_obj[::10], refs * sb * scc).max() <= 1e-8 * max(1.0, sb * scc)
        check_kkt(glp, s)
    s = run(base, flags=_native.FLAG_FORCE_GUARD_PATH)
    assert (s.status == 0).all() and rel(s.primal_obj[::10], refs).max() <= 1e-8


@pytest.mark.gpu
def test_fixed_columns_and_determinism():
    glp = make_general(16, 30, 500, seed=8, fixed=5)
    s1 = run(glp)
    assert (s1.status == 0).all()
    assert (s1.x[:, :5] == glp.l[:, :5]).all()
    check_kkt(glp, s1)
    s2 = run(glp)
    for k in ("x", "y", "z", "s", "primal_obj", "dual_obj", "iters", "status"):
        assert np.array_equal(getattr(s1, k), getattr(s2, k)), k


@pytest.mark.gpu
def test_infeasible_and_unbounded_get_certified_statuses():
    A = np.array([[-1.0, 1.0, 0.0], [-1.0, 0.0, 1.0]])
    # LP 0: feasible; LP 1: x2 <= x0 - 4 with x0 <= 3 (infeasible); LP 2: no upper bounds, x2 <= 1 + x0 grows with x0 (unbounded)
    b = np.array([[4.0, 1.0], [4.0, -4.0], [4.0, 1.0]])
    c = np.array([[1.0, 2.0, 1.0], [1.0, 1.0, 1.0], [0.0, 0.0, 1.0]])
    u = np.array([[3.0, 3.0, 3.0], [3.0, 3.0, 3.0], [np.inf, np.inf, np.inf]])
    glp = GeneralLP(SparseMatrix(matrix=A), b, c, u=u, f=0.0)
    s = run(glp)
    assert s.kernel == "bounded group"
    assert list(s.status) == [0, 2, 4]
    assert rel(s.primal_obj[0], highs_general(glp, 0)[0]) <= 1e-8


@pytest.mark.gpu
def test_expanded_fallback_beyond_the_kernel():
    for glp in (make_general(40, 30, 64, seed=9), make_general(12, 20, 64, seed=10, per_problem_A=True)):
        s = run(glp)
        assert s.kernel == "expanded"
        assert (s.status == 0).all()
        refs = np.array([highs_general(glp, k)[0] for k in range(glp.nproblems)])
        assert rel(s.primal_obj, refs).max() <= 1e-8
        check_kkt(glp, s)
    glp = make_general(20, 30, 64, seed=12)
    s = run(glp)
    assert s.kernel == "bounded group"
    assert rel(s.primal_obj, gpu_solver().solve_expanded(glp)["primal_obj"]).max() <= 1e-8


@pytest.mark.gpu
def test_bounded_entry_declines_a_handle_without_identity_tail():
    import torch
    L = _native.lib()
    A = torch.tensor(np.random.default_rng(0).uniform(-1, 1, (4, 8)), dtype=torch.float64, device="cuda:0")
    h = ctypes.c_void_p()
    _native.check(L.pycllp_hip_dense_init(4, 8, ctypes.c_void_p(A.data_ptr()), None, ctypes.byref(h)), "init")
    try:
        p = ctypes.c_void_p(A.data_ptr())
        rc = L.pycllp_hip_dense_solve_bounded(h, 1, p, p, p, p, p, p, p, p, p, p, p, ctypes.byref(_native.default_opts()), None)
        assert rc == -2
    finally:
        L.pycllp_hip_dense_free(h)
