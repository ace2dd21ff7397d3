"""GeneralLP on the bounded wave kernel: the C ABI entry ``pycllp_hip_sparse_solve_bounded`` (CPU: argument checks) and the
solver plugin ``hip_sparse_general_primal_normal`` (GPU) against the CPU twin, HiGHS, the expansion and the lane-group kernel."""
import ctypes

import numpy as np
import pytest

import bounded_twin
from pycllp_amd import _native
from pycllp_amd.lp import GeneralLP, SparseMatrix
from test_general_solver import check_kkt, highs_general, make_general, rel

NAME = "hip_sparse_general_primal_normal"
KINDS = ("eq", "rng", "le", "ge", "free")


def mixed_kinds(m):
    """Row 0 a '<=' row (positive coefficients: bounds x from above), then eq / ranged / '<=' / '>=' / free in turn."""
    return ["le"] + [KINDS[i % len(KINDS)] for i in range(m - 1)]


def make_sparse_general(m, n, B, seed, density, fixed=0, mixed_u=False, kinds=None, with_x0=False):
    """``make_general``'s batch with a SPARSE shared A: about ``density`` of the entries of rows 1.. are non-zero, every
    column has one at least, row 0 is dense and positive.  ``kinds``: the row kinds (default ``mixed_kinds(m)``);
    ``with_x0``: return (the batch, the interior point the row bounds are built around)."""
    kinds = mixed_kinds(m) if kinds is None else kinds
    rng = np.random.default_rng(seed)
    mask = rng.uniform(size=(m, n)) < density
    mask[rng.integers(1, m, n), np.arange(n)] = True
    mask[0] = True
    A = np.where(mask, rng.uniform(-1, 1, (m, n)), 0.0)
    A[0] = rng.uniform(0.1, 1, n)
    g = make_general(m, n, B, seed, mixed_u=mixed_u, kinds=kinds, fixed=fixed)
    # same bounds, costs and offsets, the row bounds rebuilt around an interior point for the sparse A
    x0 = g.l + rng.uniform(0.2, 0.8, (B, n)) * np.where(np.isfinite(g.u), g.u - g.l, 1.0)
    x0[:, :fixed] = g.l[:, :fixed]
    Ax = x0 @ A.T
    a, b = np.full((B, m), -np.inf), np.full((B, m), np.inf)
    for i, k in enumerate(kinds):
        if k == "eq":
            a[:, i] = b[:, i] = Ax[:, i]
        elif k == "rng":
            a[:, i] = Ax[:, i] - rng.uniform(0.1, 1, B); b[:, i] = Ax[:, i] + rng.uniform(0.1, 1, B)
        elif k == "le":
            b[:, i] = Ax[:, i] + rng.uniform(0.1, 1, B)
        elif k == "ge":
            a[:, i] = Ax[:, i] - rng.uniform(0.1, 1, B)
    glp = GeneralLP(SparseMatrix(matrix=A), b, g.c, a=a, l=g.l, u=g.u, f=g.f)
    return (glp, x0) if with_x0 else glp


# ---- CPU ---------------------------------------------------------------------------------------------------------------------
def test_registered():
    from pycllp_amd.solvers import solver_registry
    assert NAME in solver_registry
    assert solver_registry[NAME].name == NAME


def test_sparse_bounded_abi_rejections_without_gpu():
    L = _native.lib()
    assert hasattr(L, "pycllp_hip_sparse_solve_bounded")
    o = _native.default_opts()
    fake = ctypes.cast(ctypes.create_string_buffer(64), ctypes.c_void_p)   # never read: the checks precede the use of the handle
    p = ctypes.c_void_p(8)
    args = lambda h, uu, oo: (h, 4, p, p, uu, p, p, p, p, p, p, p, p, ctypes.byref(oo), None)   # noqa: E731
    assert L.pycllp_hip_sparse_solve_bounded(*args(None, p, o)) == -1
    assert L.pycllp_hip_sparse_solve_bounded(*args(fake, None, o)) == -1
    assert b"bad argument" in L.pycllp_hip_last_error()
    for flag in (_native.FLAG_HSD, _native.FLAG_PREDCORR, _native.FLAG_WARM_START, _native.FLAG_WAVE_KERNEL,
                 _native.FLAG_BLOCK_KERNEL, _native.FLAG_NO_SLACK_PATH, _native.FLAG_FORCE_GUARD_PATH):
        ob = _native.default_opts(flags=flag | _native.FLAG_AUTOSCALE)
        assert L.pycllp_hip_sparse_solve_bounded(*args(fake, p, ob)) == -1, flag
        assert b"not available with upper bounds" in L.pycllp_hip_last_error(), flag


def test_solver_option_errors():
    from pycllp_amd.solvers import HipSparseGeneralPrimalNormalSolver as S
    for kw in (dict(hsd=True), dict(hsd="yes"), dict(predcorr=True), dict(warm_start=True), dict(autoscale="sometimes"),
               dict(flags=_native.FLAG_HSD), dict(flags=_native.FLAG_BLOCK_KERNEL), dict(flags=_native.FLAG_FORCE_GUARD_PATH)):
        with pytest.raises(ValueError):
            S(**kw)
    with pytest.raises(TypeError):
        S(bogus=1)
    S(hsd=False, autoscale=True, max_iter=50)


def test_native_range_and_expansion_size():
    from pycllp_amd.solvers.general import HipSparseGeneralPrimalNormalSolver as S, expansion_rows
    glp = make_sparse_general(96, 288, 4, seed=1, density=0.03, mixed_u=True)
    blp, _ = glp.to_bounded_equality_form()
    assert S.native_fits(glp, blp) and blp.ncols == 288 + blp.nrows
    assert expansion_rows(glp) > _native.lib().pycllp_hip_dense_max_rows()      # the expansion is refused
    g2 = make_general(12, 20, 4, seed=2, per_problem_A=True)
    assert not S.native_fits(g2, g2.to_bounded_equality_form()[0])
    g3 = make_general(130, 20, 2, seed=3, kinds=["le"] * 130)
    assert not S.native_fits(g3, g3.to_bounded_equality_form()[0])


# ---- GPU ---------------------------------------------------------------------------------------------------------------------
def run(glp, **kw):
    from pycllp_amd.solvers import solver_registry
    s = solver_registry[NAME](device="cuda:0", **kw)
    glp.init(s)
    glp.solve(s)
    return s


B_SLOTS = 3000     # more LPs than the launch has wave slots (256 CUs x 4 waves, x 2 for m' <= 64): slots refill

# (label, generator, compare with the expansion)
SHAPES = [
    ("dense40x30", lambda: make_general(40, 30, B_SLOTS, seed=201, kinds=mixed_kinds(40), fixed=2, mixed_u=True), True),
    ("dense60x120", lambda: make_general(60, 120, B_SLOTS, seed=202, kinds=mixed_kinds(60), fixed=2, mixed_u=True), True),
    ("sparse64x192", lambda: make_sparse_general(64, 192, B_SLOTS, seed=203, density=0.05, fixed=2, mixed_u=True), False),
    ("sparse96x288", lambda: make_sparse_general(96, 288, B_SLOTS, seed=204, density=0.03, fixed=2, mixed_u=True), False),
]


@pytest.mark.gpu
@pytest.mark.parametrize("label,make,expand", SHAPES, ids=[s[0] for s in SHAPES])
def test_shape_matches_twin_highs_and_expansion(label, make, expand):
    from pycllp_amd.solvers.hip import autoscale_wanted
    glp = make()
    if label == "sparse96x288":
        with pytest.raises(NotImplementedError):
            from pycllp_amd.solvers import HipGeneralPrimalNormalSolver
            s0 = HipGeneralPrimalNormalSolver(device="cuda:0")
            glp.init(s0)
            glp.solve(s0)
    s = run(glp)
    assert s.kernel == "bounded wave"
    assert (s.status == 0).all(), np.unique(s.status, return_counts=True)
    blp, _ = glp.to_bounded_equality_form()
    assert np.isinf(blp.u).any() and (blp.u == 0).any() and blp.nrows < glp.nrows
    sel = np.arange(0, B_SLOTS, B_SLOTS // 128)[:128]
    tw = bounded_twin.solve(blp.A.todense(), blp.b[sel], blp.c[sel], blp.u[sel], autoscale=autoscale_wanted(blp.b, blp.c, blp.u))
    assert (tw["status"] == 0).all()
    assert rel(s.primal_obj[sel], tw["pobj"] + blp.f[sel]).max() <= 1e-9
    assert np.abs(s.iters[sel] - tw["iters"]).max() <= 1, np.abs(s.iters[sel] - tw["iters"]).max()
    for k in range(0, B_SLOTS, B_SLOTS // 24):
        ref, _ = highs_general(glp, k)
        assert rel(s.primal_obj[k], ref) <= 1e-8 and rel(s.dual_obj[k], ref) <= 1e-8, k
    check_kkt(glp, s)
    if expand:
        ex = s.solve_expanded(glp)
        assert (ex["status"] == 0).all()
        assert rel(s.primal_obj, ex["primal_obj"]).max() <= 1e-8


@pytest.mark.gpu
def test_agrees_with_the_lane_group_kernel():
    from pycllp_amd.solvers import HipGeneralPrimalNormalSolver
    glp = make_general(24, 64, 2000, seed=205, kinds=mixed_kinds(24), fixed=1, mixed_u=True)
    g = HipGeneralPrimalNormalSolver(device="cuda:0")
    glp.init(g)
    glp.solve(g)
    s = run(glp)
    assert g.kernel == "bounded group" and s.kernel == "bounded wave"
    assert (g.status == 0).all() and (s.status == 0).all()
    assert rel(s.primal_obj, g.primal_obj).max() <= 1e-9
    assert rel(s.dual_obj, g.dual_obj).max() <= 1e-9


@pytest.mark.gpu
def test_autoscale():
    base = make_sparse_general(64, 160, 400, seed=206, density=0.05, fixed=2)
    refs = np.array([highs_general(base, k)[0] for k in range(0, 400, 20)])
    for sb, scc in ((1e3, 1e-3), (1e-3, 1e3)):
        glp = GeneralLP(SparseMatrix(matrix=base.A.todense()), base.b * sb, base.c * scc, a=base.a * sb, l=base.l * sb,
                        u=base.u * sb, f=base.f * sb * scc)
        s = run(glp)                                   # autoscale='auto' switches itself on
        assert s.kernel == "bounded wave" and (s.status == 0).all()
        assert rel(s.primal_obj[::20], refs * sb * scc).max() <= 1e-8 * max(1.0, sb * scc)
        check_kkt(glp, s)


@pytest.mark.gpu
def test_determinism_and_batch_independence():
    from pycllp_amd.solvers.general import subset
    from pycllp_amd.solvers.hip import autoscale_wanted
    g0 = make_sparse_general(48, 128, 1500, seed=207, density=0.08, fixed=3)
    A, b = g0.A.todense(), g0.b.copy()
    A[0] /= 20; b[:, 0] /= 20                                  # row 0 ('<=') brought into the autoscale band
    glp = GeneralLP(SparseMatrix(matrix=A), b, g0.c, a=g0.a, l=g0.l, u=g0.u, f=g0.f)
    blp, _ = glp.to_bounded_equality_form()
    assert not autoscale_wanted(blp.b, blp.c, blp.u)           # in-band data: the same scaling alone and in the batch
    s1 = run(glp)
    s2 = run(glp)
    assert s1.kernel == "bounded wave" and (s1.status == 0).all()
    keys = ("x", "y", "z", "s", "primal_obj", "dual_obj", "iters", "status")
    for k in keys:
        assert np.array_equal(getattr(s1, k), getattr(s2, k)), k
    for j in (0, 777, 1499):
        one = subset(glp, np.array([j]))
        assert not autoscale_wanted(*(lambda b_: (b_.b, b_.c, b_.u))(one.to_bounded_equality_form()[0]))
        s3 = run(one)
        for k in keys:
            assert np.array_equal(getattr(s3, k)[0], getattr(s1, k)[j]), (j, k)


def certificate_lps():
    A = np.array([[-1.0, 1.0, 0.0], [-1.0, 0.0, 1.0]])
    # LP 0: feasible; LP 1: x2 <= x0 - 4 with x0 <= 3 (infeasible); LP 2: no upper bounds, x2 <= 1 + x0 grows with x0 (unbounded)
    b = np.array([[4.0, 1.0], [4.0, -4.0], [4.0, 1.0]])
    c = np.array([[1.0, 2.0, 1.0], [1.0, 1.0, 1.0], [0.0, 0.0, 1.0]])
    u = np.array([[3.0, 3.0, 3.0], [3.0, 3.0, 3.0], [np.inf, np.inf, np.inf]])
    return GeneralLP(SparseMatrix(matrix=A), b, c, u=u, f=0.0)


@pytest.mark.gpu
def test_infeasible_and_unbounded_statuses():
    glp = certificate_lps()
    s = run(glp, hsd=False)
    assert s.kernel == "bounded wave"
    assert s.status[0] == 0 and s.status[1] != 0 and s.status[2] != 0
    s = run(glp)
    assert s.kernel == "bounded wave"
    assert list(s.status) == [0, 2, 4]
    assert rel(s.primal_obj[0], highs_general(glp, 0)[0]) <= 1e-8
    A, tol = glp.A.todense(), 1e-6
    # LP 1, Farkas: A'y - z + s = 0 with z, s >= 0 and y >= 0 on the '<=' rows, b'y + u's < 0
    y, z, sv = s.y[1], s.z[1], s.s[1]
    val = glp.b[1] @ y + glp.u[1] @ sv
    assert (y >= -tol * abs(val)).all() and z.min() >= -tol * abs(val) and sv.min() >= -tol * abs(val) and val < 0
    assert np.abs(A.T @ y - z + sv).max() <= tol * -val * (1 + np.linalg.norm(glp.c[1]))
    # LP 2, a ray: d = x - l >= 0 with A d <= 0 and c'd > 0
    d = s.x[2] - glp.l[2]
    cd = glp.c[2] @ d
    assert cd > 0 and d.min() >= -tol * cd and (A @ d).max() <= tol * cd * (1 + np.linalg.norm(glp.b[2]))


@pytest.mark.gpu
def test_per_problem_a_takes_the_expansion():
    glp = make_general(12, 20, 64, seed=208, per_problem_A=True, kinds=mixed_kinds(12), fixed=1)
    s = run(glp)
    assert s.kernel == "expanded"
    assert (s.status == 0).all()
    refs = np.array([highs_general(glp, k)[0] for k in range(glp.nproblems)])
    assert rel(s.primal_obj, refs).max() <= 1e-8
    check_kkt(glp, s)
