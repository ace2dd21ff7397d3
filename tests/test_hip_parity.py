"""GPU parity tests: HipDensePrimalNormalSolver (through the C ABI of libpycllp_hip.so) against
  (1) the committed golden vectors produced by the reference's own CPU solver (ipo.py / hsd.c), tolerance 1e-8
      relative on primal AND dual objectives (BASELINE.json north_star);
  (2) the oracle restatement on the same seeded inputs (same algorithm: iteration counts must be identical and
      objectives agree to 1e-9);
  (3) size-independent properties at BASELINE.json's full batch size (65 536 x (m=32, n=64)).
They read like the reference's tests/test_vanderbei.py, test_simple.py, test_random.py, test_ldl.py.
"""
import numpy as np
import pytest
import torch

from conftest import golden, rel_err, status_cases, check_certificates
from pycllp_amd import problems
from pycllp_amd.lp import SparseMatrix, EqualityLP, StandardLP
from pycllp_amd.solvers import solver_registry

pytestmark = pytest.mark.gpu
OBJ_TOL = 1e-8


def solve_lp(lp, **opts):
    elp = lp.to_equality_form() if isinstance(lp, StandardLP) else lp
    solver = solver_registry["hip_dense_primal_normal"](**opts)
    elp.init(solver)
    status = elp.solve(solver)
    assert status is solver.status
    return elp, solver


def solve_arrays(A, b, c, **opts):
    return solve_lp(StandardLP(SparseMatrix(matrix=np.asarray(A)), b, c, 0.0), **opts)


def oracle_on(elp, auto=True, **opts):
    """The oracle on the LP's arrays; mirrors the plugins' default autoscale='auto' (flag 8 when some LP of the batch has
    max|b| or max|c| outside [0.1, 10]) so that it runs the arithmetic lp.solve(solver) runs."""
    from oracle import port
    from pycllp_amd.solvers.hip import autoscale_wanted
    if auto and autoscale_wanted(elp.b, elp.c):
        opts["flags"] = int(opts.get("flags", 0)) | 8
    return port.dense_solve(elp.A.todense(), elp.b, elp.c, nthreads=8, **opts)


# ---- textbook problems (reference tests/test_vanderbei.py, tests/test_simple.py) ----------------------

def test_vanderbei_2_9():
    g = golden("vanderbei.npz")
    lp, xopt = problems.vanderbei_2_9()
    elp, s = solve_lp(lp)
    np.testing.assert_equal(s.status, 0)
    np.testing.assert_allclose(s.x[0, :lp.ncols], xopt, rtol=1e-6, atol=1e-6)
    assert rel_err(s.primal_obj, g["v29_pobj"]).max() < OBJ_TOL and rel_err(s.dual_obj, g["v29_dobj"]).max() < OBJ_TOL
    assert s.x.shape == (1, 6) and s.status.shape == (1,)


def test_vanderbei_2_10_equality_lp():
    lp, xopt = problems.vanderbei_2_10()
    elp, s = solve_lp(lp)
    np.testing.assert_equal(s.status, 0)
    np.testing.assert_allclose(s.x[0], xopt, rtol=1e-6, atol=1e-6)
    assert abs(s.primal_obj[0] - 9.0) < 1e-7 and abs(s.dual_obj[0] - 9.0) < 1e-7


def test_small_problem_and_parallel_perturbations():
    g = golden("small_problem.npz")
    elp, s = solve_arrays(g["A"], g["b"], g["c"])
    np.testing.assert_equal(s.status, 0)
    np.testing.assert_allclose(s.x[0, :3], (1.00997e-13, 1.22527e-12, 5.18790e+00), rtol=1e-1, atol=1e-1)
    # 32 perturbed copies: batched result vs the CPU solver per problem (tests/test_simple.py:70-93)
    elp, s = solve_arrays(g["A"], g["bb"], g["cc"])
    r = oracle_on(elp)
    np.testing.assert_array_equal(s.status, r["status"])
    np.testing.assert_allclose(s.x, r["x"], rtol=1e-3, atol=1e-3)
    np.testing.assert_allclose(s.x[:, :3], g["x"], rtol=1e-3, atol=1e-3)
    assert rel_err(s.primal_obj, g["pobj"]).max() < OBJ_TOL and rel_err(s.dual_obj, g["dobj"]).max() < OBJ_TOL


@pytest.mark.parametrize("shape", ["10x10", "20x20"])
def test_helpers_random_problems(shape):
    g = golden("random_helpers.npz")   # inputs of tests/test_random.py:14-17; HSD stands in for the absent GLPK
    k = "r%s_" % shape
    elp, s = solve_arrays(g[k + "A"], g[k + "b"], g[k + "c"])
    assert np.all(s.status == 0)
    ind = np.where(np.abs(elp.c[0]) > 0.0)[0]                   # non-slack variables, tests/helpers.py:100-102
    np.testing.assert_allclose(s.x[0, ind], g[k + "x"][0], rtol=1e-3, atol=1e-3)
    assert rel_err(s.primal_obj, g[k + "pobj"]).max() < OBJ_TOL and rel_err(s.dual_obj, g[k + "dobj"]).max() < OBJ_TOL


# ---- BASELINE configs against goldens and the oracle --------------------------------------------------

@pytest.mark.parametrize("m,n", [(16, 32), (32, 64)])
def test_baseline_config_golden_and_oracle_parity(m, n):
    g = golden("config_%dx%d.npz" % (m, n))
    nobj = int(g["nobj"])
    A, b, c = problems.random_dense_arrays(m, n, nobj, seed=int(g["seed"]))
    elp, s = solve_arrays(A, b, c)
    assert (s.status == 0).all()
    assert rel_err(s.primal_obj, g["pobj"]).max() < OBJ_TOL
    assert rel_err(s.dual_obj, g["dobj"]).max() < OBJ_TOL
    nf = g["x"].shape[0]
    np.testing.assert_allclose(s.x[:nf, :n], g["x"], rtol=1e-5, atol=1e-6)
    np.testing.assert_allclose(s.y[:nf], g["y"], rtol=1e-5, atol=1e-6)
    r = oracle_on(elp)
    np.testing.assert_array_equal(s.status, r["status"])
    np.testing.assert_array_equal(s.iters, r["iters"])          # same algorithm, same path
    assert rel_err(s.primal_obj, r["pobj"]).max() < 1e-9 and rel_err(s.dual_obj, r["dobj"]).max() < 1e-9
    # iterates of (near-)degenerate LPs amplify summation-order differences: looser than the objectives
    np.testing.assert_allclose(s.x, r["x"], rtol=1e-5, atol=1e-6)
    np.testing.assert_allclose(s.z, r["z"], rtol=1e-5, atol=1e-6)


def test_full_size_batch_properties():
    """65 536 x (32, 64): the oracle cannot run this in seconds, so check what must hold for any size."""
    m, n, B = 32, 64, 65536
    A, b, c = problems.random_dense_arrays(m, n, B, seed=0)
    elp, s = solve_arrays(A, b, c)
    assert (s.status == 0).all() and s.iters.max() < 60
    # optimality certificate: primal/dual feasibility and zero gap
    Ae = elp.A.todense()
    assert np.abs(s.x @ Ae.T - elp.b).max() < 1e-8
    assert (s.x > -1e-12).all() and (s.z > -1e-12).all()
    assert np.abs(s.y @ Ae - s.z - elp.c).max() < 1e-8
    assert rel_err(s.primal_obj, s.dual_obj).max() < 1e-8
    np.testing.assert_allclose(s.primal_obj, np.einsum("ij,ij->i", elp.c, s.x), rtol=1e-12)
    # first 4096 are the golden LPs (the stream depends on B, so compare through a re-generated prefix)
    g = golden("config_32x64.npz")
    A2, b2, c2 = problems.random_dense_arrays(m, n, int(g["nobj"]), seed=0)
    np.testing.assert_array_equal(A, A2)
    # batch-order independence: a permuted batch gives the permuted result bit for bit
    perm = np.random.RandomState(1).permutation(B)
    elp_p, sp = solve_arrays(A, b[perm], c[perm])
    np.testing.assert_array_equal(sp.x, s.x[perm])
    np.testing.assert_array_equal(sp.iters, s.iters[perm])
    # scaling: (alpha c, beta b) has objective alpha*beta*obj
    sub = slice(0, 2048)
    _, s2 = solve_arrays(A, 2.0 * b[sub], 0.5 * c[sub])
    assert (s2.status == 0).all()
    assert rel_err(s2.primal_obj, s.primal_obj[sub]).max() < 1e-8


def test_repeat_solve_with_mutated_b_c():
    """init once, solve many (README 'repeat solve'; A captured at init, cl.py:39,46)."""
    g = golden("config_16x32.npz")
    A, b, c = problems.random_dense_arrays(16, 32, int(g["nobj"]), seed=0)
    lp = StandardLP(SparseMatrix(matrix=A), b[:256], c[:256], 0.0).to_equality_form()
    s = solver_registry["hip_dense_primal_normal"]()
    lp.init(s)
    lp.solve(s)
    first = s.primal_obj.copy()
    assert rel_err(first, g["pobj"][:256]).max() < OBJ_TOL
    lp.b[:] = b[256:512]
    lp.c[:, :32] = c[256:512]
    lp.solve(s)
    assert rel_err(s.primal_obj, g["pobj"][256:512]).max() < OBJ_TOL
    lp.b[:] = b[:256]
    lp.c[:, :32] = c[:256]
    lp.solve(s)
    np.testing.assert_array_equal(s.primal_obj, first)           # deterministic


# ---- Newton step (reference tests/test_ldl.py:196-273) ------------------------------------------------

@pytest.mark.parametrize("key", ["t16x32_", "t32x64_", "t20x30_"])
def test_newton_step_known_answer(key):
    g = golden("newton_states.npz")
    A = g[key + "A"]
    lp = EqualityLP(SparseMatrix(matrix=A), g[key + "b"], g[key + "c"], 0.0)
    s = solver_registry["hip_dense_primal_normal"](pivot_floor=0.0)
    lp.init(s)
    dy = s.newton_step(g[key + "x"], g[key + "z"], g[key + "y"], g[key + "b"], g[key + "c"], float(g[key + "mu"]))
    np.testing.assert_allclose(dy, g[key + "dy"], rtol=1e-7, atol=1e-9)
    from oracle import port
    for i in range(0, dy.shape[0], 7):
        ref = port.solve_primal_normal(A, g[key + "x"][i], g[key + "z"][i], g[key + "y"][i], g[key + "b"][i],
                                       g[key + "c"][i], float(g[key + "mu"]), pivot_floor=0.0)
        np.testing.assert_allclose(dy[i], ref, rtol=1e-9, atol=1e-12)


def test_newton_step_trajectory_states():
    from test_oracle import TRAJ_RTOL
    g = golden("newton_states.npz")
    lp = EqualityLP(SparseMatrix(matrix=g["traj_A"]), g["traj_b"], g["traj_c"], 0.0)
    s = solver_registry["hip_dense_primal_normal"]()
    lp.init(s)
    for i in range(g["traj_x"].shape[0]):   # mu differs per state: one launch each
        dy = s.newton_step(g["traj_x"][i], g["traj_z"][i], g["traj_y"][i], g["traj_b"][i], g["traj_c"][i],
                           float(g["traj_mu"][i]))[0]
        ref = g["traj_dy"][i]
        assert np.abs(dy - ref).max() <= TRAJ_RTOL[i % 4] * np.abs(ref).max()


# ---- edge cases -----------------------------------------------------------------------------------------

@pytest.mark.parametrize("B", [1, 2, 63, 511, 4097])
def test_ragged_batch_sizes(B):
    A, b, c = problems.random_dense_arrays(12, 20, B, seed=3)
    elp, s = solve_arrays(A, b, c)
    r = oracle_on(elp)
    np.testing.assert_array_equal(s.status, r["status"])
    np.testing.assert_array_equal(s.iters, r["iters"])
    assert rel_err(s.primal_obj, r["pobj"]).max() < 1e-9


def test_host_pipeline_equals_device_resident_solve():
    """lp.solve() on numpy inputs runs the chunked upload/solve/download pipeline; it must give exactly what one
    device-resident launch over the whole batch gives, and a second solve must reuse the buffers correctly."""
    A, b, c = problems.random_dense_arrays(12, 20, 20011, seed=5)     # 2 ragged chunks
    elp, s = solve_arrays(A, b, c)
    assert isinstance(s.x, np.ndarray) and s.x.shape == (20011, 32)
    host = {k: np.array(getattr(s, k)) for k in ("x", "y", "z", "primal_obj", "dual_obj", "status", "iters")}
    buf = s.solve_device(elp.b, elp.c, slot=1)
    torch.cuda.synchronize()
    for k, kb in (("x", "x"), ("y", "y"), ("z", "z"), ("primal_obj", "pobj"), ("dual_obj", "dobj"),
                  ("status", "status"), ("iters", "iters")):
        np.testing.assert_array_equal(host[k], buf[kb].cpu().numpy(), err_msg=k)
    b0 = elp.b
    elp.b = b0 * 1.5
    elp.solve(s)
    assert not np.array_equal(s.primal_obj, host["primal_obj"])
    elp.b = b0
    elp.solve(s)
    np.testing.assert_array_equal(s.x, host["x"])


def test_concurrent_solves_on_two_streams_share_one_handle():
    """The C ABI is re-entrant per handle: two solves in flight on different streams (each with its own work-queue
    counter and its own output buffers) must both give what a lone solve gives."""
    A, b, c = problems.random_dense_arrays(16, 32, 6000, seed=21)
    elp, s = solve_arrays(A, b, c)
    ref = np.array(s.primal_obj)
    bd = torch.as_tensor(elp.b, device="cuda"); cd = torch.as_tensor(elp.c, device="cuda")
    s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
    outs = []
    for rep in range(4):
        for k, st in enumerate((s1, s2)):
            s.stream = st
            half = slice(0, 3000) if k == 0 else slice(3000, 6000)
            st.wait_stream(torch.cuda.current_stream())
            outs.append((half, s.solve_device(bd[half], cd[half], slot=10 + 2 * rep + k)))
    torch.cuda.synchronize()
    s.stream = None
    for half, buf in outs:
        np.testing.assert_array_equal(buf["pobj"].cpu().numpy(), ref[half])
        assert int((buf["status"] != 0).sum()) == 0


def test_reserve_cus_leaves_compute_units_idle_and_changes_nothing_else():
    A, b, c = problems.random_dense_arrays(32, 64, 8192, seed=2)
    elp, s0 = solve_arrays(A, b, c)
    g0 = s0.launch_info()["grid"]
    elp2, s8 = solve_arrays(A, b, c, reserve_cus=8)
    assert s8.launch_info()["grid"] == g0 - 8
    np.testing.assert_array_equal(s8.primal_obj, s0.primal_obj)
    np.testing.assert_array_equal(s8.iters, s0.iters)


def test_empty_batch():
    A = np.random.RandomState(0).rand(4, 6)
    lp = StandardLP(SparseMatrix(matrix=A), np.zeros((0, 4)), np.zeros((0, 6)), np.zeros(0)).to_equality_form()
    s = solver_registry["hip_dense_primal_normal"]()
    lp.init(s)
    st = lp.solve(s)
    assert st.shape == (0,) and s.x.shape == (0, 10)


@pytest.mark.parametrize("m,n", [(1, 1), (3, 2), (16, 16), (17, 40), (32, 96), (5, 123)])
def test_shapes_up_to_the_maximum(m, n):
    """(m, n) of the StandardLP; the solver sees n+m columns, up to 32 x 128."""
    A, b, c = problems.random_dense_arrays(m, n, 96, seed=11)
    elp, s = solve_arrays(A, b, c)
    assert elp.ncols == n + m <= 128
    r = oracle_on(elp)
    np.testing.assert_array_equal(s.status, r["status"])
    assert (s.status == 0).all()
    assert rel_err(s.primal_obj, r["pobj"]).max() < 1e-9 and rel_err(s.dual_obj, r["dobj"]).max() < 1e-9


def test_unsupported_size_raises():
    """Round 3: the cap moved from (128, 512) to m = 256 rows, 1280 columns of the equality form (csrc/ipm_big.hip)."""
    A, b, c = problems.random_dense_arrays(257, 20, 2, seed=0)
    lp = StandardLP(SparseMatrix(matrix=A), b, c, 0.0).to_equality_form()
    with pytest.raises(NotImplementedError):
        lp.init(solver_registry["hip_dense_primal_normal"]())
    A, b, c = problems.random_dense_arrays(8, 1274, 2, seed=0)
    lp = StandardLP(SparseMatrix(matrix=A), b, c, 0.0).to_equality_form()
    with pytest.raises(NotImplementedError):
        lp.init(solver_registry["hip_dense_primal_normal"]())


@pytest.mark.parametrize("case", ["dense 200x200", "dense 129x40", "dense 60x700", "dense 256x300", "sparse 256x512 d0.02",
                                  "sparse 150x900 d0.03", "sparse 256x1024 d0.01", "equality 140x300 signed"])
@pytest.mark.parametrize("hsd", [False, True])
def test_large_lps_on_the_workgroup_per_lp_kernel(case, hsd):
    """the reference's hosts take any (m, n) (pycllp/solvers/cl.py:28-83, 127-278;
    examples/random_problem.py:30-49).  Beyond m = 128 / n = 512 both plugins run csrc/ipm_big.hip (one LP per workgroup,
    the factor as 16 x 16 blocks in LDS or an L2-resident workspace, Gram on the matrix cores for a dense A, from a term list
    for a sparse one).  Against the oracle LP by LP: same status, iterations within 1, objectives to 1e-9."""
    kind, shape = case.split()[0], case.split()[1]
    m, n = [int(v) for v in shape.split("x")]
    B = 12
    rs = np.random.RandomState(m + n)
    if kind == "dense":
        A, b, c = problems.random_dense_arrays(m, n, B, seed=m)
        lp = StandardLP(SparseMatrix(matrix=A), b, c, 0.0).to_equality_form()
        name, variant = "hip_dense_primal_normal", "MFMA Gram"
    elif kind == "sparse":
        dens = float(case.split()[2][1:])
        A, b, c = problems.random_sparse_arrays(m, n, B, density=dens, seed=m)
        lp = StandardLP(SparseMatrix(matrix=A), b, c, 0.0).to_equality_form()
        name, variant = "hip_sparse_primal_normal", "term list"
    else:
        A = rs.randn(m, n) * (rs.rand(m, n) < 0.5)
        x0 = rs.rand(B, n) + 0.1; y0 = rs.randn(B, m)
        b = x0 @ A.T; c = y0 @ A - (rs.rand(B, n) + 0.1)          # strictly feasible primal-dual pair, no identity columns
        lp = EqualityLP(SparseMatrix(matrix=A), b, c, 0.0)
        name, variant = "hip_dense_primal_normal", None       # (half-dense: either Gram path may be the cheaper one)
    s = solver_registry[name](hsd=hsd)
    lp.init(s)
    st = lp.solve(s)
    info = s.launch_info()
    assert info["kernel"] == "big" and variant in (None, info["variant"]), info
    r = oracle_on(lp, flags=32 if hsd else 0)
    np.testing.assert_array_equal(st, r["status"])
    assert (st == 0).all() and np.abs(s.iters.astype(int) - r["iters"]).max() <= 1
    from pycllp_amd.solvers.hip import autoscale_wanted
    tol = 1e-8 if autoscale_wanted(lp.b, lp.c) else 1e-9
    assert rel_err(s.primal_obj, r["pobj"]).max() < tol and rel_err(s.dual_obj, r["dobj"]).max() < tol
    np.testing.assert_allclose(s.x, r["x"], rtol=1e-5, atol=1e-6)
    # the optimality conditions themselves, from the returned vectors
    Ae = np.asarray(lp.A.todense())
    assert (np.linalg.norm(lp.b - s.x @ Ae.T, axis=1) / (1 + np.linalg.norm(lp.b, axis=1))).max() < 1e-8
    assert (np.linalg.norm(lp.c - s.y @ Ae + s.z, axis=1) / (1 + np.linalg.norm(lp.c, axis=1))).max() < 1e-8
    assert s.x.min() >= 0 and s.z.min() >= 0


@pytest.mark.parametrize("hsd", [False, True])
def test_large_lp_guarded_cold_path(hsd):
    """The large-LP kernel's blocked factorisation only RECORDS whether the Nocedal-Wright guard (ldl.cl:368) would have
    bitten; when it would, M is re-formed and a column-by-column cold path applies the guard exactly (found by
    tests/dev/fuzz_r3.py: an HSD solve at m = 154 used to end with status 3 where the oracle, whose factorisation applies the
    guard, ends optimal).  PYCLLP_FLAG_FORCE_GUARD_PATH runs that path on every iteration: where the guard is inactive the
    results must not change."""
    A, b, c = problems.random_dense_arrays(150, 60, 6, seed=5)
    lp = StandardLP(SparseMatrix(matrix=A), b, c, 0.0).to_equality_form()
    s = solver_registry["hip_dense_primal_normal"](hsd=hsd, flags=4)
    lp.init(s)
    st = lp.solve(s)
    assert s.launch_info()["kernel"] == "big"
    r = oracle_on(lp, flags=32 if hsd else 0)
    np.testing.assert_array_equal(st, r["status"])
    assert (st == 0).all() and np.abs(s.iters.astype(int) - r["iters"]).max() <= 1
    assert rel_err(s.primal_obj, r["pobj"]).max() < 1e-9 and rel_err(s.dual_obj, r["dobj"]).max() < 1e-9
    # the fuzz case itself (seed 1, case 15: dense 154 x 676, two LPs): the guard bites on one of them under HSD
    if hsd:
        import os, sys
        sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "dev"))
        from fuzz_cases import big_cases
        case = [cs for cs in big_cases(1, 16)][15]
        assert case[:2] == (154, 676) and case[4]
        A2, b2, c2 = case[6], case[7], case[8]
        lp2 = StandardLP(SparseMatrix(matrix=A2), b2, c2, 0.0).to_equality_form()
        s2 = solver_registry["hip_dense_primal_normal"](hsd=True)
        lp2.init(s2)
        st2 = lp2.solve(s2)
        r2 = oracle_on(lp2, flags=32)
        np.testing.assert_array_equal(st2, r2["status"])
        assert rel_err(s2.primal_obj, r2["pobj"]).max() < 1e-8


def test_large_lp_golden_objectives():
    """tests/golden/config_dense_200x200.npz: objectives of the reference's hsd.c on 16 dense LPs of a shape only the
    large-LP kernel covers (SURVEY 8d generator, tools/gen_golden.py large_lp_config); default plugin, 1e-8."""
    g = golden("config_dense_200x200.npz")
    A, b, c = problems.random_dense_arrays(200, 200, int(g["nobj"]), seed=0)
    assert np.allclose(g["input_checksum"], [A.sum(), b.sum(), c.sum()], rtol=1e-12)
    elp, s = solve_arrays(A, b, c)
    assert s.launch_info()["kernel"] == "big" and (s.status == 0).all()
    assert rel_err(s.primal_obj, g["pobj"]).max() < OBJ_TOL and rel_err(s.dual_obj, g["dobj"]).max() < OBJ_TOL
    np.testing.assert_allclose(s.x[:8, :200], g["x"], rtol=1e-4, atol=1e-6)


def test_large_lp_newton_step_and_statuses():
    """The stand-alone Newton step (ldl.cl:602-653 / 656-712) and the verdicts of the embedding at a size only the large-LP
    kernel covers: dy against the known-answer formula of the reference's tests/test_ldl.py:196-216; an infeasible and an
    unbounded LP (m = 160) end with the true status and a Farkas certificate under the default hsd='auto'."""
    from oracle import port
    m, n, nb = 160, 100, 6
    rs = np.random.RandomState(123456)
    A = np.c_[rs.rand(m, n), np.eye(m)]
    x = rs.rand(nb, m + n) + 0.05; z = rs.rand(nb, m + n) + 0.05
    y = rs.rand(nb, m); b = rs.rand(nb, m)
    c = np.c_[rs.rand(nb, n), np.zeros((nb, m))]
    lp = EqualityLP(SparseMatrix(matrix=A), b, c, 0.0)
    s = solver_registry["hip_dense_primal_normal"]()
    lp.init(s)
    dy = s.newton_step(x, z, y, b, c, 1.0)
    for i in range(nb):
        ref = port.newton_step_known_answer(A, x[i], z[i], y[i], b[i], c[i], 1.0)
        np.testing.assert_allclose(dy[i], ref, rtol=1e-5, atol=1e-5)
    # infeasible: x_0 + ... <= -1 among ordinary rows; unbounded: a column that no row bounds
    As = rs.rand(m, 60)
    bs = 0.5 + rs.rand(4, m); cs = 0.5 + rs.rand(4, 60)
    bs[1, 7] = -1.0                                   # LP 1: row 7 reads a'x <= -1 with a > 0, x >= 0: infeasible
    As2 = As.copy(); As2[:, 5] = 0.0                  # column 5 unbounded above with c_5 > 0 -> every LP unbounded
    lp1 = StandardLP(SparseMatrix(matrix=As), bs, cs, 0.0).to_equality_form()
    d = solver_registry["hip_dense_primal_normal"]()
    lp1.init(d)
    st = lp1.solve(d)
    assert d.launch_info()["kernel"] == "big"
    assert list(st) == [0, 2, 0, 0]
    check_certificates(np.asarray(lp1.A.todense()), lp1.b, lp1.c, dict(status=d.status, x=d.x, y=d.y, z=d.z))
    As2[0, 5] = 1e-300                                # (keeps the column in the structure)
    lp2 = StandardLP(SparseMatrix(matrix=As2), bs[:1], cs[:1], 0.0).to_equality_form()
    d2 = solver_registry["hip_dense_primal_normal"]()
    lp2.init(d2)
    assert list(lp2.solve(d2)) == [4]
    check_certificates(np.asarray(lp2.A.todense()), lp2.b, lp2.c, dict(status=d2.status, x=d2.x, y=d2.y, z=d2.z))


@pytest.mark.parametrize("m,n,B", [(100, 80, 24), (33, 20, 40), (8, 200, 40), (128, 256, 12)])
def test_dense_solver_beyond_the_lane_group_kernels(m, n, B):
    """The reference's dense host has no size cap (pycllp/solvers/cl.py:28-83): beyond m = 32 / N = 128 the dense plugin
    hands the LP to the kernels of the sparse path (up to m = 128, N = 512).  Parity against the oracle as everywhere."""
    A, b, c = problems.random_dense_arrays(m, n, B, seed=m + n)
    elp, s = solve_arrays(A, b, c)
    r = oracle_on(elp)
    np.testing.assert_array_equal(s.status, r["status"])
    assert (s.status == 0).all()
    assert np.abs(s.iters.astype(int) - r["iters"]).max() <= 1
    assert rel_err(s.primal_obj, r["pobj"]).max() < 1e-9 and rel_err(s.dual_obj, r["dobj"]).max() < 1e-9
    np.testing.assert_allclose(s.x, r["x"], rtol=1e-5, atol=1e-6)
    elp2, s2 = solve_arrays(A, b, c, hsd=True)
    assert (s2.status == 0).all() and rel_err(s2.primal_obj, r["pobj"]).max() < 1e-8


def test_dense_newton_step_reference_recipe():
    """The reference's own test of its stand-alone kernel solve_primal_normal (tests/test_ldl.py:219-273: seed 123456,
    m = 100, n = 80 dense (+100 slack), 32 systems, mu = 1) through the DENSE plugin, against the known-answer formula of
    tests/test_ldl.py:196-216 at the reference's tolerance (rtol 1e-5)."""
    from oracle import port
    m, n, cl_size = 100, 80, 32
    np.random.seed(123456)
    A = np.c_[np.random.rand(m, n), np.eye(m)]
    x = np.random.rand(m + n, cl_size); z = np.random.rand(m + n, cl_size)
    y = np.random.rand(m, cl_size); b = np.random.rand(m, cl_size)
    c = np.r_[np.random.rand(n, cl_size), np.zeros((m, cl_size))]
    lp = EqualityLP(SparseMatrix(matrix=A), b.T[:1], c.T[:1], 0.0)
    s = solver_registry["hip_dense_primal_normal"]()
    lp.init(s)
    dy = s.newton_step(x.T, z.T, y.T, b.T, c.T, 1.0)
    for i in range(cl_size):
        ref = port.newton_step_known_answer(A, x[:, i], z[:, i], y[:, i], b[:, i], c[:, i], 1.0)
        np.testing.assert_allclose(dy[i], ref, rtol=1e-5, atol=1e-5)


def test_infeasible_and_unbounded_lps_reference_path_and_default():
    """Two 1 x 2 LPs, one infeasible, one unbounded.
    (a) hsd=False, the reference's path (10x-growth heuristic, primal_normal.cl:261-269): kernel and oracle walk the SAME
    trajectory -- x, y, z after k iterations agree to 1e-12 relative for every k (measured 5e-15 over 59 iterations,
    tests/dev/dbg_diverge.py) -- and give the same verdict.  The iteration AT WHICH the heuristic fires is not comparable:
    it is tripped by a 10x bump of |sigma| = |c - A'y + z|, which on these diverging iterates (|y|, |z| ~ 1e7..1e8, x -> 0)
    is pure cancellation noise of size eps |y|; the kernel carries A'y incrementally, the oracle recomputes it, so the two
    noises differ and the exits fall 10-40 iterations apart (kernel 96 vs oracle 136 here).
    (b) the default hsd='auto' re-solves what did not end optimal on the homogeneous self-dual embedding: true verdicts
    (2 = primal infeasible, 4 = unbounded) with verified Farkas certificates."""
    from oracle import port
    cases = [
        (np.array([[1.0, 1.0]]), np.array([[-1.0]]), np.array([[1.0, 1.0]]), 2),     # primal infeasible
        (np.array([[1.0, -1.0]]), np.array([[0.0]]), np.array([[1.0, 0.0]]), 4),     # unbounded
    ]
    for A, b, c, truth in cases:
        lp = EqualityLP(SparseMatrix(matrix=A), b, c, 0.0)
        s = solver_registry["hip_dense_primal_normal"](hsd=False)
        lp.init(s)
        st = lp.solve(s)
        r = port.dense_solve(A, b, c)
        assert st[0] != 0 and st[0] == r["status"][0]
        rel = lambda a, ref: np.abs(a - ref).max() / np.abs(ref).max()
        for k in (5, 20, 35):
            g = s.solve_device(b, c, max_iter=k); torch.cuda.synchronize()
            rk = port.dense_solve(A, b, c, max_iter=k)
            assert int(g["iters"][0]) == k == rk["iters"][0]
            for f in ("x", "y", "z"):
                assert rel(g[f].cpu().numpy()[0], rk[f][0]) < 1e-12, (k, f)
        d = solver_registry["hip_dense_primal_normal"]()          # default: hsd='auto'
        lp.init(d)
        assert lp.solve(d)[0] == truth
        check_certificates(A, b, c, dict(status=d.status, x=d.x, y=d.y, z=d.z))


def test_default_solver_gives_true_verdicts_on_a_mixed_batch():
    """hsd='auto' (default) on the mixed-sign fixture: optimal LPs keep the reference path's result (same iterations as
    the oracle's plain path), every other LP ends with the true status (HiGHS / reference hsd.c) and a valid certificate."""
    for A, b, c, ref_status, highs, ref_pobj in status_cases()[:4]:
        elp, s = solve_arrays(A, b, c)
        np.testing.assert_array_equal(s.status, highs)
        r = oracle_on(elp)
        opt = (highs == 0) & (r["status"] == 0)
        if opt.any():
            np.testing.assert_array_equal(s.iters[opt], r["iters"][opt])
            assert rel_err(s.primal_obj[opt], r["pobj"][opt]).max() < 1e-9
        check_certificates(elp.A.todense(), elp.b, elp.c, dict(status=s.status, x=s.x, y=s.y, z=s.z))


def test_all_status_zero_lps_satisfy_the_true_primal_residual():
    """The finishing verdict of the dense kernel is taken on rho = b - A x recomputed from x, not on the recurrence that
    predicts it: for every LP reported optimal |b - A x| <= eps (1 + |b|) holds for the x that is returned."""
    rs = np.random.RandomState(11)
    for m, n, B in ((6, 14, 300), (20, 60, 200), (32, 64, 256)):
        A = rs.randn(m, n)
        x0 = rs.rand(B, n) * (rs.rand(B, n) < 0.5) * 10.0 ** rs.uniform(-2, 4, size=(B, 1))
        b = x0 @ A.T
        c = -rs.rand(B, n) - 0.1
        lp = EqualityLP(SparseMatrix(matrix=A), b, c, 0.0)
        s = solver_registry["hip_dense_primal_normal"](hsd=False, autoscale=False)    # the reference path's own tolerances
        lp.init(s); lp.solve(s)
        ok = s.status == 0
        assert ok.sum() > B // 2
        res = np.linalg.norm(b - s.x @ A.T, axis=1)
        assert (res[ok] <= 1.0001e-10 * (1.0 + np.linalg.norm(b, axis=1))[ok] + 1e-13 * np.abs(s.x[ok]).max(axis=1)).all()


def test_objective_offset_and_options():
    A, b, c = problems.random_dense_arrays(8, 12, 16, seed=2)
    lp = StandardLP(SparseMatrix(matrix=A), b, c, 3.5).to_equality_form()
    s = solver_registry["hip_dense_primal_normal"](eps=1e-6, max_iter=50)
    lp.init(s)
    lp.solve(s)
    r = oracle_on(lp, eps=1e-6, max_iter=50)
    np.testing.assert_array_equal(s.iters, r["iters"])
    np.testing.assert_allclose(s.primal_obj, r["pobj"] + 3.5, rtol=1e-9)
    s2 = solver_registry["hip_dense_primal_normal"](max_iter=3, hsd=False)
    lp.init(s2)
    assert (lp.solve(s2) == 5).all() and (s2.iters == 3).all()           # iteration limit


def test_warm_start_from_previous_solution():
    """Intent of primal_normal.cl:213-219: a second solve may start where the first ended."""
    A, b, c = problems.random_dense_arrays(16, 32, 512, seed=4)
    Ae, be, ce = problems.equality_arrays(A, b, c)
    lp = EqualityLP(SparseMatrix(matrix=Ae), be, ce, 0.0)
    s = solver_registry["hip_dense_primal_normal"]()
    lp.init(s)
    buf = s.solve_device(be, ce, eps=1e-4)
    torch.cuda.synchronize()
    cold_it = buf["iters"].cpu().numpy().copy()
    x0, y0, z0 = buf["x"].cpu().numpy().copy(), buf["y"].cpu().numpy().copy(), buf["z"].cpu().numpy().copy()
    buf = s.solve_device(be, ce, warm_start=True)           # continue from the loose solution to full accuracy
    torch.cuda.synchronize()
    from oracle import port
    r = port.dense_solve(Ae, be, ce, nthreads=8, x0=x0, y0=y0, z0=z0, flags=1)
    np.testing.assert_array_equal(buf["iters"].cpu().numpy(), r["iters"])
    assert rel_err(buf["pobj"].cpu().numpy(), r["pobj"]).max() < 1e-9
    full = port.dense_solve(Ae, be, ce, nthreads=8)
    assert (buf["status"].cpu().numpy() == 0).all()
    assert rel_err(buf["pobj"].cpu().numpy(), full["pobj"]).max() < 1e-8
    assert (buf["iters"].cpu().numpy() + cold_it).mean() < full["iters"].mean() + 3


@pytest.mark.parametrize("name,m,n", [("hip_dense_primal_normal", 16, 32), ("hip_sparse_primal_normal", 40, 90)])
def test_repeat_solve_warm_start_through_the_plugin_api(name, m, n):
    """warm_start=True: lp.solve(solver) -- the reference's own calling convention, lp.py:531-535 -- starts every LP from the
    solution the previous solve() left on the device (README.md:5-6 'repeat solve', primal_normal.cl:213-219)."""
    from oracle import port
    rs = np.random.RandomState(3)
    if name.startswith("hip_dense"):
        A, b, c = problems.random_dense_arrays(m, n, 300, seed=6)
    else:
        A, b, c = problems.random_sparse_arrays(m, n, 300, density=0.1, seed=6)
    lp = StandardLP(SparseMatrix(matrix=A), b, c, 0.0).to_equality_form()
    cold = solver_registry[name]()
    lp.init(cold); lp.solve(cold)
    it_cold = cold.iters.copy()
    s = solver_registry[name](warm_start=True)
    lp.init(s)
    lp.solve(s)                                                  # first solve: cold by definition
    np.testing.assert_array_equal(s.iters, it_cold)
    x0, y0, z0 = s.x.copy(), s.y.copy(), s.z.copy()
    lp.b[:] = lp.b * (1.0 + 0.01 * rs.rand(*lp.b.shape))         # slowly varying data
    lp.c[:, :n] = lp.c[:, :n] * (1.0 + 0.01 * rs.rand(300, n))
    lp.solve(s)
    from pycllp_amd.solvers.hip import warm_lifted
    r = port.dense_solve(lp.A.todense(), lp.b, lp.c, nthreads=8, x0=warm_lifted(x0), y0=y0, z0=warm_lifted(z0), flags=1)
    full = port.dense_solve(lp.A.todense(), lp.b, lp.c, nthreads=8)
    assert (s.status == 0).all() and (r["status"] == 0).all()
    # Round 3 (profiles/r03/warm_start_band.txt, tests/dev/warm_band.py, warm_outlier.py): the RAW previous optimum sits on the
    # boundary (x z ~ 1e-10); restarted from there kernel and oracle trajectories separate ~30x per iteration (2e-15 after
    # one iteration, 4e-10 after eight), 2-4 % of the LPs stop more than one iteration apart, and about one LP in 300 JAMS
    # (steps collapse, the growth heuristic ends it with status 2 after 55 iterations).  warm_start=True therefore lifts the
    # start into the interior (warm_lift = 1e-3, HipDensePrimalNormalSolver.__init__): no jam, 10 instead of 12-18
    # iterations on average, at most 19 -- and a well-conditioned restart, on which kernel and oracle agree like on a cold one.
    diff = np.abs(s.iters.astype(int) - r["iters"])
    assert (diff <= 1).mean() > 0.98 and diff.max() <= 3
    assert s.iters.max() <= 25
    # the raw restart (warm_lift=0) stays available and is what the C flag alone does; it needs more iterations
    raw = solver_registry[name](warm_start=True, warm_lift=0.0)
    lp0 = StandardLP(SparseMatrix(matrix=A), b, c, 0.0).to_equality_form()
    lp0.init(raw); lp0.solve(raw)
    lp0.b[:] = lp.b; lp0.c[:] = lp.c
    lp0.solve(raw)
    assert (raw.status == 0).all() and raw.iters.mean() > s.iters.mean()
    assert rel_err(raw.primal_obj, full["pobj"]).max() < 1e-8
    assert np.median(s.iters) < 0.7 * np.median(it_cold)
    assert rel_err(s.primal_obj, full["pobj"]).max() < 1e-8


@pytest.mark.parametrize("flags,what", [(4, "guarded (cold) LDL' path of the group kernel"),
                                        (16, "generic group kernel although A = [A | I]"), (16 + 4, "generic group kernel, guarded path")])
@pytest.mark.parametrize("m,n", [(16, 32), (32, 64), (7, 20)])
def test_alternative_kernel_paths_agree_with_oracle(flags, what, m, n):
    """PYCLLP_FLAG_FORCE_GUARD_PATH and PYCLLP_FLAG_NO_SLACK_PATH select code that the default launch (almost) never
    runs; it must give the oracle's answers too."""
    A, b, c = problems.random_dense_arrays(m, n, 1024, seed=9)
    elp, s = solve_arrays(A, b, c, flags=flags)
    r = oracle_on(elp)
    np.testing.assert_array_equal(s.status, r["status"])
    assert (s.status == 0).all()
    assert np.abs(s.iters.astype(int) - r["iters"]).max() <= 1 and (s.iters == r["iters"]).mean() > 0.99
    assert rel_err(s.primal_obj, r["pobj"]).max() < 1e-9 and rel_err(s.dual_obj, r["dobj"]).max() < 1e-9


# ---- Mehrotra predictor-corrector (PYCLLP_FLAG_PREDCORR) ---------------------------------------------

@pytest.mark.parametrize("m,n", [(16, 32), (32, 64)])
@pytest.mark.parametrize("extra", [0, 16, 8])
def test_predictor_corrector_on_baseline_configs(m, n, extra):
    """predcorr=True: one factorisation, two solves per iteration (oracle ipm_one_pc; the reference's CPU solver alternates
    predictor and centering iterations instead, ipo/hsd.c:133-143, 222-260).  Same optimum as the reference solver's
    goldens to 1e-8, LP by LP the oracle's iterations (+-1) and objectives (1e-9), ~27 % fewer iterations than the
    reference's rule at its own step fraction.  extra: 16 = generic (not slack-aware) kernel, 8 = autoscale."""
    g = golden("config_%dx%d.npz" % (m, n))
    A, b, c = problems.random_dense_arrays(m, n, int(g["nobj"]), seed=0)
    elp, s = solve_arrays(A, b, c, predcorr=True, hsd=False, flags=extra)
    assert (s.status == 0).all()
    assert rel_err(s.primal_obj, g["pobj"]).max() < OBJ_TOL and rel_err(s.dual_obj, g["dobj"]).max() < OBJ_TOL
    r = oracle_on(elp, auto=False, flags=128 | (extra & 8))
    np.testing.assert_array_equal(s.status, r["status"])
    assert np.abs(s.iters.astype(int) - r["iters"]).max() <= 1 and (s.iters == r["iters"]).mean() > 0.98
    assert rel_err(s.primal_obj, r["pobj"]).max() < 1e-9 and rel_err(s.dual_obj, r["dobj"]).max() < 1e-9
    plain = oracle_on(elp, auto=False, flags=extra & 8)
    assert s.iters.mean() < 0.8 * plain["iters"].mean()
    if extra == 0:      # a longer step fraction pays more with the corrector: r = 0.99
        elp, s2 = solve_arrays(A[:, :], b[:512], c[:512], predcorr=True, hsd=False, r=0.99)
        assert (s2.status == 0).all() and s2.iters.mean() < 0.6 * plain["iters"].mean()
        assert rel_err(s2.primal_obj, g["pobj"][:512]).max() < OBJ_TOL


def test_predictor_corrector_options_and_large_lps():
    """The option through the default plugin (hsd='auto': what does not end optimal is re-solved on the embedding), on the
    large-LP kernel, and where it is refused: with hsd=True."""
    for A, b, c, ref_status, highs, ref_pobj in status_cases()[:3]:
        elp, s = solve_arrays(A, b, c, predcorr=True)
        np.testing.assert_array_equal(s.status, highs)
        check_certificates(elp.A.todense(), elp.b, elp.c, dict(status=s.status, x=s.x, y=s.y, z=s.z))
    with pytest.raises(ValueError):
        solver_registry["hip_dense_primal_normal"](predcorr=True, hsd=True)
    A, b, c = problems.random_dense_arrays(150, 120, 10, seed=3)
    lp = StandardLP(SparseMatrix(matrix=A), b, c, 0.0).to_equality_form()
    s = solver_registry["hip_dense_primal_normal"](predcorr=True, hsd=False)
    lp.init(s)
    st = lp.solve(s)
    assert s.launch_info()["kernel"] == "big" and (st == 0).all()
    r = oracle_on(lp, flags=128)
    assert np.abs(s.iters.astype(int) - r["iters"]).max() <= 1
    assert rel_err(s.primal_obj, r["pobj"]).max() < 1e-9 and rel_err(s.dual_obj, r["dobj"]).max() < 1e-9
    assert s.iters.mean() < 0.8 * oracle_on(lp)["iters"].mean()


def test_predictor_corrector_on_the_sparse_path():
    """The same option on the wavefront-per-LP kernel: config 5's golden LPs (reference hsd.c) to 1e-8, the oracle's
    ipm_one_pc LP by LP, about half the iterations of the reference's rule on this structure (52.7 -> 25.5); a smaller
    sparse shape; the dense-image and per-problem-A variants; where no kernel with the option serves the LP it is refused."""
    g = golden("config_sparse_128x256.npz")
    import scipy.sparse as sp
    A = sp.csr_matrix((g["A_data"], g["A_indices"], g["A_indptr"]), shape=(128, 256))
    lp = StandardLP(SparseMatrix(matrix=A), g["b"], g["c"], 0.0).to_equality_form()
    s = solver_registry["hip_sparse_primal_normal"](predcorr=True, hsd=False)
    lp.init(s)
    st = lp.solve(s)
    assert s.launch_info()["kernel"] == "wave" and (st == 0).all()
    assert rel_err(s.primal_obj, g["pobj"]).max() < OBJ_TOL and rel_err(s.dual_obj, g["dobj"]).max() < OBJ_TOL
    r = oracle_on(lp, flags=128)
    assert np.abs(s.iters.astype(int) - r["iters"]).max() <= 1
    assert rel_err(s.primal_obj, r["pobj"]).max() < 1e-9 and rel_err(s.dual_obj, r["dobj"]).max() < 1e-9
    assert s.iters.mean() < 0.6 * oracle_on(lp)["iters"].mean()
    A2, b2, c2 = problems.random_sparse_arrays(40, 90, 64, density=0.1, seed=5)
    lp2 = StandardLP(SparseMatrix(matrix=A2), b2, c2, 0.0).to_equality_form()
    s2 = solver_registry["hip_sparse_primal_normal"](predcorr=True)          # default hsd='auto'
    lp2.init(s2)
    assert (lp2.solve(s2) == 0).all()
    r2 = oracle_on(lp2, flags=128)
    assert np.abs(s2.iters.astype(int) - r2["iters"]).max() <= 1 and rel_err(s2.primal_obj, r2["pobj"]).max() < 1e-9
    Ad, bd, cd = problems.random_dense_arrays(100, 80, 24, seed=1)            # dense-image variant of the wave kernel
    lpd = StandardLP(SparseMatrix(matrix=Ad), bd, cd, 0.0).to_equality_form()
    sd = solver_registry["hip_dense_primal_normal"](predcorr=True, hsd=False)
    lpd.init(sd)
    assert (lpd.solve(sd) == 0).all() and sd.launch_info()["variant"] == "dense image"
    rd = oracle_on(lpd, flags=128)
    assert np.abs(sd.iters.astype(int) - rd["iters"]).max() <= 1 and rel_err(sd.primal_obj, rd["pobj"]).max() < 1e-9
    # per-problem values of A: every LP against the oracle's ipm_one_pc with ITS OWN matrix
    from oracle import port
    rows, cols, data = problems.per_problem_values(A2, 8, seed=1)
    lpp = StandardLP(SparseMatrix(rows, cols, data), b2[:8], c2[:8], 0.0).to_equality_form()
    sp_ = solver_registry["hip_sparse_primal_normal"](predcorr=True, hsd=False)
    lpp.init(sp_)
    assert (lpp.solve(sp_) == 0).all() and sp_.launch_info()["kernel"] == "wave"
    for k in range(8):
        rk = port.dense_solve(lpp.A.todense(k), lpp.b[k:k + 1], lpp.c[k:k + 1], flags=128)
        assert abs(int(sp_.iters[k]) - int(rk["iters"][0])) <= 1 and rel_err(sp_.primal_obj[k], rk["pobj"][0]) < 1e-9
    # where no kernel with the option serves the LP (the block kernel, forced here) it is refused, not ignored
    from pycllp_amd import _native
    sb_ = solver_registry["hip_sparse_primal_normal"](predcorr=True, hsd=False, flags=_native.FLAG_BLOCK_KERNEL)
    lp2.init(sb_)
    with pytest.raises(NotImplementedError):
        lp2.solve(sb_)


# ---- homogeneous self-dual embedding (PYCLLP_FLAG_HSD) -----------------------------------------------------

def test_hsd_statuses_against_reference_highs_and_oracle():
    """Mixed-sign LPs, most of them infeasible or unbounded (tests/golden/status_cases.npz: statuses of the reference's
    hsd.c and of HiGHS): the HSD kernel must report the true status for every LP, agree with the oracle restatement
    LP by LP, match the reference's objectives on the optimal ones and return valid certificates."""
    for A, b, c, ref_status, highs, ref_pobj in status_cases():
        elp, s = solve_arrays(A, b, c, hsd=True)
        np.testing.assert_array_equal(s.status, highs)
        right = ref_status == highs
        np.testing.assert_array_equal(s.status[right], ref_status[right])
        r = oracle_on(elp, flags=32)
        np.testing.assert_array_equal(s.status, r["status"])
        assert np.abs(s.iters.astype(int) - r["iters"]).max() <= 1
        opt = highs == 0
        if opt.any():
            assert rel_err(s.primal_obj[opt], ref_pobj[opt]).max() < OBJ_TOL
            assert rel_err(s.primal_obj[opt], r["pobj"][opt]).max() < 1e-9
        check_certificates(elp.A.todense(), elp.b, elp.c, dict(status=s.status, x=s.x, y=s.y, z=s.z))


def test_hsd_slowly_collapsing_infeasible_lps_at_the_baseline_shape():
    """(32, 64) batch with mixed-sign A, b, c: ~94 % primal infeasible, some of them only after 30-50 iterations with x
    shrinking to 1e-13 (a kernel that carried rho = b tau - A x from step to step instead of recomputing it lost 0.4 %
    of these to the iteration limit).  Statuses and iteration counts must be the oracle's."""
    rs = np.random.RandomState(11)
    A = rs.rand(32, 64) * 2 - 0.3
    b = rs.rand(65536, 32) * 2 - 0.2; c = rs.rand(65536, 64) * 2 - 0.3
    pick = np.r_[0:1024, [270, 356, 394, 516, 839, 1006, 1187, 1312, 1588, 1806, 1976, 2166, 3502, 3587, 4136, 4540]]
    elp, s = solve_arrays(A, b[pick], c[pick], hsd=True)
    r = oracle_on(elp, flags=32)
    np.testing.assert_array_equal(s.status, r["status"])
    assert set(np.unique(s.status)) <= {0, 2} and (s.status == 2).mean() > 0.9
    assert np.abs(s.iters.astype(int) - r["iters"]).max() <= 1 and s.iters.max() < 80
    opt = s.status == 0
    assert rel_err(s.primal_obj[opt], r["pobj"][opt]).max() < 1e-9
    check_certificates(elp.A.todense(), elp.b, elp.c, dict(status=s.status, x=s.x, y=s.y, z=s.z))


@pytest.mark.parametrize("solver_name", ["hip_dense_primal_normal", "hip_sparse_primal_normal"])
@pytest.mark.parametrize("hsd", [False, True])
def test_rank_deficient_constraints(solver_name, hsd):
    """Duplicated constraint rows (with duplicated right-hand sides): the pivot floors -- absolute 1e-6 on the plain
    path, 1e-12 of each pivot's own diagonal on the HSD path -- must catch the numerically-zero pivots.  Checked against
    the oracle and, as absolute truth, against HiGHS (the reference's hsd.c is off by up to 40 % on these LPs)."""
    from scipy.optimize import linprog
    rs = np.random.RandomState(3)
    A = rs.rand(6, 14); A = np.vstack([A, A[:3]])
    b = 0.5 + rs.rand(40, 6); b = np.hstack([b, b[:, :3]]); c = 0.5 + rs.rand(40, 14)
    lp = StandardLP(SparseMatrix(matrix=A), b, c, 0.0).to_equality_form()
    s = solver_registry[solver_name](hsd=hsd)
    lp.init(s); lp.solve(s)
    r = oracle_on(lp, flags=32 if hsd else 0)
    assert (s.status == 0).all() and (r["status"] == 0).all() and s.iters.max() < 40
    assert rel_err(s.primal_obj, r["pobj"]).max() < 1e-8
    truth = np.array([-linprog(-c[i], A_ub=A, b_ub=b[i], bounds=(0, None), method="highs").fun for i in range(8)])
    assert rel_err(s.primal_obj[:8], truth).max() < 1e-8


@pytest.mark.parametrize("m,n", [(16, 32), (32, 64)])
@pytest.mark.parametrize("flags", [0, 16, 4, 8])
def test_hsd_objective_parity_on_baseline_configs(m, n, flags):
    """The HSD kernel on the BASELINE shapes -- slack-aware and generic (16) variants, guarded LDL' path (4),
    autoscale (8) -- against the reference goldens (1e-8) and the oracle (1e-9, same iteration counts)."""
    g = golden("config_%dx%d.npz" % (m, n))
    A, b, c = problems.random_dense_arrays(m, n, int(g["nobj"]), seed=0)
    elp, s = solve_arrays(A, b, c, hsd=True, flags=flags)
    assert (s.status == 0).all()
    assert rel_err(s.primal_obj, g["pobj"]).max() < OBJ_TOL and rel_err(s.dual_obj, g["dobj"]).max() < OBJ_TOL
    r = oracle_on(elp, flags=32 | (flags & 8))
    # ~1.5 % of the LPs stop one iteration apart: on this path all three residuals shrink in lockstep, so the stop
    # test often lands within rounding (summation order) of its threshold
    assert np.abs(s.iters.astype(int) - r["iters"]).max() <= 1 and (s.iters == r["iters"]).mean() > 0.97
    assert rel_err(s.primal_obj, r["pobj"]).max() < 1e-9 and rel_err(s.dual_obj, r["dobj"]).max() < 1e-9
    nfull = g["x"].shape[0]
    np.testing.assert_allclose(s.x[:nfull, :n], g["x"], rtol=1e-5, atol=1e-6)


@pytest.mark.parametrize("m,n", [(1, 1), (2, 3), (17, 40), (32, 96), (5, 123)])
def test_hsd_shapes_up_to_the_maximum(m, n):
    rs = np.random.RandomState(m * 131 + n)
    A = rs.rand(m, n) * 2 - 0.4
    b = rs.rand(96, m) * 2 - 0.3; c = rs.rand(96, n) * 2 - 0.4
    lp = EqualityLP(SparseMatrix(matrix=A), b, c, 0.0)       # general dense A: no slack columns
    s = solver_registry["hip_dense_primal_normal"](hsd=True)
    lp.init(s); lp.solve(s)
    r = oracle_on(lp, flags=32)
    np.testing.assert_array_equal(s.status, r["status"])
    assert np.abs(s.iters.astype(int) - r["iters"]).max() <= 1
    opt = s.status == 0
    if opt.any():
        assert rel_err(s.primal_obj[opt], r["pobj"][opt]).max() < 1e-8


def test_first_generation_kernel_flag_is_refused():
    """the round-1 wave-per-LP kernel has been removed; the library answers its flag with
    PYCLLP_E_UNSUPPORTED -> NotImplementedError, never with a silent other path."""
    A, b, c = problems.random_dense_arrays(8, 12, 4, seed=1)
    with pytest.raises(NotImplementedError):
        solve_arrays(A, b, c, hsd=False, flags=2)


def test_hsd_flag_is_rejected_where_it_is_not_implemented():
    A, b, c = problems.random_dense_arrays(8, 12, 4, seed=1)
    with pytest.raises(ValueError):
        solve_arrays(A, b, c, hsd=True, flags=2)


def test_keep_on_device_returns_cuda_tensors():
    A, b, c = problems.random_dense_arrays(16, 32, 128, seed=6)
    lp = StandardLP(SparseMatrix(matrix=A), b, c, 0.0).to_equality_form()
    s = solver_registry["hip_dense_primal_normal"](keep_on_device=True)
    lp.init(s)
    st = lp.solve(s)
    assert st.is_cuda and s.x.is_cuda and s.x.shape == (128, 48) and int((st != 0).sum()) == 0


# ---- stand-alone LDL' kernels (reference tests/test_ldl.py:139-193: 32 random SPD matrices of 100 x 100) ------------

def _spd_batch(n, B, seed):
    from scipy.sparse import rand as sparse_rand
    rs = np.random.RandomState(seed)
    out = np.empty((B, n, n))
    for i in range(B):
        X = sparse_rand(n, 80, density=0.1, random_state=rs).toarray()       # fixture A of tests/test_ldl.py:27-31
        out[i] = X @ X.T + np.eye(n) * n
    return out


@pytest.mark.parametrize("n,B", [(100, 32), (7, 5), (64, 3), (65, 2), (128, 2), (1, 4)])
def test_ldl_kernels_against_oracle_and_cholesky(n, B):
    from pycllp_amd import ldl as hip_ldl
    from oracle import port
    AA = _spd_batch(n, B, seed=n)
    D, L = hip_ldl.ldl(AA)
    assert D.shape == (B, n) and L.shape == (B, n, n)
    for i in range(B):
        Lo, Do = port.ldl(AA[i])
        np.testing.assert_allclose(D[i], Do, rtol=1e-6, atol=1e-7)                   # tests/test_ldl.py:178-179
        np.testing.assert_allclose(L[i], Lo, rtol=1e-6, atol=1e-7)
        np.testing.assert_allclose(L[i] * np.sqrt(D[i]), np.linalg.cholesky(AA[i]), rtol=1e-9, atol=1e-10)
    beta = float(np.sqrt(AA.max()))                                                   # tests/test_ldl.py:182
    D2, L2 = hip_ldl.modified_ldl(AA, delta=1e-6, beta=beta)
    for i in range(B):
        Lo, Do = port.ldl(AA[i], modified=True, beta=beta, delta=1e-6)
        np.testing.assert_allclose(D2[i], Do, rtol=1e-6, atol=1e-7)
        np.testing.assert_allclose(L2[i], Lo, rtol=1e-6, atol=1e-7)
    Ds, Ls = hip_ldl.ldl(AA[0])                                                       # single-matrix form, (D, L) order
    np.testing.assert_array_equal(Ds, D[0]); np.testing.assert_array_equal(Ls, L[0])


def test_modified_ldl_guard_bites_on_semidefinite_matrix():
    from pycllp_amd import ldl as hip_ldl
    from oracle import port
    rs = np.random.RandomState(4)
    X = rs.rand(12, 5)
    S = X @ X.T                       # rank 5 < 12: the guard must act (tests/test_ldl.py:79-87)
    D, L = hip_ldl.modified_ldl(S, delta=1e-6)
    Lo, Do = port.ldl(S, modified=True, delta=1e-6)
    assert np.isfinite(L).all() and (D >= 1e-6).all()
    np.testing.assert_allclose(D[:5], Do[:5], rtol=1e-6)           # beyond the rank the pivots are rounding noise
    with pytest.raises(NotImplementedError):
        hip_ldl.ldl(np.eye(129))


# ---- sparse shared-A path (reference cl_sparse_primal_normal; BASELINE config 5) -------------------------------------

def _sparse_case(m, n, B, density, seed):
    import scipy.sparse as sp
    A, b, c = problems.random_sparse_arrays(m, n, B, density=density, seed=seed)
    lp = StandardLP(SparseMatrix(matrix=A), b, c, 0.0).to_equality_form()
    s = solver_registry["hip_sparse_primal_normal"]()
    lp.init(s)
    st = lp.solve(s)
    return A, b, c, lp, s, st


@pytest.mark.parametrize("m,n,B,density", [(128, 256, 96, 0.025), (128, 256, 16, 0.1), (40, 90, 64, 0.1), (12, 20, 33, 0.3),
                                           (100, 80, 8, 1.0)])
def test_sparse_solver_matches_oracle_and_reference_solver(m, n, B, density):
    from oracle import port
    A, b, c, lp, s, st = _sparse_case(m, n, B, density, seed=m + n)
    r = port.dense_solve(lp.A.todense(), lp.b, lp.c, nthreads=8)
    np.testing.assert_array_equal(st, r["status"])
    assert (st == 0).all()
    assert np.abs(s.iters.astype(int) - r["iters"]).max() <= 1
    assert rel_err(s.primal_obj, r["pobj"]).max() < 1e-9 and rel_err(s.dual_obj, r["dobj"]).max() < 1e-9
    np.testing.assert_allclose(s.x, r["x"], rtol=1e-5, atol=1e-6)
    # the reference's own CPU solver on the same StandardLPs (first few: it is slow at this size), stored by
    # tools/gen_golden.py sparse_solver_cases
    g = golden("sparse_solver_cases.npz")
    key = "%dx%d_B%d_d%g_" % (m, n, B, density)
    np.testing.assert_allclose(g[key + "input_checksum"], [A.sum(), b.sum(), c.sum()], rtol=1e-12)
    k = len(g[key + "pobj"])
    assert k == min(B, 8) and (g[key + "status"] == 0).all()
    assert rel_err(s.primal_obj[:k], g[key + "pobj"]).max() < OBJ_TOL and rel_err(s.dual_obj[:k], g[key + "dobj"]).max() < OBJ_TOL


def test_sparse_solver_guarded_path_agrees():
    """PYCLLP_FLAG_FORCE_GUARD_PATH makes the block kernel re-assemble M and run the guarded LDL' sweep."""
    from oracle import port
    A, b, c = problems.random_sparse_arrays(70, 120, 24, density=0.06, seed=5)
    lp = StandardLP(SparseMatrix(matrix=A), b, c, 0.0).to_equality_form()
    s = solver_registry["hip_sparse_primal_normal"](flags=4)
    lp.init(s)
    st = lp.solve(s)
    r = port.dense_solve(lp.A.todense(), lp.b, lp.c, nthreads=8)
    np.testing.assert_array_equal(st, r["status"])
    assert (st == 0).all() and np.abs(s.iters.astype(int) - r["iters"]).max() <= 1
    assert rel_err(s.primal_obj, r["pobj"]).max() < 1e-9 and rel_err(s.dual_obj, r["dobj"]).max() < 1e-9


def test_sparse_solver_edge_cases():
    import scipy.sparse as sp
    A, b, c = problems.random_sparse_arrays(20, 30, 5, density=0.2, seed=1)
    lp = StandardLP(SparseMatrix(matrix=A), b, c, 0.0).to_equality_form()
    s = solver_registry["hip_sparse_primal_normal"]()
    lp.init(s)
    first = lp.solve(s).copy(); x1 = s.x.copy()
    lp.solve(s)
    np.testing.assert_array_equal(s.x, x1)                      # deterministic: no atomics in the Gram assembly
    big = StandardLP(SparseMatrix(matrix=sp.random(257, 10, density=0.5, random_state=0)), np.ones((1, 257)), np.ones((1, 10)), 0.0)
    with pytest.raises(NotImplementedError):
        big.to_equality_form().init(solver_registry["hip_sparse_primal_normal"]())
    empty = StandardLP(SparseMatrix(matrix=A), np.zeros((0, 20)), np.zeros((0, 30)), np.zeros(0)).to_equality_form()
    s2 = solver_registry["hip_sparse_primal_normal"]()
    empty.init(s2)
    assert empty.solve(s2).shape == (0,)


def test_sparse_config5_against_golden_objectives():
    import scipy.sparse as sp
    g = golden("config_sparse_128x256.npz")
    A = sp.csr_matrix((g["A_data"], g["A_indices"], g["A_indptr"]), shape=(int(g["m"]), int(g["n"])))
    lp = StandardLP(SparseMatrix(matrix=A), g["b"], g["c"], 0.0).to_equality_form()
    s = solver_registry["hip_sparse_primal_normal"]()
    lp.init(s)
    st = lp.solve(s)
    assert (st == 0).all() and (g["status"] == 0).all()
    assert rel_err(s.primal_obj, g["pobj"]).max() < OBJ_TOL and rel_err(s.dual_obj, g["dobj"]).max() < OBJ_TOL
    np.testing.assert_allclose(s.x[:16, :int(g["n"])], g["x"], rtol=1e-5, atol=1e-6)
    np.testing.assert_allclose(s.y[:16], g["y"], rtol=1e-5, atol=1e-6)


def test_sparse_solver_hsd_statuses_and_certificates():
    """PYCLLP_FLAG_HSD through the sparse (one LP per workgroup) kernel: the mixed-sign fixture again -- true status for
    every LP, the oracle's answer LP by LP, valid certificates."""
    for A, b, c, ref_status, highs, ref_pobj in status_cases():
        lp = StandardLP(SparseMatrix(matrix=A), b, c, 0.0).to_equality_form()
        s = solver_registry["hip_sparse_primal_normal"](hsd=True)
        lp.init(s); lp.solve(s)
        np.testing.assert_array_equal(s.status, highs)
        r = oracle_on(lp, flags=32)
        np.testing.assert_array_equal(s.status, r["status"])
        assert np.abs(s.iters.astype(int) - r["iters"]).max() <= 1
        opt = highs == 0
        if opt.any():
            assert rel_err(s.primal_obj[opt], ref_pobj[opt]).max() < OBJ_TOL
            assert rel_err(s.primal_obj[opt], r["pobj"][opt]).max() < 1e-9
        check_certificates(lp.A.todense(), lp.b, lp.c, dict(status=s.status, x=s.x, y=s.y, z=s.z))


@pytest.mark.parametrize("flags", [0, 4, 8])
def test_sparse_solver_hsd_config5_golden_objectives(flags):
    import scipy.sparse as sp
    g = golden("config_sparse_128x256.npz")
    A = sp.csr_matrix((g["A_data"], g["A_indices"], g["A_indptr"]), shape=(int(g["m"]), int(g["n"])))
    lp = StandardLP(SparseMatrix(matrix=A), g["b"], g["c"], 0.0).to_equality_form()
    s = solver_registry["hip_sparse_primal_normal"](hsd=True, flags=flags)
    lp.init(s)
    st = lp.solve(s)
    assert (st == 0).all()
    assert rel_err(s.primal_obj, g["pobj"]).max() < OBJ_TOL and rel_err(s.dual_obj, g["dobj"]).max() < OBJ_TOL
    r = oracle_on(lp, flags=32 | (flags & 8))
    assert np.abs(s.iters.astype(int) - r["iters"]).max() <= 1
    np.testing.assert_allclose(s.x[:16, :int(g["n"])], g["x"], rtol=1e-5, atol=1e-6)


# ---- autoscale option (not in the reference) -------------------------------------------------------------------------

def assert_same_results(s, t):
    for k in ("x", "y", "z", "status", "iters", "primal_obj", "dual_obj"):
        np.testing.assert_array_equal(getattr(s, k), getattr(t, k), err_msg=k)


@pytest.mark.parametrize("kind", ["dense", "sparse", "pipeline", "pipeline on a caller's stream", "pipeline per-problem A"])
def test_autoscale_on_badly_scaled_lps(kind):
    """b ~ 1e-3, c ~ 1e+2: the reference algorithm needs up to 170 iterations and is only 1e-7 accurate; with
    autoscale=True the solve behaves as on a well-scaled LP.  Parity against the oracle running the same option.
    The pipeline cases: a host batch with B (m + n) >= 65536, for which the host pipeline of lp.solve() decides
    autoscale='auto' on the device while it already solves; the verdict must be the one autoscale=True / False give."""
    from oracle import port
    rs = np.random.RandomState(5)
    kw = {}
    if kind == "sparse":
        m, n, B = 60, 140, 24
        A, _, _ = problems.random_sparse_arrays(m, n, 1, density=0.08, seed=3)
        name = "hip_sparse_primal_normal"
    else:
        m, n, B = 11, 33, 130 if kind == "dense" else 16384
        A = rs.rand(m, n)
        name = "hip_dense_primal_normal"
        if kind == "pipeline on a caller's stream":
            kw = dict(stream=torch.cuda.Stream())
    if kind == "pipeline per-problem A":
        coo = SparseMatrix(matrix=A)
        Amat = SparseMatrix(coo._rows, coo._cols, coo.data * (0.75 + 0.5 * rs.rand(B, coo.nnzeros)))
    else:
        Amat = SparseMatrix(matrix=A)
    b = 1e-3 * (0.5 + rs.rand(B, m)); c = 1e2 * (0.5 + rs.rand(B, n))
    lp = StandardLP(Amat, b, c, 0.0).to_equality_form()
    s = solver_registry[name](autoscale=True, **kw)
    lp.init(s)
    st = lp.solve(s)
    assert (st == 0).all() and s.iters.max() < 60
    pure = lambda a, ref: (np.abs(a - ref) / np.abs(ref)).max()
    assert pure(s.primal_obj, s.dual_obj) < 1e-9                                   # scale-free optimality
    if not kind.startswith("pipeline"):
        r = port.dense_solve(lp.A.todense(), lp.b, lp.c, nthreads=8, flags=8)
        np.testing.assert_array_equal(st, r["status"])
        assert np.abs(s.iters.astype(int) - r["iters"]).max() <= 1
        assert pure(s.primal_obj, r["pobj"]) < 1e-9 and pure(s.dual_obj, r["dobj"]) < 1e-9
        Ae = lp.A.todense()
        assert np.abs(s.x @ Ae.T - lp.b).max() < 1e-9 * np.abs(lp.b).max() * 10
        np.testing.assert_allclose(s.x, r["x"], rtol=1e-5, atol=1e-9)
        np.testing.assert_allclose(s.y, r["y"], rtol=1e-5, atol=1e-4)
    # the DEFAULT solver (autoscale='auto') switches the option on for this batch by itself -- same
    # arithmetic, same results bit for bit -- and leaves a batch inside the band [0.1, 10] alone
    from pycllp_amd.solvers.hip import autoscale_wanted
    assert autoscale_wanted(lp.b, lp.c)
    d = solver_registry[name](hsd=False, **kw)
    lp.init(d)
    lp.solve(d)
    s_plain = solver_registry[name](autoscale=True, hsd=False, **kw)
    lp.init(s_plain); lp.solve(s_plain)
    assert_same_results(d, s_plain)
    off = solver_registry[name](autoscale=False, hsd=False, **kw)
    lp.init(off); lp.solve(off)
    assert off.iters.mean() > 1.5 * d.iters.mean()            # what the option saves on such a batch
    b1 = 0.5 + rs.rand(B, m); c1 = 0.5 + rs.rand(B, n)
    lp1 = StandardLP(Amat, b1, c1, 0.0).to_equality_form()
    assert not autoscale_wanted(lp1.b, lp1.c)
    lp1.init(d); lp1.solve(d)
    lp1.init(off); lp1.solve(off)
    assert_same_results(d, off)


# ---- register-resident wavefront-per-LP kernel of the sparse path (csrc/wreg_wave.h) ----------------------------------

def test_sparse_wave_and_block_kernels_agree():
    """The default (register-resident, one LP per wavefront) kernel and the workgroup-per-LP kernel (PYCLLP_FLAG_BLOCK_KERNEL)
    are two implementations of the same semantics: same status, iterations within 1, objectives to 1e-9."""
    from pycllp_amd import _native
    A, b, c = problems.random_sparse_arrays(128, 256, 200, density=0.025, seed=11)
    lp = StandardLP(SparseMatrix(matrix=A), b, c, 0.0).to_equality_form()
    for hsd in (False, True):
        res = {}
        for name, fl in (("wave", 0), ("block", _native.FLAG_BLOCK_KERNEL)):
            s = solver_registry["hip_sparse_primal_normal"](flags=fl, hsd=hsd)
            lp.init(s); lp.solve(s)
            assert s.launch_info()["kernel"] == name
            res[name] = s
        w, k = res["wave"], res["block"]
        np.testing.assert_array_equal(w.status, k.status)
        assert (w.status == 0).all()
        assert np.abs(w.iters.astype(int) - k.iters).max() <= 1
        assert rel_err(w.primal_obj, k.primal_obj).max() < 1e-9 and rel_err(w.dual_obj, k.dual_obj).max() < 1e-9


@pytest.mark.parametrize("m,n,variant", [(48, 200, "n <= 256"), (100, 280, "n <= 384"), (60, 440, "n <= 512"),
                                         (80, 200, "m <= 80 / 96 (rows beyond the LDS m-vector entries of those variants)"), (40, 120, "m <= 48"), (90, 300, "m <= 96"),
                                         (10, 200, "m <= 16"), (30, 200, "m <= 32")])
def test_sparse_wave_kernel_column_variants(m, n, variant):
    """The register-resident kernel is compiled for 4, 6 and 8 N-vector registers per lane (N <= 256, 384, 512 columns of the
    equality form) and for 4, 6 and 8 block rows (m <= 64, 96, 128): one shape per variant, on the wave kernel, against the
    oracle LP by LP."""
    A, b, c = problems.random_sparse_arrays(m, n, 24, density=0.02, seed=5)
    lp = StandardLP(SparseMatrix(matrix=A), b, c, 0.0).to_equality_form()
    assert lp.ncols == m + n
    for hsd in (False, True):
        s = solver_registry["hip_sparse_primal_normal"](hsd=hsd)
        lp.init(s)
        st = lp.solve(s)
        assert s.launch_info()["kernel"] == "wave", variant
        r = oracle_on(lp, flags=32 if hsd else 0)
        np.testing.assert_array_equal(st, r["status"])
        assert (st == 0).all() and np.abs(s.iters.astype(int) - r["iters"]).max() <= 1
        assert rel_err(s.primal_obj, r["pobj"]).max() < 1e-9 and rel_err(s.dual_obj, r["dobj"]).max() < 1e-9


@pytest.mark.parametrize("case", ["standard 64x64", "standard 90x80", "standard 100x80", "equality 40x100 without identity columns"])
def test_dense_image_variant_of_the_wave_kernel(case):
    """A matrix whose Gram term list does not fit into LDS but whose dense image does runs on the dense-image variant of the
    register-resident kernel (MFMA Gram straight from the image, image mat-vecs): dense StandardLPs -- the identity columns of
    the equality form stay out of the image -- and a dense EqualityLP that has none.  Against the oracle LP by LP."""
    rs = np.random.RandomState(8)
    if case.startswith("standard"):
        m, n = {"64x64": (64, 64), "90x80": (90, 80), "100x80": (100, 80)}[case.split()[1]]
        A, b, c = problems.random_dense_arrays(m, n, 48, seed=m)
        lp = StandardLP(SparseMatrix(matrix=A), b, c, 0.0).to_equality_form()
    else:
        m, n, B = 40, 100, 48
        A = rs.randn(m, n)
        x0 = rs.rand(B, n) + 0.1; y0 = rs.randn(B, m)
        b = x0 @ A.T; c = y0 @ A - (rs.rand(B, n) + 0.1)          # strictly feasible primal-dual pair
        lp = EqualityLP(SparseMatrix(matrix=A), b, c, 0.0)
    for hsd in (False, True):
        s = solver_registry["hip_sparse_primal_normal"](hsd=hsd)
        lp.init(s)
        st = lp.solve(s)
        assert s.launch_info()["kernel"] == "wave" and s.launch_info()["variant"] == "dense image"
        r = oracle_on(lp, flags=32 if hsd else 0)
        np.testing.assert_array_equal(st, r["status"])
        assert (st == 0).all() and np.abs(s.iters.astype(int) - r["iters"]).max() <= 1
        # (the equality case has |b| ~ 20: the default autoscale='auto' solves it scaled, where the stopping tolerance is
        # eps (1 + |obj| / (max|b| max|c|)) in scaled units, i.e. up to max|b| max|c| / |obj| times wider in the caller's
        # units -- two solvers that both meet it may then be 2e-9 apart; measured 2.4e-9)
        from pycllp_amd.solvers.hip import autoscale_wanted
        tol = 1e-8 if autoscale_wanted(lp.b, lp.c) else 1e-9
        assert rel_err(s.primal_obj, r["pobj"]).max() < tol and rel_err(s.dual_obj, r["dobj"]).max() < tol
        np.testing.assert_allclose(s.x, r["x"], rtol=1e-5, atol=1e-6)


def test_sparse_config5_full_share_properties():
    """BASELINE configs[4], the full per-GPU share (16 384 LPs, shared sparse A 128 x 256): size-independent properties, as
    test_full_size_batch_properties does for configs[2] -- every LP optimal, KKT residuals, zero gap, bit-identical
    results under a permutation of the batch."""
    B = 16384
    A, b, c = problems.random_sparse_arrays(128, 256, B, density=0.025, seed=0)
    lp = StandardLP(SparseMatrix(matrix=A), b, c, 0.0).to_equality_form()
    for hsd in (False, True):
        s = solver_registry["hip_sparse_primal_normal"](hsd=hsd)
        lp.init(s)
        st = lp.solve(s).copy()
        assert s.launch_info()["kernel"] == "wave"
        assert (st == 0).all()
        x, y, z = s.x.copy(), s.y.copy(), s.z.copy()
        po, du = s.primal_obj.copy(), s.dual_obj.copy()
        Ae = lp.A.tocsr()
        nb = 1.0 + np.linalg.norm(lp.b, axis=1); nc = 1.0 + np.linalg.norm(lp.c, axis=1)
        assert (np.linalg.norm(lp.b - (Ae @ x.T).T, axis=1) / nb).max() < 1e-8          # primal feasibility
        assert (np.linalg.norm(lp.c - (Ae.T @ y.T).T + z, axis=1) / nc).max() < 1e-8    # dual feasibility
        assert x.min() >= 0 and z.min() >= 0
        assert (np.abs(po - du) / np.maximum(1.0, np.abs(po))).max() < 1e-8             # zero gap
        assert np.abs(np.einsum("ij,ij->i", lp.c, x) - po).max() < 1e-8 * np.abs(po).max()
        assert s.iters.max() < 200 and 35 < s.iters.mean() < 60
        perm = np.random.RandomState(1).permutation(B)                                  # batch order is immaterial
        lp2 = StandardLP(SparseMatrix(matrix=A), b[perm], c[perm], 0.0).to_equality_form()
        lp2.solve(s)
        np.testing.assert_array_equal(s.primal_obj, po[perm])
        np.testing.assert_array_equal(s.x, x[perm])


def test_hsd_refinement_default_is_resolved_inside_the_library():
    """a C caller that takes pycllp_hip_default_opts and sets PYCLLP_FLAG_HSD must get the 20-pass
    refinement cap (the struct carries PYCLLP_MAX_REFINE_AUTO = -1, resolved inside the entry points) -- checked through
    raw ctypes calls on the 256 LPs of config 5's share around the degenerate LP 7557, which with a cap of 5 sits at a
    1.6e-10 gap for 58-200 iterations; an explicit 5 is still honoured (more iterations, same optimum)."""
    import ctypes
    from pycllp_amd import _native
    L = _native.lib()
    A, b, c = problems.random_sparse_arrays(128, 256, 16384, density=0.025, seed=0)
    lo, hi = 7424, 7680
    lp = StandardLP(SparseMatrix(matrix=A), b[lo:hi], c[lo:hi], 0.0).to_equality_form()
    Ae = lp.A.tocsr(); Ae.sort_indices()
    dev = torch.device("cuda", 0)
    t = lambda a, dt: torch.as_tensor(np.ascontiguousarray(a, dtype=dt), device=dev)
    data, indptr, indices = t(Ae.data, np.float64), t(Ae.indptr, np.int32), t(Ae.indices, np.int32)
    bd, cd = t(lp.b, np.float64), t(lp.c, np.float64)
    B, m, n = hi - lo, 128, 384
    h = ctypes.c_void_p()
    p = lambda x: ctypes.c_void_p(x.data_ptr())
    assert L.pycllp_hip_sparse_init(m, n, int(Ae.nnz), p(data), p(indptr), p(indices), None, ctypes.byref(h)) == 0
    try:
        out = {}
        for cap in (-1, 5):
            o = _native.Opts()
            L.pycllp_hip_default_opts(ctypes.byref(o))
            assert o.max_refine == -1
            o.flags = _native.FLAG_HSD
            o.max_refine = cap
            x = torch.empty((B, n), dtype=torch.float64, device=dev); z = torch.empty_like(x)
            y = torch.empty((B, m), dtype=torch.float64, device=dev)
            po = torch.empty(B, dtype=torch.float64, device=dev); do = torch.empty_like(po)
            st = torch.empty(B, dtype=torch.int32, device=dev); it = torch.empty_like(st)
            torch.cuda.synchronize()
            assert L.pycllp_hip_sparse_solve(h, B, p(bd), p(cd), p(x), p(y), p(z), p(po), p(do), p(st), p(it),
                                             ctypes.byref(o), None) == 0
            torch.cuda.synchronize()
            out[cap] = (st.cpu().numpy(), it.cpu().numpy(), po.cpu().numpy())
        st, it, po = out[-1]
        assert (st == 0).all() and it.max() <= 60, (it.max(), it.argmax() + lo)
        ref = oracle_on(lp, flags=32)                      # the oracle's HSD default is the same 20 passes
        diff = np.abs(it.astype(int) - ref["iters"])       # (the degenerate LP's tail is rounding sensitive: measured 3 apart)
        assert (ref["status"] == 0).all() and (diff <= 1).mean() > 0.99 and diff.max() <= 5
        assert rel_err(po, ref["pobj"]).max() < 1e-9
        st5, it5, po5 = out[5]
        assert it5[7557 - lo] > it[7557 - lo]              # the explicit cap is honoured: LP 7557 stalls with it
        ok = st5 == 0
        assert rel_err(po5[ok], po[ok]).max() < 1e-8
    finally:
        L.pycllp_hip_sparse_free(h)


def test_sparse_newton_step_reference_recipe():
    """The reference's own test of its stand-alone kernel sparse_solve_primal_normal (tests/test_ldl.py:276-361: seed
    123456, m = 100, n = 80 (+100 slack), density 0.025, 32 systems, mu = 1) against the known-answer formula of
    tests/test_ldl.py:196-216, at the reference's tolerance."""
    from scipy.sparse import rand
    from oracle import port
    m, n, cl_size = 100, 80, 32
    np.random.seed(123456)
    A = np.c_[rand(m, n, density=0.025).toarray(), np.eye(m)]
    x = np.random.rand(m + n, cl_size); z = np.random.rand(m + n, cl_size)
    y = np.random.rand(m, cl_size); b = np.random.rand(m, cl_size)
    c = np.r_[np.random.rand(n, cl_size), np.zeros((m, cl_size))]
    mu = 1.0
    lp = EqualityLP(SparseMatrix(matrix=A), b.T[:1], c.T[:1], 0.0)
    s = solver_registry["hip_sparse_primal_normal"]()
    lp.init(s)
    dy = s.newton_step(x.T, z.T, y.T, b.T, c.T, mu)
    for i in range(cl_size):
        ref = port.newton_step_known_answer(A, x[:, i], z[:, i], y[:, i], b[:, i], c[:, i], mu)
        np.testing.assert_allclose(dy[i], ref, rtol=1e-5, atol=1e-5)
        np.testing.assert_allclose(dy[i], port.solve_primal_normal(A, x[:, i], z[:, i], y[:, i], b[:, i], c[:, i], mu), rtol=1e-7, atol=1e-9)


@pytest.mark.parametrize("n,B", [(100, 32), (128, 5), (37, 9), (16, 3), (1, 2)])
def test_ldl_solves_against_numpy(n, B):
    """solve_ldl, forward_backward_ldl, forward_backward and forward_backward_modified_ldl (pycllp/ldl.py:147-281) on the
    device against numpy.linalg.solve, as the reference's tests/test_ldl.py:119-136 do."""
    from pycllp_amd import ldl as hip_ldl
    A = _spd_batch(n, B, seed=n)
    rs = np.random.RandomState(n + 1)
    b = rs.rand(B, n)
    ref = np.linalg.solve(A, b[..., None])[..., 0]
    np.testing.assert_allclose(hip_ldl.solve_ldl(A, b), ref, rtol=1e-9, atol=1e-12)
    np.testing.assert_allclose(hip_ldl.solve_ldl(A[0], b[0]), ref[0], rtol=1e-9, atol=1e-12)
    D, L = hip_ldl.ldl(A)
    np.testing.assert_allclose(hip_ldl.forward_backward_ldl(L, D, b), ref, rtol=1e-9, atol=1e-12)
    C = np.linalg.cholesky(A)
    np.testing.assert_allclose(hip_ldl.forward_backward(C, np.swapaxes(C, -1, -2), b), ref, rtol=1e-9, atol=1e-12)
    np.testing.assert_allclose(hip_ldl.forward_backward(L * D[:, None, :], np.swapaxes(L, -1, -2), b), ref, rtol=1e-9, atol=1e-12)
    # the guard is inactive on a positive definite matrix with a tiny delta: same answer
    np.testing.assert_allclose(hip_ldl.forward_backward_modified_ldl(A, b, delta=1e-300), ref, rtol=1e-9, atol=1e-12)
    with pytest.raises(NotImplementedError):
        hip_ldl.solve_ldl(np.eye(129), np.ones(129))


def test_reference_lp_surface_replay():
    """The LP objects of tests/golden/reference_lp_surface.npz -- raw inputs and the attribute surface that REFERENCE-built
    pycllp.lp objects exposed for them (tools/check_reference_boundary.py) -- solved through the plugin API."""
    from test_host import _surface_cases
    for key, g, lp in _surface_cases():
        s = solver_registry["hip_dense_primal_normal"]()
        lp.init(s)
        st = lp.solve(s)
        r = oracle_on(lp)
        np.testing.assert_array_equal(st, r["status"])
        assert (st == 0).all()
        np.testing.assert_array_equal(s.iters, r["iters"])
        assert rel_err(s.primal_obj, r["pobj"] + float(g[key + "_in_f"])).max() < 1e-9


# ---- per-problem values of A, GeneralLP conversion ---------------------------------------------------------

@pytest.mark.parametrize("name", ["hip_sparse_primal_normal", "hip_dense_primal_normal"])
@pytest.mark.parametrize("hsd", [False, True])
def test_per_problem_values_of_A(name, hsd):
    """One structure, a different set of values for every LP (SparseMatrix.data[nproblems, nnz], pycllp/lp.py:16-54, which the
    reference's LP classes refuse, lp.py:335-336): every LP is checked against the oracle run with ITS OWN matrix."""
    from oracle import port
    import scipy.sparse as sp
    m, n, B = 24, 40, 48
    rs = np.random.RandomState(2)
    S = sp.random(m, n, density=0.2, random_state=rs, format="coo")
    rows, cols = np.r_[S.row, np.arange(m)], np.r_[S.col, rs.randint(n, size=m)]           # every row non-empty
    key = rows * n + cols
    _, first = np.unique(key, return_index=True)
    rows, cols = rows[first], cols[first]
    cover = np.setdiff1d(np.arange(n), cols)                                                # every column non-empty
    rows, cols = np.r_[rows, rs.randint(m, size=cover.size)], np.r_[cols, cover]
    data = 0.1 + rs.rand(B, rows.size)
    b = 0.5 + rs.rand(B, m); c = 0.5 + rs.rand(B, n)
    lp = StandardLP(SparseMatrix(rows, cols, data), b, c, 0.0).to_equality_form()
    s = solver_registry[name](hsd=hsd)
    lp.init(s)
    st = lp.solve(s)
    assert (st == 0).all()
    assert s.launch_info()["kernel"] == "wave"       # round 3: per-problem values run on the wavefront-per-LP kernel too
    for k in range(B):
        r = port.dense_solve(lp.A.todense(k), lp.b[k:k + 1], lp.c[k:k + 1], flags=32 if hsd else 0)
        assert r["status"][0] == 0 and abs(int(s.iters[k]) - int(r["iters"][0])) <= 1
        assert rel_err(s.primal_obj[k], r["pobj"][0]) < 1e-9 and rel_err(s.dual_obj[k], r["dobj"][0]) < 1e-9
        np.testing.assert_allclose(s.x[k], r["x"][0], rtol=1e-5, atol=1e-7)
    # the values matter: LP 0 solved with LP 1's matrix gives another optimum
    assert abs(s.primal_obj[0] - port.dense_solve(lp.A.todense(1), lp.b[:1], lp.c[:1])["pobj"][0]) > 1e-6


@pytest.mark.parametrize("hsd", [False, True])
def test_per_problem_values_of_A_against_the_reference_solver_and_the_block_kernel(hsd):
    """tests/golden/config_perA_128x256.npz: the first 32 LPs of bench.py's `perA` workload (config 5's structure, every LP
    its own values), each solved by the REFERENCE's hsd.c with its own matrix (tools/gen_golden.py per_problem_a_config) --
    the reference pins this extension LP by LP although its LP classes refuse such a batch (lp.py:335-336).  Also: the
    wave kernel's per-problem-A variant and the workgroup-per-LP kernel (PYCLLP_FLAG_BLOCK_KERNEL) agree, and a wave count
    that does not divide the batch (three waves per workgroup at this structure) loses no LP."""
    from pycllp_amd import _native
    g = golden("config_perA_128x256.npz")
    k, B = int(g["nobj"]), int(g["batch"])
    A, b, c = problems.random_sparse_arrays(128, 256, B, density=0.025, seed=0)
    nb = 1000 + 1                                                   # not a multiple of 3 or 4
    rows, cols, data = problems.per_problem_values(A, nb, seed=7)
    assert np.allclose(g["input_checksum"], [data[:k].sum(), b[:k].sum(), c[:k].sum()], rtol=1e-12)
    lp = StandardLP(SparseMatrix(rows, cols, data), b[:nb], c[:nb], 0.0).to_equality_form()
    s = solver_registry["hip_sparse_primal_normal"](hsd=hsd)
    lp.init(s)
    st = lp.solve(s).copy()
    info = s.launch_info()
    assert info["kernel"] == "wave" and (st == 0).all()
    assert rel_err(s.primal_obj[:k], g["pobj"]).max() < OBJ_TOL and rel_err(s.dual_obj[:k], g["dobj"]).max() < OBJ_TOL
    po, it = s.primal_obj.copy(), s.iters.copy()
    blk = solver_registry["hip_sparse_primal_normal"](hsd=hsd, flags=_native.FLAG_BLOCK_KERNEL)
    lp.init(blk)
    assert (lp.solve(blk) == 0).all() and blk.launch_info()["kernel"] == "block"
    assert rel_err(po, blk.primal_obj).max() < 1e-9 and np.abs(it.astype(int) - blk.iters).max() <= 1


def test_general_lp_through_the_plugin():
    """GeneralLP -> to_standard_form -> to_equality_form -> hip solver (pycllp/lp.py:725-792, 551-567), finite upper bounds
    and per-problem bounds included; the optimum is checked against scipy's HiGHS on the ORIGINAL general form."""
    from scipy.optimize import linprog
    import scipy.sparse as sp
    from pycllp_amd.lp import GeneralLP
    rs = np.random.RandomState(4)
    m, n, B = 6, 9, 12
    A = rs.rand(m, n)
    lo = np.where(rs.rand(m) < 0.5, 0.2 * rs.rand(m), -np.inf)
    hi = 2.0 + rs.rand(B, m)
    l = 0.1 * rs.rand(n)
    u = np.where(rs.rand(n) < 0.4, 0.5 + rs.rand(n), np.inf)
    glp = GeneralLP(SparseMatrix(matrix=sp.coo_matrix(A)), b=hi, c=rs.rand(B, n), a=lo, l=l, u=u, f=0.75)
    lp = glp.to_standard_form().to_equality_form()
    s = solver_registry["hip_dense_primal_normal"]()
    lp.init(s)
    assert (lp.solve(s) == 0).all()
    for k in range(B):
        keep = np.isfinite(lo)
        ref = linprog(-glp.c[k], A_ub=np.vstack([A, -A[keep]]), b_ub=np.r_[hi[k], -lo[keep]],
                      bounds=[(l[j], None if np.isinf(u[j]) else u[j]) for j in range(n)], method="highs")
        assert ref.status == 0
        assert abs(s.primal_obj[k] - (-ref.fun + 0.75)) < 1e-7 * max(1.0, abs(ref.fun))
        np.testing.assert_allclose(s.x[k, :n] + l, ref.x, atol=1e-6)


@pytest.mark.parametrize("mode", ["plain", "hsd", "predcorr"])
@pytest.mark.parametrize("case,kernel", [
    ("dense 32x64", "group"), ("dense 100x80", "wave"), ("sparse 128x256 d0.025", "wave"), ("sparse 128x256 d0.03", "block"),
    ("perA 60x120 d0.05", "wave"),
    ("dense 60x700", "big"), ("dense 200x200", "big"), ("sparse 256x512 d0.02", "big")])
def test_every_kernel_family_is_deterministic(case, kernel, mode):
    """The same batch solved three times -- with the device allocator's free blocks (workspaces, per-LP buffers) overwritten with
    a different bit pattern in between -- gives bit-identical x, y, z, objectives and iteration counts on every kernel family.
    A data race or a read of uninitialised memory shows up here as a difference in the last digits long before it costs an LP its
    status: round 3 found a missing workgroup barrier in the large-LP kernel's embedding path this way (objectives differing
    by 1e-12 from run to run; the parity tests had passed)."""
    if mode == "predcorr" and kernel == "block":
        pytest.skip("the block kernel has no predictor-corrector step (the option is refused there)")
    hsd, kw = mode == "hsd", ({"predcorr": True} if mode == "predcorr" else {})
    kind, shape = case.split()[0], case.split()[1]
    m, n = [int(v) for v in shape.split("x")]
    B = 40 if kernel != "big" else 10
    if kind == "dense":
        A, b, c = problems.random_dense_arrays(m, n, B, seed=m + n)
        lp = StandardLP(SparseMatrix(matrix=A), b, c, 0.0).to_equality_form()
        name = "hip_dense_primal_normal"
    else:
        dens = float(case.split()[2][1:])
        A, b, c = problems.random_sparse_arrays(m, n, B, density=dens, seed=m)
        if kind == "perA":
            rows, cols, data = problems.per_problem_values(A, B, seed=3)
            lp = StandardLP(SparseMatrix(rows, cols, data), b, c, 0.0).to_equality_form()
        else:
            lp = StandardLP(SparseMatrix(matrix=A), b, c, 0.0).to_equality_form()
        name = "hip_sparse_primal_normal"
    runs = []
    for rep in range(3):
        s = solver_registry[name](hsd=hsd, **kw)
        lp.init(s)
        st = lp.solve(s)
        assert s.launch_info().get("kernel", "group") == kernel, s.launch_info()
        runs.append((st.copy(), s.iters.copy(), s.x.copy(), s.y.copy(), s.z.copy(), s.primal_obj.copy(), s.dual_obj.copy()))
        del s
        torch.cuda.synchronize()
        # overwrite what the caching allocator now holds as free blocks, then hand it back
        junk = [torch.full((1 << 22,), float(rep + 1) * 1e300, dtype=torch.float64, device="cuda") for _ in range(8)]
        torch.cuda.synchronize()
        del junk
    for r in runs[1:]:
        for a, b_ in zip(runs[0], r):
            assert np.array_equal(a, b_, equal_nan=True)


@pytest.mark.parametrize("hsd", [False, True])
@pytest.mark.parametrize("m,n", [(32, 64), (16, 32), (7, 20)])
def test_results_do_not_depend_on_batch_size_or_slot(m, n, hsd):
    """An LP's x, y, z, objectives and iteration count are bit-identical whether it is solved alone, in a small batch (one LP per
    wavefront, idle lane groups), or as part of a batch that fills every slot and is refilled from the queue: the launch plan of
    the lane-group kernels (waves per workgroup, group-major slots) changes where an LP runs, never what is computed."""
    B = 5000
    A, b, c = problems.random_dense_arrays(m, n, B, seed=11 * m + n)
    lp = StandardLP(SparseMatrix(matrix=A), b, c, 0.0).to_equality_form()
    s = solver_registry["hip_dense_primal_normal"](hsd=hsd)
    lp.init(s)
    bd, cd = torch.as_tensor(lp.b, device="cuda"), torch.as_tensor(lp.c, device="cuda")
    full = {k: v.clone() for k, v in s.solve_device(bd, cd).items() if isinstance(v, torch.Tensor)}
    torch.cuda.synchronize()
    assert (full["status"] == 0).all()
    rs = np.random.RandomState(5)
    for nb in (1, 2, 3, 64, 255, 257, 1024, 1025, 1500, 2049, 4096):
        idx = torch.as_tensor(np.sort(rs.choice(B, size=nb, replace=False)), device="cuda")
        part = s.solve_device(bd[idx].contiguous(), cd[idx].contiguous(), slot=1)
        torch.cuda.synchronize()
        for k in ("x", "y", "z", "pobj", "dobj", "status", "iters"):
            assert torch.equal(part[k][:nb], full[k][idx]), (nb, k)


@pytest.mark.parametrize("hsd", [False, True])
def test_sparse_results_do_not_depend_on_batch_size(hsd):
    """The same property on the wavefront-per-LP kernel of the sparse solver (config 5's shape)."""
    B = 600
    A, b, c = problems.random_sparse_arrays(128, 256, B, density=0.025, seed=3)
    lp = StandardLP(SparseMatrix(matrix=A), b, c, 0.0).to_equality_form()
    s = solver_registry["hip_sparse_primal_normal"](hsd=hsd)
    lp.init(s)
    bd, cd = torch.as_tensor(lp.b, device="cuda"), torch.as_tensor(lp.c, device="cuda")
    full = {k: v.clone() for k, v in s.solve_device(bd, cd).items() if isinstance(v, torch.Tensor)}
    torch.cuda.synchronize()
    assert s.launch_info()["kernel"] == "wave"
    rs = np.random.RandomState(6)
    for nb in (1, 5, 300):
        idx = torch.as_tensor(np.sort(rs.choice(B, size=nb, replace=False)), device="cuda")
        part = s.solve_device(bd[idx].contiguous(), cd[idx].contiguous(), slot=1)
        torch.cuda.synchronize()
        for k in ("x", "y", "z", "pobj", "dobj", "status", "iters"):
            assert torch.equal(part[k][:nb], full[k][idx]), (nb, k)


def test_dense_handle_beyond_the_lane_groups_is_the_sparse_handle_of_its_csr():
    """pycllp_hip_dense_init beyond the lane-group kernels (m = 33 > 32) builds its sparse handle from the host CSR arrays of A's
    non-zeros: pycllp_hip_dense_solve on it and pycllp_hip_sparse_solve on a handle pycllp_hip_sparse_init made from the same
    CSR arrays run the same kernel on the same plan and return the same bits.  The LPs are feasible and bounded by construction
    (b = A x0, c = A'y0 + z0 with x0, z0 > 0)."""
    import ctypes
    from pycllp_amd import _native
    L = _native.lib()
    m, n, B = 33, 40, 8
    rs = np.random.RandomState(33)
    A = np.c_[rs.rand(m, n - m) + 0.1, np.eye(m)]
    x0, y0, z0 = rs.rand(B, n) + 0.5, rs.rand(B, m), rs.rand(B, n) + 0.5
    b, c = x0 @ A.T, y0 @ A + z0
    nz = A != 0.0
    data, indices = A[nz], np.nonzero(nz)[1]                    # row-major: CSR order
    indptr = np.r_[0, np.cumsum(nz.sum(axis=1))]
    dev = torch.device("cuda", 0)
    t = lambda a, dt: torch.as_tensor(np.ascontiguousarray(a, dtype=dt), device=dev)
    p = lambda x: ctypes.c_void_p(x.data_ptr())
    Ad, bd, cd = t(A, np.float64), t(b, np.float64), t(c, np.float64)
    vd, pd, id_ = t(data, np.float64), t(indptr, np.int32), t(indices, np.int32)
    hd, hs = ctypes.c_void_p(), ctypes.c_void_p()
    torch.cuda.synchronize()
    _native.check(L.pycllp_hip_dense_init(m, n, p(Ad), None, ctypes.byref(hd)), "dense_init")
    try:
        _native.check(L.pycllp_hip_sparse_init(m, n, int(data.size), p(vd), p(pd), p(id_), None, ctypes.byref(hs)), "sparse_init")
        try:
            out, info = {}, {}
            for name, solve, h in (("dense", L.pycllp_hip_dense_solve, hd), ("sparse", L.pycllp_hip_sparse_solve, hs)):
                x = torch.empty((B, n), dtype=torch.float64, device=dev); z = torch.empty_like(x)
                y = torch.empty((B, m), dtype=torch.float64, device=dev)
                po = torch.empty(B, dtype=torch.float64, device=dev); do = torch.empty_like(po)
                st = torch.empty(B, dtype=torch.int32, device=dev); it = torch.empty_like(st)
                torch.cuda.synchronize()
                _native.check(solve(h, B, p(bd), p(cd), p(x), p(y), p(z), p(po), p(do), p(st), p(it), None, None), name)
                torch.cuda.synchronize()
                out[name] = dict(x=x, y=y, z=z, pobj=po, dobj=do, status=st, iters=it)
            g, bl, lds, kern = (ctypes.c_int() for _ in range(4))
            mp, np_ = ctypes.c_int(), ctypes.c_int()
            assert L.pycllp_hip_dense_launch_info(hd, ctypes.byref(g), ctypes.byref(bl), ctypes.byref(lds), ctypes.byref(mp), ctypes.byref(np_)) == 0
            info["dense"] = (g.value, bl.value, lds.value, L.pycllp_hip_dense_kernel_kind(hd))
            assert L.pycllp_hip_sparse_launch_info(hs, ctypes.byref(g), ctypes.byref(bl), ctypes.byref(lds), ctypes.byref(kern)) == 0
            info["sparse"] = (g.value, bl.value, lds.value, kern.value)
            print("launch_info (grid, block, lds, kernel kind):", info)
            assert info["dense"] == info["sparse"] and info["dense"][0] > 0 and info["dense"][3] > 0
            assert (out["dense"]["status"] == 0).all()
            for k in ("x", "y", "z", "pobj", "dobj", "status", "iters"):
                assert torch.equal(out["dense"][k], out["sparse"][k]), k
        finally:
            L.pycllp_hip_sparse_free(hs)
    finally:
        L.pycllp_hip_dense_free(hd)
