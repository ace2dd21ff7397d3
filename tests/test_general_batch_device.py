"""GeneralLP batches with per-problem values of A to the bounded form on the device: the gather plans of ``pycllp_amd.lp``
(CPU: against ``bounded_matrices`` / ``bounded_values``), the C ABI entry ``pycllp_hip_general_to_bounded_batch`` (CPU: argument
checks; GPU: the host conversion's bits, the memory footprint, invalid LPs) and the two per-problem plugins on top of it
(``solve(lp)`` with the bits of the host conversion, ``solve_device_general`` in the original variables)."""
import ctypes
import functools
import types

import numpy as np
import pytest
import torch

import footprint as fp
import general_batch_cases as gbc
import sparse_general_batch_cases as sgbc
from general_device_cases import (DEV, KINDS5, RESULTS, P, assert_same_results, dev, fake_solution, fh_bound, frozen,
                                  same_bits)
from pycllp_amd import _native
from pycllp_amd.lp import (GATHER_ONE, GeneralLP, SparseMatrix, bounded_gather_csr, bounded_gather_dense, bounded_rowmap)
from test_general_solver import make_general

ENTRY = "pycllp_hip_general_to_bounded_batch"
CHUNK = 256                                           # kChunk of csrc/general_form.hip: terms of an LP staged in LDS at a time
TILE_BYTES = 32 * 1024                                # kBatchTileBytes there


def shuffled(glp, seed):
    """The same LPs with the coordinate lists of A in a random order (NOT sorted by row; per-problem values follow)."""
    p = np.random.default_rng(seed).permutation(glp.A.nnzeros)
    assert (np.diff(glp.A._rows[p]) < 0).any()
    A = SparseMatrix(glp.A._rows[p], glp.A._cols[p], glp.A.data[:, p])
    A._shape = (glp.nrows, glp.ncols)
    return GeneralLP(A, glp.b, glp.c, a=glp.a, l=glp.l, u=glp.u, f=glp.f)


@functools.lru_cache(maxsize=None)
def case(name):
    """(batch, 'dense' | 'csr': the plan it is converted with) of the conversion tests (shared, read-only); l != 0 unless stated."""
    if name == "1x1":
        return frozen(make_general(1, 1, 1, seed=601)), "dense"
    if name == "5x7":             # B = 37: a multiple of no tile; two fixed columns, u = +inf in half of the LPs
        return frozen(shuffled(make_general(5, 7, 37, seed=602, per_problem_A=True, mixed_u=True, kinds=KINDS5, fixed=2), 1)), "dense"
    if name == "5x7 l=0":
        g = shuffled(make_general(5, 7, 37, seed=603, per_problem_A=True, mixed_u=True, kinds=KINDS5, fixed=2), 2)
        return frozen(GeneralLP(g.A, g.b, g.c, a=g.a, l=np.zeros_like(g.l), u=g.u - g.l, f=g.f)), "dense"
    if name == "24x40":
        return gbc.make(24, 40), "dense"
    if name == "12x16":
        return gbc.make(12, 16), "dense"
    if name == "P2":              # 40 x 120 at 8 %
        return sgbc.make("P2"), "csr"
    if name == "32x96":           # 3 072 terms per LP: twelve chunks of CHUNK; 37 LPs: four tiles of 9 and a remainder of 1
        return frozen(make_general(32, 96, 37, seed=604, per_problem_A=True, mixed_u=True, fixed=2)), "dense"
    raise KeyError(name)


def tile_lps(glp):
    """G of the batch kernel of csrc/general_form.hip: the LPs of one workgroup's tile."""
    per_lp = 8 * ((glp.ncols | 1) + 3 * (glp.nrows | 1) + (min(glp.A.nnzeros, CHUNK) | 1))
    return min(64, TILE_BYTES // per_lp, glp.nproblems)


def csr_perm(Ah):
    from pycllp_amd.solvers.sparse_general_batch import csr_structure
    return csr_structure(Ah)[0]


def plan_of(glp, kind):
    """(gather plan, keep, sign) from the batch-wide structure and LP 0's values alone."""
    Ah, keep, sign = glp.bounded_structure(problem=0)
    assert Ah.data.shape[0] == 1
    if kind == "dense":
        return bounded_gather_dense(glp.A, keep, sign), keep, sign
    return bounded_gather_csr(glp.A, keep, sign, csr_perm(Ah)), keep, sign


def host_matrix(blp, kind):
    """[B, out_len]: what the plugins' host conversion hands to the solve entry."""
    if kind == "dense":
        from pycllp_amd.solvers.general_batch import HipGeneralBatchPrimalNormalSolver as D
        return D.bounded_matrices(blp).reshape(blp.nproblems, -1)
    from pycllp_amd.solvers.sparse_general_batch import HipSparseGeneralBatchPrimalNormalSolver as S
    return S.bounded_values(types.SimpleNamespace(_perm=csr_perm(blp.A)), blp)


def gathered(plan, data):
    """The plan carried out by numpy on ``data [B, nnz]``."""
    g = plan.astype(np.int64)
    v = data[:, np.clip(np.abs(g) - 1, 0, max(data.shape[1] - 1, 0))]
    return np.where(g == GATHER_ONE, 1.0, np.where(g == 0, 0.0, np.where(g > 0, v, -v)))


# ---- CPU -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["5x7", "12x16", "P2"])
def test_gather_plans_carry_the_host_matrices(name):
    glp, kind = case(name)
    blp, _ = glp.to_bounded_equality_form()
    plan, keep, sign = plan_of(glp, kind)
    want = host_matrix(blp, kind)
    assert plan.dtype == np.int32 and plan.shape == (want.shape[1],)
    same_bits(gathered(plan, np.asarray(glp.A.data)), want, "the plan against the host")
    if name == "5x7":
        assert keep.size == 4 and (sign < 0).any() and (plan == 0).sum() == 0 and (plan < 0).sum() == 7
    if kind == "csr":
        assert (plan == GATHER_ONE).sum() == keep.size and (plan == 0).sum() == 0
    order = glp.A.term_order()
    data, indptr, indices = glp.A.csr_term_order(3)
    same_bits(np.asarray(glp.A.data)[3][order], data, "term order")
    assert np.array_equal(glp.A._cols[order], indices)


def duplicate_entry_batch():
    g = make_general(5, 7, 6, seed=605, per_problem_A=True, mixed_u=True, kinds=KINDS5, fixed=2)
    rows, cols = np.append(g.A._rows, 2), np.append(g.A._cols, 3)                   # (2, 3) a second time
    data = np.concatenate([g.A.data, np.full((6, 1), 0.25)], axis=1)
    A = SparseMatrix(rows, cols, data)
    A._shape = (5, 7)
    return GeneralLP(A, g.b + 0.25 * g.u[:, 3:4], g.c, a=g.a, l=g.l, u=g.u, f=g.f)


def test_duplicate_entries_have_no_dense_plan():
    from pycllp_amd.solvers.general_batch import HipGeneralBatchPrimalNormalSolver
    glp = duplicate_entry_batch()
    Ah, keep, sign = glp.bounded_structure(problem=0)
    assert bounded_gather_dense(glp.A, keep, sign) is None
    s = HipGeneralBatchPrimalNormalSolver()
    assert s._ensure_conversion(glp, keep, sign) is None and s.conversion == "host"


ARRAYS = ("rowmap", "nnz", "Aorder", "Aindptr", "Aindices", "Avals", "out_len", "gather", "a", "b", "c", "l", "u", "f",
          "Ah", "bh", "ch", "uh", "fh", "invalid")
REQUIRED = tuple(k for k in ARRAYS if k not in ("nnz", "out_len", "l", "f"))


def raw_call(m=5, n=7, mk=4, B=4, nnz=9, out_len=28, null=()):
    args = [nnz if k == "nnz" else out_len if k == "out_len" else (None if k in null else P) for k in ARRAYS]
    return getattr(_native.lib(), ENTRY)(m, n, mk, B, *args, None)


def test_entry_refuses_bad_arguments_without_gpu():
    L = _native.lib()
    bad = ENTRY.encode() + b": bad argument"
    for name in REQUIRED:
        assert raw_call(null=(name,)) == -1 and L.pycllp_hip_last_error() == bad, name
    for kw in (dict(nnz=-1), dict(out_len=0), dict(out_len=-5), dict(mk=6), dict(m=0), dict(n=0), dict(mk=0), dict(B=-1)):
        assert raw_call(**kw) == -1 and L.pycllp_hip_last_error() == bad, kw
    for kw in (dict(m=257, mk=200), dict(n=1277, mk=4), dict(m=256, n=1025, mk=256)):
        assert raw_call(**kw) == -2, kw
        assert L.pycllp_hip_last_error().startswith(ENTRY.encode() + b": "), kw
    assert raw_call(B=0) == 0                                       # nothing to do, nothing launched
    assert raw_call(B=0, null=("Avals", "a", "b", "c", "u", "Ah", "bh", "ch", "uh", "fh", "invalid")) == 0


def test_symbol_is_declared_and_exported():
    import os
    from conftest import ROOT
    assert ENTRY in _native.EXPORTS and hasattr(ctypes.CDLL(_native.LIB_PATH), ENTRY)
    assert ENTRY + "(" in open(os.path.join(ROOT, "include", "pycllp_hip.h")).read()
    assert _native.lib().pycllp_hip_abi_version() == 1


# ---- GPU: the conversion ---------------------------------------------------------------------------------------------------------
def conversion(glp, kind):
    from pycllp_amd.solvers.general import BatchDeviceConversion
    plan, keep, sign = plan_of(glp, kind)
    return BatchDeviceConversion(glp, keep, sign, torch.device(DEV), plan)


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["1x1", "5x7", "5x7 l=0", "24x40", "P2", "32x96"])
def test_conversion_carries_the_bits_of_the_host(name):
    glp, kind = case(name)
    if name == "32x96":           # more terms than one staging chunk, three full tiles and a remainder
        G = tile_lps(glp)
        assert glp.A.nnzeros == 3072 > CHUNK and glp.nproblems >= 3 * G + 1 and glp.nproblems % G != 0, G
    blp, bmap = glp.to_bounded_equality_form()
    cv = conversion(glp, kind)
    l = None if name.endswith("l=0") else dev(glp.l)                # (l_dev = NULL on the l = 0 batch)
    bl = cv.to_bounded(None, dev(glp.A.data), dev(glp.a), dev(glp.b), dev(glp.c), l, dev(glp.u), dev(glp.f))
    torch.cuda.synchronize()
    got = {k: v.cpu().numpy() for k, v in bl.items()}
    assert not got["invalid"].any()
    same_bits(got["A"], host_matrix(blp, kind), "A^")
    for k in ("b", "c", "u"):
        same_bits(got[k], getattr(blp, k), k + "^")
    df, bound = np.abs(got["f"] - blp.f), fh_bound(glp)
    print("%s: max |f^ - host| = %.3g, bound there %.3g" % (name, df.max(), bound[df.argmax()]))
    assert (df <= bound).all()
    if name in ("5x7", "P2"):     # and back: the shared-A entry serves
        r = fake_solution(blp, 7)
        out = {k: dev(v) for k, v in r.items()}
        res = cv.from_bounded(None, l, bl["f"], bl["invalid"], out)
        torch.cuda.synchronize()
        x, y, z, s = bmap.general(r["x"], r["y"], r["z"], r["s"])
        for k, want in (("x", x), ("y", y), ("z", z), ("s", s)):
            same_bits(res[k].cpu().numpy(), want, k)
        assert np.array_equal(res["status"].cpu().numpy(), r["status"]) and np.array_equal(res["iters"].cpu().numpy(), r["iters"])


def to_specs(glp, kind):
    plan, keep, sign = plan_of(glp, kind)
    _, indptr, indices = glp.A.csr_term_order()
    B, m, n, mk = glp.nproblems, glp.nrows, glp.ncols, keep.size
    specs = [fp.inp("rowmap", bounded_rowmap(keep, sign, m), fp.I32), fp.inp("Aorder", glp.A.term_order(), fp.I32),
             fp.inp("Aindptr", indptr, fp.I32), fp.inp("Aindices", indices, fp.I32), fp.inp("Avals", glp.A.data),
             fp.inp("gather", plan, fp.I32)]
    specs += [fp.inp(k, getattr(glp, k)) for k in ("a", "b", "c", "l", "u", "f")]
    specs += [fp.out("Ah", (B, plan.size)), fp.out("bh", (B, mk)), fp.out("ch", (B, n + mk)), fp.out("uh", (B, n + mk)),
              fp.out("fh", (B,)), fp.out("invalid", (B,), fp.I32)]
    return specs, (m, n, mk, B), glp.A.nnzeros, int(plan.size)


def arena_call(arena, sizes, nnz, out_len):
    args = [nnz if k == "nnz" else ctypes.c_long(out_len) if k == "out_len" else fp._ptr(arena[k]) for k in ARRAYS]
    st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    return getattr(_native.lib(), ENTRY)(*sizes, *args, st)


@pytest.mark.gpu
@pytest.mark.parametrize("placement", ["aligned", "natural"])
@pytest.mark.parametrize("name", ["5x7", "P2"])
def test_footprint_of_the_entry(name, placement):
    glp, kind = case(name)
    blp, _ = glp.to_bounded_equality_form()
    specs, sizes, nnz, out_len = to_specs(glp, kind)
    ar = fp.Arena(specs, placement, DEV)
    assert arena_call(ar, sizes, nnz, out_len) == 0
    ar.check()                                                     # guard bands intact, inputs unchanged, every output written
    same_bits(ar.result("Ah"), host_matrix(blp, kind), "A^")
    for k in ("b", "c", "u"):
        same_bits(ar.result(k + "h"), getattr(blp, k), k + "^")
    assert (np.abs(ar.result("fh") - blp.f) <= fh_bound(glp)).all() and not ar.result("invalid").any()
    m, n, mk, B = sizes
    refused = fp.Arena(specs, placement, DEV)
    assert arena_call(refused, (m, n, m + 1, B), nnz, out_len) == -1
    assert arena_call(refused, sizes, nnz, 0) == -1
    assert arena_call(refused, (m, 1281 - mk, mk, B), nnz, out_len) == -2
    refused.check(outputs_written=False)


@pytest.mark.gpu
def test_invalid_lps_get_their_code_a_harmless_lp_and_nan_results():
    from pycllp_amd.solvers.general import subset
    from pycllp_amd.solvers.hip import Handle, bounded_outputs, solve_opts
    clean = shuffled(make_general(5, 7, 11, seed=606, per_problem_A=True, mixed_u=True, kinds=KINDS5, fixed=2), 3)
    cv = conversion(clean, "dense")                                # the plan of the batch as it should be
    plan, keep, sign = plan_of(clean, "dense")
    a, b, c, l, u = (v.copy() for v in (clean.a, clean.b, clean.c, clean.l, clean.u))
    l[1, 0] = -np.inf; c[1, 1] = np.nan                            # 1 (and 5: the smallest failing check counts)
    u[3, 3] = l[3, 3] - 1.0                                        # 2
    a[5, 2], b[5, 2] = b[5, 2], a[5, 2]                            # 3: the ranged row, a > b
    b[7, 0] = np.inf                                               # 4: a '+' row without its b
    c[9, 6] = np.inf                                               # 5
    bad, valid = np.array([1, 3, 5, 7, 9]), np.array([0, 2, 4, 6, 8, 10])      # a valid neighbour on each side
    bl = cv.to_bounded(None, dev(clean.A.data), dev(a), dev(b), dev(c), dev(l), dev(u), dev(clean.f))
    torch.cuda.synchronize()
    got = {k: v.cpu().numpy() for k, v in bl.items()}
    assert got["invalid"].tolist() == [0, 1, 0, 2, 0, 3, 0, 4, 0, 5, 0]
    blp, _ = subset(clean, valid).to_bounded_equality_form()
    for k in ("b", "c", "u"):
        same_bits(got[k][valid], getattr(blp, k), k + "^ of the valid LPs")
    same_bits(got["A"], gathered(plan, clean.A.data), "A^ of every LP, the invalid ones included")
    newrow = np.full(5, -1)
    newrow[keep] = np.arange(keep.size)
    for k in bad:
        ones = np.zeros(keep.size)                                 # A^_k 1: the row's signed terms in their order, the slack's 1 last
        for t in range(clean.A.nnzeros):
            r = newrow[clean.A._rows[t]]
            if r >= 0:
                ones[r] += sign[r] * clean.A.data[k, t]
        same_bits(got["b"][k], ones + 1.0, "b^ of LP %d" % k)
        assert not got["c"][k].any() and np.isposinf(got["u"][k]).all() and got["f"][k] == 0.0
    # a bounded solve and the way back
    Ah0 = clean.bounded_structure(problem=0)[0]
    h = Handle(np.ascontiguousarray(Ah0.todense()), torch.device(DEV), None)
    out = bounded_outputs(11, cv.mk, cv.n + cv.mk, torch.device(DEV))
    h.solve_batch_bounded(None, bl["A"].view(11, cv.mk, cv.n), bl["b"], bl["c"], bl["u"], out, solve_opts({}))
    res = cv.from_bounded(None, dev(l), bl["f"], bl["invalid"], out)
    torch.cuda.synchronize()
    r = {k: v.cpu().numpy() for k, v in res.items()}
    assert (r["status"][bad] == _native.STATUS_NUMERICAL).all() and (r["iters"][bad] == 0).all()
    for k in ("x", "y", "z", "s", "primal_obj", "dual_obj"):
        assert np.isnan(r[k][bad]).all(), k
    assert (r["status"][valid] == 0).all() and (r["iters"][valid] > 0).all()


# ---- GPU: the plugins ------------------------------------------------------------------------------------------------------------
DENSE, SPARSE = "hip_general_batch_primal_normal", "hip_sparse_general_batch_primal_normal"
POINTS = {"12x16": (DENSE, "bounded group per-problem"), "24x40": (DENSE, "bounded group per-problem"),
          "P1": (SPARSE, "bounded wave per-problem"), "P2": (SPARSE, "bounded wave per-problem")}


@functools.lru_cache(maxsize=None)
def point(name, factor):
    """The batch of a plugin test: inside the autoscale band at factor 1 (row 0 divided by 20, per-LP row factors near 1), and
    with a, b, l, u times ``factor``."""
    base = sgbc.make(name) if name.startswith("P") else case(name)[0]
    g = gbc.scaled_rows(sgbc.in_band(base), np.linspace(0.9, 1.1, base.nproblems))
    return frozen(gbc.scaled_data(g, factor, 1.0))


@pytest.mark.parametrize("name", sorted(POINTS))
def test_plugin_points_lie_inside_and_outside_the_autoscale_band(name):
    from pycllp_amd.solvers.hip import autoscale_wanted
    for factor, want in ((1.0, False), (100.0, True)):
        blp, _ = point(name, factor).to_bounded_equality_form()
        assert autoscale_wanted(blp.b, blp.c, blp.u) == want


def parent_arithmetic(plugin, glp, init_lp=None):
    """What ``solve(lp)`` computed before the device conversion: the bounded form and the per-problem array from the host, the
    existing ``solve_device(A, b, c, u)`` with the flag ``autoscale_wanted`` gives, ``BoundedMap.general`` and the bounded
    form's f on the results.  ``init_lp``: the LP the solver was initialised with, where it is another."""
    from pycllp_amd.solvers import solver_registry
    from pycllp_amd.solvers.hip import autoscale_wanted
    blp, bmap = glp.to_bounded_equality_form()
    s = solver_registry[plugin](device=DEV, autoscale=False, hsd=False)
    (glp if init_lp is None else init_lp).init(s)
    flags = _native.FLAG_AUTOSCALE if autoscale_wanted(blp.b, blp.c, blp.u) else 0
    out = s.solve_device(s._values(blp), blp.b, blp.c, blp.u, flags=flags)
    torch.cuda.synchronize()
    r = {k: v.cpu().numpy() for k, v in out.items()}
    x, y, z, sl = bmap.general(r["x"], r["y"], r["z"], r["s"])
    return dict(x=x, y=y, z=z, s=sl, status=r["status"], iters=r["iters"], primal_obj=r["pobj"] + blp.f, dual_obj=r["dobj"] + blp.f)


@pytest.mark.gpu
@pytest.mark.parametrize("factor", [1.0, 100.0], ids=["in band", "b,u x100"])
@pytest.mark.parametrize("name", sorted(POINTS))
def test_solve_carries_the_bits_of_the_host_conversion(name, factor):
    from pycllp_amd.solvers import solver_registry
    plugin, kernel = POINTS[name]
    glp = point(name, factor)
    s = solver_registry[plugin](device=DEV, hsd=False)
    glp.init(s)
    glp.solve(s)
    assert s.kernel == kernel and s.conversion == "device"
    want = parent_arithmetic(plugin, glp)
    assert (want["status"] == 0).sum() > glp.nproblems // 2
    assert_same_results({k: getattr(s, k) for k in RESULTS}, want, RESULTS)


@pytest.mark.gpu
def test_conversion_is_remade_when_sign_and_structure_change():
    """After ``init``, a ``solve`` on LPs whose row 3 ('<=' at init) has become a '>=' row -- the same m', another sign -- and
    whose coordinate lists stand in another order: the plan of ``init`` would negate the wrong terms and read the wrong ones."""
    from pycllp_amd.solvers import solver_registry
    first = point("12x16", 1.0)
    a, b = first.a.copy(), first.b.copy()
    assert np.isneginf(a[:, 3]).all() and np.isfinite(b[:, 3]).all()
    a[:, 3], b[:, 3] = b[:, 3] - 1.25, np.inf                       # (the slack of the '<=' row at x0 is below 1.1: still feasible)
    second = shuffled(GeneralLP(first.A, b, first.c, a=a, l=first.l, u=first.u, f=first.f), 4)
    s = solver_registry[DENSE](device=DEV, hsd=False)
    first.init(s)
    first.solve(s)
    plan = s._conv.gather.cpu().numpy()
    second.solve(s)
    assert s.conversion == "device" and not np.array_equal(s._conv.gather.cpu().numpy(), plan)
    want = parent_arithmetic(DENSE, second, init_lp=first)
    assert (want["status"] == 0).sum() > second.nproblems // 2
    assert_same_results({k: getattr(s, k) for k in RESULTS}, want, RESULTS)


@pytest.mark.gpu
def test_duplicate_entries_keep_the_host_conversion():
    from pycllp_amd.solvers import solver_registry
    glp = duplicate_entry_batch()
    s = solver_registry[DENSE](device=DEV, hsd=False)
    glp.init(s)
    glp.solve(s)
    assert s.kernel == POINTS["12x16"][1] and s.conversion == "host"
    assert_same_results({k: getattr(s, k) for k in RESULTS}, parent_arithmetic(DENSE, glp), RESULTS)
    with pytest.raises(RuntimeError):
        s.solve_device_general(glp.A.data, glp.a, glp.b, glp.c, glp.l, glp.u)


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["24x40", "P2"])
def test_solve_device_general_in_the_original_variables(name):
    from pycllp_amd.solvers import solver_registry
    plugin, kernel = POINTS[name]
    glp = point(name, 1.0)
    s = solver_registry[plugin](device=DEV, autoscale=False, hsd=False)
    glp.init(s)
    glp.solve(s)
    want = {k: getattr(s, k) for k in RESULTS}
    s.kernel = None
    res = s.solve_device_general(dev(glp.A.data), dev(glp.a), dev(glp.b), glp.c, dev(glp.l), dev(glp.u), glp.f)   # (tensors, and numpy)
    assert all(isinstance(v, torch.Tensor) and v.is_cuda for v in res.values()) and set(res) == set(RESULTS) | {"invalid"}
    torch.cuda.synchronize()
    got = {k: v.cpu().numpy() for k, v in res.items()}
    assert s.kernel == kernel and not got["invalid"].any()
    assert_same_results(got, want, ("x", "y", "z", "s", "status", "iters"))
    for k in ("primal_obj", "dual_obj"):
        assert (np.abs(got[k] - want[k]) <= fh_bound(glp)).all(), k
    with pytest.raises(ValueError):
        s.solve_device_general(dev(glp.A.data)[:5], dev(glp.a), dev(glp.b), glp.c, dev(glp.l), dev(glp.u))
    empty = s.solve_device_general(*(np.zeros((0,) + v.shape[1:]) for v in (glp.A.data, glp.a, glp.b, glp.c, glp.l, glp.u)))
    assert set(empty) == set(RESULTS) | {"invalid"} and all(v.is_cuda and v.shape[0] == 0 for v in empty.values())


@pytest.mark.gpu
@pytest.mark.parametrize("plugin", [DENSE, SPARSE])
def test_solve_device_general_needs_the_native_kernel(plugin):
    from pycllp_amd.solvers import solver_registry
    glp = make_general(5, 7, 4, seed=607)                           # a shared A: the plugin behind the mix-in serves it
    s = solver_registry[plugin](device=DEV)
    glp.init(s)
    with pytest.raises(RuntimeError):
        s.solve_device_general(np.broadcast_to(glp.A.data, (4, glp.A.nnzeros)), glp.a, glp.b, glp.c, glp.l, glp.u, glp.f)
    glp.solve(s)
    assert s.conversion is None and (s.status == 0).all()
