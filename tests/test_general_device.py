"""GeneralLP batches to and from the bounded form on the device: ``GeneralLP.bounded_structure`` (CPU), the C ABI entries
``pycllp_hip_general_to_bounded`` / ``pycllp_hip_general_from_bounded`` (CPU: argument checks; GPU: the host conversion's bits,
the memory footprint, invalid LPs) and the two shared-A general plugins on top of them (``solve(lp)`` with the bits of the host
conversion, ``solve_device`` in the original variables)."""
import ctypes
import functools
import types

import numpy as np
import pytest
import torch

import footprint as fp
from general_device_cases import (DEV, KINDS5, RESULTS, P, assert_same_results, dev, fake_solution, fh_bound, frozen,
                                  same_bits)
from pycllp_amd import _native
from pycllp_amd.lp import GeneralLP, SparseMatrix, bounded_rowmap
from test_general_solver import check_kkt, make_general
from test_sparse_general_solver import make_sparse_general

TO, FROM = "pycllp_hip_general_to_bounded", "pycllp_hip_general_from_bounded"


@functools.lru_cache(maxsize=None)
def case(name):
    """The batches of the conversion tests (shared, read-only); all with l != 0 unless stated."""
    if name == "1x1":
        return frozen(make_general(1, 1, 1, seed=401))
    if name == "5x7":             # all row kinds, two fixed columns (l == u), u = +inf in LP 0 only
        return frozen(make_general(5, 7, 3, seed=402, mixed_u=True, kinds=KINDS5, fixed=2))
    if name == "24x64":
        return frozen(make_general(24, 64, 1000, seed=403, mixed_u=True, fixed=2))
    if name == "130x300":         # sparse at 3 %: dropped rows, a dense row 0 of 300 terms, n > 256, B a multiple of nothing
        return frozen(make_sparse_general(130, 300, 70, seed=404, density=0.03, mixed_u=True, fixed=3))
    if name == "5x7 l=0":
        g = make_general(5, 7, 3, seed=405, mixed_u=True, kinds=KINDS5, fixed=2)
        return frozen(GeneralLP(g.A, g.b, g.c, a=g.a, l=np.zeros_like(g.l), u=g.u - g.l, f=g.f))
    raise KeyError(name)


# ---- CPU -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["5x7", "130x300"])
def test_bounded_structure_is_the_batch_wide_part_of_the_conversion(name):
    glp = case(name)
    blp, bmap = glp.to_bounded_equality_form()
    Ah, keep, sign = glp.bounded_structure()
    assert np.array_equal(Ah._rows, blp.A._rows) and np.array_equal(Ah._cols, blp.A._cols)
    same_bits(Ah.data, blp.A.data, "values of A^")
    assert Ah._shape == blp.A._shape == (keep.size, glp.ncols + keep.size)
    assert np.array_equal(keep, bmap.rows) and np.array_equal(sign, bmap.sign)
    assert keep.size < glp.nrows                                    # (a row is dropped)
    rowmap = bounded_rowmap(keep, sign, glp.nrows)
    assert rowmap.dtype == np.int32 and np.count_nonzero(rowmap) == keep.size
    assert np.array_equal(np.abs(rowmap[keep]) - 1, np.arange(keep.size)) and np.array_equal(np.sign(rowmap[keep]), sign)
    data, indptr, indices = glp.A.csr_term_order()
    assert indptr[0] == 0 and indptr[-1] == glp.A.nnzeros and np.array_equal(np.diff(indptr), np.bincount(glp.A._rows, minlength=glp.nrows))
    for i in (0, glp.nrows - 1):                                    # a row's terms in the order of the coordinate lists
        sel = glp.A._rows == i
        assert np.array_equal(indices[indptr[i]:indptr[i + 1]], glp.A._cols[sel])
        same_bits(data[indptr[i]:indptr[i + 1]], glp.A.data[0][sel], "row %d" % i)


def test_bounded_structure_raises_the_mixed_row_error():
    g = case("5x7")
    b = g.b.copy()
    b[1, 0] = np.inf                                                # row 0 ('<='): no bound in LP 1 only
    bad = GeneralLP(g.A, b, g.c, a=g.a, l=g.l, u=g.u, f=g.f)
    with pytest.raises(ValueError) as e1:
        bad.bounded_structure()
    with pytest.raises(ValueError) as e2:
        bad.to_bounded_equality_form()
    assert str(e1.value) == str(e2.value) and "Can not keep row 0" in str(e1.value)


TO_ARRAYS = ("rowmap", "nnz", "Adata", "Aindptr", "Aindices", "a", "b", "c", "l", "u", "f", "bh", "ch", "uh", "fh", "invalid")
FROM_ARRAYS = ("rowmap", "l", "fh", "invalid", "xh", "yh", "zh", "sh", "x", "y", "z", "s", "pobj", "dobj", "status", "iters")
REQUIRED = {TO: ("rowmap", "Adata", "Aindptr", "Aindices", "a", "b", "c", "u", "bh", "ch", "uh", "fh", "invalid"),
            FROM: ("rowmap", "fh", "invalid", "xh", "yh", "x", "y", "status")}


def raw_call(entry, m=5, n=7, mk=4, B=4, nnz=9, null=()):
    names = TO_ARRAYS if entry == TO else FROM_ARRAYS
    args = [nnz if k == "nnz" else (None if k in null else P) for k in names]
    return getattr(_native.lib(), entry)(m, n, mk, B, *args, None)


@pytest.mark.parametrize("entry", [TO, FROM])
def test_entries_refuse_bad_arguments_without_gpu(entry):
    L = _native.lib()
    bad = entry.encode() + b": bad argument"
    for name in REQUIRED[entry]:
        assert raw_call(entry, null=(name,)) == -1 and L.pycllp_hip_last_error() == bad, name
    sizes = [dict(m=0), dict(n=0), dict(mk=0), dict(m=-3), dict(mk=6), dict(B=-1)] + ([dict(nnz=-1)] if entry == TO else [])
    for kw in sizes:
        assert raw_call(entry, **kw) == -1 and L.pycllp_hip_last_error() == bad, kw
    if entry == FROM:                                               # z / s without the z^ / s^ they are taken from
        assert raw_call(entry, null=("zh",)) == -1 and raw_call(entry, null=("sh",)) == -1
        assert L.pycllp_hip_last_error() == bad
    for kw in (dict(m=257, mk=200), dict(n=1277, mk=4), dict(m=256, n=1025, mk=256)):
        assert raw_call(entry, **kw) == -2, kw
        assert L.pycllp_hip_last_error().startswith(entry.encode() + b": "), kw
    with pytest.raises(NotImplementedError):
        _native.check(-2, entry)
    assert raw_call(entry, B=0) == 0                                # nothing to do, nothing launched
    assert raw_call(entry, B=0, null=("a", "b", "c", "u", "xh", "yh", "x", "y")) == 0


# ---- GPU: the conversion ---------------------------------------------------------------------------------------------------------
def conversion(glp):
    from pycllp_amd.solvers.general import DeviceConversion
    Ah, keep, sign = glp.bounded_structure()
    return DeviceConversion(glp, keep, sign, torch.device(DEV))


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["1x1", "5x7", "24x64", "130x300", "5x7 l=0"])
def test_conversion_carries_the_bits_of_the_host(name):
    glp = case(name)
    blp, bmap = glp.to_bounded_equality_form()
    cv = conversion(glp)
    l = None if name.endswith("l=0") else dev(glp.l)                # (l_dev = NULL on the l = 0 batch)
    bl = cv.to_bounded(None, dev(glp.a), dev(glp.b), dev(glp.c), l, dev(glp.u), dev(glp.f))
    torch.cuda.synchronize()
    got = {k: v.cpu().numpy() for k, v in bl.items()}
    assert not got["invalid"].any()
    for k in ("b", "c", "u"):
        same_bits(got[k], getattr(blp, k), k + "^")
    assert np.isposinf(blp.u).any() or name == "1x1"
    df, bound = np.abs(got["f"] - blp.f), fh_bound(glp)
    print("%s: max |f^ - host| = %.3g, bound there %.3g" % (name, df.max(), bound[df.argmax()]))
    assert (df <= bound).all()
    # and back
    r = fake_solution(blp, 7)
    out = {k: dev(v) for k, v in r.items()}
    res = cv.from_bounded(None, l, bl["f"], bl["invalid"], out)
    torch.cuda.synchronize()
    x, y, z, s = bmap.general(r["x"], r["y"], r["z"], r["s"])
    for k, want in (("x", x), ("y", y), ("z", z), ("s", s)):
        same_bits(res[k].cpu().numpy(), want, k)
    same_bits(res["primal_obj"].cpu().numpy(), r["pobj"] + got["f"], "pobj + f^")
    same_bits(res["dual_obj"].cpu().numpy(), r["dobj"] + got["f"], "dobj + f^")
    assert np.array_equal(res["status"].cpu().numpy(), r["status"]) and np.array_equal(res["iters"].cpu().numpy(), r["iters"])


def to_specs(glp):
    Ah, keep, sign = glp.bounded_structure()
    data, indptr, indices = glp.A.csr_term_order()
    B, m, n, mk = glp.nproblems, glp.nrows, glp.ncols, keep.size
    specs = [fp.inp("rowmap", bounded_rowmap(keep, sign, m), fp.I32), fp.inp("Adata", data), fp.inp("Aindptr", indptr, fp.I32),
             fp.inp("Aindices", indices, fp.I32)]
    specs += [fp.inp(k, getattr(glp, k)) for k in ("a", "b", "c", "l", "u", "f")]
    specs += [fp.out("bh", (B, mk)), fp.out("ch", (B, n + mk)), fp.out("uh", (B, n + mk)), fp.out("fh", (B,)),
              fp.out("invalid", (B,), fp.I32)]
    return specs, (m, n, mk, B), int(data.size)


def from_specs(glp, blp, r):
    Ah, keep, sign = glp.bounded_structure()
    B, m, n = glp.nproblems, glp.nrows, glp.ncols
    specs = [fp.inp("rowmap", bounded_rowmap(keep, sign, m), fp.I32), fp.inp("l", glp.l), fp.inp("fh", blp.f),
             fp.inp("invalid", np.zeros(B), fp.I32)]
    specs += [fp.inp(k + "h", r[k]) for k in ("x", "y", "z", "s")]
    specs += [fp.out("x", (B, n)), fp.out("y", (B, m)), fp.out("z", (B, n)), fp.out("s", (B, n)), fp.out("pobj", (B,)),
              fp.out("dobj", (B,)), fp.out("status", (B,), fp.I32), fp.out("iters", (B,), fp.I32)]
    return specs, (m, n, keep.size, B)


def arena_call(entry, arena, sizes, nnz=None):
    """``entry`` on the arena's arrays, straight through the library (``footprint.call`` knows the solve entries only)."""
    names = [k for k in (TO_ARRAYS if entry == TO else FROM_ARRAYS)]
    args = [nnz if k == "nnz" else fp._ptr(arena[k]) for k in names]
    st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    return getattr(_native.lib(), entry)(*sizes, *args, st)


@pytest.mark.gpu
@pytest.mark.parametrize("placement", ["aligned", "natural"])
@pytest.mark.parametrize("name", ["5x7", "130x300"])
def test_footprint_of_both_entries(name, placement):
    glp = case(name)
    blp, bmap = glp.to_bounded_equality_form()
    specs, sizes, nnz = to_specs(glp)
    ar = fp.Arena(specs, placement, DEV)
    assert arena_call(TO, ar, sizes, nnz) == 0
    ar.check()
    for k in ("b", "c", "u"):
        same_bits(ar.result(k + "h"), getattr(blp, k), k + "^")
    assert (np.abs(ar.result("fh") - blp.f) <= fh_bound(glp)).all() and not ar.result("invalid").any()
    m, n, mk, B = sizes
    refused = fp.Arena(specs, placement, DEV)
    assert arena_call(TO, refused, (m, n, m + 1, B), nnz) == -1
    assert arena_call(TO, refused, (m, 1281 - mk, mk, B), nnz) == -2
    refused.check(outputs_written=False)

    r = fake_solution(blp, 8)
    x, y, z, s = bmap.general(r["x"], r["y"], r["z"], r["s"])
    specs, sizes = from_specs(glp, blp, r)
    inout = ("pobj", "dobj", "status", "iters")
    for null in ((), ("z", "s", "pobj", "dobj", "iters")):
        ar = fp.Arena(specs, placement, DEV, null=null)
        for k in inout:                                            # in/out arrays: the solve's values stand in them
            if k not in null:
                ar.views[k].copy_(dev(r[k]))
        assert arena_call(FROM, ar, sizes) == 0
        ar.check()                                                 # (guards, inputs; NULL outputs still all sentinel)
        got = ar.results()
        for k, want in (("x", x), ("y", y), ("z", z), ("s", s), ("pobj", r["pobj"] + blp.f), ("dobj", r["dobj"] + blp.f)):
            if k not in null:
                same_bits(got[k], want, k)
        assert np.array_equal(got["status"], r["status"]) and ("iters" in null or np.array_equal(got["iters"], r["iters"]))
    refused = fp.Arena(specs, placement, DEV)
    assert arena_call(FROM, refused, (m, n, 0, B)) == -1
    assert arena_call(FROM, refused, (257, n, mk, B)) == -2
    refused.check(outputs_written=False)


@pytest.mark.gpu
def test_invalid_lps_get_their_code_a_harmless_lp_and_nan_results():
    from pycllp_amd.solvers.general import subset
    from pycllp_amd.solvers.hip import Handle, bounded_outputs, solve_opts
    clean = make_general(5, 7, 8, seed=406, mixed_u=True, kinds=KINDS5, fixed=2)
    cv = conversion(clean)                                         # the plan of the batch as it should be
    Ah, keep, sign = clean.bounded_structure()
    a, b, c, l, u = (v.copy() for v in (clean.a, clean.b, clean.c, clean.l, clean.u))
    l[1, 0] = -np.inf; c[1, 1] = np.nan                            # 1 (and 5: the first failing check counts)
    u[2, 3] = l[2, 3] - 1.0                                        # 2
    a[3, 2], b[3, 2] = b[3, 2], a[3, 2]                            # 3: the ranged row, a > b
    b[4, 0] = np.inf                                               # 4: a '+' row without its b
    c[5, 6] = np.inf                                               # 5
    valid = np.array([0, 6, 7])
    bl = cv.to_bounded(None, dev(a), dev(b), dev(c), dev(l), dev(u), dev(clean.f))
    torch.cuda.synchronize()
    got = {k: v.cpu().numpy() for k, v in bl.items()}
    assert got["invalid"].tolist() == [0, 1, 2, 3, 4, 5, 0, 0]
    blp, _ = subset(clean, valid).to_bounded_equality_form()
    for k in ("b", "c", "u"):
        same_bits(got[k][valid], getattr(blp, k), k + "^ of the valid LPs")
    ones = np.zeros(keep.size)                                     # A^ 1: a row's terms in their order, the slack's 1 last
    for t in range(Ah.nnzeros):
        ones[Ah._rows[t]] += Ah.data[0, t]
    for k in range(1, 6):
        same_bits(got["b"][k], ones, "b^ of LP %d" % k)
        assert not got["c"][k].any() and np.isposinf(got["u"][k]).all() and got["f"][k] == 0.0
    # a bounded solve and the way back
    h = Handle(np.ascontiguousarray(Ah.todense()), torch.device(DEV), None)
    out = bounded_outputs(8, cv.mk, cv.n + cv.mk, torch.device(DEV))
    h.solve_bounded(None, bl["b"], bl["c"], bl["u"], out, solve_opts({}))
    res = cv.from_bounded(None, dev(l), bl["f"], bl["invalid"], out)
    torch.cuda.synchronize()
    r = {k: v.cpu().numpy() for k, v in res.items()}
    bad = np.arange(1, 6)
    assert (r["status"][bad] == _native.STATUS_NUMERICAL).all() and (r["iters"][bad] == 0).all()
    for k in ("x", "y", "z", "s", "primal_obj", "dual_obj"):
        assert np.isnan(r[k][bad]).all(), k
    assert (r["status"][valid] == 0).all() and (r["iters"][valid] > 0).all()
    check_kkt(subset(clean, valid), types.SimpleNamespace(**{k: r[k][valid] for k in ("x", "y", "z", "s")}))


# ---- GPU: the plugins ------------------------------------------------------------------------------------------------------------
def row_scaled(g, scale):
    """The LPs of ``g`` with row i of A and its bounds times scale[i] (> 0): the same feasible set."""
    A = g.A.todense() * scale[:, None]
    return GeneralLP(SparseMatrix(matrix=A), g.b * scale, g.c, a=g.a * scale, l=g.l, u=g.u, f=g.f)


@functools.lru_cache(maxsize=None)
def point(name, factor):
    """(plugin, kernel, batch): l != 0, fixed columns, mixed u; rows scaled so that the bounded form lies inside the autoscale
    band at factor 1, and b^, u^ times ``factor`` (a, b, l, u times it)."""
    if name == "group":
        g = make_general(24, 64, 300, seed=411, mixed_u=True, fixed=2)
        g = row_scaled(g, np.concatenate([[0.05], np.full(23, 0.25)]))
        plugin, kernel = "hip_general_primal_normal", "bounded group"
    else:
        g = make_sparse_general(40, 120, 300, seed=412, density=0.08, mixed_u=True, fixed=2)
        g = row_scaled(g, np.concatenate([[0.025], np.full(39, 0.5)]))
        plugin, kernel = "hip_sparse_general_primal_normal", "bounded wave"
    g = GeneralLP(g.A, g.b * factor, g.c, a=g.a * factor, l=g.l * factor, u=g.u * factor, f=g.f)
    return plugin, kernel, frozen(g)


@pytest.mark.parametrize("name", ["group", "wave"])
def test_plugin_points_lie_inside_and_outside_the_autoscale_band(name):
    from pycllp_amd.solvers.hip import autoscale_wanted
    for factor, want in ((1.0, False), (100.0, True)):
        blp, _ = point(name, factor)[2].to_bounded_equality_form()
        assert autoscale_wanted(blp.b, blp.c, blp.u) == want
        assert autoscale_wanted(torch.as_tensor(blp.b), torch.as_tensor(blp.c), torch.as_tensor(blp.u)) == want   # (the device's rule)


def parent_arithmetic(plugin_class, glp):
    """What ``solve(lp)`` computed before the device conversion: the bounded form from the host, ``Handle.solve_bounded`` on it,
    ``BoundedMap.general`` and the bounded form's f on the results."""
    from pycllp_amd.solvers.hip import Handle, autoscale_wanted, bounded_outputs, solve_opts
    blp, bmap = glp.to_bounded_equality_form()
    A, _ = plugin_class._bounded_matrix(blp.A)
    h = Handle(A, torch.device(DEV), None)
    o = solve_opts({}, _native.FLAG_AUTOSCALE if autoscale_wanted(blp.b, blp.c, blp.u) else 0)
    out = bounded_outputs(blp.nproblems, blp.nrows, blp.ncols, torch.device(DEV))
    h.solve_bounded(None, dev(blp.b), dev(blp.c), dev(blp.u), out, o)
    torch.cuda.synchronize()
    r = {k: v.cpu().numpy() for k, v in out.items()}
    x, y, z, s = bmap.general(r["x"], r["y"], r["z"], r["s"])
    return dict(x=x, y=y, z=z, s=s, status=r["status"], iters=r["iters"], primal_obj=r["pobj"] + blp.f, dual_obj=r["dobj"] + blp.f)


@pytest.mark.gpu
@pytest.mark.parametrize("factor", [1.0, 100.0], ids=["in band", "b,u x100"])
@pytest.mark.parametrize("name", ["group", "wave"])
def test_solve_carries_the_bits_of_the_host_conversion(name, factor):
    from pycllp_amd.solvers import solver_registry
    plugin, kernel, glp = point(name, factor)
    s = solver_registry[plugin](device=DEV)
    glp.init(s)
    glp.solve(s)
    assert s.kernel == kernel
    want = parent_arithmetic(solver_registry[plugin], glp)
    assert (want["status"] == 0).all()                             # (no LP for hsd='auto' to solve again)
    assert_same_results({k: getattr(s, k) for k in RESULTS}, want, RESULTS)


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["group", "wave"])
def test_solve_device_in_the_original_variables(name):
    from pycllp_amd.solvers import solver_registry
    plugin, kernel, glp = point(name, 1.0)
    s = solver_registry[plugin](device=DEV, autoscale=False, hsd=False)
    glp.init(s)
    glp.solve(s)
    want = {k: getattr(s, k) for k in RESULTS}
    s.kernel = None
    res = s.solve_device(dev(glp.a), dev(glp.b), glp.c, dev(glp.l), dev(glp.u), glp.f)       # (tensors, and numpy to upload)
    assert all(isinstance(v, torch.Tensor) and v.is_cuda for v in res.values()) and set(res) == set(RESULTS) | {"invalid"}
    torch.cuda.synchronize()
    got = {k: v.cpu().numpy() for k, v in res.items()}
    assert s.kernel == kernel and not got["invalid"].any() and (got["status"] == 0).all()
    assert_same_results(got, want, ("x", "y", "z", "s", "status", "iters"))
    for k in ("primal_obj", "dual_obj"):
        d = np.abs(got[k] - want[k])
        print("%s %s: max deviation %.3g, bound there %.3g" % (name, k, d.max(), fh_bound(glp)[d.argmax()]))
        assert (d <= fh_bound(glp)).all(), k
    with pytest.raises(ValueError):
        s.solve_device(dev(glp.a), dev(glp.b)[:5], glp.c, dev(glp.l), dev(glp.u))


@pytest.mark.gpu
def test_solve_device_needs_the_native_kernel():
    from pycllp_amd.solvers import solver_registry
    glp = make_general(40, 30, 4, seed=413)                         # 40 kept rows: the lane-group plugin takes the expansion
    s = solver_registry["hip_general_primal_normal"](device=DEV)
    glp.init(s)
    with pytest.raises(RuntimeError):
        s.solve_device(glp.a, glp.b, glp.c, glp.l, glp.u, glp.f)
    glp.solve(s)
    assert s.kernel == "expanded"
