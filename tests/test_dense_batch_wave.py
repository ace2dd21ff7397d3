"""Per-problem DENSE matrices beyond the lane-group kernels (m > 32 or n > 128): the wavefront-per-LP kernel with a dense image
per wave (csrc/ipm_wreg_dapa.hip, plan wreg_plan_create_dense_pa) behind pycllp_hip_dense_solve_batch, and the route of the
plugin hip_dense_batch_primal_normal to it.  The reference of every comparison is oracle.port.dense_solve run LP by LP with that
LP's own matrix; bounds are the project's (dense_batch_cases.assert_matches_oracle).

GPU tests run B = 37 LPs on a grid of two workgroups (``reserve_cus``): every wave takes several LPs in turn."""
import ctypes
import os
import re

import numpy as np
import pytest

import dense_batch_cases as dbc
import dense_batch_wave_cases as wc
import footprint as fp
from conftest import ROOT
from pycllp_amd import _native
from pycllp_amd.lp import SparseMatrix
from pycllp_amd.solvers import solver_registry
from pycllp_amd.solvers.dense_batch import densify_batch, fully_dense, identity_tail

NAME = "hip_dense_batch_primal_normal"
KEYS = ("x", "y", "z", "pobj", "dobj", "status", "iters")
CSRC = os.path.join(ROOT, "pycllp_amd", "csrc")


# ---- CPU ------------------------------------------------------------------------------------------------------------------
def test_plan_rule_reproduces_the_lds_table():
    """(shape, bytes per wave, waves per workgroup) by the geometry of wreg.h, on the dense-image shape list; then what the
    compiled list (without (8, 6)) makes of the two points that list serves alone."""
    da = wc.WAVE_DA_SHAPES
    assert wc.plan(33, 38, True, da) == ((3, 4), 21184, 4)
    assert wc.plan(48, 176, True, da) == ((3, 4), 65280, 2)
    assert wc.plan(64, 128, True, da) == ((4, 2), 49792, 3)
    assert wc.plan(64, 128, False, da) == ((4, 2), 82560, 1)
    assert wc.plan(100, 180, True, da) == ((7, 4), 90304, 1)
    assert wc.plan(128, 256, True, da) == ((8, 4), 156800, 1)
    assert wc.plan(80, 256, False, da) == ((5, 4), 183808, 0)                  # refused: not even one wave fits
    assert wc.plan(113, 257, True, da) == ((8, 6), 168000, 0)
    assert wc.plan(3, 257, False, da)[0] == (8, 6) and wc.plan(3, 257, False, da)[2] >= 1
    for m, n, tail in ((33, 38, True), (48, 176, True), (64, 128, True), (64, 128, False), (100, 180, True), (128, 256, True),
                       (80, 256, False)):
        assert wc.plan(m, n, tail) == wc.plan(m, n, tail, da)
    assert wc.plan(113, 257, True) is None and wc.plan(3, 257, False) is None   # (8, 6) is not compiled for per-problem matrices
    assert wc.plan(129, 140, True) is None and wc.plan(40, 385, True, da) is None


def test_shape_lists_are_those_of_the_sources():
    text = open(os.path.join(CSRC, "wreg.h")).read()
    shapes = lambda macro: [(int(a), int(b)) for a, b in
                            re.findall(r"X\((\d+),\s*(\d+)\)", re.search(r"#define %s\(X\)(.*)" % macro, text).group(1))]
    assert shapes("WREG_DA_SHAPES") == wc.WAVE_DA_SHAPES and shapes("WREG_DAPA_SHAPES") == wc.WAVE_DAPA_SHAPES
    unit = open(os.path.join(CSRC, "ipm_wreg_dapa.hip")).read()
    assert "WREG_TABLE(kWDAPA, WREG_DAPA_SHAPES," in unit and "ipm_wreg_kernel<MB, NQ, true, true>" in unit
    assert "hsd_wreg_kernel" not in unit and "newton_wreg_kernel" not in unit        # the plain kernel only
    assert "ipm_wreg_dapa.o" in open(os.path.join(CSRC, "Makefile")).read()


def test_every_point_is_served_by_its_shape_and_fits():
    assert sorted(wc.POINTS) == sorted(wc.WAVE_DAPA_SHAPES)
    for shape, points in wc.POINTS.items():
        for which, (m, n, tail) in enumerate(points):
            assert m > 32 or n > 128                                                # beyond the lane-group kernels
            got = wc.plan(m, n, tail)
            assert got[0] == shape and got[2] >= 1, (shape, m, n, tail, got)
        m, n, tail = points[1]                                                      # full: one more row or column does not fit
        assert m == 16 * shape[0] and n == 64 * shape[1]
    tails = [p[w][2] for p in wc.POINTS.values() for w in (0, 1)]
    assert tails.count(False) >= 7                                                  # both forms, on ragged and on full points
    assert {p[1][2] for p in wc.POINTS.values()} == {True, False}


def _structure(lp):
    return lp.A._rows, lp.A._cols, lp.A.data


def test_dense_structure_predicate():
    tail, general = dbc.make(33, 38, True, B=3), dbc.make(33, 70, False, B=3)
    assert fully_dense(*_structure(tail), 33, 38) and identity_tail(*_structure(tail), 33, 38)
    assert fully_dense(*_structure(general), 33, 70) and not identity_tail(*_structure(general), 33, 70)
    for lp, (m, n) in ((tail, (33, 38)), (general, (33, 70))):
        order = np.random.RandomState(4).permutation(np.asarray(lp.A._rows).size)      # shuffled coordinate order
        r, c, d = np.asarray(lp.A._rows)[order], np.asarray(lp.A._cols)[order], np.asarray(lp.A.data)[:, order]
        assert fully_dense(r, c, d, m, n)
        hole = np.ones(r.size, dtype=bool)
        hole[np.flatnonzero(c == 2)[5]] = False
        assert not fully_dense(r[hole], c[hole], d[:, hole], m, n)
        k = int(np.flatnonzero(c == 1)[3])
        assert not fully_dense(np.r_[r, r[k]], np.r_[c, c[k]], np.c_[d, d[:, k]], m, n)          # a duplicate
        assert not fully_dense(np.r_[r[hole], r[k]], np.r_[c[hole], c[k]], np.c_[d[:, hole], d[:, k]], m, n)    # both: the count is right
    # the 20 % structure of test_dense_batch.test_plugin_delegates_beyond_the_lane_group_kernels
    from pycllp_amd import problems
    from pycllp_amd.lp import StandardLP
    A, b, c = problems.random_sparse_arrays(40, 60, 24, density=0.2, seed=4)
    rows, cols, data = problems.per_problem_values(A, 24, seed=9)
    lp = StandardLP(SparseMatrix(rows, cols, data), b, c, 0.0).to_equality_form()
    assert not fully_dense(*_structure(lp), lp.nrows, lp.ncols)
    assert not fully_dense([], [], np.zeros((1, 0)), 3, 4)


def test_entry_checks_its_arguments_before_any_device_call():
    """The checks of pycllp_hip_dense_solve_batch come before the handle is read, whatever kernel would serve it."""
    L = _native.lib()
    buf = np.zeros(64)
    fake = buf.ctypes.data
    o = _native.default_opts()

    def args(h, B, flags, A=8):
        o.flags = flags
        return (h, B, A, 5, 8, 8, 8, 8, 8, 8, 8, 8, 8, ctypes.byref(o), None)
    assert L.pycllp_hip_dense_solve_batch(*args(None, 1, 0)) == -1
    assert L.pycllp_hip_dense_solve_batch(*args(fake, -1, 0)) == -1
    assert L.pycllp_hip_dense_solve_batch(*args(fake, 1, 0, A=None)) == -1
    for flag in (_native.FLAG_HSD, _native.FLAG_PREDCORR, _native.FLAG_WARM_START, _native.FLAG_WAVE_KERNEL):
        assert L.pycllp_hip_dense_solve_batch(*args(fake, 1, flag)) == -1
        assert L.pycllp_hip_last_error() == (b"pycllp_hip_dense_solve_batch: HSD, PREDCORR, WARM_START and WAVE_KERNEL are not "
                                             b"available with per-problem matrices")
    assert L.pycllp_hip_dense_solve_batch(*args(fake, 1, _native.FLAG_AUTOSCALE | _native.FLAG_AUTOSCALE_PER_LP)) == -1
    assert b"exclude each other" in L.pycllp_hip_last_error()


def test_header_documents_the_new_range():
    header = open(os.path.join(ROOT, "include", "pycllp_hip.h")).read()
    doc = header[:header.index("int pycllp_hip_dense_solve_batch(")].rsplit("/*", 1)[1]
    for text in ("m = 128", "n = 256", "image", "PER WAVE", "PYCLLP_STATUS_NUMERICAL", "PYCLLP_E_UNSUPPORTED", "(80, 256)"):
        assert text in doc, text


# ---- GPU ------------------------------------------------------------------------------------------------------------------
def ncu():
    import torch
    return torch.cuda.get_device_properties(0).multi_processor_count


def two_workgroups(m, n, tail):
    """``reserve_cus`` under which ipm_wreg.hip's solve_grid launches two workgroups."""
    shape, per_wave, waves = wc.plan(m, n, tail)
    return ncu() - (1 if wc.doubled(shape, per_wave, waves) else 2)


def results(s):
    return dict(x=s.x, y=s.y, z=s.z, pobj=s.primal_obj, dobj=s.dual_obj, status=s.status, iters=s.iters)


def solve(lp, tail, **kw):
    kw = dict(dict(hsd=False, autoscale=False, reserve_cus=two_workgroups(lp.nrows, lp.ncols, tail)), **kw)
    s = solver_registry[NAME](device="cuda:0", **kw)
    lp.init(s)
    lp.solve(s)
    return s, results(s)


def assert_plan(info, m, n, tail):
    shape, per_wave, waves = wc.plan(m, n, tail)
    assert info.get("kernel") == "wave" and info.get("variant") == "dense image" and info.get("wave_shape") == shape, info
    assert info["block"] == 64 * waves and info["lds_bytes"] == waves * per_wave and info["grid"] == 2, (info, per_wave, waves)
    assert "group_shape" not in info


def same_bits(got, ref, idx=None, ridx=None, keys=KEYS):
    for k in keys:
        a = got[k] if idx is None else got[k][idx]
        b = ref[k] if ridx is None else ref[k][ridx]
        assert np.array_equal(a.view(np.uint8), b.view(np.uint8)), k


@pytest.mark.gpu
@pytest.mark.parametrize("case", wc.EVERY, ids=[wc.every_id(c) for c in wc.EVERY])
def test_every_instantiation(case):
    shape, which = case
    m, n, tail = wc.POINTS[shape][which]
    lp = wc.batch(m, n, tail)
    s, got = solve(lp, tail)
    assert s.kernel == "wave per-problem" and s.slack == tail and s.a_cols == (n - m if tail else n)
    assert_plan(s.launch_info(), m, n, tail)
    dbc.assert_matches_oracle(got, wc.oracle(m, n, tail))


@pytest.mark.gpu
@pytest.mark.parametrize("m,n,tail", [(3, 257, False), (113, 257, True), (80, 256, False)])
def test_shapes_without_a_plan_are_declined_and_delegated(m, n, tail):
    """(8, 6) is not compiled for per-problem matrices and (80, 256) without a tail leaves no room for a wave: the entry keeps
    its PYCLLP_E_UNSUPPORTED and its message, and the plugin delegates."""
    import torch
    from pycllp_amd.solvers.hip import Handle, solve_opts
    lp = dbc.make(m, n, tail, B=2)
    dev = torch.device("cuda:0")
    h = Handle(np.ascontiguousarray(lp.A.todense(0)), dev, None)
    a_cols = n - m if tail else n
    t = lambda *shape: torch.zeros(shape, dtype=torch.float64, device=dev)
    out = dict(x=t(2, n), y=t(2, m), z=t(2, n), pobj=t(2), dobj=t(2), status=torch.zeros(2, dtype=torch.int32, device=dev),
               iters=torch.zeros(2, dtype=torch.int32, device=dev))
    with pytest.raises(NotImplementedError, match=r"per-problem dense matrices stop at m = 32, n = 128 \(beyond: "
                                                  r"pycllp_hip_sparse_solve_batch\)"):
        h.solve_batch_dense(None, t(2, m, a_cols), t(2, m), t(2, n), out, solve_opts({}))
    if (m, n) == (80, 256):
        s = solver_registry[NAME](device="cuda:0", hsd=False, autoscale=False)
        lp.init(s)
        assert s._delegate is not None and s._handle is None
        with pytest.raises(RuntimeError):
            s.solve_device(t(2, m, a_cols), t(2, m), t(2, n))


@pytest.mark.gpu
@pytest.mark.parametrize("m,n,tail", [(41, 78, True), (48, 130, False)])
def test_no_stale_image(m, n, tail):
    lp = wc.batch(m, n, tail)
    B = lp.nproblems
    s, got = solve(lp, tail)
    assert_plan(s.launch_info(), m, n, tail)
    dbc.assert_matches_oracle(got, wc.oracle(m, n, tail))
    rev = np.arange(B)[::-1]
    _, back = solve(dbc.reorder(lp, rev), tail)
    same_bits(back, got, ridx=rev)
    _, alone = solve(dbc.reorder(lp, np.array([5])), tail)
    same_bits(alone, got, ridx=np.array([5]))
    # odd LPs with their matrices scaled by 2 (the identity tail is not part of an LP's matrix: it stays)
    data = np.array(lp.A.data)
    scaled = np.asarray(lp.A._cols) < (n - m if tail else n)
    data[1::2] = np.where(scaled, 2.0 * data[1::2], data[1::2])
    A2 = SparseMatrix(np.asarray(lp.A._rows), np.asarray(lp.A._cols), data)
    A2._shape = (m, n)
    from pycllp_amd.lp import EqualityLP
    lp2 = EqualityLP(A2, lp.b.copy(), lp.c.copy(), 0.0)
    _, g2 = solve(lp2, tail)
    r2 = dbc.oracle_each(lp2)
    dbc.assert_matches_oracle(g2, r2)
    same_bits(g2, got, idx=np.arange(0, B, 2), ridx=np.arange(0, B, 2))
    assert (g2["pobj"][1::2] != got["pobj"][1::2]).all()


@pytest.mark.gpu
def test_plugin():
    m, n, tail = 41, 78, True
    lp = wc.batch(m, n, tail)
    s, got = solve(lp, tail)
    assert s.kernel == "wave per-problem"
    A = densify_batch(lp.A._rows, lp.A._cols, lp.A.data, m, s.a_cols)
    out = s.solve_device(A, lp.b, lp.c)
    same_bits({k: out[k].cpu().numpy() for k in KEYS}, got)
    # NO_SLACK_PATH: the full matrices, identity included, on the plan with every column in the image
    s2, g2 = solve(lp, False, flags=_native.FLAG_NO_SLACK_PATH)
    assert s2.kernel == "wave per-problem" and s2.a_cols == n and not s2.slack
    assert_plan(s2.launch_info(), m, n, False)
    dbc.assert_matches_oracle(g2, wc.oracle(m, n, tail))
    # no LDS plan: delegated, as before
    big = dbc.make(80, 256, False, B=3)
    s3 = solver_registry[NAME](device="cuda:0", hsd=False, autoscale=False)
    big.init(s3)
    assert s3._delegate is not None and s3._handle is None
    try:                                  # (the sparse path serves such a batch on its block kernel or, as here, refuses it)
        big.solve(s3)
        assert s3.kernel == "delegated"
    except NotImplementedError:
        assert s3.kernel is None


@pytest.mark.gpu
def test_plugin_resolves_an_infeasible_lp():
    m, nd, B, bad = 40, 20, 30, 17
    base = dbc.standard_batch(m, nd, B, seed=31)
    b = base.b.copy()
    b[bad] = -b[bad]                                          # A > 0, x >= 0, A x <= b < 0: infeasible
    lp = dbc.reorder(base, np.arange(B))
    lp.b = b
    s0, raw = solve(lp, True)                                 # hsd=False: the kernel's verdict
    assert s0.kernel == "wave per-problem"
    assert raw["status"][bad] != 0 and (np.delete(raw["status"], bad) == 0).all()
    s, got = solve(lp, True, hsd="auto")
    assert s.kernel == "wave per-problem" and got["status"][bad] == 2
    rest = np.delete(np.arange(B), bad)
    same_bits(got, raw, idx=rest, ridx=rest)


@pytest.mark.gpu
def test_trajectory():
    """x, y, z and the objectives of every LP after k = 1, 2, 4, 8 iterations against the oracle at the same k (deviation and
    tolerance of tests/trajectory.py).  At the iteration limit the wave kernel returns, as the oracle does, the objectives of
    the iterate before the last step: the reference's are the oracle's own."""
    import trajectory as tj
    m, n, tail = wc.TRAJECTORY_POINT
    lp = wc.trajectory_lp()
    s = solver_registry[NAME](device="cuda:0", hsd=False, autoscale=False, reserve_cus=two_workgroups(m, n, tail))
    lp.init(s)
    assert s._wave
    A = densify_batch(lp.A._rows, lp.A._cols, lp.A.data, m, n - m)
    for k in tj.K:
        out = s.solve_device(A, lp.b, lp.c, max_iter=k)
        got = {q: out[q].cpu().numpy() for q in KEYS}
        ref, tol = wc.trajectory_reference(k), wc.trajectory_tolerance(k)
        dev = {q: tj.deviation(got[q], ref[q]) for q in tj.QUANTITIES}
        print("k=%d %s" % (k, "  ".join("%s %.1e (tol %.1e)" % (q, dev[q].max(), tol[q]) for q in tj.QUANTITIES)))
        for side in (got, ref):
            assert (side["status"] == 5).all() and (side["iters"] == k).all(), (k, side["status"], side["iters"])
        for q in tj.QUANTITIES:
            assert dev[q].shape == (lp.nproblems,)
            assert dev[q].max() <= tol[q], "after %d iterations: %s off by %.2e on LP %d (bound %.2e)" % (
                k, q, dev[q].max(), int(dev[q].argmax()), tol[q])
    assert_plan(s.launch_info(), m, n, tail)


@pytest.mark.gpu
def test_nonfinite_data():
    m, n, tail = 41, 78, True
    lp = wc.batch(m, n, tail)
    B = lp.nproblems
    s, clean = solve(lp, tail)
    A = densify_batch(lp.A._rows, lp.A._cols, lp.A.data, m, s.a_cols)
    b = lp.b.copy()
    A[3, 7, 11] = np.nan
    b[20, 5] = np.inf
    out = s.solve_device(A, b, lp.c)
    got = {k: out[k].cpu().numpy() for k in KEYS}
    assert got["status"][3] == _native.STATUS_NUMERICAL and got["status"][20] == _native.STATUS_NUMERICAL
    rest = np.delete(np.arange(B), [3, 20])
    same_bits(got, clean, idx=rest, ridx=rest)


# ---- footprint ----------------------------------------------------------------------------------------------------------------
OPTIONAL = ("y", "z", "pobj", "dobj", "iters")


class Footprint(object):
    def __init__(self, m, n, tail, B, reserve):
        import torch
        from pycllp_amd.solvers.hip import Handle
        self.lp = lp = dbc.make(m, n, tail, B=B)
        self.m, self.n, self.B, self.a_cols = m, n, B, (n - m if tail else n)
        self.handle = Handle(np.ascontiguousarray(lp.A.todense(0)), torch.device("cuda:0"), None)
        self.A = densify_batch(lp.A._rows, lp.A._cols, lp.A.data, m, self.a_cols)
        self.flags = 0 if tail else _native.FLAG_NO_SLACK_PATH
        self.reserve = reserve

    def specs(self):
        B, m, n = self.B, self.m, self.n
        I32 = fp.I32
        return [fp.inp("A", self.A), fp.inp("b", self.lp.b), fp.inp("c", self.lp.c), fp.out("x", (B, n)), fp.out("y", (B, m)),
                fp.out("z", (B, n)), fp.out("pobj", (B,)), fp.out("dobj", (B,)), fp.out("status", (B,), I32),
                fp.out("iters", (B,), I32)]

    def call(self, placement, null=(), a_cols=None, flags=0, expect=0, untouched=()):
        import torch
        mem = fp.Arena(self.specs(), placement, torch.device("cuda:0"), null=null)
        o = _native.default_opts(flags=self.flags | flags, reserve_cus=self.reserve)
        rc = fp.call("dense_solve_batch", mem.arrays(), self.B, handle=self.handle, opts=o,
                     a_cols=self.a_cols if a_cols is None else a_cols)
        assert rc == expect, (rc, _native.lib().pycllp_hip_last_error())
        mem.check(outputs_written=(rc == 0), untouched=untouched)
        return mem.results()


@pytest.mark.gpu
@pytest.mark.parametrize("batch", ["B=3", "hand-over"])
@pytest.mark.parametrize("m,n,tail", [(33, 38, True), (49, 54, False)])
def test_footprint(m, n, tail, batch):
    shape, per_wave, waves = wc.plan(m, n, tail)
    one_cu = ncu() - 1
    slots = waves * (2 if wc.doubled(shape, per_wave, waves) else 1)           # one compute unit left to the solve
    B = 3 if batch == "B=3" else 2 * slots + 3
    run = Footprint(m, n, tail, B, one_cu)
    ref = run.call("aligned")
    info = run.handle.launch_info()
    assert info.get("kernel") == "wave" and info.get("wave_shape") == shape and info["block"] == 64 * waves, info
    assert info["grid"] * waves == (slots if batch == "hand-over" else waves) and B > (0 if batch == "B=3" else slots)
    dbc.assert_matches_oracle(ref, dbc.oracle_each(run.lp))
    same_bits(run.call("natural"), ref)
    kept = [k for k in KEYS if k not in OPTIONAL]
    same_bits(run.call("natural", null=OPTIONAL), ref, keys=kept)
    for k in ("z", "y"):
        same_bits(run.call("aligned", null=(k,)), ref, keys=[q for q in KEYS if q != k])
    # a wrong a_cols: refused, nothing touched
    run.call("natural", a_cols=run.a_cols + 1, expect=-1)
    assert b"a_cols = %d, expected %d" % (run.a_cols + 1, run.a_cols) in _native.lib().pycllp_hip_last_error()
    # PYCLLP_FLAG_FORCE_GUARD_PATH: every LP is deferred and ends NUMERICAL with status its only output
    forced = run.call("aligned", flags=_native.FLAG_FORCE_GUARD_PATH, untouched=("x", "y", "z", "pobj", "dobj", "iters"))
    assert (forced["status"] == _native.STATUS_NUMERICAL).all()
