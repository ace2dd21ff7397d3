"""Upper bounds on per-problem DENSE matrices beyond the lane-group kernels: the wave kernel ipm_wreg_bounded_dapa_kernel
(csrc/ipm_wreg_bounded.inc on WReg<MB, NQ, true, true>, compiled by ipm_wreg_bddapa.hip), its plan (WPLAN_BOUNDED_DENSE_PA), the
entry pycllp_hip_dense_solve_batch_bounded on a handle beyond m = 32 / n = 128, and hip_general_batch_primal_normal with
dense_wave=True.  The reference of every numerical comparison is tests/bounded_twin.solve run LP by LP with that LP's own
matrix; bounds are the project's (general_batch_cases.assert_parity): status equal and 0, iterations within 1, objectives 1e-9
relative, x at rtol 1e-5 / atol 1e-7; HiGHS at 1e-8 on one point.

test_trajectory and test_shared_matrix_twin append what they measured to the file PYCLLP_TRAJECTORY_REPORT names
(profiles/bounded_wave_dense_perA/trajectory.txt)."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

import footprint as fp
import general_batch_cases as gbc
import general_batch_wave_cases as wc
import test_plan_host as tph
from conftest import ROOT
from pycllp_amd import _native
from pycllp_amd.lp import GeneralLP, SparseMatrix
from pycllp_amd.solvers import solver_registry
from pycllp_amd.solvers.general import subset
from test_general_solver import highs_general, make_general

NAME = "hip_general_batch_primal_normal"
ENTRY = "pycllp_hip_dense_solve_batch_bounded"
KEYS = gbc.OUTPUTS
CSRC = os.path.join(ROOT, "pycllp_amd", "csrc")
REJECTED_FLAGS = (_native.FLAG_HSD, _native.FLAG_PREDCORR, _native.FLAG_WARM_START, _native.FLAG_WAVE_KERNEL,
                  _native.FLAG_NO_SLACK_PATH)
KERNEL = "bounded wave per-problem"


def report(line):
    print(line)
    path = os.environ.get("PYCLLP_TRAJECTORY_REPORT")
    if path:
        with open(path, "a") as f:
            f.write(line + "\n")


# ---- CPU ------------------------------------------------------------------------------------------------------------------
def kind8(mk, N, max_lds=wc.MAX_LDS):
    A = wc.form_matrix(mk, N)
    rc, p, _ = tph.build_plan(wc.PLAN_KIND, A, max_lds)
    if rc == 0:
        tph.check_wave_invariants(p, A.nnz, (mk, N))
    return rc, p


@pytest.mark.parametrize("point", sorted(wc.TABLE) + [pt for pts in wc.POINTS.values() for pt in pts], ids=str)
def test_plan_kind_8_follows_the_rule(point):
    """Fails without the feature: pycllp_hip_debug_plan answers -1 to kind 8."""
    mk, N = point
    want = wc.plan(mk, N)
    if point in wc.TABLE:
        assert want == wc.TABLE[point]
    rc, p = kind8(mk, N)
    assert rc == 0 and want is not None, (rc, want)
    shape, per_wave, waves = want
    assert (p["mb"], p["nq"]) == shape and 8 * p["wave_doubles"] == per_wave and p["wpb"] == waves
    assert p["lds_bytes"] == waves * per_wave and p["o_wave"] == 0 and p["o_img"] == 0
    assert p["variant"] == 2 and p["pa"] == 1 and p["bd"] == 1 and p["nd"] == N - mk
    assert p["img_rows"] == (mk + 7) // 8 * 8 and p["as"] == (N - mk + 15) // 16 * 16 + 1
    # t and s start behind the image at an even offset (16-byte aligned), and end with the wave's area
    ts = wc.dwc.wave_doubles(*shape) + p["img_rows"] * p["as"]
    assert ts % 2 == 0 and ts + 2 * 64 * shape[1] == p["wave_doubles"]
    # the plan without bounds (kind 5) is this one less t and s
    rc5, p5, _ = tph.build_plan(tph.DENSE_PA, wc.form_matrix(mk, N))
    if rc5 == 0:
        assert p5["wave_doubles"] + 2 * 64 * shape[1] == p["wave_doubles"] and (p5["mb"], p5["nq"]) == shape


def test_plan_kind_8_declines():
    assert wc.plan(100, 257) is None and kind8(100, 257)[0] == 1                    # no shape with 64 NQ >= 257
    assert wc.plan(129, 200) is None and kind8(129, 200)[0] == 1
    per_wave = wc.TABLE[(128, 256)][1]
    assert kind8(128, 256, per_wave)[0] == 0 and wc.plan(128, 256, per_wave)[2] == 1
    assert kind8(128, 256, per_wave - 8)[0] == 1 and wc.plan(128, 256, per_wave - 8) is None
    assert wc.MAX_LDS - per_wave == 2944
    rc, p = kind8(48, 176, 2 * wc.TABLE[(48, 176)][1] - 8)                           # one byte count short of two waves: one
    assert rc == 0 and p["wpb"] == 1
    for kind in range(8):                                                            # kinds 0 .. 7 keep their meaning
        assert tph.build_plan(kind, wc.form_matrix(10, 160))[0] in (0, 1)
    assert tph.entry()(9, 1, 1, 0, None, None, None, wc.MAX_LDS, None, None) == -1


def test_plan_check_builds_and_passes(tmp_path):
    """The stand-alone program over the plan headers (no GPU), plain and under the host sanitizers."""
    for extra in ("", "-Xarch_host -fsanitize=address,undefined"):
        out = str(tmp_path) + "/"
        subprocess.check_call(["make", "-s", "-C", CSRC, "OUT=" + out, "EXTRA=" + extra, "plan_check"])
        r = subprocess.run([out + "plan_check"], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, universal_newlines=True)
        assert r.returncode == 0 and "0 checks failed" in r.stdout, r.stdout[-2000:]
    assert "kind <= WPLAN_BOUNDED_DENSE_PA" in open(os.path.join(CSRC, "plan_check.hip")).read()


def test_shape_list_unit_and_makefile():
    src = {f: open(os.path.join(CSRC, f)).read() for f in ("wreg.h", "wreg_plan.h", "ipm_wreg_bddapa.hip", "ipm_wreg_bdpa.hip",
                                                           "ipm_wreg_bounded.inc", "ipm_wreg.hip", "Makefile")}
    shapes = lambda name: [tuple(map(int, s)) for s in re.findall(
        r"X\((\d+),\s*(\d+)\)", re.search(r"#define %s\(X\)(.*)" % name, src["wreg.h"]).group(1))]
    assert shapes("WREG_BDDAPA_SHAPES") == wc.WAVE_BDDAPA_SHAPES
    assert shapes("WREG_DAPA_SHAPES") == wc.dwc.WAVE_DAPA_SHAPES and shapes("WREG_DA_SHAPES") == wc.dwc.WAVE_DA_SHAPES
    unit = src["ipm_wreg_bddapa.hip"]
    assert unit.index("#define PYCLLP_WREG_BOUNDED_DAPA") < unit.index('#include "ipm_wreg_bounded.inc"')
    assert "WREG_TABLE(kWBDDAPA, WREG_BDDAPA_SHAPES," in unit and "ipm_wreg_bounded_dapa_kernel<MB, NQ>" in unit
    assert "PYCLLP_WREG_BOUNDED_DAPA" not in src["ipm_wreg_bdpa.hip"]
    text = src["ipm_wreg_bounded.inc"]
    assert "WReg<MB, NQ, true, true> w;" in text and "G::WAVE_D(NQ) + T.img_rows * T.as" in text
    assert re.search(r"#if defined\(PYCLLP_WREG_BOUNDED_PA\) \|\| defined\(PYCLLP_WREG_BOUNDED_DAPA\)\s*\n\s*load_lp_values\(", text)
    assert "template <int MB, int NQ, bool DA>" in text          # the shared-A kernel keeps its template: no new argument
    assert "WPLAN_DENSE_PA_KEEP,\n                    WPLAN_BOUNDED_DENSE_PA };" in src["wreg_plan.h"]        # appended last
    objs = re.search(r"OBJS := (.*?)\n\n", src["Makefile"], re.S).group(1)
    assert "ipm_wreg_bddapa.o" in objs.split()
    # the scheduling flags of ipm_wreg_bdpa.o: none of its own
    for line in src["Makefile"].splitlines():
        if "SCHED :=" in line and ":" in line.split("SCHED")[0]:
            assert "ipm_wreg_bddapa" not in line and "ipm_wreg_bdpa" not in line


def _entry_args(h, B, u, flags):
    o = _native.default_opts(flags=flags)
    return (h, B, 8, 5, 8, 8, u, 8, 8, 8, 8, 8, 8, 8, 8, ctypes.byref(o), None)


def test_entry_checks_its_arguments_before_any_device_call():
    f = getattr(_native.lib(), ENTRY)
    buf = np.zeros(64)
    fake = buf.ctypes.data                  # never dereferenced: every argument check comes before the handle is read
    assert f(*_entry_args(None, 1, 8, 0)) == -1
    assert f(*_entry_args(fake, -1, 8, 0)) == -1
    assert f(*_entry_args(fake, 0, None, 0)) == -1 and f(*_entry_args(fake, 1, None, 0)) == -1
    assert f(*_entry_args(fake, 1, 8, _native.FLAG_AUTOSCALE | _native.FLAG_AUTOSCALE_PER_LP)) == -1
    for flag in REJECTED_FLAGS:
        assert f(*_entry_args(fake, 1, 8, flag)) == -1
        assert b"not available with upper bounds on per-problem matrices" in _native.lib().pycllp_hip_last_error()
    header = open(os.path.join(ROOT, "include", "pycllp_hip.h")).read()
    at = header.index("int " + ENTRY)
    assert "ipm_wreg_bddapa.hip" in header[at - 2500:at]


def dense_structure(mk, n, B=3, seed=5, shared=False):
    return make_general(mk, n, B, seed, per_problem_A=not shared, fixed=1, mixed_u=True, kinds=gbc.kinds(mk))


def fits(glp, **kw):
    S = solver_registry[NAME]
    return S(**kw).native_fits(glp, S._form(glp)[0])


def test_dense_wave_option():
    S = solver_registry[NAME]
    assert S().dense_wave is False and S(dense_wave=True).dense_wave is True
    for bad in (1, "yes", None, 0):
        with pytest.raises(ValueError, match="dense_wave"):
            S(dense_wave=bad)
    assert "dense_wave" not in S(dense_wave=True).options
    g = dense_structure(40, 30)
    assert not fits(g) and fits(g, dense_wave=True)                                  # 40 kept rows x 30 columns
    assert not S.native_fits(g, S._form(g)[0])                                       # (the class's rule is the default's)
    small = dense_structure(20, 30)
    assert fits(small) and fits(small, dense_wave=True)                              # the lane-group range: as before
    assert not fits(dense_structure(40, 30, shared=True), dense_wave=True)           # a shared A
    hole = GeneralLP(SparseMatrix(g.A._rows[1:], g.A._cols[1:], g.A.data[:, 1:]), g.b, g.c, a=g.a, l=g.l, u=g.u, f=g.f)
    hole.A._shape = (40, 30)
    assert not fits(hole, dense_wave=True)                                           # a hole in the structure
    dup = GeneralLP(SparseMatrix(np.r_[g.A._rows, g.A._rows[:1]], np.r_[g.A._cols, g.A._cols[:1]],
                                 np.c_[g.A.data, g.A.data[:, :1]]), g.b, g.c, a=g.a, l=g.l, u=g.u, f=g.f)
    dup.A._shape = (40, 30)
    assert not fits(dup, dense_wave=True)                                            # a duplicate entry
    assert fits(dense_structure(128, 128), dense_wave=True)                          # the cap: m' = 128, N = 256
    assert not fits(dense_structure(129, 100), dense_wave=True)                      # m' = 129
    assert not fits(dense_structure(100, 157), dense_wave=True)                      # N = 257
    assert not fits(dense_structure(20, 100), dense_wave=True)                       # m' <= 32, 96 < n, N <= 128: a lane-group handle
    assert fits(dense_structure(20, 109), dense_wave=True)                           # ... N = 129: beyond it


def test_registry_still_has_seven_hip_plugins():
    assert len([k for k in solver_registry if k.startswith("hip_")]) == 7


def test_twin_lp_by_lp_matches_highs():
    glp = wc.make(40, 70, 4, 13)                                                     # 40 kept rows x 30 columns
    r = wc.twin_of(glp)
    assert (r["status"] == 0).all(), r["status"]
    for k in range(glp.nproblems):
        ref, _ = highs_general(glp, k)
        assert gbc.rel(r["pobj"][k], ref) <= 1e-8 and gbc.rel(r["dobj"][k], ref) <= 1e-8


# ---- GPU ------------------------------------------------------------------------------------------------------------------
def two_workgroups():
    import torch
    return torch.cuda.get_device_properties(0).multi_processor_count - 2


def solve(glp, **kw):
    s = solver_registry[NAME](device="cuda:0", **dict(dict(hsd=False, autoscale=False, dense_wave=True,
                                                          reserve_cus=two_workgroups()), **kw))
    glp.init(s)
    glp.solve(s)
    return s, gbc.plugin_results(s)


def assert_plan(info, mk, N):
    shape, per_wave, waves = wc.plan(mk, N)
    assert info.get("kernel") == "wave" and info.get("variant") == "dense image" and info.get("wave_shape") == shape, info
    assert info["block"] == 64 * waves and info["lds_bytes"] == waves * per_wave and "group_shape" not in info, info


@pytest.mark.gpu
@pytest.mark.parametrize("case", wc.EVERY, ids=[wc.every_id(c) for c in wc.EVERY])
def test_every_instantiation(case):
    shape, which = case
    mk, N = wc.POINTS[shape][which]
    assert wc.dwc.first_covering(wc.WAVE_BDDAPA_SHAPES, mk, N) == shape and not (mk <= 32 and N <= 128)
    glp = wc.make(mk, N)
    assert glp.nproblems == 37 and np.isinf(glp.u).any() and (glp.u == glp.l).any() and np.isfinite(glp.u).any()
    s, got = solve(glp)
    info = s.launch_info()
    assert s.kernel == KERNEL and s.conversion == "device"
    assert_plan(info, mk, N)
    # two compute units (two workgroups; four where solve_grid puts two on each): every wave takes several LPs
    assert info["grid"] <= 4 and glp.nproblems > 2 * info["grid"] * (info["block"] // 64), info
    # the twin LP by LP; beyond 64 x 256 on a sample that holds the last LPs (those that entered refilled waves)
    idx = None if mk * N <= 64 * 256 else np.unique(np.r_[0:37:3, 33:37])
    gbc.assert_parity(got, wc.twin(mk, N) if idx is None else wc.twin_of(glp, idx), idx)
    assert (got["status"] == 0).all()
    for name, res in zip(("primal", "dual", "bound", "gap"), gbc.residuals(glp, got)):
        assert res.max() < 1e-8, (name, res.max(), int(res.argmax()))


@pytest.mark.gpu
def test_the_cap_runs_with_one_wave():
    glp = wc.make(128, 256)
    s, got = solve(glp)
    info = s.launch_info()
    assert info["block"] == 64 and info["lds_bytes"] == 160896 and info["wave_shape"] == (8, 4), info
    assert (got["status"] == 0).all()


def device_run(s, glp, idx=None, **options):
    """The kernel through solve_device on the LPs ``idx`` of ``glp``, in the bounded form's variables."""
    blp, _ = (glp if idx is None else subset(glp, idx)).to_bounded_equality_form()
    out = s.solve_device(s.bounded_matrices(blp), blp.b, blp.c, blp.u, **options)
    return {k: out[k].cpu().numpy() for k in KEYS}, blp


@pytest.mark.gpu
def test_no_stale_image_t_or_s():
    mk, N = 40, 140                                            # (3, 4): pad rows 40..47 and pad columns 100..111 of the image
    glp = wc.make(mk, N)
    B = glp.nproblems
    s, _ = solve(glp)
    fwd, _ = device_run(s, glp)
    assert (fwd["status"] == 0).all()
    rev, _ = device_run(s, glp, np.arange(B)[::-1])
    for k in KEYS:
        assert np.array_equal(rev[k], fwd[k][::-1]), k
    one, _ = device_run(s, glp, np.array([5]))
    for k in KEYS:
        assert np.array_equal(one[k][0], fwd[k][5]), k
    factor = np.where(np.arange(B) % 2 == 1, 2.0, 1.0)
    g2 = gbc.scaled_rows(glp, factor)
    mixed, blp2 = device_run(s, g2)
    odd, even = np.arange(1, B, 2), np.arange(0, B, 2)
    gbc.assert_parity(mixed, gbc.twin_each(blp2, odd), odd)
    for k in KEYS:
        assert np.array_equal(mixed[k][even], fwd[k][even]), k
    assert not np.array_equal(mixed["y"][odd], fwd["y"][odd])


@pytest.mark.gpu
def test_shared_matrix_twin():
    """All matrices equal: within the project's bounds of the shared-A bounded wave kernel (pycllp_hip_sparse_solve_bounded) on the
    same A^; whether the bits are equal is reported, not asserted."""
    import scipy.sparse as sp
    import torch
    from pycllp_amd.solvers.hip import Handle, bounded_outputs, solve_opts
    mk, n = 48, 128
    blp, _ = make_general(mk, n, 37, seed=12, fixed=1, mixed_u=True, kinds=gbc.kinds(mk)).to_bounded_equality_form()
    dev = torch.device("cuda:0")
    A0 = np.ascontiguousarray(blp.A.todense())
    B, N = blp.nproblems, blp.ncols
    t = lambda a: torch.as_tensor(np.ascontiguousarray(a), device=dev)
    b, c, u = t(blp.b), t(blp.c), t(blp.u)
    shared, batch = bounded_outputs(B, mk, N, dev), bounded_outputs(B, mk, N, dev)
    o = solve_opts({}, reserve_cus=two_workgroups())
    hs = Handle(sp.csr_matrix(A0), dev, None)
    hs.solve_bounded(None, b, c, u, shared, o)
    torch.cuda.synchronize()
    assert hs.launch_info()["wave_shape"] == (3, 4) and hs.launch_info()["variant"] == "dense image"
    hd = Handle(A0, dev, None)
    hd.solve_batch_bounded(None, t(np.broadcast_to(A0[:, :n], (B, mk, n))), b, c, u, batch, o)
    torch.cuda.synchronize()
    assert_plan(hd.launch_info(), mk, N)
    sh, ba = ({k: v.cpu().numpy() for k, v in r.items()} for r in (shared, batch))
    report("all matrices equal (48 x 176): bit-exact with the shared-A bounded dense-image kernel: %s"
           % {k: bool(np.array_equal(sh[k], ba[k])) for k in KEYS})
    gbc.assert_parity(ba, sh)


@pytest.mark.gpu
@pytest.mark.parametrize("B", [0, 1, 2, 63])
def test_batch_sizes(B):
    full = wc.make(33, 133, 63, 23)
    blp, _ = subset(full, np.arange(max(B, 1))).to_bounded_equality_form()
    s = solver_registry[NAME](device="cuda:0", hsd=False, autoscale=False, dense_wave=True)
    full.init(s)
    assert s._handle is not None
    A = s.bounded_matrices(blp)[:B]
    out = s.solve_device(A, blp.b[:B], blp.c[:B], blp.u[:B])
    got = {k: out[k].cpu().numpy() for k in KEYS}
    assert got["x"].shape == (B, 133) and got["s"].shape == (B, 133) and got["y"].shape == (B, 33)
    if B:
        assert_plan(s.launch_info(), 33, 133)
        gbc.assert_parity(got, gbc.twin_each(blp))


@pytest.mark.gpu
@pytest.mark.parametrize("sb,sc", [(1e3, 1e-3), (1e-3, 1e3)])
def test_autoscale(sb, sc):
    glp = gbc.scaled_data(wc.make(40, 140, 20, 22), sb, sc)
    ref = wc.twin_of(glp, autoscale=True)
    for kw in (dict(autoscale=True), dict(autoscale="auto"), dict(autoscale="per_lp")):
        s, got = solve(glp, **kw)
        assert s.kernel == KERNEL
        gbc.assert_parity(got, ref)


@pytest.mark.gpu
def test_trajectory():
    """x, y, z, s and the objectives of every LP (bounded form's variables) after k = 1, 2, 4, 8 iterations against the twin at
    the same k, LP by LP with that LP's matrix (deviation and tolerance of tests/trajectory.py), at one (3, 4) point."""
    import trajectory as tj
    glp = wc.trajectory_lp()
    s = solver_registry[NAME](device="cuda:0", hsd=False, autoscale=False, dense_wave=True)
    glp.init(s)
    for k in tj.K:
        got, _ = device_run(s, glp, max_iter=k)
        assert s.launch_info()["wave_shape"] == (3, 4)
        ref, tol = wc.trajectory_reference(k), wc.trajectory_tolerance(k)
        dev = {q: tj.deviation(got[q], ref[q]) for q in gbc.TRAJ_QUANTITIES}
        report("%dx%d k=%d %s" % (wc.TRAJECTORY_POINT + (k, "  ".join("%s %.1e (tol %.1e)" % (q, dev[q].max(), tol[q])
                                                                         for q in gbc.TRAJ_QUANTITIES))))
        for side in (got, ref):
            assert (side["status"] == 5).all() and (side["iters"] == k).all(), (k, side["status"], side["iters"])
        for q in gbc.TRAJ_QUANTITIES:
            assert dev[q].shape == (glp.nproblems,)
            assert dev[q].max() <= tol[q], "after %d iterations: %s off by %.2e on LP %d (bound %.2e)" % (
                k, q, dev[q].max(), int(dev[q].argmax()), tol[q])


@pytest.mark.gpu
def test_plugin_entries_agree():
    """solve, solve_device and solve_device_general on one batch: the same kernel, the same bits."""
    glp = wc.make(40, 70, 24, 9)                               # 40 kept rows x 30 columns
    s, got = solve(glp)
    assert s.kernel == KERNEL
    gbc.assert_parity(got, wc.twin(40, 70, 24, 9))
    blp, bmap = glp.to_bounded_equality_form()
    dev, _ = device_run(s, glp, reserve_cus=two_workgroups())
    mapped = gbc.general_results(bmap, blp, dev)
    for k in KEYS:
        assert np.array_equal(mapped[k], got[k]), k
    out = s.solve_device_general(np.asarray(glp.A.data), glp.a, glp.b, glp.c, glp.l, glp.u, glp.f, reserve_cus=two_workgroups())
    gen = {k: v.cpu().numpy() for k, v in out.items()}
    assert (gen["invalid"] == 0).all() and s.kernel == KERNEL
    for k, q in (("x", "x"), ("y", "y"), ("z", "z"), ("s", "s"), ("status", "status"), ("iters", "iters")):
        assert np.array_equal(gen[k], got[q]), k
    assert gbc.rel(gen["primal_obj"], got["pobj"]).max() < 1e-12 and gbc.rel(gen["dual_obj"], got["dobj"]).max() < 1e-12
    # the default plugin on the same batch: the expansion, as before, and no solve_device
    d = solver_registry[NAME](device="cuda:0")
    glp.init(d)
    glp.solve(d)
    assert d.kernel == "expanded" and d.dense_wave is False
    with pytest.raises(RuntimeError, match="solve_device"):
        d.solve_device(np.zeros((1, 40, 30)), np.zeros((1, 40)), np.zeros((1, 70)), np.zeros((1, 70)))


@pytest.mark.gpu
def test_plugin_resolves_an_infeasible_lp():
    B, bad = 24, 17
    base = wc.make(40, 70, B, 9)
    b = base.b.copy()
    b[bad, 0] = base.A.todense(bad)[0] @ base.l[bad] - 1.0      # row 0 (positive coefficients) below what x >= l allows
    glp = GeneralLP(base.A, b, base.c, a=base.a, l=base.l, u=base.u, f=base.f)
    _, raw = solve(glp)                                        # hsd=False: the kernel's verdict
    assert raw["status"][bad] != 0 and (np.delete(raw["status"], bad) == 0).all(), raw["status"]
    s, got = solve(glp, hsd="auto")
    assert s.kernel == KERNEL and got["status"][bad] == 2
    rest = np.delete(np.arange(B), bad)
    for k in KEYS:
        assert np.array_equal(got[k][rest], raw[k][rest]), k


@pytest.mark.gpu
def test_default_plugin_refuses_workload_a_as_today():
    glp = wc.make(48, 176, 4)
    with pytest.raises(NotImplementedError):
        d = solver_registry[NAME](device="cuda:0")
        glp.init(d)
        glp.solve(d)
    s, got = solve(glp)
    assert s.kernel == KERNEL
    gbc.assert_parity(got, wc.twin(48, 176, 4))


@pytest.mark.gpu
def test_non_finite_data():
    glp = wc.make(40, 140)
    s, _ = solve(glp)
    clean, blp = device_run(s, glp)
    A = s.bounded_matrices(blp).copy()
    b = blp.b.copy()
    A[7, 11, 3] = np.nan
    b[20, 5] = np.inf
    out = s.solve_device(A, b, blp.c, blp.u)
    got = {k: out[k].cpu().numpy() for k in KEYS}
    assert got["status"][7] == 3 and got["status"][20] == 3, got["status"]
    rest = np.delete(np.arange(glp.nproblems), [7, 20])
    for k in KEYS:
        assert np.array_equal(got[k][rest], clean[k][rest]), k


@pytest.mark.gpu
@pytest.mark.parametrize("B", [3, 11])
def test_footprint(B):
    """Guard bands around every array in both placements, NULL optional outputs, a wrong a_cols refused with nothing touched;
    B = 3 and B = 11 > the 8 waves of two workgroups."""
    import torch
    import test_memory_footprint as tmf
    from pycllp_amd.solvers.hip import Handle
    mk, N = 33, 133
    blp, _ = wc.make(mk, N, 11, 77).to_bounded_equality_form()
    n = N - mk
    dev = torch.device("cuda", 0)
    h = Handle(np.ascontiguousarray(blp.A.todense(0)), dev, None)
    ins = dict(A=np.stack([blp.A.todense(k)[:, :n] for k in range(B)]), b=blp.b[:B], c=blp.c[:B], u=blp.u[:B])
    entry = "dense_solve_batch_bounded"
    specs = lambda: tmf.specs_of(entry, ins, B, mk, N)
    outs, optional = fp.OUTPUTS[entry], fp.ENTRIES[entry][3]

    def call(mem, a_cols=n):
        o = _native.default_opts(reserve_cus=two_workgroups())
        return fp.call(entry, mem.arrays(), B, handle=h, opts=o, a_cols=a_cols)

    plain = fp.Plain(specs(), dev)
    assert call(plain) == 0, _native.lib().pycllp_hip_last_error()
    plain.check()
    ref = plain.results()
    info = h.launch_info()
    assert_plan(info, mk, N)
    assert B == 3 or B > info["grid"] * (info["block"] // 64)
    gbc.assert_parity(ref, gbc.twin_each(blp, range(B)))
    for placement in ("aligned", "natural"):
        mem = fp.Arena(specs(), placement, dev)
        assert call(mem) == 0
        mem.check()
        tmf.same_bits(mem.results(), ref, outs, placement)
    mem = fp.Arena(specs(), "natural", dev, null=optional)
    assert call(mem) == 0
    mem.check()
    tmf.same_bits(mem.results(), ref, [k for k in outs if k not in optional], "all optional outputs NULL")
    for k in ("z", "y", "s"):
        mem = fp.Arena(specs(), "aligned", dev, null=(k,))
        assert call(mem) == 0
        mem.check()
        tmf.same_bits(mem.results(), ref, [q for q in outs if q != k], "%s NULL" % k)
    for a_cols in (N, n - 1):
        mem = fp.Arena(specs(), "natural", dev)
        assert call(mem, a_cols) == -1 and b"expected %d" % n in _native.lib().pycllp_hip_last_error()
        mem.check(outputs_written=False)
    h.free()


@pytest.mark.gpu
def test_entry_declines_what_it_cannot_serve():
    """N = 257 has no plan, and the lane-group sliver stays declined (the sparse entry's refusal of a dense 48 x 176 structure is
    pinned by test_sparse_general_batch)."""
    import torch
    from pycllp_amd.solvers.hip import Handle
    dev = torch.device("cuda", 0)
    A = np.ascontiguousarray(wc.form_matrix(40, 257).toarray())
    h = Handle(A, dev, None)
    with pytest.raises(NotImplementedError, match="m = 128, n = 256"):
        h.plan_batch_bounded(None, 217)
    h.free()
    A = np.ascontiguousarray(wc.form_matrix(20, 120).toarray())      # m' <= 32, n = 100 > 96, N <= 128: a lane-group handle
    h = Handle(A, dev, None)
    with pytest.raises(NotImplementedError, match=r"\[A_dense \| I\]"):
        h.plan_batch_bounded(None, 100)
    h.free()
