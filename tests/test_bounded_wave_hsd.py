"""Bounded LPs on the homogeneous self-dual embedding, on the wavefront-per-LP kernel: ipm_wreg_bounded_hsd_kernel
(csrc/ipm_wreg_bdhsd.inc), its entry pycllp_hip_sparse_solve_bounded_hsd and ``hsd='device'`` of the two shared-A general plugins
(DESIGN.md section 27).

The references are the CPU twin of section 26 (tests/bounded_hsd_twin.py, which takes any dense A) and HiGHS; the fixtures and
their cached references are tests/bounded_wave_hsd_cases.py.  The bounds are those of tests/test_bounded_hsd.py, where the
lane-group kernel meets them against the same twin: statuses equal, iterations within 1, objectives of optimal LPs within 1e-9 in
the units of the unscaled batch, certificate ratio at most 1e-7.  The k-iterate bounds follow tests/trajectory.py: the twin's own
spread under NPERM seeded row and column permutations, times FACTOR, floored at FLOOR, capped at CEILING.

CPU: the fixtures' criteria and the plan that serves each; the symbol; the entry's refusals on a fake handle; the plugins' option
checks.  GPU: the kernel against the twin on every fixture (also with every optional output NULL), its iterates, autoscale, few LPs,
repeatability, footprint, a NaN in b; the plugin against HiGHS where the expansion fits and where it does not.
Set PYCLLP_TRAJECTORY_REPORT to a file name to get the measured deviations."""
import ctypes
import os
import re

import numpy as np
import pytest
import scipy.sparse as sp

import bounded_hsd_twin as tw
import bounded_wave_hsd_cases as cs
import footprint as fp
from pycllp_amd import _native
from pycllp_amd.solvers import solver_registry
from test_bounded_hsd import highs_general_status
from test_sparse_general_solver import make_sparse_general

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRY = "pycllp_hip_sparse_solve_bounded_hsd"
NPERM, FACTOR, FLOOR, CEILING = 4, 32.0, 1e-13, 1e-9        # tests/trajectory.py's rule
K = (1, 2, 4)
CERT = 1e-7
GENERAL = ("hip_general_primal_normal", "hip_sparse_general_primal_normal", "hip_general_batch_primal_normal",
           "hip_sparse_general_batch_primal_normal")
SIZES = [f.size for f in cs.FIXTURES]
OUT = fp.BOUNDED_OUT
OPTIONAL = ("y", "z", "s", "pobj", "dobj", "iters")
WAVE_BD = 3              # the bounded plan's kind of pycllp_hip_debug_plan (tests/test_plan_host.py)


def report(lines):
    path = os.environ.get("PYCLLP_TRAJECTORY_REPORT")
    if path:
        with open(path, "a") as fh:
            fh.write("\n".join(lines) + "\n")


def csr(A):
    """A^ as ``HipSparseGeneralPrimalNormalSolver`` hands it to the library."""
    A = sp.csr_matrix(A)
    A.sum_duplicates(); A.eliminate_zeros(); A.sort_indices()
    return A


# ---- CPU: the fixtures ----------------------------------------------------------------------------------------------------
def bounded_plan(A):
    """(return code, variant, (MB, NQ)) of the bounded plan the host builds for ``A``, without a GPU."""
    f = ctypes.CDLL(_native.LIB_PATH).pycllp_hip_debug_plan
    f.restype = ctypes.c_int
    f.argtypes = [ctypes.c_int] * 4 + [ctypes.c_void_p] * 3 + [ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p]
    A = csr(A)
    val, ptr, col = (np.ascontiguousarray(v, dtype=t) for v, t in ((A.data, np.float64), (A.indptr, np.int32), (A.indices, np.int32)))
    scalars, digest = np.zeros(32, dtype=np.int64), np.zeros(1, dtype=np.uint64)
    rc = f(WAVE_BD, A.shape[0], A.shape[1], len(val), val.ctypes.data, ptr.ctypes.data, col.ctypes.data, 160 * 1024,
           scalars.ctypes.data, digest.ctypes.data)
    return rc, {1: "tables", 2: "dense image"}.get(int(scalars[13])), (int(scalars[0]), int(scalars[1]))


@pytest.mark.parametrize("size", SIZES, ids=str)
def test_fixtures_meet_their_criteria(size):
    """The seeds' criteria, on the references alone, and the path each size is there for."""
    A, b, c, u = cs.batch(size)
    ref = cs.twin(size)
    status, _ = cs.highs(size)
    assert np.array_equal(ref["status"], status), (ref["status"], status)
    assert set(status.tolist()) == {0, 2, 4}
    assert (status[0::3] == 0).all() and (status[1::3] == 2).all()
    assert (ref["floored"] == 0).all(), ref["floored"]
    assert ref["iters"].max() <= cs.MAX_TWIN_ITERS, ref["iters"].max()
    assert (np.isinf(u).any(axis=1) & (u == 0).any(axis=1) & (np.isfinite(u) & (u > 0)).any(axis=1)).all() or size == (1, 1)
    f = cs.BY_SIZE[size]
    assert bounded_plan(A) == (0, f.variant, f.shape)
    if f.density is not None:         # structural zeros, two entries per row and one per column at least
        D = A[:, :size[1]] != 0
        assert D.mean() < 2 * f.density and D.sum(axis=1).min() >= 2 and D.sum(axis=0).min() >= 1
    assert (16 * f.shape[0] > 64) == (size == (65, 100))          # MR = 2 at that size alone


# ---- CPU: the entry and the plugins ---------------------------------------------------------------------------------------
def test_symbol_is_declared_and_exported():
    header = open(os.path.join(ROOT, "include", "pycllp_hip.h")).read()
    assert re.search(r"\bint\s+%s\s*\(" % ENTRY, header)
    sig = dict((n, (a, r)) for n, a, r in _native.SIGNATURES)[ENTRY]
    assert ENTRY in _native.EXPORTS and len(sig[0]) == 15      # handle, B, b, c, u, eight outputs, opts, stream
    assert ENTRY in _native.LATER_ENTRIES
    assert hasattr(ctypes.CDLL(_native.LIB_PATH), ENTRY)


def _entry_args(h, B, u, flags):
    o = _native.default_opts(flags=flags)
    return (h, B, 8, 8, u, 8, 8, 8, 8, 8, 8, 8, 8, ctypes.byref(o), None)


REJECTED = ("PREDCORR", "WARM_START", "WAVE_KERNEL", "BLOCK_KERNEL", "NO_SLACK_PATH", "FORCE_GUARD_PATH")


def test_entry_checks_its_arguments_before_the_handle_is_read():
    L = _native.lib()
    f = getattr(L, ENTRY)
    buf = np.zeros(8)                        # 64 bytes, never dereferenced
    fake = buf.ctypes.data
    refused = [(None, 1, 8, 0), (fake, -1, 8, 0), (fake, 1, None, 0),
               (fake, 1, 8, _native.FLAG_AUTOSCALE | _native.FLAG_AUTOSCALE_PER_LP)]
    refused += [(fake, 1, 8, getattr(_native, "FLAG_" + name)) for name in REJECTED]
    refused += [(fake, 1, 8, _native.FLAG_HSD | getattr(_native, "FLAG_" + name)) for name in REJECTED]
    for args in refused:
        assert f(*_entry_args(*args)) == -1, args
        assert ENTRY.encode() in L.pycllp_hip_last_error(), (args, L.pycllp_hip_last_error())
    # ... and pycllp_hip_sparse_solve_bounded still refuses the embedding
    g = L.pycllp_hip_sparse_solve_bounded
    assert g(*_entry_args(fake, 1, 8, _native.FLAG_HSD)) == -1 and b"not available" in L.pycllp_hip_last_error()


def test_device_is_an_option_of_the_two_shared_plugins():
    for name in GENERAL[:2]:
        s = solver_registry[name](hsd="device")
        assert s.hsd_native and s.hsd == "auto"
        assert not solver_registry[name]().hsd_native and solver_registry[name]().hsd == "auto"
        assert solver_registry[name](hsd=False).hsd is False
    for name in GENERAL[2:]:
        with pytest.raises(ValueError):
            solver_registry[name](hsd="device")
    s = solver_registry[GENERAL[0]](hsd="native")            # 'native' behaves as it did on all four
    assert s.hsd_native and s.hsd == "auto"
    for name in GENERAL[1:]:
        with pytest.raises(ValueError):
            solver_registry[name](hsd="native")
    for name in GENERAL:
        with pytest.raises(ValueError):
            solver_registry[name](hsd="yes")
        with pytest.raises(ValueError):
            solver_registry[name](hsd=True)


# ---- GPU: the kernel ------------------------------------------------------------------------------------------------------
def launch(A, b, c, u, flags=0, null=(), arena=None, **opts):
    """One call of the entry with all but one CU reserved (waves refill from the queue) -> (results by name, launch_info);
    ``null``: outputs passed as NULL; ``arena``: a placement of tests/footprint.py to run the call in."""
    import torch
    from pycllp_amd.solvers.hip import Handle, solve_opts
    dev = torch.device("cuda:0")
    B, (m, N) = len(b), A.shape
    specs = [fp.inp("b", b), fp.inp("c", c), fp.inp("u", u), fp.out("x", (B, N)), fp.out("y", (B, m)), fp.out("z", (B, N)),
             fp.out("s", (B, N)), fp.out("pobj", (B,)), fp.out("dobj", (B,)), fp.out("status", (B,), fp.I32),
             fp.out("iters", (B,), fp.I32)]
    ar = fp.Arena(specs, arena, device=dev, null=null) if arena else fp.Plain(specs, device=dev)
    ar.null = set(null)
    h = Handle(csr(A), dev, None)
    o = solve_opts({}, flags, reserve_cus=torch.cuda.get_device_properties(dev).multi_processor_count - 1, **opts)
    ptr = lambda t: ctypes.c_void_p(None if t is None else t.data_ptr())      # noqa: E731
    st = ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
    with torch.cuda.device(dev):
        rc = getattr(_native.lib(), ENTRY)(h, B, *(ptr(ar[k]) for k in ("b", "c", "u") + OUT), ctypes.byref(o), st)
    assert rc == 0, _native.lib().pycllp_hip_last_error()
    torch.cuda.synchronize(dev)
    if arena:
        ar.check()
    info = h.launch_info()
    return ar.results(), info


def assert_served(size, info):
    f = cs.BY_SIZE[size]
    assert info.get("kernel") == "wave" and info.get("variant") == f.variant and info.get("wave_shape") == f.shape, info
    assert info["grid"] <= 2, info          # one CU is left to the solve: a shape with MB <= 4 puts two workgroups on it


def assert_follows_the_twin(size, variant, got, info, label, take=None):
    A, b, c, u = cs.batch(size, variant)
    ref = cs.twin(size, variant, take=take)
    nb = len(ref["status"])
    b, c, u = b[:nb], c[:nb], u[:nb]
    assert_served(size, info)
    opt = ref["status"] == 0
    dev_it = np.abs(got["iters"].astype(int) - ref["iters"]).max()
    # objectives in the units of the 'plain' batch: a scaled LP is that LP with its objective times SCALE_B SCALE_C = 10
    units = np.ones(nb)
    units[{"plain": slice(0, 0), "autoscale": slice(None), "per_lp": slice(0, None, 2)}[variant]] = cs.SCALE_B * cs.SCALE_C
    dev_obj = max((np.abs(got[k] - ref[k]) / units)[opt].max() for k in ("pobj", "dobj"))
    # certificates of the LP the kernel solved (under autoscale: in its units, see certificate_ratio)
    sb, sc = tw.scale_factors(b, c, u, variant == "autoscale", variant == "per_lp")
    certs = [tw.certificate_ratio(A, b, c, u, got, i, sb[i], sc[i]) for i in np.flatnonzero(got["status"] != 0)
             if got["status"][i] in (2, 4)]
    report(["wave kernel %dx%d B=%d %-9s statuses equal %s  iters +-%d  objectives %.2e  certificates %.2e"
            % (size + (nb, label, np.array_equal(got["status"], ref["status"]), dev_it, dev_obj, max(certs, default=0.0)))])
    assert np.array_equal(got["status"], ref["status"]), (got["status"], ref["status"])
    assert dev_it <= 1, (got["iters"], ref["iters"])
    assert dev_obj <= 1e-9, dev_obj
    assert max(certs, default=0.0) <= CERT, certs


@pytest.mark.gpu
@pytest.mark.parametrize("size", SIZES, ids=str)
def test_kernel_follows_the_twin(size):
    A, b, c, u = cs.batch(size)
    got, info = launch(A, b, c, u)
    assert_follows_the_twin(size, "plain", got, info, "plain")
    # every optional output NULL: x and status keep their bits
    bare, _ = launch(A, b, c, u, null=OPTIONAL)
    assert sorted(bare) == ["status", "x"]
    assert np.array_equal(bare["status"], got["status"]) and np.array_equal(bare["x"].view(np.int64), got["x"].view(np.int64))


def per_lp_deviation(a, ref):
    """tests/trajectory.py's: per LP max|a - ref| / max|ref| of a vector (max|ref| = 0: absolute)."""
    scale = np.abs(ref).max(axis=1)
    return np.abs(a - ref).max(axis=1) / np.where(scale > 0, scale, 1.0)


@pytest.mark.gpu
@pytest.mark.parametrize("size", [(17, 48), (65, 100)], ids=str)
def test_iterates_follow_the_twin(size):
    """x, y, z, s after k = 1, 2, 4 iterations, over the LPs still at status 5 in both: a step that is wrong but still converges
    shows here.  The bound is the twin's own spread under NPERM permutations of the LP, by tests/trajectory.py's rule."""
    A, b, c, u = cs.batch(size)
    lines, failures = [], []
    for k in K:
        ref = cs.twin(size, k=k)
        got, info = launch(A, b, c, u, max_iter=k)
        assert_served(size, info)
        live = (ref["status"] == 5) & (got["status"] == 5)
        assert live.sum() >= cs.B // 2 and (got["iters"][live] == k).all()
        runs = [cs.twin(size, k=k, perm=p) for p in range(NPERM)]
        for q in ("x", "y", "z", "s"):
            both = [live & (r["status"] == 5) for r in runs]
            spread = max(per_lp_deviation(r[q][sel], ref[q][sel]).max() for r, sel in zip(runs, both))
            tol = min(max(FACTOR * spread, FLOOR), CEILING)
            dev = per_lp_deviation(got[q][live], ref[q][live]).max()
            lines.append("wave kernel %dx%d k=%d %s %.2e (bound %.2e)" % (size + (k, q, dev, tol)))
            if not dev <= tol:
                failures.append(lines[-1])
    report(lines)
    print("\n".join(lines))
    assert not failures, failures


@pytest.mark.gpu
@pytest.mark.parametrize("size", [(17, 48), (33, 160)], ids=str)
@pytest.mark.parametrize("variant", ["autoscale", "per_lp"])
def test_kernel_follows_the_twin_under_autoscale(size, variant):
    A, b, c, u = cs.batch(size, variant)
    got, info = launch(A, b, c, u, flags=_native.FLAG_AUTOSCALE if variant == "autoscale" else _native.FLAG_AUTOSCALE_PER_LP)
    assert_follows_the_twin(size, variant, got, info, variant)
    if variant == "per_lp":      # an LP in band carries the bits of a launch without the flag
        plain, _ = launch(A, b, c, u)
        inband = ~(tw.out_of_band(np.abs(b).max(1)) | tw.out_of_band(np.abs(c).max(1))
                   | tw.out_of_band(np.where(np.isfinite(u), u, 0.0).max(1)))
        assert inband.any() and not inband[0::2].any()
        for k in OUT:
            assert np.array_equal(got[k][inband], plain[k][inband], equal_nan=True), k


@pytest.mark.gpu
@pytest.mark.parametrize("nb", [1, 3])
def test_fewer_lps_than_waves(nb):
    size = (17, 48)
    A, b, c, u = cs.batch(size)
    got, info = launch(A, b[:nb], c[:nb], u[:nb])
    assert_follows_the_twin(size, "plain", got, info, "B=%d" % nb, take=nb)


@pytest.mark.gpu
def test_same_call_twice_gives_the_same_bits():
    A, b, c, u = cs.batch((40, 130))
    one, _ = launch(A, b, c, u)
    two, _ = launch(A, b, c, u)
    for k in OUT:
        assert np.array_equal(one[k].view(np.uint8), two[k].view(np.uint8)), k


@pytest.mark.gpu
@pytest.mark.parametrize("placement", ["aligned", "natural"])
def test_call_writes_its_outputs_and_nothing_else(placement):
    size = (17, 48)
    A, b, c, u = cs.batch(size)
    got, _ = launch(A, b, c, u, arena=placement)                     # (Arena.check() runs inside)
    assert np.array_equal(got["status"], cs.twin(size)["status"])
    launch(A, b, c, u, arena=placement, null=OPTIONAL)


@pytest.mark.gpu
def test_nan_in_b_ends_numerical_and_leaves_its_batch_mates_alone():
    A, b, c, u = cs.batch((17, 48))
    clean, _ = launch(A, b, c, u)
    bad = b.copy()
    bad[17, 3] = np.nan
    got, _ = launch(A, bad, c, u)
    assert got["status"][17] == _native.STATUS_NUMERICAL
    mates = np.arange(cs.B) != 17
    for k in OUT:
        assert np.array_equal(got[k][mates].view(np.uint8), clean[k][mates].view(np.uint8)), k


# ---- GPU: the plugin ------------------------------------------------------------------------------------------------------
RESULTS = ("x", "y", "z", "s", "status", "iters", "primal_obj", "dual_obj")


def infeasible_every_third(glp, row=1):
    """Every third LP of ``glp`` made infeasible as ``test_bounded_hsd.general_batch`` does: the equality row ``row`` asks for more
    than its columns can give (their u made finite first where the batch mixes finite and infinite u)."""
    A = np.asarray(glp.A.todense())
    sel = np.arange(1, glp.nproblems, 3)
    cols = np.flatnonzero(A[row] != 0)
    for k in sel:
        inf = cols[~np.isfinite(glp.u[k, cols])]
        glp.u[k, inf] = glp.l[k, inf] + 1.0
    reach = np.maximum(A[row, cols] * glp.l[:, cols], A[row, cols] * glp.u[:, cols]).sum(axis=1)
    glp.a[sel, row] = glp.b[sel, row] = reach[sel] + 5.0
    return glp


def run(glp, **kw):
    s = solver_registry[GENERAL[1]](device="cuda:0", **kw)
    glp.init(s)
    glp.solve(s)
    return s


@pytest.mark.gpu
def test_plugin_device_resolves_on_the_device_where_the_expansion_fits():
    import torch
    from pycllp_amd.solvers.general import NATIVE_MAX_ROWS, expansion_rows
    glp = infeasible_every_third(make_sparse_general(48, 40, 256, seed=81, density=0.12))
    blp, _ = glp.to_bounded_equality_form()
    assert blp.nrows > NATIVE_MAX_ROWS                              # beyond the lane-group range
    assert expansion_rows(glp) <= _native.lib().pycllp_hip_dense_max_rows()      # ... and the expansion serves it
    status = np.array([highs_general_status(glp, k)[0] for k in range(glp.nproblems)])
    assert (status[1::3] == 2).all() and (status[0::3] == 0).all()
    plain = run(glp, hsd=False)
    first = {k: np.array(getattr(plain, k)) for k in RESULTS}
    s = run(glp, hsd="device")
    assert s.kernel == "bounded wave"
    assert np.array_equal(np.array(s.status), status), (np.array(s.status), status)
    kept = first["status"] == 0
    assert kept.any() and not kept[status != 0].any()
    for k, v in first.items():
        assert np.array_equal(np.asarray(getattr(s, k))[kept], v[kept]), k
    res = s.solve_device(glp.a, glp.b, glp.c, glp.l, glp.u, glp.f, hsd=True)
    torch.cuda.synchronize()
    assert s.kernel == "bounded wave"
    assert np.array_equal(res["status"].cpu().numpy(), status)
    assert (res["invalid"].cpu().numpy() == 0).all()


def general_certificate_ratio(glp, s, k):
    """Residual over value of LP k's certificate in the GeneralLP's variables, from the returned vectors alone (conventions of
    ``test_general_solver.check_kkt``: A'y - z + s = c, y > 0 on the upper row bound, y < 0 on the lower).  Status 2: |A'y - z + s|
    over -(b'y+ - a'y- + u's - l'z); status 4, the ray r = x - l: the largest violation of A r <= 0 (finite b), A r >= 0 (finite
    a), r <= 0 (finite u), r >= 0 over c'r."""
    A = np.asarray(glp.A.todense())
    a, b, l, u = glp.a[k], glp.b[k], glp.l[k], glp.u[k]
    part = lambda w, bound: float((w[w != 0] * bound[w != 0]).sum())       # noqa: E731  (a multiplier of 0 meets no bound)
    if s.status[k] == 2:
        y, z, sv = s.y[k], s.z[k], s.s[k]
        val = -(part(np.maximum(y, 0), b) - part(np.maximum(-y, 0), a) + part(sv, u) - part(z, l))
        resid = np.abs(A.T @ y - z + sv).max()
    else:
        r = s.x[k] - l
        Ar = A @ r
        val = glp.c[k] @ r
        resid = max(np.where(np.isfinite(b), Ar, 0.0).max(), np.where(np.isfinite(a), -Ar, 0.0).max(),
                    np.where(np.isfinite(u), r, 0.0).max(), (-r).max(), 0.0)
    return resid / val if val > 0 and np.isfinite(val) else np.inf


@pytest.mark.gpu
def test_plugin_device_certifies_where_the_expansion_cannot_serve():
    from pycllp_amd.solvers.general import expansion_rows
    glp = infeasible_every_third(make_sparse_general(96, 288, 48, seed=82, density=0.03, mixed_u=True))
    assert expansion_rows(glp) > _native.lib().pycllp_hip_dense_max_rows()
    status = np.array([highs_general_status(glp, k)[0] for k in range(glp.nproblems)])
    assert (status[1::3] == 2).all() and (status[0::3] == 0).all()
    plain, auto = run(glp, hsd=False), run(glp, hsd="auto")
    assert auto.kernel == "bounded wave" and np.array_equal(auto.status, plain.status)       # the heuristic verdicts stand
    s = run(glp, hsd="device")
    rc, _, shape = bounded_plan(glp.bounded_structure()[0].tocsr())
    assert s.kernel == "bounded wave" and rc == 0 and s.launch_info()["wave_shape"] == shape and shape[0] >= 5, (shape, s.launch_info())
    assert np.array_equal(np.array(s.status), status), (np.array(s.status), status)
    ratios = [general_certificate_ratio(glp, s, k) for k in np.flatnonzero(status != 0)]
    report(["plugin 96x288 hsd='device': %d certificates, ratio at most %.2e; hsd='auto' statuses %s"
            % (len(ratios), max(ratios), np.unique(np.array(auto.status)[status != 0]).tolist())])
    assert max(ratios) <= CERT, ratios
