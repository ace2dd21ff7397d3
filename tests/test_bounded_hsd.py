"""Bounded LPs on the homogeneous self-dual embedding: ipm_bounded_hsd_kernel (csrc/ipm_group_bdhsd.inc), its entry
pycllp_hip_dense_solve_bounded_hsd and ``hsd='native'`` of ``hip_general_primal_normal``.

CPU: the twin (tests/bounded_hsd_twin.py) against the oracle's hsd_one_raw on the EXPLICIT expansion, LP by LP and iterate by
iterate, and against HiGHS with the certificates verified from the vectors; the entry's refusals on a fake handle; the plugins'
option checks.  GPU: the kernel against the twin for every compiled shape, under autoscale, the forced guard and NULL outputs;
repeatability, footprint, a NaN in b; the plugin against HiGHS.

The k-iterate bounds follow tests/trajectory.py: the spread of the REFERENCE under seeded row and column permutations of the
expansion, times its FACTOR, floored at its FLOOR.  Set PYCLLP_TRAJECTORY_REPORT to a file name to get the measured deviations."""
import ctypes
import functools
import os
import re

import numpy as np
import pytest
from scipy.optimize import linprog

import bounded_hsd_twin as tw
import footprint as fp
from oracle import port
from pycllp_amd import _native
from pycllp_amd.solvers import solver_registry
from test_general_solver import make_general

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRY = "pycllp_hip_dense_solve_bounded_hsd"
NPERM, FACTOR, FLOOR, CEILING = 4, 32.0, 1e-13, 1e-9        # tests/trajectory.py's rule
K = (1, 2, 4, 8)
CPU_SHAPES = ((3, 4), (6, 10), (12, 20))
CERT = 1e-7
GENERAL = ("hip_general_primal_normal", "hip_sparse_general_primal_normal", "hip_general_batch_primal_normal",
           "hip_sparse_general_batch_primal_normal")


def report(lines):
    path = os.environ.get("PYCLLP_TRAJECTORY_REPORT")
    if path:
        with open(path, "a") as fh:
            fh.write("\n".join(lines) + "\n")


def deviation(a, ref):
    """tests/trajectory.py's: max|a - ref| / max|ref| of a vector (max|ref| = 0: absolute)."""
    scale = np.abs(ref).max() if ref.size else 0.0
    return (np.abs(a - ref).max() if ref.size else 0.0) / (scale if scale > 0 else 1.0)


# ---- CPU: fixtures and references, computed once --------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def cpu_batch(shape):
    """The recipe at ``shape``: 40 LPs with random b (p_inf 0.25, 0.5, 0.9 in turn) and 20 of the feasible family."""
    mp, nd = shape
    parts = [tw.random_batch(mp, nd, 14 if i else 12, 1000 * mp + i, p_inf=p) for i, p in enumerate((0.25, 0.5, 0.9))]
    parts.append(tw.random_batch(mp, nd, 20, 1000 * mp + 7, p_inf=0.5, feasible=True))
    return parts


def oracle_on_expansion(A, b, c, u, perm=None, **opts):
    """The oracle's hsd_one_raw (flags = 32) on the explicit expansion of ONE LP -> x, y, z, s in the LP's own variables (zero
    where a column takes no part), status, iters, pobj.  ``perm``: seed of a row and column permutation of the expansion."""
    Ae, be, ce, act, bnd = tw.expansion(A, b, c, u)
    me, Ne = Ae.shape
    pr, pc = np.arange(me), np.arange(Ne)
    if perm is not None:
        rs = np.random.RandomState(100 + perm)
        pr, pc = rs.permutation(me), rs.permutation(Ne)
    o = port.dense_solve(Ae[pr][:, pc], be[pr], ce[pc], flags=32, **opts)
    xe, ze, ye = np.empty(Ne), np.empty(Ne), np.empty(me)
    xe[pc], ze[pc], ye[pr] = o["x"][0], o["z"][0], o["y"][0]
    na, m = int(act.sum()), A.shape[0]
    x, z, s = (np.zeros(len(u)) for _ in range(3))
    x[act], z[act], s[bnd] = xe[:na], ze[:na], ze[na:]
    return dict(x=x, y=ye[:m], z=z, s=s, status=int(o["status"][0]), iters=int(o["iters"][0]), pobj=float(o["pobj"][0]))


@functools.lru_cache(maxsize=None)
def cpu_reference(shape, k=None):
    """Per part of cpu_batch(shape): (the twin's results, the oracle's LP by LP), at max_iter = k (None: to the end)."""
    opts = {} if k is None else dict(max_iter=k)
    return [(tw.solve(A, b, c, u, **opts), [oracle_on_expansion(A, b[i], c[i], u[i], **opts) for i in range(len(b))])
            for A, b, c, u in cpu_batch(shape)]


@pytest.mark.parametrize("shape", CPU_SHAPES, ids=str)
def test_twin_ends_where_the_oracle_on_the_expansion_ends(shape):
    seen = set()
    for twin, orc in cpu_reference(shape):
        for i, o in enumerate(orc):
            assert twin["status"][i] == o["status"], (i, twin["status"][i], o["status"])
            assert abs(int(twin["iters"][i]) - o["iters"]) <= 1, (i, twin["iters"][i], o["iters"])
            if o["status"] == 0:
                assert abs(twin["pobj"][i] - o["pobj"]) <= 1e-9, (i, twin["pobj"][i], o["pobj"])
            seen.add(o["status"])
    assert seen <= {0, 2, 4} and {0, 2} <= seen, seen


@pytest.mark.parametrize("shape", CPU_SHAPES, ids=str)
def test_twin_follows_the_oracle_iterate_by_iterate(shape):
    """x, y, s after k iterations: within 1e-11 at k = 1; at k = 2, 4, 8 within FACTOR times the oracle's own spread under NPERM
    permutations of the expansion, capped at CEILING (near the end of a short solve the oracle's own spread exceeds it).  LPs that ended before k in either are left to the test above."""
    lines = []
    for k in K:
        worst = dict(x=0.0, y=0.0, s=0.0)
        spread = dict(x=0.0, y=0.0, s=0.0)
        for (A, b, c, u), (twin, orc) in zip(cpu_batch(shape), cpu_reference(shape, k)):
            for i, o in enumerate(orc):
                if o["status"] != 5 or twin["status"][i] != 5:
                    continue
                runs = [oracle_on_expansion(A, b[i], c[i], u[i], perm=p, max_iter=k) for p in range(NPERM)] if k > 1 else []
                bnd = (u[i] > 0) & np.isfinite(u[i])          # (a fixed column's s is its reduced cost: not part of the expansion)
                for q in worst:
                    worst[q] = max(worst[q], deviation(np.where(bnd, twin[q][i], 0.0) if q == "s" else twin[q][i], o[q]))
                    spread[q] = max([spread[q]] + [deviation(r[q], o[q]) for r in runs if r["status"] == 5])
        tol = {q: 1e-11 if k == 1 else min(max(FACTOR * spread[q], FLOOR), CEILING) for q in worst}
        lines.append("twin %dx%d k=%d  " % (shape + (k,)) + "  ".join("%s %.2e (bound %.2e)" % (q, worst[q], tol[q]) for q in worst))
        for q in worst:
            assert worst[q] <= tol[q], (k, q, worst[q], tol[q])
    report(lines)


@pytest.mark.parametrize("shape", CPU_SHAPES, ids=str)
def test_twin_agrees_with_highs_and_its_certificates_hold(shape):
    for (A, b, c, u), (twin, _) in zip(cpu_batch(shape), cpu_reference(shape)):
        status, obj = tw.highs_verdicts(A, b, c, u)
        assert np.array_equal(twin["status"], status), (twin["status"], status)
        assert (twin["floored"] == 0).all(), twin["floored"]          # the fixtures keep every pivot off its floor
        opt = status == 0
        assert (np.abs(twin["pobj"] - obj)[opt] <= 1e-9 * np.maximum(1.0, np.abs(obj[opt]))).all()
        for i in np.flatnonzero(~opt):
            assert tw.certificate_ratio(A, b, c, u, twin, i) <= CERT, (i, twin["status"][i])


@pytest.mark.parametrize("size", list(tw.MIXED_SEEDS), ids=str)
def test_gpu_batches_interleave_the_three_verdicts(size):
    A, b, c, u, ref = gpu_case(size)
    status, _ = tw.highs_verdicts(A, b, c, u)
    assert np.array_equal(ref["status"], status) and (ref["floored"] == 0).all()
    assert (status[0::3] == 0).all() and (status[1::3] == 2).all() and (status == 4).any()
    assert (np.isinf(u).any(axis=1) & (u == 0).any(axis=1) & (np.isfinite(u) & (u > 0)).any(axis=1)).all() or size == (1, 1)


# ---- CPU: the entry and the plugins ---------------------------------------------------------------------------------------
def test_symbol_is_declared_and_exported():
    header = open(os.path.join(ROOT, "include", "pycllp_hip.h")).read()
    assert re.search(r"\bint\s+%s\s*\(" % ENTRY, header)
    sig = dict((n, (a, r)) for n, a, r in _native.SIGNATURES)[ENTRY]
    assert ENTRY in _native.EXPORTS and len(sig[0]) == 15      # handle, B, b, c, u, eight outputs, opts, stream
    assert hasattr(ctypes.CDLL(_native.LIB_PATH), ENTRY)


def _entry_args(h, B, u, flags):
    o = _native.default_opts(flags=flags)
    return (h, B, 8, 8, u, 8, 8, 8, 8, 8, 8, 8, 8, ctypes.byref(o), None)


def test_entry_checks_its_arguments_before_the_handle_is_read():
    L = _native.lib()
    f = getattr(L, ENTRY)
    buf = np.zeros(8)                        # 64 bytes, never dereferenced
    fake = buf.ctypes.data
    refused = [(None, 1, 8, 0), (fake, -1, 8, 0), (fake, 1, None, 0),
               (fake, 1, 8, _native.FLAG_AUTOSCALE | _native.FLAG_AUTOSCALE_PER_LP)]
    refused += [(fake, 1, 8, fl) for fl in (_native.FLAG_PREDCORR, _native.FLAG_WARM_START, _native.FLAG_WAVE_KERNEL,
                                             _native.FLAG_NO_SLACK_PATH, _native.FLAG_HSD | _native.FLAG_PREDCORR)]
    for args in refused:
        assert f(*_entry_args(*args)) == -1, args
        assert ENTRY.encode() in L.pycllp_hip_last_error(), (args, L.pycllp_hip_last_error())
    # ... and pycllp_hip_dense_solve_bounded still refuses the embedding
    g = L.pycllp_hip_dense_solve_bounded
    assert g(*_entry_args(fake, 1, 8, _native.FLAG_HSD)) == -1 and b"not available" in L.pycllp_hip_last_error()


def test_native_is_an_option_of_the_shared_dense_plugin_alone():
    s = solver_registry[GENERAL[0]](hsd="native")
    assert s.hsd_native and s.hsd == "auto"
    assert not solver_registry[GENERAL[0]]().hsd_native and solver_registry[GENERAL[0]]().hsd == "auto"
    assert solver_registry[GENERAL[0]](hsd=False).hsd is False
    for name in GENERAL[1:]:
        with pytest.raises(ValueError):
            solver_registry[name](hsd="native")
    for name in GENERAL:
        with pytest.raises(ValueError):
            solver_registry[name](hsd="yes")
        with pytest.raises(ValueError):
            solver_registry[name](hsd=True)


# ---- GPU ------------------------------------------------------------------------------------------------------------------
B_GPU = 64
OUT = fp.BOUNDED_OUT
SCALE_B, SCALE_C = 1e4, 1e-3


@functools.lru_cache(maxsize=None)
def gpu_case(size, variant="plain"):
    """(A, b, c, u, the twin's results) of the batch of ``size`` = (m', n): 'plain'; 'autoscale': b, u x 1e4 and c x 1e-3 (u scales
    with b: the same LPs in other units) under PYCLLP_FLAG_AUTOSCALE; 'per_lp': every other LP so, under _AUTOSCALE_PER_LP."""
    A, b, c, u = tw.mixed_batch(size[0], size[1], B_GPU, tw.MIXED_SEEDS[size])
    if variant != "plain":
        sel = slice(None) if variant == "autoscale" else slice(0, None, 2)
        b, c, u = b.copy(), c.copy(), u.copy()
        b[sel] *= SCALE_B; u[sel] *= SCALE_B; c[sel] *= SCALE_C
    ref = tw.solve(A, b, c, u, autoscale=variant == "autoscale", per_lp=variant == "per_lp")
    for v in (A, b, c, u) + tuple(ref.values()):
        v.setflags(write=False)
    return A, b, c, u, ref


def launch(A, b, c, u, flags=0, null=(), arena=None, **opts):
    """One call of the entry with all but one CU reserved (slots refill, lane groups finish at different passes) -> (results by
    name, launch_info); ``null``: outputs passed as NULL; ``arena``: a placement of tests/footprint.py to run the call in."""
    import torch
    from pycllp_amd.solvers.hip import Handle, solve_opts
    dev = torch.device("cuda:0")
    B, (m, N) = len(b), A.shape
    specs = [fp.inp("b", b), fp.inp("c", c), fp.inp("u", u), fp.out("x", (B, N)), fp.out("y", (B, m)), fp.out("z", (B, N)),
             fp.out("s", (B, N)), fp.out("pobj", (B,)), fp.out("dobj", (B,)), fp.out("status", (B,), fp.I32),
             fp.out("iters", (B,), fp.I32)]
    ar = fp.Arena(specs, arena, device=dev, null=null) if arena else fp.Plain(specs, device=dev)
    ar.null = set(null)
    h = Handle(np.array(A), dev, None)
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


def group_shape(size):
    mp, n = size
    return next(s for s in ((16, 32), (16, 48), (16, 64), (32, 64), (32, 96), (32, 128)) if mp <= s[0] and n <= s[1] - s[0])


def assert_follows_the_twin(size, variant, got, info, label):
    A, b, c, u, ref = gpu_case(size, variant)
    assert info["group_shape"] == group_shape(size) and info["slack"] == 1 and info["grid"] == 1, info
    opt = ref["status"] == 0
    dev_it = np.abs(got["iters"].astype(int) - ref["iters"]).max()
    # objectives in the units of the 'plain' batch: a scaled LP is that LP with its objective times SCALE_B SCALE_C = 10, and so
    # is the distance between two points that both meet the relative stop test
    units = np.ones(B_GPU)
    units[{"plain": slice(0, 0), "autoscale": slice(None), "per_lp": slice(0, None, 2)}[variant]] = SCALE_B * SCALE_C
    dev_obj = max((np.abs(got[k] - ref[k]) / units)[opt].max() for k in ("pobj", "dobj"))
    # certificates of the LP the kernel solved (under autoscale: in its units, see certificate_ratio)
    sb, sc = tw.scale_factors(b, c, u, variant == "autoscale", variant == "per_lp")
    certs = [tw.certificate_ratio(A, b, c, u, got, i, sb[i], sc[i]) for i in np.flatnonzero(~opt)]
    report(["kernel %dx%d %-9s statuses equal %s  iters +-%d  objectives %.2e  certificates %.2e"
            % (size + (label, np.array_equal(got["status"], ref["status"]), dev_it, dev_obj, max(certs)))])
    assert np.array_equal(got["status"], ref["status"]), (got["status"], ref["status"])
    assert dev_it <= 1, (got["iters"], ref["iters"])
    assert dev_obj <= 1e-9, dev_obj
    assert max(certs) <= CERT, certs


@pytest.mark.gpu
@pytest.mark.parametrize("size", list(tw.MIXED_SEEDS), ids=str)
def test_kernel_follows_the_twin(size):
    A, b, c, u, ref = gpu_case(size)
    got, info = launch(A, b, c, u)
    assert_follows_the_twin(size, "plain", got, info, "plain")
    # every optional output NULL: x and status keep their bits
    bare, _ = launch(A, b, c, u, null=("y", "z", "s", "pobj", "dobj", "iters"))
    assert sorted(bare) == ["status", "x"]
    assert np.array_equal(bare["status"], got["status"]) and np.array_equal(bare["x"].view(np.int64), got["x"].view(np.int64))
    # the guarded factor: same verdicts, objectives within 1e-9
    forced, info = launch(A, b, c, u, flags=_native.FLAG_FORCE_GUARD_PATH)
    assert_follows_the_twin(size, "plain", forced, info, "guard")


@pytest.mark.gpu
@pytest.mark.parametrize("size", list(tw.MIXED_SEEDS), ids=str)
@pytest.mark.parametrize("variant", ["autoscale", "per_lp"])
def test_kernel_follows_the_twin_under_autoscale(size, variant):
    A, b, c, u, ref = gpu_case(size, variant)
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
def test_same_call_twice_gives_the_same_bits():
    A, b, c, u, _ = gpu_case((24, 64))
    one, _ = launch(A, b, c, u)
    two, _ = launch(A, b, c, u)
    for k in OUT:
        assert np.array_equal(one[k].view(np.uint8), two[k].view(np.uint8)), k


@pytest.mark.gpu
@pytest.mark.parametrize("placement", ["aligned", "natural"])
def test_call_writes_its_outputs_and_nothing_else(placement):
    A, b, c, u, ref = gpu_case((14, 30))
    got, _ = launch(A, b, c, u, arena=placement)                     # (Arena.check() runs inside)
    assert np.array_equal(got["status"], ref["status"])
    launch(A, b, c, u, arena=placement, null=("y", "z", "s", "pobj", "dobj", "iters"))


@pytest.mark.gpu
def test_nan_in_b_ends_numerical_and_leaves_its_batch_mates_alone():
    A, b, c, u, _ = gpu_case((24, 32))
    clean, _ = launch(A, b, c, u)
    bad = b.copy()
    bad[17, 3] = np.nan
    got, _ = launch(A, bad, c, u)
    assert got["status"][17] == _native.STATUS_NUMERICAL
    mates = np.arange(B_GPU) != 17
    for k in OUT:
        assert np.array_equal(got[k][mates].view(np.uint8), clean[k][mates].view(np.uint8)), k


def general_batch():
    """256 GeneralLPs, 12 rows x 16 columns, mixed row kinds, finite u; every third one is made infeasible (an equality row asks
    for more than its columns can give)."""
    glp = make_general(12, 16, 256, seed=77)
    A = glp.A.todense()
    reach = (np.maximum(A[1] * glp.l, A[1] * glp.u)).sum(axis=1)          # row 1 is an 'eq' row
    glp.a[1::3, 1] = glp.b[1::3, 1] = reach[1::3] + 5.0
    return glp


def highs_general_status(glp, k):
    A = glp.A.todense()
    hi, lo = np.isfinite(glp.b[k]), np.isfinite(glp.a[k])
    r = linprog(-glp.c[k], A_ub=np.vstack([A[hi], -A[lo]]), b_ub=np.concatenate([glp.b[k][hi], -glp.a[k][lo]]),
                bounds=list(zip(glp.l[k], glp.u[k])), method="highs")
    return {0: 0, 2: 2, 3: 4}[r.status], (-r.fun + glp.f[k] if r.status == 0 else np.nan)


@pytest.mark.gpu
def test_plugin_native_resolves_on_the_device():
    import torch
    glp = general_batch()
    ref = [highs_general_status(glp, k) for k in range(glp.nproblems)]
    status = np.array([r[0] for r in ref])
    assert (status[1::3] == 2).all() and (status[0::3] == 0).all()
    plain = solver_registry[GENERAL[0]](device="cuda:0", hsd=False)
    glp.init(plain); glp.solve(plain)
    first = {k: np.array(getattr(plain, k)) for k in ("x", "y", "z", "s", "status", "iters", "primal_obj", "dual_obj")}
    s = solver_registry[GENERAL[0]](device="cuda:0", hsd="native")
    glp.init(s)
    glp.solve(s)
    got = np.array(s.status)
    assert s.kernel == "bounded group"
    assert np.array_equal(got, status), (got, status)
    kept = first["status"] == 0
    assert kept.any() and not kept[status != 0].any()
    for k, v in first.items():
        assert np.array_equal(np.asarray(getattr(s, k))[kept], v[kept]), k
    res = s.solve_device(glp.a, glp.b, glp.c, glp.l, glp.u, glp.f, hsd=True)
    torch.cuda.synchronize()
    assert np.array_equal(res["status"].cpu().numpy(), status)
    assert (res["invalid"].cpu().numpy() == 0).all()
