"""Bounded LPs with per-problem dense matrices on the homogeneous self-dual embedding: ipm_bounded_pa_hsd_kernel
(csrc/ipm_group_pabdhsd.inc), its entry pycllp_hip_dense_solve_batch_bounded_hsd, ``hsd_device=True`` of
``hip_general_batch_primal_normal`` and ``hsd=True`` of its device-resident entries.

The reference is the twin of the embedding (tests/bounded_hsd_twin.py), run LP by LP with that LP's own matrix.  CPU: the
fixture against HiGHS; the symbol; the entry's refusals on a fake handle; the plugins' option checks; the shape list.  GPU: the
kernel against the twin for every compiled shape, under autoscale, the forced guard and NULL outputs; iterates after k
iterations; equal matrices against the shared-A entry; small batches, repeatability, footprint, non-finite data; the plugin
against HiGHS.  The bounds are those of tests/test_bounded_hsd.py; the k-iterate bounds follow tests/trajectory.py.  Set
PYCLLP_TRAJECTORY_REPORT to a file name to get the measured deviations."""
import ctypes
import functools
import os
import re

import numpy as np
import pytest

import bounded_hsd_twin as tw
import bounded_pa_hsd_cases as pc
import general_batch_cases as gbc
import trajectory as tj
from pycllp_amd import _native
from pycllp_amd.solvers import solver_registry
from test_bounded_hsd import deviation, oracle_on_expansion, report

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRY, OUT, B_GPU, CERT = pc.ENTRY, pc.OUT, pc.B_GPU, pc.CERT
BATCH, SPARSE_BATCH = "hip_general_batch_primal_normal", "hip_sparse_general_batch_primal_normal"
K = (1, 2, 4)
TRAJ_SIZES, B_TRAJ = ((14, 30), (24, 64)), 16


# ---- CPU ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("size", pc.SIZES, ids=str)
def test_batches_interleave_the_three_verdicts_on_their_own_matrices(size):
    Ad, b, c, u, ref = pc.gpu_case(size)
    assert Ad.shape == (B_GPU, size[0], size[1])
    assert size == (1, 1) or not np.array_equal(Ad[0], Ad[1])
    status = pc.highs_each(Ad, b, c, u)
    assert np.array_equal(ref["status"], status), (ref["status"], status)
    assert (status[0::3] == 0).all() and (status[1::3] == 2).all() and (status == 4).any()
    assert (ref["floored"] == 0).all()                     # the fixtures keep every pivot off its floor
    for i in np.flatnonzero(status != 0):
        assert pc.certificate(Ad, b, c, u, ref, i) <= CERT, (i, status[i])


@pytest.mark.parametrize("size", pc.SIZES, ids=str)
def test_twin_ends_every_lp_within_30_iterations(size):
    """The bound the batches are specified with (the twin LP by LP, B = 1)."""
    ref = pc.gpu_case(size)[4]
    print("twin iterations at %dx%d: at most %d" % (size + (int(ref["iters"].max()),)))
    assert ref["iters"].max() <= 30


@pytest.mark.parametrize("size", pc.SIZES, ids=str)
def test_batches_have_the_properties_they_are_specified_with(size):
    """... and the offset of U's generator is 7919, or the first one above it under which they have them."""
    assert pc.fixture_holds(pc.gpu_case(size)[4])
    for offset in range(pc.PA_SEED, pc.PA_OFFSETS.get(size, pc.PA_SEED)):
        assert not pc.fixture_holds(pc.twin_each(*pc.mixed_batch_pa(size[0], size[1], B_GPU, tw.MIXED_SEEDS[size], offset)))


def test_sizes_select_every_shape_and_refill_their_slots():
    assert [pc.group_shape(s) for s in pc.SIZES[:6]] == gbc.GROUP_SHAPES
    assert pc.SIZES[6:] == [(1, 1), (16, 16), (32, 64)]
    for size in pc.SIZES:      # one CU: eight LPs per slot with MP = 32 and four waves, four with MP = 16 (more with fewer waves)
        assert pc.refills(size) >= (8 if pc.group_shape(size)[0] == 32 else 4)


def test_symbol_is_declared_bound_and_exported():
    header = open(os.path.join(ROOT, "include", "pycllp_hip.h")).read()
    assert re.search(r"\bint\s+%s\s*\(" % ENTRY, header)
    sig = dict((n, (a, r)) for n, a, r in _native.SIGNATURES)[ENTRY]
    assert ENTRY in _native.EXPORTS and len(sig[0]) == 17      # handle, B, A, a_cols, b, c, u, eight outputs, opts, stream
    assert sig[0] == dict((n, (a, r)) for n, a, r in _native.SIGNATURES)["pycllp_hip_dense_solve_batch_bounded"][0]
    assert ENTRY in _native.LATER_ENTRIES
    assert hasattr(ctypes.CDLL(_native.LIB_PATH), ENTRY)
    assert _native.lib().pycllp_hip_abi_version() == 1


def _entry_args(h, B, A, u, flags):
    o = _native.default_opts(flags=flags)
    return (h, B, A, 5, 8, 8, u, 8, 8, 8, 8, 8, 8, 8, 8, ctypes.byref(o), None)


def test_entry_checks_its_arguments_before_the_handle_is_read():
    L = _native.lib()
    f = getattr(L, ENTRY)
    buf = np.zeros(8)                        # 64 bytes, never dereferenced
    fake = buf.ctypes.data
    refused = [(None, 1, 8, 8, 0), (fake, -1, 8, 8, 0), (fake, 1, 8, None, 0), (fake, 0, 8, None, 0), (fake, 1, None, 8, 0),
               (fake, 1, 8, 8, _native.FLAG_AUTOSCALE | _native.FLAG_AUTOSCALE_PER_LP)]
    refused += [(fake, 1, 8, 8, fl) for fl in (_native.FLAG_PREDCORR, _native.FLAG_WARM_START, _native.FLAG_WAVE_KERNEL,
                                                _native.FLAG_NO_SLACK_PATH, _native.FLAG_HSD | _native.FLAG_PREDCORR)]
    for args in refused:
        assert f(*_entry_args(*args)) == -1, args
        assert ENTRY.encode() in L.pycllp_hip_last_error(), (args, L.pycllp_hip_last_error())
    assert not buf.any()
    # ... and pycllp_hip_dense_solve_batch_bounded still refuses the embedding
    g = L.pycllp_hip_dense_solve_batch_bounded
    assert g(*_entry_args(fake, 1, 8, 8, _native.FLAG_HSD)) == -1 and b"not available" in L.pycllp_hip_last_error()
    assert b"pycllp_hip_dense_solve_batch_bounded:" in L.pycllp_hip_last_error()


def test_hsd_device_is_an_option_of_the_dense_batch_plugin_alone():
    s = solver_registry[BATCH](hsd_device=True)
    assert s.hsd_device is True and s.hsd == "auto" and not s.hsd_native
    assert solver_registry[BATCH]().hsd_device is False
    assert solver_registry[BATCH](hsd_device=True, hsd="auto", dense_wave=True).dense_wave
    for bad in (dict(hsd_device=True, hsd=False), dict(hsd_device=1), dict(hsd_device="auto"), dict(hsd_device=None)):
        with pytest.raises(ValueError):
            solver_registry[BATCH](**bad)
    assert solver_registry[BATCH](hsd_device=False, hsd=False).hsd is False
    for name in ("hip_general_primal_normal", "hip_sparse_general_primal_normal", SPARSE_BATCH):
        with pytest.raises(TypeError):
            solver_registry[name](hsd_device=True)
    assert solver_registry[BATCH]._hsd_entry and not solver_registry[SPARSE_BATCH]._hsd_entry


@pytest.mark.parametrize("name", [BATCH, SPARSE_BATCH])
@pytest.mark.parametrize("hsd", [True, "device", "native"])
def test_the_batch_plugins_still_refuse_the_other_spellings(name, hsd):
    with pytest.raises(ValueError):
        solver_registry[name](hsd=hsd)
    with pytest.raises(ValueError):
        solver_registry[name](hsd=hsd, **(dict(hsd_device=True) if name == BATCH else {}))


def test_shape_list_is_the_list_of_the_lane_group_kernels():
    csrc = os.path.join(ROOT, "pycllp_amd", "csrc")
    tab = open(os.path.join(csrc, "dense_tab.h")).read()
    shapes = lambda t: [tuple(map(int, s)) for s in re.findall(r"X\((\d+),\s*(\d+)\)", t)]      # noqa: E731
    line = re.search(r"#else\s*\n#define PABDHSD_SHAPES\(X\)(.*)", tab).group(1)
    assert shapes(line) == gbc.GROUP_SHAPES          # every shape ships: none has scratch (profiles/bounded_perA_hsd)
    for dev, only in (("PYCLLP_DEV_ONLY_3296", (32, 96)), ("PYCLLP_DEV_ONLY_1648", (16, 48))):
        assert shapes(re.search(r"defined\(%s\).*\n#define PABDHSD_SHAPES\(X\)(.*)" % dev, tab).group(1)) == [only]
    unit = open(os.path.join(csrc, "ipm_group_pabdh.hip")).read()
    assert "GROUP_SHAPES(GROUP_PABDH_VARIANT)" in unit and "pabdhsd_ships(MP, NP)" in unit
    assert "extern const GroupPaVariants kGroupPABDH;" in open(os.path.join(csrc, "group_pa.h")).read()
    mk = open(os.path.join(csrc, "Makefile")).read()
    assert "ipm_group_pabdh.o" in mk and re.search(r"ipm_group_pabdh\.o: SCHED := \$\(DENSE_SCHED\)", mk)


# ---- GPU ------------------------------------------------------------------------------------------------------------------
def assert_follows_the_twin(size, variant, got, info, label):
    Ad, b, c, u, ref = pc.gpu_case(size, variant)
    assert info["group_shape"] == pc.group_shape(size) and info["slack"] == 1 and info["grid"] == 1, info
    opt = ref["status"] == 0
    dev_it = np.abs(got["iters"].astype(int) - ref["iters"]).max()
    # objectives in the units of the 'plain' batch (see tests/test_bounded_hsd.py)
    units = np.ones(B_GPU)
    units[{"plain": slice(0, 0), "autoscale": slice(None), "per_lp": slice(0, None, 2)}[variant]] = pc.SCALE_B * pc.SCALE_C
    dev_obj = max((np.abs(got[k] - ref[k]) / units)[opt].max() for k in ("pobj", "dobj"))
    sb, sc = tw.scale_factors(b, c, u, variant == "autoscale", variant == "per_lp")
    certs = [pc.certificate(Ad, b, c, u, got, i, sb[i], sc[i]) for i in np.flatnonzero(~opt)]
    report(["perA kernel %dx%d %-9s statuses equal %s  iters +-%d  objectives %.2e  certificates %.2e"
            % (size + (label, np.array_equal(got["status"], ref["status"]), dev_it, dev_obj, max(certs)))])
    assert np.array_equal(got["status"], ref["status"]), (got["status"], ref["status"])
    assert dev_it <= 1, (got["iters"], ref["iters"])
    assert dev_obj <= 1e-9, dev_obj
    assert max(certs) <= CERT, certs


@pytest.mark.gpu
@pytest.mark.parametrize("size", pc.SIZES, ids=str)
def test_kernel_follows_the_twin(size):
    Ad, b, c, u, ref = pc.gpu_case(size)
    got, info = pc.launch(Ad, b, c, u)
    assert_follows_the_twin(size, "plain", got, info, "plain")
    # every optional output NULL: x and status keep their bits
    bare, _ = pc.launch(Ad, b, c, u, null=("y", "z", "s", "pobj", "dobj", "iters"))
    assert sorted(bare) == ["status", "x"]
    assert np.array_equal(bare["status"], got["status"]) and np.array_equal(bare["x"].view(np.int64), got["x"].view(np.int64))
    # the guarded factor: same verdicts, objectives within 1e-9
    forced, info = pc.launch(Ad, b, c, u, flags=_native.FLAG_FORCE_GUARD_PATH)
    assert_follows_the_twin(size, "plain", forced, info, "guard")


@pytest.mark.gpu
@pytest.mark.parametrize("size", pc.SIZES, ids=str)
@pytest.mark.parametrize("variant", ["autoscale", "per_lp"])
def test_kernel_follows_the_twin_under_autoscale(size, variant):
    Ad, b, c, u, ref = pc.gpu_case(size, variant)
    got, info = pc.launch(Ad, b, c, u, flags=_native.FLAG_AUTOSCALE if variant == "autoscale" else _native.FLAG_AUTOSCALE_PER_LP)
    assert_follows_the_twin(size, variant, got, info, variant)
    if variant == "per_lp":      # an LP in band carries the bits of a launch without the flag
        plain, _ = pc.launch(Ad, b, c, u)
        inband = ~(tw.out_of_band(np.abs(b).max(1)) | tw.out_of_band(np.abs(c).max(1))
                   | tw.out_of_band(np.where(np.isfinite(u), u, 0.0).max(1)))
        assert inband.any() and not inband[0::2].any()
        for k in OUT:
            assert np.array_equal(got[k][inband], plain[k][inband], equal_nan=True), k


@functools.lru_cache(maxsize=None)
def trajectory_reference(size, k):
    """(the twin after k iterations, the bound per quantity) on the first B_TRAJ LPs of the batch of ``size``: the spread of
    the oracle on the explicit expansion of each LP under NPERM seeded permutations, times FACTOR, floored at FLOOR, never
    above CEILING (tests/trajectory.py)."""
    Ad, b, c, u, _ = pc.gpu_case(size)
    ref = pc.twin_each(Ad, b, c, u, idx=range(B_TRAJ), max_iter=k)
    spread = dict(x=0.0, y=0.0, z=0.0, s=0.0)
    for i in range(B_TRAJ):
        A = pc.full(Ad, i)
        o = oracle_on_expansion(A, b[i], c[i], u[i], max_iter=k)
        if o["status"] != 5:
            continue
        for p in range(tj.NPERM):
            r = oracle_on_expansion(A, b[i], c[i], u[i], perm=p, max_iter=k)
            if r["status"] == 5:
                for q in spread:
                    spread[q] = max(spread[q], deviation(r[q], o[q]))
    return ref, {q: min(max(tj.FACTOR * v, tj.FLOOR), tj.CEILING) for q, v in spread.items()}


@pytest.mark.gpu
@pytest.mark.parametrize("size", TRAJ_SIZES, ids=str)
def test_iterates_follow_the_twin(size):
    Ad, b, c, u, _ = pc.gpu_case(size)
    sub = tuple(np.ascontiguousarray(v[:B_TRAJ]) for v in (Ad, b, c, u))
    lines = []
    failures = []
    for k in K:
        ref, tol = trajectory_reference(size, k)
        got, _ = pc.launch(*sub, max_iter=k)
        both = (ref["status"] == 5) & (got["status"] == 5)
        assert both.any() and np.array_equal(got["status"], ref["status"])
        worst = {q: max(deviation(got[q][i], ref[q][i]) for i in np.flatnonzero(both)) for q in tol}
        lines.append("perA kernel %dx%d k=%d  " % (size + (k,)) + "  ".join("%s %.2e (bound %.2e)" % (q, worst[q], tol[q]) for q in tol))
        failures += [(k, q, worst[q], tol[q]) for q in tol if not worst[q] <= tol[q]]
    report(lines)
    print("\n".join(lines))
    assert not failures, failures


@pytest.mark.gpu
def test_equal_matrices_agree_with_the_shared_entry():
    import torch
    from pycllp_amd.solvers.hip import Handle
    A, b, c, u = tw.mixed_batch(24, 64, B_GPU, tw.MIXED_SEEDS[(24, 64)])
    Ad = np.ascontiguousarray(np.broadcast_to(A[:, :64], (B_GPU, 24, 64)))
    h = Handle(A, torch.device("cuda:0"), None)
    own, _ = pc.launch(Ad, b, c, u, handle=h)
    shared, _ = pc.launch(Ad, b, c, u, handle=h, entry=pc.SHARED_ENTRY)
    assert np.array_equal(own["status"], shared["status"]) and np.array_equal(own["iters"], shared["iters"])
    opt = shared["status"] == 0
    assert opt.any() and max(np.abs(own[k] - shared[k])[opt].max() for k in ("pobj", "dobj")) <= 1e-9
    same = all(np.array_equal(own[k].view(np.uint8), shared[k].view(np.uint8)) for k in OUT)
    line = "perA kernel 24x64 equal matrices against the shared-A entry: bits equal %s" % same
    report([line])
    print(line)


@pytest.mark.gpu
def test_small_batches_and_repeatability():
    import torch
    from pycllp_amd.solvers.hip import Handle
    Ad, b, c, u, ref = pc.gpu_case((24, 64))
    one, _ = pc.launch(Ad, b, c, u)
    two, _ = pc.launch(Ad, b, c, u)
    for k in OUT:
        assert np.array_equal(one[k].view(np.uint8), two[k].view(np.uint8)), k
    for B in (1, 3):          # parked slots whose image stays zero
        got, info = pc.launch(*(np.ascontiguousarray(v[:B]) for v in (Ad, b, c, u)))
        assert info["grid"] == 1
        assert np.array_equal(got["status"], ref["status"][:B])
        assert np.abs(got["iters"].astype(int) - ref["iters"][:B]).max() <= 1
        opt = ref["status"][:B] == 0
        assert np.abs(got["pobj"] - ref["pobj"][:B])[opt].max() <= 1e-9
    # B = 0 launches nothing: the handle's last launch stays what it was (none), and NULL arrays are fine
    h = Handle(pc.full(Ad, 0), torch.device("cuda:0"), None)
    before = h.launch_info()
    o = _native.default_opts()
    rc = getattr(_native.lib(), ENTRY)(h, 0, None, ctypes.c_long(64), None, None, ctypes.c_void_p(8), *([None] * 8), ctypes.byref(o), None)
    assert rc == 0 and h.launch_info() == before


@pytest.mark.gpu
@pytest.mark.parametrize("placement", ["aligned", "natural"])
def test_call_writes_its_outputs_and_nothing_else(placement):
    Ad, b, c, u, ref = pc.gpu_case((14, 30))
    got, _ = pc.launch(Ad, b, c, u, arena=placement)                     # (Arena.check() runs inside)
    assert np.array_equal(got["status"], ref["status"])
    pc.launch(Ad, b, c, u, arena=placement, null=("y", "z", "s", "pobj", "dobj", "iters"))
    pc.launch(Ad, b, c, u, arena=placement, a_cols=31, expect=-1)       # refused: nothing touched
    assert ENTRY.encode() in _native.lib().pycllp_hip_last_error()


@pytest.mark.gpu
@pytest.mark.parametrize("where", ["A", "b"])
def test_non_finite_data_ends_numerical_and_leaves_its_batch_mates_alone(where):
    Ad, b, c, u, _ = pc.gpu_case((24, 32))
    clean, _ = pc.launch(Ad, b, c, u)
    bad_A, bad_b = Ad.copy(), b.copy()
    if where == "A":
        bad_A[17, 3, 5] = np.nan
    else:
        bad_b[17, 3] = np.nan
    got, _ = pc.launch(bad_A, bad_b, c, u)
    assert got["status"][17] == _native.STATUS_NUMERICAL
    mates = np.arange(B_GPU) != 17          # (the LP that takes LP 17's slot next among them: every slot serves eight LPs)
    for k in OUT:
        assert np.array_equal(got[k][mates].view(np.uint8), clean[k][mates].view(np.uint8)), k


@pytest.mark.gpu
def test_plugin_resolves_on_the_device():
    import torch
    glp = pc.general_batch()
    status = np.array([pc.highs_general_status(glp, k) for k in range(glp.nproblems)])
    assert (status[1::3] == 2).all() and (status[0::3] == 0).all()
    plain = solver_registry[BATCH](device="cuda:0", hsd=False)
    glp.init(plain); glp.solve(plain)
    assert plain.kernel == "bounded group per-problem"
    first = {k: np.array(getattr(plain, k)) for k in ("x", "y", "z", "s", "status", "iters", "primal_obj", "dual_obj")}
    s = solver_registry[BATCH](device="cuda:0", hsd_device=True)
    glp.init(s)
    glp.solve(s)
    got = np.array(s.status)
    assert s.kernel == "bounded group per-problem" and s._device_resolved
    assert s.launch_info()["group_shape"] == (16, 32)
    assert np.array_equal(got, status), (got, status)
    kept = first["status"] == 0
    assert kept.any() and not kept[status != 0].any()
    for k, v in first.items():
        assert np.array_equal(np.asarray(getattr(s, k))[kept], v[kept]), k
    res = s.solve_device_general(glp.A.data, glp.a, glp.b, glp.c, glp.l, glp.u, glp.f, hsd=True)
    torch.cuda.synchronize()
    assert np.array_equal(res["status"].cpu().numpy(), status)
    assert (res["invalid"].cpu().numpy() == 0).all()
    blp, _ = glp.to_bounded_equality_form()
    for solver in (s, plain):          # with or without hsd_device
        out = solver.solve_device(solver.bounded_matrices(blp), blp.b, blp.c, blp.u, hsd=True)
        torch.cuda.synchronize()
        assert np.array_equal(out["status"].cpu().numpy(), status)
    sparse = solver_registry[SPARSE_BATCH](device="cuda:0")
    glp.init(sparse)
    with pytest.raises(ValueError):
        sparse.solve_device_general(glp.A.data, glp.a, glp.b, glp.c, glp.l, glp.u, glp.f, hsd=True)


@pytest.mark.gpu
def test_handle_beyond_the_lane_group_kernels_takes_the_route_of_auto():
    """``dense_wave=True`` at 40 x 30: the entry answers UNSUPPORTED (no embedding on the wave kernel with an image per wave), so
    with ``hsd_device=True`` the LP that does not end optimal is solved again through the expansion, as ``hsd='auto'`` does."""
    import general_batch_wave_cases as wc
    from pycllp_amd.lp import GeneralLP
    B, bad = 24, 17
    base = wc.make(40, 70, B, 9)
    b = base.b.copy()
    b[bad, 0] = base.A.todense(bad)[0] @ base.l[bad] - 1.0      # row 0 (positive coefficients) below what x >= l allows
    glp = GeneralLP(base.A, b, base.c, a=base.a, l=base.l, u=base.u, f=base.f)
    got = {}
    for kw in (dict(), dict(hsd_device=True)):
        s = solver_registry[BATCH](device="cuda:0", dense_wave=True, **kw)
        glp.init(s)
        glp.solve(s)
        assert s.kernel == "bounded wave per-problem" and not s._device_resolved
        assert (s._hsd_refused is s._handle) == bool(kw)       # the refusal is the handle's: asked once, then nothing is gathered
        glp.solve(s)
        assert s.kernel == "bounded wave per-problem" and not s._device_resolved
        got[bool(kw)] = {k: np.array(getattr(s, k)) for k in ("x", "y", "z", "s", "status", "iters", "primal_obj", "dual_obj")}
    assert got[True]["status"][bad] == 2 and (np.delete(got[True]["status"], bad) == 0).all()
    for k, v in got[False].items():
        assert np.array_equal(got[True][k], v, equal_nan=True), k
    blp, _ = glp.to_bounded_equality_form()
    with pytest.raises(NotImplementedError):
        s.solve_device(s.bounded_matrices(blp), blp.b, blp.c, blp.u, hsd=True)
