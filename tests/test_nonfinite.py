"""Non-finite data: the PYCLLP_STATUS_NUMERICAL exit of every kernel family, and what a poisoned LP leaves to the others.

One row per (kernel family, kind) of tests/nonfinite_cases.py.  CPU: the table covers every family and kind of the cold
trajectory rows plus the three per-problem entries; on every row's inputs the references end each poison with status 3 at
iteration 0 and leave the other LPs' bits alone (what the GPU assertions rest on); the placement rule picks wave neighbours;
the assertion helper fails on five fakes; the mid-run cases hold under the reference's permutations.  GPU: a batch of at least
three LPs per slot on four compute units, up to six of them poisoned, once without and once with autoscale -- a poisoned LP has
the reference's status (3) and iteration count (+-1) and every output written, every other LP of the batch carries the bits of
the clean run, and a sample of them the reference's verdict; a poisoned warm start; an LP that goes non-finite mid-run; the
stand-alone Newton and LDL' entries; the plugin's default options (``autoscale='auto'``, ``hsd='auto'``, ``warm_start``)."""
import numpy as np
import pytest

import footprint as fp
import nonfinite_cases as nf
import trajectory as tj

ROW_IDS = [r.id for r in nf.ROWS]


def small_batch(row):
    """LPs of a CPU check (the twin costs ~ m^3 per LP and iteration)."""
    return 6 if row.id.startswith("image") and row.kind == "bounded" else 10


def sample_limit(setup):
    return 16 if setup.bounded and setup.m > 96 else nf.SAMPLE


# ---- CPU ------------------------------------------------------------------------------------------------------------------
def test_table_holds_every_family_and_kind():
    cold = {(c.family, c.kind) for c in tj.CASES if c.mode == "cold"}
    have = {(r.family, r.kind) for r in nf.ROWS if r.case is not None}
    assert have == cold, (cold - have, have - cold)
    assert [r.entry for r in nf.ROWS if r.case is None] == ["pycllp_hip_dense_solve_batch", "pycllp_hip_dense_solve_batch_bounded",
                                                           "pycllp_hip_sparse_solve_batch_bounded"]
    # every row sits at an existing point: the trajectory case it names, its key, what serves it and its flags
    for r in nf.ROWS:
        if r.case is not None:
            assert tj.BY_ID[r.id] is r.case and r.case.mode == "cold"
    # the points of the table: the smallest of each family
    points = {(r.family, r.point) for r in nf.ROWS if r.case is not None}
    assert {p for f, p in points if f == "slack"} == {"16x32", "32x64", "24x30"}
    assert {p for f, p in points if f == "group"} == {"17x33"} and {p for f, p in points if f == "tables"} == {"33x193"}
    assert {p for f, p in points if f == "image"} == {"40x100", [c.point for c in tj.CASES if c.family == "image" and c.kind == "bounded"][0]}
    assert len({p for f, p in points if f == "block"}) == 2 and len({p for f, p in points if f == "big"}) == 2
    for r in nf.ROWS:
        if r.family == "big":
            assert r.case.where[1][0] == "L"                # the factor in LDS
    assert set(nf.WARM_ROWS) <= set(nf.BY_ID) and set(nf.MIDRUN) <= set(nf.BY_ID)
    assert len(nf.ROWS) == 33


@pytest.mark.parametrize("grid,block,shape", [(4, 512, (16, 48)), (4, 512, (32, 64)), (3, 256, (16, 32))])
def test_placement_picks_wave_neighbours(grid, block, shape):
    """The lane-group kernels' slot of LP i < slots: lane group i // W of wave i % W (ipm_group.inc: lp = grp W + blockIdx
    wpb + wave).  The healthy neighbours share a wavefront with a poisoned LP, and two more poisoned LPs enter used slots."""
    info = dict(grid=grid, block=block, group_shape=shape)
    slots, W = nf.slots_of(info)
    assert W == grid * block // 64 and slots == W * (64 // shape[0])
    B = 3 * slots + 5
    idx, near = nf.placement(info, B, 6)
    wave = lambda i: i % W
    first = [i for i in idx if i < slots]
    assert len(first) >= 2 and len({i // W for i in first[:2]}) == 2              # in two different lane groups
    for k in near:
        assert k < slots and k not in idx
        assert any(wave(k) == wave(i) and k // W != i // W for i in first), (k, idx)
    assert sum(i >= slots for i in idx) >= 2 and B - 1 in idx and len(idx) <= nf.MAX_POISONED
    with pytest.raises(AssertionError):
        nf.placement(info, 3 * slots - 1, 6)                                         # a slot would be refilled only once


@pytest.mark.parametrize("info", [dict(grid=4, block=256, kernel="wave"), dict(grid=16, block=256, kernel="block"),
                                  dict(grid=12, block=256, kernel="big")], ids=["wave", "block", "big"])
def test_placement_on_the_other_kernels(info):
    slots, W = nf.slots_of(info)
    assert W is None and slots == (16 if info["kernel"] == "wave" else info["grid"])
    idx, near = nf.placement(info, 3 * slots + 5, 6)
    assert idx[:3] == [1, slots + 1, 3 * slots + 4] and not set(idx) & set(near)


@pytest.mark.parametrize("row", nf.ROWS, ids=ROW_IDS)
def test_references_end_every_poison_with_status_3(row):
    """What the GPU assertions rest on: on the row's inputs (a small B) and under the row's kind flags, without and with
    autoscale, the reference ends each poisoned LP with status 3 at iteration 0 and every other LP keeps every bit."""
    B = small_batch(row)
    setup = nf.Setup(row, B)
    todo = nf.poisons(setup)
    assert 4 <= len(todo) <= nf.MAX_POISONED
    assert ("NaN in c of a slack column" in [t[0] for t in todo]) == bool(setup.tail)
    assert ("NaN in a value of A" in [t[0] for t in todo]) == (row.kind.startswith("pa") or row.case is None)
    idx = [1, B - 1, 4, 3, 2, 0][:len(todo)]
    arrays, what = nf.poisoned(setup, idx)
    for q, v in setup.arrays.items():                        # one poison per poisoned LP, nothing else changed
        changed = np.argwhere(nf.bits(arrays[q]) != nf.bits(v))
        assert {int(c[0]) for c in changed} <= set(idx) and len(changed) == sum(t[1] == q for t in todo), q
    healthy = np.setdiff1d(np.arange(B), idx)
    for autoscale in (False, True):
        clean = nf.reference(setup, setup.arrays, range(B), autoscale=autoscale)
        ref = nf.reference(setup, arrays, range(B), autoscale=autoscale)
        assert (clean["status"] == 0).all(), clean["status"]
        assert (ref["status"][idx] == 3).all() and (ref["iters"][idx] == 0).all(), (what, ref["status"][idx], ref["iters"][idx])
        for q in nf.outputs_of(setup):
            assert np.array_equal(nf.bits(ref[q])[healthy], nf.bits(clean[q])[healthy]), (q, autoscale)
        assert nf.check(nf.outputs_of(setup), ref, clean, ref, range(B), idx) == B - len(idx)


@pytest.mark.parametrize("rid", nf.WARM_ROWS)
def test_references_end_a_poisoned_start_with_status_3(rid):
    setup = nf.Setup(nf.BY_ID[rid], 10)
    start, what = nf.poisoned_start(setup, [1, 8])
    clean = nf.reference(setup, setup.arrays, range(10), start=tj.warm_point(10, setup.m, setup.N))
    ref = nf.reference(setup, setup.arrays, range(10), start=start)
    assert (clean["status"] == 0).all() and (ref["status"][[1, 8]] == 3).all() and (ref["iters"][[1, 8]] == 0).all()
    assert nf.check(fp.SOLVE_OUT, ref, clean, ref, range(10), [1, 8]) == 8


def _fake_base():
    """A reference result standing in for the kernel's: poisoned batch, clean batch, the poisoned LPs."""
    setup = nf.Setup(nf.BY_ID["slack-16x32-plain"], 12)
    idx = [1, 5, 11, 7, 3]
    arrays, _ = nf.poisoned(setup, idx)
    clean = nf.reference(setup, setup.arrays, range(12))
    ref = nf.reference(setup, arrays, range(12))
    return idx, clean, ref


def test_check_fails_on_the_five_fakes():
    idx, clean, ref = _fake_base()
    names = fp.SOLVE_OUT
    copy = lambda r: {q: v.copy() for q, v in r.items()}
    assert nf.check(names, copy(ref), clean, ref, range(12), idx) == 7
    # a NaN copied into one entry of a healthy neighbour's x
    got = copy(ref)
    got["x"][2, 4] = np.nan
    with pytest.raises(AssertionError, match="healthy LP 2: x differs from the clean run"):
        nf.check(names, got, clean, ref, range(12), idx)
    # a poisoned LP reported optimal
    got = copy(ref)
    got["status"][5] = 0
    with pytest.raises(AssertionError, match="poisoned LP 5: status 0, the reference's 3"):
        nf.check(names, got, clean, ref, range(12), idx)
    # a poisoned LP at the iteration limit with iters = max_iter
    got = copy(ref)
    got["status"][11], got["iters"][11] = 5, 200
    with pytest.raises(AssertionError, match="poisoned LP 11: status 5, the reference's 3"):
        nf.check(names, got, clean, ref, range(12), idx)
    got["status"][11] = 3                                    # ... and the count alone
    with pytest.raises(AssertionError, match="poisoned LP 11: iters 200, the reference's 0"):
        nf.check(names, got, clean, ref, range(12), idx)
    # an output left at its sentinel
    got = copy(ref)
    got["z"].view(np.int64)[7, 3] = fp._SENT64_I
    with pytest.raises(AssertionError, match="output 'z' not written for LP 7"):
        nf.check(names, got, clean, ref, range(12), idx)
    got = copy(ref)
    got["iters"][3] = fp.SENT32
    with pytest.raises(AssertionError, match="output 'iters' not written for LP 3"):
        nf.check(names, got, clean, ref, range(12), idx)
    # one healthy LP's iters off by one against the clean run
    got = copy(ref)
    got["iters"][6] += 1
    with pytest.raises(AssertionError, match="healthy LP 6: iters differs from the clean run"):
        nf.check(names, got, clean, ref, range(12), idx)


@pytest.mark.parametrize("rid", sorted(nf.MIDRUN))
def test_midrun_cases_hold_under_the_references_permutations(rid):
    """Finite data on which the reference ends with status 3 after at least two iterations, the same status and iteration
    count under the NPERM seeded row-and-column permutations of ``trajectory.run_reference``."""
    case = nf.midrun_case(rid)
    lp = tj.inputs(case.key)
    assert np.isfinite(lp.b).all() and np.isfinite(lp.c).all()
    base = tj.run_reference(case, 200)
    assert base["status"].tolist() == [3] and base["iters"][0] >= 2, (base["status"], base["iters"])
    for p in range(tj.NPERM):
        r = tj.run_reference(case, 200, perm=p)
        assert (r["status"][0], r["iters"][0]) == (3, base["iters"][0]), (p, r["status"], r["iters"], base["iters"])
    # the same LP without the factor is an ordinary optimal one
    setup, k, factor = nf.midrun_lp(rid)
    assert nf.reference(setup, setup.arrays, [k])["status"].tolist() == [0]


def test_kinds_without_a_midrun_case_have_none_on_the_lead():
    """plain, hsd and bounded: b of an LP times 1e80 .. 1e150 never ends with status 3 in the references (on the smallest lane-group
    point; the search of the module docstring of nonfinite_cases.py) -- the table leaves these kinds out."""
    assert {nf.BY_ID[r].kind for r in nf.MIDRUN} == {"pc"}
    for rid in ("slack-16x32-plain", "slack-16x32-hsd", "slack-24x30-bounded"):
        setup = nf.Setup(nf.BY_ID[rid], 4)
        for e in (80, 100, 150):
            arrays = dict(setup.arrays, b=setup.arrays["b"] * 10.0 ** e)
            assert not (nf.reference(setup, arrays, range(4))["status"] == 3).any(), (rid, e)


# ---- GPU ------------------------------------------------------------------------------------------------------------------
def run_row(row, label, setup, gpu, clean, info, make, autoscale=False, start=None, clean_start=None):
    """One poisoned launch of ``row`` against its clean run ``clean`` (``info``: its launch): ``make(idx slots)`` -> (arrays,
    start, [(LP, what)]); asserts everything of the module docstring and records one line."""
    nf.assert_served(row, info, setup)
    assert (clean["status"] == 0).all(), np.unique(clean["status"], return_counts=True)
    slots, _ = nf.slots_of(info)
    arrays, start, what, idx, near = make(info)
    got, info2 = gpu.launch(arrays, autoscale=autoscale, start=start)
    nf.assert_served(row, info2, setup)                      # the poison does not reroute the launch
    assert {q: info2[q] for q in ("grid", "block")} == {q: info[q] for q in ("grid", "block")}, (info, info2)
    sample = nf.sample_of(setup.B, idx, near, info, sample_limit(setup))
    assert set(near) <= set(sample) and setup.B - 2 in sample + idx
    ref_idx = list(idx) + sample
    ref = nf.reference(setup, arrays, ref_idx, autoscale=autoscale, start=start)
    names = nf.outputs_of(setup)
    k = len(idx)
    line = "%-34s | %-9s | %-38s | B=%-4d slots=%-4d poisoned=%s | reference status %s iters %s | kernel status %s iters %s" % (
        row.id, label, nf.served_text(info), setup.B, slots, list(idx), ref["status"][:k].tolist(), ref["iters"][:k].tolist(),
        got["status"][idx].tolist(), got["iters"][idx].tolist())
    print(line)
    try:
        n = nf.check(names, got, clean, ref, ref_idx, idx)
    except AssertionError:
        nf.record(line + " | FAILED")
        raise
    gap = int(np.abs(got["iters"][idx].astype(int) - ref["iters"][:k]).max())
    nf.record(line + " | healthy: %d of %d bit-identical%s" % (n, setup.B - k, " | iteration gap %d" % gap if label == "mid-run" else ""))
    return what


@pytest.mark.gpu
@pytest.mark.parametrize("row", nf.ROWS, ids=ROW_IDS)
def test_poisoned_lps_end_numerical_and_the_others_keep_their_bits(row):
    setup, gpu, clean, info = nf.sized(row, nf.first_guess(row))

    def make(info):
        idx, near = nf.placement(info, setup.B, len(nf.poisons(setup)))
        arrays, what = nf.poisoned(setup, idx)
        return arrays, None, what, idx, near

    run_row(row, "plain", setup, gpu, clean, info, make)
    clean, info = gpu.launch(setup.arrays, autoscale=True)    # the scale factors come from fmax reductions over the poisoned data
    run_row(row, "autoscale", setup, gpu, clean, info, make, autoscale=True)


@pytest.mark.gpu
@pytest.mark.parametrize("rid", nf.WARM_ROWS)
def test_poisoned_warm_start(rid):
    """A NaN in x and an Inf in z of the start point of two LPs (PYCLLP_FLAG_WARM_START reads x, y, z from the outputs)."""
    row = nf.BY_ID[rid]
    setup, gpu, _, _ = nf.sized(row, nf.first_guess(row))
    clean, info = gpu.launch(setup.arrays, start=tj.warm_point(setup.B, setup.m, setup.N))

    def make(info):
        idx, near = nf.placement(info, setup.B, 2)
        start, what = nf.poisoned_start(setup, idx)
        return setup.arrays, start, what, idx, near

    run_row(row, "warm", setup, gpu, clean, info, make)


@pytest.mark.gpu
@pytest.mark.parametrize("rid", sorted(nf.MIDRUN))
def test_lp_that_goes_non_finite_mid_run(rid):
    """Finite data: the stop test on a predicted residual and the ``!isfinite(dy)`` reductions, reached after some iterations."""
    row = nf.BY_ID[rid]
    setup, gpu, _, _ = nf.sized(row, nf.first_guess(row))
    small, k, factor = nf.midrun_lp(rid)
    assert np.array_equal(small.A0, setup.A0)
    base = {q: v.copy() for q, v in setup.arrays.items()}
    slots, _ = nf.slots_of(gpu.handle.launch_info())
    where, near = nf.placement(gpu.handle.launch_info(), setup.B, 2)
    for p in where:                                           # the LP itself, unscaled, in both places: the clean run
        base["b"][p], base["c"][p] = small.arrays["b"][k], small.arrays["c"][k]
    clean, info = gpu.launch(base)

    def make(info):
        arrays = {q: v.copy() for q, v in base.items()}
        for p in where:
            arrays["b"][p] *= factor
        return arrays, None, [(p, "b x %g" % factor) for p in where], where, near

    run_row(row, "mid-run", setup, gpu, clean, info, make)


def _sentinel(shape, dtype, dev):
    import torch
    if dtype == torch.int32:
        return torch.full(shape, fp.SENT32, dtype=torch.int32, device=dev)
    return torch.full(shape, fp._SENT64_I, dtype=torch.int64, device=dev).view(torch.float64)


@pytest.mark.gpu
@pytest.mark.parametrize("family", ["dense", "sparse"])
@pytest.mark.parametrize("batch", ["B=9", "B>slots"])
def test_newton_entry_with_a_poisoned_state(family, batch):
    """pycllp_hip_dense_newton / _sparse_newton: a NaN in x of one state; every other state's dy and nrefine carry the bits of
    the clean call, and the poisoned state's outputs are written."""
    import torch
    from pycllp_amd import _native
    from pycllp_amd.solvers import solver_registry
    lp = tj.inputs(("standard", 16, 32, 8, 1632) if family == "dense" else ("sparse", 40, 90, 8, 0.1, 5, False))
    s = solver_registry["hip_%s_primal_normal" % family](device="cuda:0", reserve_cus=nf.reserve())
    lp.init(s)
    m, N, dev = lp.nrows, lp.ncols, torch.device("cuda:0")
    o = _native.default_opts(**s.options)

    def call(B, bad):
        rs = np.random.RandomState(7)
        x, z = 0.5 + rs.rand(B, N), 0.5 + rs.rand(B, N)
        y, b, c = rs.rand(B, m), rs.rand(B, m), rs.rand(B, N)
        for k in bad:
            x[k, N // 2] = np.nan
        t = [torch.as_tensor(v, device=dev) for v in (x, z, y, b, c)]
        dy, nref = _sentinel((B, m), torch.float64, dev), _sentinel((B,), torch.int32, dev)
        s._handle.newton(None, *t, 1.0, dy, nref, o)
        torch.cuda.synchronize()
        return dict(dy=dy.cpu().numpy(), nrefine=nref.cpu().numpy()), s.launch_info()

    waves = lambda info: info["grid"] * (info["block"] // 64)      # both Newton kernels: one state per wavefront at a time
    B = 9
    clean, info = call(B, [])
    assert info.get("kernel", "wave") == "wave", info
    if batch != "B=9":
        # these launches do not follow reserve_cus: up to two workgroups of eight waves on every compute unit
        B = 16 * torch.cuda.get_device_properties(0).multi_processor_count + 3
        for _ in range(4):
            clean, info = call(B, [])
            if B > waves(info):
                break
            B = 2 * waves(info) + 3
        assert B > waves(info), (B, info)
    bad = [1] if batch == "B=9" else [1, B - 2]
    got, _ = call(B, bad)
    healthy = np.setdiff1d(np.arange(B), bad)
    for q in ("dy", "nrefine"):
        assert not nf.unwritten(got[q]).any(), q
        assert np.array_equal(nf.bits(got[q])[healthy], nf.bits(clean[q])[healthy]), q
    assert np.isfinite(clean["dy"]).all()


LDL_ENTRIES = [("ldl", 0), ("ldl", 1), ("ldl_solve", 0), ("ldl_solve", 1), ("forward_backward_ldl", 0)]


@pytest.mark.gpu
@pytest.mark.parametrize("entry,modified", LDL_ENTRIES, ids=["%s-%s" % (e, "modified" if mod else "plain") for e, mod in LDL_ENTRIES])
@pytest.mark.parametrize("batch", ["B=9", "B>slots"])
def test_ldl_entries_with_a_poisoned_matrix(entry, modified, batch):
    """The LDL' entries (pycllp_amd/ldl.py), the kernel that runs four matrices per workgroup among them (ldl_solve, plain): a
    NaN in one matrix (one factor); every other matrix's outputs carry the bits of the clean call."""
    import torch
    import test_memory_footprint as tmf
    from pycllp_amd import _native
    n = 17
    B = 9 if batch == "B=9" else tmf.ldl_slots(entry, modified) + 3
    A = tmf.spd_batch(n, B, n)
    beta = float(np.sqrt(A.max()))                            # (one value per launch, from the clean data)
    rs = np.random.RandomState(n + 1)
    bad = [1] if batch == "B=9" else [1, B - 2]
    if entry == "ldl":
        ins, target = dict(A=A), "A"
    elif entry == "ldl_solve":
        ins, target = dict(A=A, rhs=rs.rand(B, n)), "A"
    else:
        L = np.tril(rs.rand(B, n, n) - 0.5, -1) / n + np.eye(n)
        ti = np.tril_indices(n)
        ins, target = dict(L=L[:, ti[0], ti[1]], D=0.5 + rs.rand(B, n), b=rs.rand(B, n)), "D"

    def call(ins):
        mem = fp.Plain(tmf.specs_of(entry, ins, B, n, n), torch.device("cuda", 0))
        rc = fp.call(entry, mem.arrays(), B, n=n, modified=modified, beta=beta, delta=1e-6)
        assert rc == 0, (rc, _native.lib().pycllp_hip_last_error())
        mem.check()                                           # every output written, the inputs as they were
        return mem.results()

    clean = call(ins)
    poisoned = {q: v.copy() for q, v in ins.items()}
    for k in bad:
        poisoned[target].reshape(B, -1)[k, 3] = np.nan
    got = call(poisoned)
    healthy = np.setdiff1d(np.arange(B), bad)
    for q in fp.OUTPUTS[entry]:
        assert np.isfinite(clean[q]).all(), q
        assert np.array_equal(nf.bits(got[q])[healthy], nf.bits(clean[q])[healthy]), q


@pytest.mark.gpu
@pytest.mark.parametrize("B", [130, 1366])
def test_plugin_defaults_with_poisoned_lps(B):
    """``hip_dense_primal_normal`` with its default options (hsd='auto', autoscale='auto') on 16 x 32: at B = 130 the band test
    of 'auto' runs on the host, at B = 1 366 (B (m + n) >= 65 536) on the device.  Three poisoned LPs, one with +Inf -- which
    must not switch autoscale on for the batch -- end with status 3, also after the embedding's re-solve; every other LP
    carries the bits of the clean batch's solve.  With ``warm_start=True`` a poisoned batch followed by the clean data: the
    three LPs start cold, the others from their previous optimum."""
    from pycllp_amd.lp import EqualityLP
    from pycllp_amd.solvers import solver_registry
    from pycllp_amd.solvers.hip import autoscale_wanted
    lp = tj.inputs(("standard", 16, 32, B, 1632))
    m, N = lp.nrows, lp.ncols
    assert (B * (m + N) >= 1 << 16) == (B == 1366) and not autoscale_wanted(lp.b, lp.c)
    b, c = np.array(lp.b), np.array(lp.c)
    bad = [1, B // 2, B - 1]
    b[bad[0], m - 1], b[bad[1], 0], c[bad[2], 3] = np.nan, np.inf, np.nan
    sick = EqualityLP(lp.A, b, c, 0.0)
    healthy = np.setdiff1d(np.arange(B), bad)
    names = ("x", "y", "z", "primal_obj", "dual_obj", "status", "iters")

    def solves(batches, **kw):
        s = solver_registry["hip_dense_primal_normal"](device="cuda:0", **kw)
        lp.init(s)
        out = []
        for one in batches:
            one.solve(s)
            out.append({q: np.array(getattr(s, q)) for q in names})
        return out

    clean, = solves([lp])
    got, = solves([sick])
    assert (clean["status"] == 0).all()
    assert got["status"][bad].tolist() == [3, 3, 3], got["status"][bad]
    for q in names:
        assert np.array_equal(nf.bits(got[q])[healthy], nf.bits(clean[q])[healthy]), q
    # warm start: the poisoned batch, then the clean data
    _, after_sick = solves([sick, lp], warm_start=True)
    _, after_clean = solves([lp, lp], warm_start=True)
    assert (after_sick["status"] == 0).all() and (after_clean["status"] == 0).all()
    for q in names:
        assert np.array_equal(nf.bits(after_sick[q])[healthy], nf.bits(after_clean[q])[healthy]), "warm, healthy: " + q
        assert np.array_equal(nf.bits(after_sick[q])[bad], nf.bits(clean[q])[bad]), "warm, the three LPs start cold: " + q
