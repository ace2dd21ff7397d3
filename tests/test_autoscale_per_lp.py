"""PYCLLP_FLAG_AUTOSCALE_PER_LP / ``autoscale='per_lp'``: the scaling decision of one LP does not depend on its batch.

CPU: ``autoscale_mask`` against a plain loop (numpy and torch; empty arrays, u=None, non-finite entries, the band edges) and
``autoscale_wanted == autoscale_mask.any()``; ``plugin_options``; the constant in the header and the loader; the refusals of
the solve entries, called with a handle of zero bytes before any HIP call.  GPU (tests/autoscale_cases.py): on every row of
tests/nonfinite_cases.py a batch with some LPs scaled out of band is launched without a scaling flag, with
PYCLLP_FLAG_AUTOSCALE and with the new flag, and under the new flag every output of every LP carries the bits of the
PYCLLP_FLAG_AUTOSCALE launch where ``autoscale_mask`` is set and of the flag-less launch elsewhere; an in-band LP keeps its bits
whatever else is in the batch; the band edges; an LP deferred to the block kernel; non-finite neighbours; the seven plugins."""
import ctypes
import os
import re

import numpy as np
import pytest

import autoscale_cases as ac
import nonfinite_cases as nf
from pycllp_amd import _native
from pycllp_amd.solvers import hip, solver_registry

ROW_IDS = [r.id for r in nf.ROWS]
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- CPU ------------------------------------------------------------------------------------------------------------------
def mask_inputs():
    """[(name, b, c, u)]: batches for the rule, the band edges and non-finite entries among them."""
    rs = np.random.RandomState(3)
    lo_out, hi_out = np.nextafter(0.1, 0.0), np.nextafter(10.0, np.inf)
    b = 0.5 + rs.rand(12, 5)
    c = 0.5 + rs.rand(12, 7)
    u = 0.5 + rs.rand(12, 7)
    for k, t in enumerate((10.0, hi_out, 0.1, lo_out)):
        b[k] = ac.with_max(b[k], t)
        c[4 + k] = -ac.with_max(c[4 + k], t)
        u[8 + k] = ac.with_max(u[8 + k], t)
    out = [("edges", b, c, u), ("edges, no u", b, c, None)]
    b2, c2, u2 = 0.5 + rs.rand(10, 4), 0.5 + rs.rand(10, 6), 0.5 + rs.rand(10, 6)
    b2[0, 1] = np.nan; b2[1, 0] = np.inf; c2[2, 3] = -np.inf; c2[3, 5] = np.nan
    b2[4] *= 1e3; b2[4, 2] = np.nan                      # out of band but for the NaN: the maximum is not finite
    b2[5] = 0.0                                          # b = 0 is out of band
    u2[6] = np.inf; u2[7] = 0.0; u2[8] = [np.inf, 0.0, -1.0, np.nan, np.inf, 0.0]      # no finite positive u: left out
    u2[9] = [np.inf, 0.0, 25.0, np.nan, 1.0, -3.0]                                     # ... one of 25: out of band
    c2[6] *= 1e-3
    out.append(("non-finite", b2, c2, u2))
    out.append(("non-finite, no u", b2, c2, None))
    out.append(("no LPs", np.zeros((0, 4)), np.zeros((0, 6)), np.zeros((0, 6))))
    out.append(("no rows", np.zeros((3, 0)), 0.5 + rs.rand(3, 6), None))
    out.append(("no columns", 0.5 + rs.rand(3, 4), np.zeros((3, 0)), None))
    out.append(("one LP as vectors", np.array([0.5, 20.0]), np.array([1.0, 2.0, 3.0]), None))
    return out


MASK_INPUTS = mask_inputs()


@pytest.mark.parametrize("name,b,c,u", MASK_INPUTS, ids=[t[0] for t in MASK_INPUTS])
def test_autoscale_mask_is_the_rule_per_lp(name, b, c, u):
    import torch
    want = ac.plain_mask(b, c, u)
    got = hip.autoscale_mask(b, c, u)
    assert isinstance(got, np.ndarray) and got.dtype == bool and got.shape == want.shape, (got, want)
    assert np.array_equal(got, want), (name, got, want)
    tt = lambda v: None if v is None else torch.as_tensor(v)
    gt = hip.autoscale_mask(tt(b), tt(c), tt(u))
    assert isinstance(gt, torch.Tensor) and gt.dtype == torch.bool and np.array_equal(gt.numpy(), want), (name, gt, want)
    assert bool(hip.autoscale_wanted(b, c, u)) == bool(want.any())
    assert bool(hip.autoscale_wanted(tt(b), tt(c), tt(u))) == bool(want.any())
    if name == "no columns":                                  # (bounds without columns: the mask alone takes them)
        assert not hip.autoscale_mask(b, c, np.zeros((3, 0))).any() and not hip.autoscale_mask(tt(b), tt(c), torch.zeros(3, 0)).any()
    if name == "edges":
        assert want.tolist() == [False, True, False, True] * 3
    if name == "non-finite":
        assert want.tolist() == [False, False, False, False, False, True, True, False, False, True]


def test_autoscale_wanted_is_any_of_the_mask_on_the_rows_inputs():
    """... on the inputs of the existing tests: every row's healthy batch, and the same with LPs scaled out of band."""
    for row in nf.ROWS:
        setup = nf.Setup(row, 6)
        for arrays in (setup.arrays, ac.mixed(setup.arrays, [1, 4])):
            m = ac.mask_of(arrays)
            assert np.array_equal(m, ac.plain_mask(arrays["b"], arrays["c"], arrays.get("u"))), row.id
            assert bool(hip.autoscale_wanted(arrays["b"], arrays["c"], arrays.get("u"))) == bool(m.any()), row.id
        assert m[[1, 4]].all(), row.id


def test_plugin_options_takes_per_lp():
    F = _native
    hsd, autoscale, warm, lift, options = hip.plugin_options({}, autoscale="per_lp")
    assert autoscale == "per_lp" and options["flags"] == F.FLAG_AUTOSCALE_PER_LP == 256
    assert hip.plugin_options({"flags": 256})[1] == "per_lp"                       # the flag alone switches it on, as 8 does True
    assert hip.plugin_options({"flags": 256 | 4}, autoscale=False)[4]["flags"] == 256 | 4
    assert hip.plugin_options({"flags": 4}, autoscale="per_lp", predcorr=True)[4]["flags"] == 4 | 256 | F.FLAG_PREDCORR
    # every other value as before
    assert hip.plugin_options({})[1] == "auto" and "flags" not in hip.plugin_options({})[4]
    assert hip.plugin_options({}, autoscale=True)[1] is True and hip.plugin_options({}, autoscale=True)[4]["flags"] == 8
    assert hip.plugin_options({}, autoscale=False)[1] is False and "flags" not in hip.plugin_options({}, autoscale=False)[4]
    assert hip.plugin_options({"flags": 8})[1] is True and hip.plugin_options({"flags": 8}, autoscale=False)[4]["flags"] == 8
    assert hip.plugin_options({}, autoscale=1)[1] is True
    with pytest.raises(ValueError):
        hip.plugin_options({}, autoscale="sometimes")
    for kw in (dict(options={"flags": 8}, autoscale="per_lp"), dict(options={"flags": 256}, autoscale=True),
               dict(options={"flags": 8 | 256})):
        with pytest.raises(ValueError):
            hip.plugin_options(**kw)
    for name, cls in sorted(solver_registry.items()):
        if name.startswith("hip_"):
            s = cls(autoscale="per_lp")
            assert s.autoscale == "per_lp" and s.options["flags"] & 256, name
            assert hip.solve_opts(s.options).flags & 256
            with pytest.raises(ValueError):
                cls(autoscale="sometimes")
    assert len([n for n in solver_registry if n.startswith("hip_")]) == 7


def test_flag_in_header_and_loader():
    text = open(os.path.join(ROOT, "include", "pycllp_hip.h")).read()
    m = re.search(r"^#define PYCLLP_FLAG_AUTOSCALE_PER_LP (\d+)", text, re.M)
    assert m and int(m.group(1)) == 256 == _native.FLAG_AUTOSCALE_PER_LP
    values = [int(v) for v in re.findall(r"^#define PYCLLP_FLAG_\w+ (\d+)", text, re.M)]
    assert 256 in values and len(values) == len(set(values)) and all(v > 0 and v & (v - 1) == 0 for v in values)


# entry -> (its device arrays, flags it rejects whatever else is set): every solve entry of the header
SOLVE = ("b", "c", "x", "y", "z", "pobj", "dobj", "status", "iters")
BOUNDED = ("b", "c", "u", "x", "y", "z", "s", "pobj", "dobj", "status", "iters")
GROUP_REJECTS = ("HSD", "PREDCORR", "WARM_START", "WAVE_KERNEL", "NO_SLACK_PATH")
WAVE_REJECTS = GROUP_REJECTS + ("BLOCK_KERNEL", "FORCE_GUARD_PATH")
SOLVE_ENTRIES = {
    "pycllp_hip_dense_solve": (SOLVE, ()),
    "pycllp_hip_sparse_solve": (SOLVE, ()),
    "pycllp_hip_sparse_solve_batch": (("Adata",) + SOLVE, ()),
    "pycllp_hip_dense_solve_bounded": (BOUNDED, GROUP_REJECTS),
    "pycllp_hip_dense_solve_batch": (("A",) + SOLVE, GROUP_REJECTS[:4]),
    "pycllp_hip_dense_solve_batch_bounded": (("A",) + BOUNDED, GROUP_REJECTS),
    "pycllp_hip_sparse_solve_bounded": (BOUNDED, WAVE_REJECTS),
    "pycllp_hip_sparse_solve_batch_bounded": (("Adata",) + BOUNDED, WAVE_REJECTS),
}


@pytest.mark.parametrize("entry", sorted(SOLVE_ENTRIES))
def test_solve_entries_refuse_both_flags_together(entry):
    """PYCLLP_E_BADARG before the handle is read (64 zero bytes stand in for it) and before any HIP call; and a flag an entry
    refuses with PYCLLP_FLAG_AUTOSCALE it refuses with the new flag, with the same code."""
    L = _native.lib()
    arrays, rejected = SOLVE_ENTRIES[entry]
    fn = getattr(L, entry)
    fake = ctypes.create_string_buffer(64)
    handle = ctypes.cast(fake, ctypes.c_void_p)

    def call(flags, B=4):
        args = [handle, B]
        for name in arrays:
            args.append(ctypes.c_void_p(8))
            if name == "A":
                args.append(5)
        return fn(*args, ctypes.byref(_native.default_opts(flags=flags)), None)

    both = _native.FLAG_AUTOSCALE | _native.FLAG_AUTOSCALE_PER_LP
    for extra in (0, _native.FLAG_FORCE_GUARD_PATH if "FORCE_GUARD_PATH" not in rejected else 0):
        assert call(both | extra) == -1, extra
        msg = L.pycllp_hip_last_error()
        # (pycllp_hip_sparse_solve_batch shares its body, and its messages, with pycllp_hip_sparse_solve)
        assert msg.startswith(b"pycllp_hip_sparse_solve:" if entry == "pycllp_hip_sparse_solve_batch" else entry.encode() + b":"), msg
        assert b"PYCLLP_FLAG_AUTOSCALE and PYCLLP_FLAG_AUTOSCALE_PER_LP exclude each other" in msg, msg
    assert call(both, B=0) == -1                              # (before the empty batch's early return, too)
    for name in rejected:
        f = getattr(_native, "FLAG_" + name)
        codes = [call(f | s) for s in (_native.FLAG_AUTOSCALE, _native.FLAG_AUTOSCALE_PER_LP)]
        assert codes == [-1, -1], (name, codes)
    assert fake.raw == bytes(64)


# ---- GPU ------------------------------------------------------------------------------------------------------------------
_SIZED = {}


def sized(rid):
    """``nonfinite_cases.sized`` of a row, once per session: (setup, gpu, clean, info)."""
    if rid not in _SIZED:
        row = nf.BY_ID[rid]
        _SIZED.clear()                                        # (one row's handle and batch at a time)
        _SIZED[rid] = nf.sized(row, nf.first_guess(row))
    return _SIZED[rid]


def mixed_batch(setup, info):
    idx, near = nf.placement(info, setup.B, ac.N_SCALED)
    arrays = ac.mixed(setup.arrays, idx)
    mask = ac.mask_of(arrays)
    assert mask[idx].all()
    return arrays, mask, idx, near


@pytest.mark.gpu
@pytest.mark.parametrize("row", nf.ROWS, ids=ROW_IDS)
def test_mixed_batch_every_lp_carries_the_bits_of_its_own_verdict(row):
    setup, gpu, clean, info = sized(row.id)
    nf.assert_served(row, info, setup)
    arrays, mask, idx, near = mixed_batch(setup, info)
    names = nf.outputs_of(setup)
    r0, r8, rp = ac.three(gpu, arrays)
    print("%-34s B=%d out of band %d, LPs that differ between the reference launches: %d" % (
        row.id, setup.B, mask.sum(), (~ac.same_bits(names, r0, r8)).sum()))
    ac.assert_bites(names, r0, r8, mask, row.id)
    for q in names:
        assert not nf.unwritten(rp[q]).any(), q
    ac.assert_per_lp(names, rp, r0, r8, mask, row.id)


@pytest.mark.gpu
@pytest.mark.parametrize("rid", ["slack-16x32-plain", "tables-33x193-plain"])
def test_in_band_lp_keeps_its_bits_whatever_else_is_in_the_batch(rid):
    """What 'auto' lacks: under the new flag an in-band LP of the mixed batch has the bits it has in the all-healthy batch."""
    setup, gpu, clean, info = sized(rid)
    arrays, mask, idx, near = mixed_batch(setup, info)
    names = nf.outputs_of(setup)
    alone, _ = ac.launch(gpu, setup.arrays, ac.PER_LP)
    among, _ = ac.launch(gpu, arrays, ac.PER_LP)
    inband = ~mask
    assert inband.sum() == setup.B - len(idx) and inband[near].all()
    same = ac.same_bits(names, alone, among)
    assert same[inband].all(), "LP %d changes with its batch mates" % np.flatnonzero(~same & inband)[0]
    # ... which the batch-wide decision does not give: with PYCLLP_FLAG_AUTOSCALE for all, as 'auto' decides for this batch,
    # the in-band LPs move
    assert hip.autoscale_wanted(arrays["b"], arrays["c"]) and not hip.autoscale_wanted(setup.arrays["b"], setup.arrays["c"])
    for_all, _ = ac.launch(gpu, arrays, ac.AUTOSCALE)
    assert not ac.same_bits(names, clean, for_all)[inband].all()


@pytest.mark.gpu
@pytest.mark.parametrize("rid", ["slack-16x32-plain", "slack-24x30-bounded"])
def test_band_edges(rid):
    """max|b|, max|c| (and the largest finite positive u) exactly 10, the next double above, exactly 0.1, the next double below;
    b = 0; bounds that are all infinite or zero: the verdict of each LP, seen through whose bits it carries, is
    ``autoscale_mask``'s."""
    setup, gpu, clean, info = sized(rid)
    n = len(ac.EDGES) * (3 if setup.bounded else 2) + (2 if setup.bounded else 1)
    idx = [int(k) for k in np.linspace(0, setup.B - 1, n).round()]
    assert len(set(idx)) == n
    arrays, what = ac.edge_lps(setup.arrays, idx)
    mask = ac.mask_of(arrays)
    want = [False, True, False, True] * 2 + [True] + ([False, True, False, True, False] if setup.bounded else [])
    assert mask[idx].tolist() == want, list(zip(what, mask[idx]))
    assert not mask[np.setdiff1d(np.arange(setup.B), idx)].any()
    names = nf.outputs_of(setup)
    r0, r8, rp = ac.three(gpu, arrays)
    differ = ~ac.same_bits(names, r0, r8)
    assert differ[idx].all(), "an edge LP whose verdict cannot be seen: %r" % ([w for (k, w) in what if not differ[k]],)
    ac.assert_per_lp(names, rp, r0, r8, mask, rid)


@pytest.mark.gpu
def test_dense_solve_refuses_the_removed_kernel_with_either_scaling_flag():
    """The one refusal that names PYCLLP_FLAG_AUTOSCALE itself (pycllp_hip_dense_solve with PYCLLP_FLAG_WAVE_KERNEL) is made
    after the handle is read, so it takes a real handle: PYCLLP_E_BADARG with either flag, PYCLLP_E_UNSUPPORTED without."""
    setup, gpu, clean, info = sized("slack-16x32-plain")
    F = _native
    for flag in (F.FLAG_AUTOSCALE, F.FLAG_AUTOSCALE_PER_LP):
        with pytest.raises(ValueError, match="PYCLLP_FLAG_AUTOSCALE"):
            ac.launch(gpu, setup.arrays, F.FLAG_WAVE_KERNEL | flag)
    with pytest.raises(NotImplementedError):
        ac.launch(gpu, setup.arrays, F.FLAG_WAVE_KERNEL)
    with pytest.raises(ValueError, match="exclude each other"):
        ac.launch(gpu, setup.arrays, F.FLAG_AUTOSCALE | F.FLAG_AUTOSCALE_PER_LP)


@pytest.mark.gpu
def test_deferred_lps_get_the_same_verdict_on_the_block_kernel():
    """PYCLLP_FLAG_FORCE_GUARD_PATH on the wave kernel hands every LP to the block kernel, which takes the verdict again.  The
    matching PYCLLP_FLAG_BLOCK_KERNEL launches carry PYCLLP_FLAG_FORCE_GUARD_PATH too: the block kernel reads that flag itself
    (its guarded LDL' for every LP), and a deferred LP is solved there under the options of the call that deferred it."""
    rid = "tables-33x193-plain"
    setup, gpu, clean, info = sized(rid)
    arrays, mask, idx, near = mixed_batch(setup, info)
    names = nf.outputs_of(setup)
    F = _native
    b0, i0 = ac.launch(gpu, arrays, F.FLAG_BLOCK_KERNEL | F.FLAG_FORCE_GUARD_PATH)
    b8, _ = ac.launch(gpu, arrays, F.FLAG_BLOCK_KERNEL | F.FLAG_FORCE_GUARD_PATH | F.FLAG_AUTOSCALE)
    assert i0.get("kernel") == "block", i0
    got, info2 = ac.launch(gpu, arrays, F.FLAG_FORCE_GUARD_PATH | F.FLAG_AUTOSCALE_PER_LP)
    assert info2.get("kernel") == "wave", info2                # (the launch that deferred them)
    ac.assert_bites(names, b0, b8, mask, rid)
    ac.assert_per_lp(names, got, b0, b8, mask, rid + " deferred")


@pytest.mark.gpu
@pytest.mark.parametrize("rid", ["slack-16x32-plain", "tables-33x193-plain"])
def test_non_finite_lps_among_mixed_neighbours(rid):
    """A NaN in b of one LP and an Inf in c of another: both end with status 3, every other LP keeps the bits of its verdict."""
    setup, gpu, clean, info = sized(rid)
    arrays, mask, idx, near = mixed_batch(setup, info)
    names = nf.outputs_of(setup)
    r0, r8, _ = ac.three(gpu, arrays)
    bad = [near[0], idx[1] + 1]                                # a first-wave neighbour of a scaled LP; the LP after another scaled one
    assert not set(bad) & set(idx)
    arrays = {q: v.copy() for q, v in arrays.items()}
    arrays["b"][bad[0], setup.m - 1] = np.nan
    arrays["c"][bad[1], 0] = np.inf
    got, _ = ac.launch(gpu, arrays, ac.PER_LP)
    assert got["status"][bad].tolist() == [3, 3], got["status"][bad]
    ac.assert_per_lp(names, got, r0, r8, mask, rid + " non-finite", skip=bad)


# plugin -> the row whose healthy LP object (EqualityLP or GeneralLP) it solves natively at its smallest point
PLUGINS = {
    "hip_dense_primal_normal": "slack-16x32-plain",
    "hip_sparse_primal_normal": "tables-33x193-plain",
    "hip_dense_batch_primal_normal": "perA-dense-plain",
    "hip_general_primal_normal": "slack-24x30-bounded",
    "hip_sparse_general_primal_normal": "tables-33x193-bounded",
    "hip_general_batch_primal_normal": "perA-dense-bounded",
    "hip_sparse_general_batch_primal_normal": "perA-sparse-bounded",
}
ATTRS = ("x", "y", "z", "s", "primal_obj", "dual_obj", "status", "iters")


def plugin_mask(lp):
    """``autoscale_mask`` on what the plugin's kernel is handed: the LP itself, or the bounded form of a GeneralLP."""
    if hasattr(lp, "to_bounded_equality_form"):
        blp, _ = lp.to_bounded_equality_form()
        return np.asarray(hip.autoscale_mask(blp.b, blp.c, blp.u))
    return np.asarray(hip.autoscale_mask(lp.b, lp.c))


def device_call(name, s, lp):
    """The plugin's device-resident entries on ``lp``'s arrays: {entry: results as numpy}."""
    import torch
    out = {}
    if name in ("hip_dense_primal_normal", "hip_sparse_primal_normal"):
        out["solve_device"] = s.solve_device(np.array(lp.b), np.array(lp.c))
    elif name == "hip_dense_batch_primal_normal":
        import dense_batch_cases as dbc
        out["solve_device"] = s.solve_device(dbc.matrices(lp)[:, :, :s.a_cols].copy(), np.array(lp.b), np.array(lp.c))
    else:
        v = ac.general_arrays(lp)
        f = np.broadcast_to(np.asarray(lp.f, dtype=np.float64), (lp.nproblems,)).copy()
        if name in ("hip_general_primal_normal", "hip_sparse_general_primal_normal"):
            out["solve_device"] = s.solve_device(v["a"], v["b"], v["c"], v["l"], v["u"], f)
        else:
            data = np.ascontiguousarray(np.broadcast_to(np.asarray(lp.A.data, dtype=np.float64), (lp.nproblems, lp.A.data.shape[1])))
            out["solve_device_general"] = s.solve_device_general(data, v["a"], v["b"], v["c"], v["l"], v["u"], f)
    torch.cuda.synchronize()
    return {e: {q: t.cpu().numpy() for q, t in r.items() if q != "B" and hasattr(t, "cpu") and t.dim() <= 2 and q not in ("packed",)}
            for e, r in out.items()}


@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(PLUGINS))
def test_plugins_take_per_lp(name):
    """``autoscale='per_lp'`` through ``solve(lp)`` and the device-resident entries: per LP the bits of ``autoscale=True`` or of
    ``autoscale=False`` by ``autoscale_mask``.  hsd=False: the native kernel's own results (the re-solves of hsd='auto' go
    through other forms of the LP, whose verdicts are their own)."""
    row = nf.BY_ID[PLUGINS[name]]
    B = 40
    lp = nf.healthy_lp(row, B)
    idx = [1, 7, 8, 22, B - 1]
    lp = ac.mixed_general(lp, idx) if hasattr(lp, "to_bounded_equality_form") else ac.mixed_equality(lp, idx)
    mask = plugin_mask(lp)
    assert mask[idx].all()
    res, dev = {}, {}
    for mode in (False, True, "per_lp"):
        s = solver_registry[name](device="cuda:0", autoscale=mode, hsd=False)
        lp.init(s)
        lp.solve(s)
        assert getattr(s, "_handle", None) is not None and getattr(s, "_delegate", None) is None, "%s does not solve %s natively" % (name, row.id)
        res[mode] = {q: np.array(getattr(s, q)) for q in ATTRS if hasattr(s, q)}
        dev[mode] = device_call(name, s, lp)
    names = sorted(res[False])
    assert {"x", "y", "z", "status", "iters", "primal_obj", "dual_obj"} <= set(names)
    ac.assert_bites(names, res[False], res[True], mask, name)
    ac.assert_per_lp(names, res["per_lp"], res[False], res[True], mask, name + " solve(lp)")
    for entry in dev[False]:
        dn = sorted(q for q in dev[False][entry] if q != "invalid")
        assert {"x", "y", "z", "status", "iters"} <= set(dn), dn
        ac.assert_bites(dn, dev[False][entry], dev[True][entry], mask, name + " " + entry)
        ac.assert_per_lp(dn, dev["per_lp"][entry], dev[False][entry], dev[True][entry], mask, name + " " + entry)


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["hip_dense_primal_normal", "hip_dense_batch_primal_normal", "hip_general_primal_normal"])
def test_hsd_auto_re_solves_carry_the_flag(name, monkeypatch):
    """max_iter = 3 ends every LP at the iteration limit, so the default hsd='auto' solves them all again: on the embedding
    (dense plugin), as a per-problem subset on the sparse plugin (per-problem dense A), through the expansion on a dense plugin
    of its own (GeneralLP).  Every launch those solvers make -- all go through ``HipDensePrimalNormalSolver._launch`` --
    carries the new flag, none PYCLLP_FLAG_AUTOSCALE, and the re-solves on the embedding carry PYCLLP_FLAG_HSD beside it."""
    F = _native
    seen = []
    inner = hip.HipDensePrimalNormalSolver._launch

    def recording(self, b, c, out, o, *a, **kw):
        seen.append((type(self).__name__, int(o.flags)))
        return inner(self, b, c, out, o, *a, **kw)

    monkeypatch.setattr(hip.HipDensePrimalNormalSolver, "_launch", recording)
    lp = nf.healthy_lp(nf.BY_ID[PLUGINS[name]], 12)
    lp = ac.mixed_general(lp, [1, 7]) if hasattr(lp, "to_bounded_equality_form") else ac.mixed_equality(lp, [1, 7])
    s = solver_registry[name](device="cuda:0", autoscale="per_lp", max_iter=3)
    assert s.hsd == "auto"
    lp.init(s)
    lp.solve(s)
    own = name == "hip_dense_primal_normal"
    assert len(seen) >= (2 if own else 1), seen
    assert all(f & F.FLAG_AUTOSCALE_PER_LP and not f & F.FLAG_AUTOSCALE for _, f in seen), seen
    assert any(f & F.FLAG_HSD for _, f in seen), seen          # a re-solve on the embedding was among them
    if own:
        assert not seen[0][1] & F.FLAG_HSD and seen[1][1] & F.FLAG_HSD, seen


@pytest.mark.gpu
def test_dense_plugin_host_pipeline_runs_once():
    """A batch large enough for the host pipeline (B (m + n) >= 65 536 at 16 x 32) with LPs out of band: 'auto' solves its
    chunks twice (the speculative pass, then the pass with the flag), 'per_lp' once -- with every LP's bits by its verdict.
    The default hsd='auto': its re-solves carry the flag too."""
    import trajectory as tj
    B = 1366
    lp0 = tj.inputs(("standard", 16, 32, B, 1632))
    assert B * (lp0.nrows + lp0.ncols) >= 1 << 16
    idx = [1, 2, 300, 700, B - 1]
    lp = ac.mixed_equality(lp0, idx)
    mask = plugin_mask(lp)
    assert mask.sum() == len(idx)
    res, launches = {}, {}
    for mode in (False, True, "auto", "per_lp"):
        s = solver_registry["hip_dense_primal_normal"](device="cuda:0", autoscale=mode)
        lp.init(s)
        count = [0]
        inner = s._launch

        def counted(*a, _inner=inner, _count=count, **kw):
            _count[0] += 1
            return _inner(*a, **kw)

        s._launch = counted
        lp.solve(s)
        res[mode] = {q: np.array(getattr(s, q)) for q in ATTRS if hasattr(s, q)}
        launches[mode] = count[0], int((res[mode]["status"] != 0).sum())
    names = sorted(res[False])
    chunks = max(1, min(s.PIPELINE_CHUNKS, B // s.PIPELINE_MIN_BATCH))
    print("launches (solve chunks + re-solves, LPs not optimal):", launches)
    # every launch beyond the chunks is one hsd='auto' re-solve, made only when some LP did not end optimal
    resolves = lambda mode: launches[mode][0] - chunks * (2 if mode == "auto" else 1)
    for mode in launches:
        assert resolves(mode) in (0, 1), (mode, launches)
    assert launches["auto"][0] - resolves("auto") == 2 * chunks and launches["per_lp"][0] - resolves("per_lp") == chunks
    ac.assert_bites(names, res[False], res[True], mask, "host pipeline")
    ac.assert_per_lp(names, res["per_lp"], res[False], res[True], mask, "host pipeline")
    assert ac.same_bits(names, res["auto"], res[True]).all()
