"""``PYCLLP_FLAG_AUTOSCALE_PER_LP`` (helpers, no tests): the scaling decision taken per LP inside the kernels.

The reference is the library itself through its two older launches.  Under the new flag an LP is either solved exactly as
under PYCLLP_FLAG_AUTOSCALE or with both scale factors 1, and x / 1.0 and x * 1.0 are exact: so an LP that
``autoscale_mask`` calls out of band must carry, in every output, the bits of the PYCLLP_FLAG_AUTOSCALE launch of the same
arrays, and every other LP the bits of the launch without either flag.  No tolerance is involved.

The rows, the healthy batches, the launches and the placement are those of tests/nonfinite_cases.py; ``mixed`` scales the LPs
at ``placement``'s indices out of band (b x 1e3, c x 1e-2 and, with bounds, u x 1e3 with b)."""
import numpy as np

import nonfinite_cases as nf

PER_LP, AUTOSCALE = 256, nf.AUTOSCALE_FLAG
B_FACTOR, C_FACTOR = 1e3, 1e-2
N_SCALED = 8                                  # LPs scaled out of band per batch (``placement`` offers eight)
EDGES = (10.0, float(np.nextafter(10.0, np.inf)), 0.1, float(np.nextafter(0.1, 0.0)))


def mask_of(arrays):
    """``autoscale_mask`` of a batch as its entry takes it (b, c and, with bounds, u), as a numpy array."""
    from pycllp_amd.solvers.hip import autoscale_mask
    return np.asarray(autoscale_mask(arrays["b"], arrays["c"], arrays.get("u")))


def plain_mask(b, c, u=None):
    """The rule as a loop over the LPs, in plain Python floats -- what ``autoscale_mask`` is held against."""
    def out(mx):
        return bool(np.isfinite(mx)) and (mx < 0.1 or mx > 10.0)
    b, c = np.atleast_2d(np.asarray(b, dtype=np.float64)), np.atleast_2d(np.asarray(c, dtype=np.float64))
    u = None if u is None else np.atleast_2d(np.asarray(u, dtype=np.float64))
    res = []
    for k in range(b.shape[0]):
        v = False
        for row in (b[k], c[k]):
            if row.size:
                a = np.abs(row)
                v = v or out(np.nan if np.isnan(a).any() else a.max())
        if u is not None:
            fin = [float(t) for t in u[k] if np.isfinite(t) and t > 0]
            v = v or (len(fin) > 0 and out(max(fin)))
        res.append(v)
    return np.array(res, dtype=bool)


def mixed(arrays, idx):
    """Copies of ``arrays`` with the LPs ``idx`` scaled out of band (infinite and zero u stay what they are)."""
    out = {q: v.copy() for q, v in arrays.items()}
    idx = np.asarray(idx, dtype=int)
    out["b"][idx] *= B_FACTOR
    out["c"][idx] *= C_FACTOR
    if "u" in out:
        out["u"][idx] *= B_FACTOR
    return out


def launch(gpu, arrays, flags, **overrides):
    """(results, launch_info) of one launch of ``gpu``'s entry with ``flags`` added to the row's own."""
    saved = gpu.flags
    gpu.flags = saved | flags
    try:
        return gpu.launch(arrays, **overrides)
    finally:
        gpu.flags = saved


def three(gpu, arrays, base=0, **overrides):
    """The results of the three launches on the same arrays: no scaling flag, PYCLLP_FLAG_AUTOSCALE, the new flag."""
    return tuple(launch(gpu, arrays, base | f, **overrides)[0] for f in (0, AUTOSCALE, PER_LP))


def same_bits(names, r1, r2):
    """bool [B]: the LPs whose outputs ``names`` agree bit for bit in the two results."""
    ok = None
    for q in names:
        same = nf.bits(np.asarray(r1[q])) == nf.bits(np.asarray(r2[q]))
        same = same if same.ndim == 1 else same.reshape(same.shape[0], -1).all(axis=1)
        ok = same if ok is None else ok & same
    return ok


def assert_bites(names, r0, r8, mask, what):
    """The two reference launches differ on at least one out-of-band LP: otherwise the verdicts cannot be observed."""
    assert mask.any(), "%s: no LP out of band" % what
    assert (~same_bits(names, r0, r8))[mask].any(), "%s: vacuous -- no out-of-band LP differs between the two reference launches" % what


def assert_per_lp(names, got, r0, r8, mask, what, skip=()):
    """Every output of every LP of ``got`` carries the bits of ``r8`` where ``mask`` is set and of ``r0`` elsewhere."""
    B = mask.shape[0]
    keep = np.ones(B, dtype=bool)
    keep[list(skip)] = False
    for q in names:
        want = np.where(mask.reshape((B,) + (1,) * (np.asarray(r0[q]).ndim - 1)), r8[q], r0[q])
        same = nf.bits(np.asarray(got[q])) == nf.bits(want)
        same = same if same.ndim == 1 else same.reshape(B, -1).all(axis=1)
        bad = np.flatnonzero(~same & keep)
        assert bad.size == 0, "%s: %s of LP %d (%s) does not carry the bits of the %s launch (%d LPs differ)" % (
            what, q, bad[0], "out of band" if mask[bad[0]] else "in band", "AUTOSCALE" if mask[bad[0]] else "flag-less", bad.size)


def with_max(v, target):
    """``v`` rescaled so that max|v| is exactly ``target`` (v / max|v| has the maximum exactly 1)."""
    v = np.asarray(v, dtype=np.float64)
    w = (v / np.abs(v).max()) * target
    assert np.abs(w).max() == target
    return w


def edge_lps(arrays, idx):
    """Copies of ``arrays`` in which the LPs ``idx`` (at least len(EDGES) * 2 + 2, with bounds len(EDGES) * 3 + 3) sit on and
    next to the band edges: max|b| = each of EDGES with max|c| = 2 (and the largest finite positive u = 2), the same for c, an LP
    with b = 0, and with bounds the same for u and an LP whose bounds are all infinite or zero.  Returns (arrays, [(LP, what)])."""
    out = {q: v.copy() for q, v in arrays.items()}
    bounded = "u" in out
    todo = [("b", t) for t in EDGES] + [("c", t) for t in EDGES] + [("b=0", None)]
    if bounded:
        todo += [("u", t) for t in EDGES] + [("u inf or 0", None)]
    assert len(idx) >= len(todo)
    what = []
    for k, (which, t) in zip(idx, todo):
        out["b"][k] = with_max(out["b"][k], 2.0)
        out["c"][k] = with_max(out["c"][k], 2.0)
        if bounded:
            u = out["u"][k]
            fin = np.isfinite(u) & (u > 0)
            assert fin.any()
            u[fin] = with_max(u[fin], 2.0)
        if which == "b=0":
            out["b"][k] = 0.0
        elif which == "u inf or 0":
            out["u"][k][fin] = np.inf
        elif which == "u":
            u[fin] = with_max(u[fin], t)
        else:
            out[which][k] = with_max(out[which][k], t)
        what.append((int(k), which if t is None else "max %s = %r" % (which, t)))
    return out, what


def general_arrays(glp):
    """The arrays of a GeneralLP that its plugins' device entries take."""
    return {q: np.array(getattr(glp, q), dtype=np.float64) for q in ("a", "b", "c", "l", "u")}


def mixed_general(glp, idx):
    """A GeneralLP with the LPs ``idx`` scaled out of band: a, b, l, u x 1e3 and c x 1e-2 (A unchanged)."""
    from pycllp_amd.lp import GeneralLP
    v = general_arrays(glp)
    idx = np.asarray(idx, dtype=int)
    for q in ("a", "b", "l", "u"):
        v[q][idx] *= B_FACTOR
    v["c"][idx] *= C_FACTOR
    return GeneralLP(A=glp.A, b=v["b"], c=v["c"], a=v["a"], l=v["l"], u=v["u"], f=np.array(glp.f))


def mixed_equality(lp, idx):
    from pycllp_amd.lp import EqualityLP
    b, c = np.array(lp.b, dtype=np.float64), np.array(lp.c, dtype=np.float64)
    idx = np.asarray(idx, dtype=int)
    b[idx] *= B_FACTOR
    c[idx] *= C_FACTOR
    return EqualityLP(lp.A, b, c, np.array(lp.f))
