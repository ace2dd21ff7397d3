"""Helpers of tests/test_general_batch_hsd.py (no tests): batches of bounded LPs in which every LP has its own dense matrix and
the three verdicts interleave, the twin of the embedding (tests/bounded_hsd_twin.py) run LP by LP with that LP's own matrix, the
launch of pycllp_hip_dense_solve_batch_bounded_hsd, and the GeneralLP batch of the plugin test."""
import ctypes
import functools

import numpy as np

import bounded_hsd_twin as tw
import footprint as fp
from pycllp_amd import _native
from test_general_solver import make_general

ENTRY = "pycllp_hip_dense_solve_batch_bounded_hsd"
SHARED_ENTRY = "pycllp_hip_dense_solve_bounded_hsd"
SIZES = list(tw.MIXED_SEEDS)       # (m', n): one per shape of the six, then 1 x 1 and the two exact fills
B_GPU = 64
OUT = fp.BOUNDED_OUT
TWIN_OUT = OUT + ("floored",)
SCALE_B, SCALE_C = 1e4, 1e-3
CERT = 1e-7
PA_SEED = 7919
GAP = 1e-9          # what the twin's own primal-dual gap must stay within where the kernel's objectives are held to 1e-9 of the twin's
# (m', n) -> the offset of U's generator where it is not PA_SEED: the first one from PA_SEED up under which the batch has the
# properties it is specified with (``fixture_holds``).  With PA_SEED itself the twin needs 31 iterations for LP 62 of 32 x 64, and
# its own gap is 1.5e-9 at LP 59 of 14 x 30 (optimum 686.57) and 1.004e-9 at 24 x 32: a reference that does not settle its own
# objective to 1e-9 cannot hold a kernel to it
PA_OFFSETS = {(14, 30): PA_SEED + 1, (24, 32): PA_SEED + 1, (32, 64): PA_SEED + 1}


def mixed_batch_pa(mp, nd, B, seed, offset=PA_SEED):
    """``tw.mixed_batch(mp, nd, B, seed)`` with LP k on its own matrix A_k = [A_dense o U[0.75, 1.25) | I] (rng ``seed + offset``)
    and b, c rebuilt by mixed_batch's own rules on A_k: b_k = A_k x0 (k mod 3 != 1), c_k = A_k'y0 - z0 + s0 (k mod 3 = 0),
    b_{k,i} = -(10 + sum over A_k,ij < 0 of |A_k,ij| u_j) (k mod 3 = 1).  x0, y0, z0, s0 are mixed_batch's: its draws are
    replayed, and the replay is checked against what it returned.  -> (Ad [B, mp, nd], b, c, u)."""
    A, b, c, u = tw.mixed_batch(mp, nd, B, seed)
    N = nd + mp
    kind = np.arange(B) % 3
    rng = np.random.default_rng(seed)
    rng.uniform(-1, 1, (mp, nd)); rng.uniform(0.5, 3, (B, N)); rng.random((B, N)); rng.random((B, mp))      # A, u, +inf, fixed
    if nd >= 2:
        rng.uniform(0.5, 3, B)
    rng.uniform(-1, 1, (B, mp)); rng.uniform(-1, 1, (B, N))                                                 # b, c
    ufeas = np.where(u > 0, np.minimum(u, 2.0), 0.0)       # (u of an LP with k mod 3 != 1 is what it was when x0 was drawn)
    x0 = rng.uniform(0.05, 0.45, (B, N)) * ufeas
    y0 = rng.uniform(-1, 1, (B, mp))
    z0 = rng.uniform(0.1, 1, (B, N))
    s0 = np.where(np.isfinite(u) & (u > 0), rng.uniform(0.1, 1, (B, N)), 0.0)
    feas = kind != 1
    assert np.array_equal(b[feas], (x0 @ A.T)[feas]) and np.array_equal(c[kind == 0], (y0 @ A - z0 + s0)[kind == 0])
    Ad = A[None, :, :nd] * np.random.default_rng(seed + offset).uniform(0.75, 1.25, (B, mp, nd))
    Af = np.concatenate([Ad, np.broadcast_to(np.eye(mp), (B, mp, mp))], axis=2)
    b, c = b.copy(), c.copy()
    b[feas] = np.einsum("kij,kj->ki", Af, x0)[feas]
    c[kind == 0] = (np.einsum("kij,ki->kj", Af, y0) - z0 + s0)[kind == 0]
    for k in np.flatnonzero(kind == 1):
        i = (k // 3) % mp
        neg = Af[k, i] < 0
        assert np.isfinite(u[k, neg]).all()       # (A_k has the signs of A: mixed_batch bounded these columns)
        b[k, i] = -(10.0 + (np.abs(Af[k, i]) * np.where(neg, u[k], 0.0)).sum())
    return Ad, b, c, u


def fixture_holds(ref):
    """The properties a batch is specified with, from the twin's results alone: every LP 3i optimal, every LP 3i + 1 infeasible,
    some LP unbounded, no other verdict, no pivot on its floor, at most 30 iterations, and the twin's own primal-dual gap of
    every optimal LP within GAP.  (That the verdicts are HiGHS's is tested beside it.)"""
    st = ref["status"]
    opt = st == 0
    return bool((st[0::3] == 0).all() and (st[1::3] == 2).all() and (st == 4).any() and np.isin(st, (0, 2, 4)).all()
                and (ref["floored"] == 0).all() and ref["iters"].max() <= 30
                and np.abs(ref["pobj"] - ref["dobj"])[opt].max() <= GAP)


def full(Ad, k):
    """[A_k | I]"""
    return np.hstack([Ad[k], np.eye(Ad.shape[1])])


def twin_each(Ad, b, c, u, idx=None, **opts):
    """tw.solve LP by LP (B = 1 per call), each with its own matrix: dict of stacked results (``TWIN_OUT``)."""
    idx = range(len(b)) if idx is None else idx
    each = [tw.solve(full(Ad, k), b[k:k + 1], c[k:k + 1], u[k:k + 1], **opts) for k in idx]
    return {q: np.concatenate([e[q] for e in each]) for q in TWIN_OUT}


def highs_each(Ad, b, c, u):
    st = [tw.highs_verdicts(full(Ad, k), b[k:k + 1], c[k:k + 1], u[k:k + 1])[0][0] for k in range(len(b))]
    return np.array(st, dtype=np.int32)


def certificate(Ad, b, c, u, res, k, sb=1.0, sc=1.0):
    return tw.certificate_ratio(full(Ad, k), b, c, u, res, k, sb, sc)


@functools.lru_cache(maxsize=None)
def gpu_case(size, variant="plain"):
    """(Ad, b, c, u, the twin's results) of the batch of ``size`` = (m', n), read-only: 'plain'; 'autoscale': b, u x 1e4 and
    c x 1e-3 under PYCLLP_FLAG_AUTOSCALE; 'per_lp': every other LP so, under _AUTOSCALE_PER_LP."""
    Ad, b, c, u = mixed_batch_pa(size[0], size[1], B_GPU, tw.MIXED_SEEDS[size], PA_OFFSETS.get(size, PA_SEED))
    if variant != "plain":
        sel = slice(None) if variant == "autoscale" else slice(0, None, 2)
        b[sel] *= SCALE_B; u[sel] *= SCALE_B; c[sel] *= SCALE_C
    ref = twin_each(Ad, b, c, u, autoscale=variant == "autoscale", per_lp=variant == "per_lp")
    for v in (Ad, b, c, u) + tuple(ref.values()):
        v.setflags(write=False)
    return Ad, b, c, u, ref


def group_shape(size):
    mp, n = size
    return next(s for s in ((16, 32), (16, 48), (16, 64), (32, 64), (32, 96), (32, 128)) if mp <= s[0] and n <= s[1] - s[0])


def refills(size):
    """LPs per slot of a launch of B_GPU LPs on one CU: the waves per workgroup of the shape times its lane groups per wave."""
    shape = group_shape(size)
    waves = {(16, 32): 4, (16, 48): 4, (16, 64): 4, (32, 64): 4, (32, 96): 3, (32, 128): 2}[shape]
    return B_GPU / (waves * (64 // shape[0]))


def specs(Ad, b, c, u, with_A=True):
    B, m, nd = Ad.shape
    N = nd + m
    lead = [fp.inp("A", Ad)] if with_A else []
    return lead + [fp.inp("b", b), fp.inp("c", c), fp.inp("u", u), fp.out("x", (B, N)), fp.out("y", (B, m)),
                   fp.out("z", (B, N)), fp.out("s", (B, N)), fp.out("pobj", (B,)), fp.out("dobj", (B,)),
                   fp.out("status", (B,), fp.I32), fp.out("iters", (B,), fp.I32)]


def launch(Ad, b, c, u, flags=0, null=(), arena=None, handle=None, a_cols=None, expect=0, entry=ENTRY, **opts):
    """One call of the entry with all but one CU reserved (slots refill, lane groups finish at different passes) -> (results by
    name, launch_info); ``null``: outputs passed as NULL; ``arena``: a placement of tests/footprint.py to run the call in;
    ``handle``: a Handle to reuse (default: one made from [A_0 | I]); ``a_cols``: what to pass for it (default n - m);
    ``expect``: the return code the call must give (a refused call is checked to have touched nothing).  ``entry`` =
    SHARED_ENTRY: the shared-A entry on the same handle (A_0 for every LP; Ad is not passed)."""
    import torch
    from pycllp_amd.solvers.hip import Handle, solve_opts
    dev = torch.device("cuda:0")
    B = len(b)
    batch = entry == ENTRY
    sp = specs(Ad, b, c, u, with_A=batch)
    ar = fp.Arena(sp, arena, device=dev, null=null) if arena else fp.Plain(sp, device=dev)
    ar.null = set(null)
    h = handle if handle is not None else Handle(full(Ad, 0), dev, None)
    o = solve_opts({}, flags, reserve_cus=torch.cuda.get_device_properties(dev).multi_processor_count - 1, **opts)
    ptr = lambda t: ctypes.c_void_p(None if t is None else t.data_ptr())      # noqa: E731
    st = ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
    lead = (ptr(ar["A"]), ctypes.c_long(Ad.shape[2] if a_cols is None else a_cols)) if batch else ()
    with torch.cuda.device(dev):
        rc = getattr(_native.lib(), entry)(h, B, *lead, *(ptr(ar[k]) for k in ("b", "c", "u") + OUT), ctypes.byref(o), st)
    assert rc == expect, (rc, _native.lib().pycllp_hip_last_error())
    torch.cuda.synchronize(dev)
    if rc != 0:
        if arena:
            ar.check(outputs_written=False)
        return None, None
    if arena:
        ar.check()
    return ar.results(), h.launch_info()


# ---- the plugin's batch -----------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def general_batch():
    """256 GeneralLPs, 12 rows x 16 columns, every LP with its own matrix, mixed row kinds, finite u; every third one is made
    infeasible (an equality row asks for more than its columns can give -- with LP k's own matrix in the reach)."""
    glp = make_general(12, 16, 256, seed=77, per_problem_A=True)
    A1 = np.stack([glp.A.todense(k)[1] for k in range(glp.nproblems)])          # row 1 is an 'eq' row
    reach = np.maximum(A1 * glp.l, A1 * glp.u).sum(axis=1)
    glp.a[1::3, 1] = glp.b[1::3, 1] = reach[1::3] + 5.0
    return glp


def highs_general_status(glp, k):
    from scipy.optimize import linprog
    A = glp.A.todense(k)
    hi, lo = np.isfinite(glp.b[k]), np.isfinite(glp.a[k])
    r = linprog(-glp.c[k], A_ub=np.vstack([A[hi], -A[lo]]), b_ub=np.concatenate([glp.b[k][hi], -glp.a[k][lo]]),
                bounds=list(zip(glp.l[k], glp.u[k])), method="highs")
    return {0: 0, 2: 2, 3: 4}[r.status]
