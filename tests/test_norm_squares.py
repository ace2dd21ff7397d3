"""The stop and growth tests of the dense lane-group kernels on SQUARED residual norms (csrc/ipm_group.inc, stop_verdict).

ipm_group_kernel (plain and predictor-corrector step) no longer takes the square roots of |rho|^2 and |sigma|^2 in every pass.
On the squares it decides only that NO test holds ("all clear": three strict compares per norm, a factor of two away from
where the square roots decide); every other pass takes the exact path, the comparisons on the square roots.

CPU: the all-clear rule restated in numpy, operation for operation, against ``np.sqrt`` on 10^6 random thresholds across the
exponent range -- their squares underflow and overflow at both ends -- with the squares drawn at and next to T^2 (1 +- 2^-40),
the band the rule was first drafted with, at and next to the rule's own edges, at 2^+-900 and at the ends of the doubles.
Wherever the rule gives a verdict it must be the square root's.

GPU: PYCLLP_FLAG_EXACT_NORMS sends every pass down the exact path, which is the text the kernels had; with and without it the
results must be the same bits (status, iterations, objectives, vectors), at every shape and option that changes the code around
the tests, and on the mixed-status fixture, whose LPs leave through the growth exits and the iteration limit.  The batches, the
oracle's results and the kernel's solves that test_fused_forward.py also uses are its cached ones."""
import numpy as np
import pytest

from conftest import rel_err, status_cases
from pycllp_amd import _native
from pycllp_amd.solvers import solver_registry
from pycllp_amd.solvers.hip import autoscale_mask
from test_fused_forward import B, BITWISE, PC_OPTS, PREDCORR, assert_matches, reference, solve, solved, standard
from test_hip_parity import oracle_on, solve_arrays

EXACT = _native.FLAG_EXACT_NORMS
GENERIC = _native.FLAG_GENERIC_SHAPE
DELTA, SQ_MIN, SQ_MAX = 2.0 ** -40, 2.0 ** -900, 2.0 ** 900
FLOOR = 1e3                                                       # PYCLLP_GROWTH_FLOOR
N = 10 ** 6


# ---- the rule, as the kernel computes it (every product rounded once, as there) ----

def not_le(s, T):
    """(a): certainly not sqrt(s) <= T."""
    return 0.5 * s > T * np.abs(T)


def not_grown(s, s0):
    """(b): certainly not sqrt(s) > 10 sqrt(s0)."""
    return 0.5 * s < s0


def below_floor(s, T):
    """(c): certainly not sqrt(s) > FLOOR T."""
    return 0.5 * s < T * np.abs(T)


def around(x, steps=(-2, -1, 0, 1, 2)):
    """x and its neighbours, one array per step."""
    out = []
    for k in steps:
        y = x.copy()
        for _ in range(abs(k)):
            y = np.nextafter(y, np.inf if k > 0 else -np.inf)
        out.append(y)
    return out


def thresholds(rs, n):
    """n thresholds: random mantissas over 2^-545 .. 2^530 (their squares underflow and overflow at the ends), and the odd
    ones -- zero, negative, infinite, NaN, the smallest and largest doubles."""
    T = np.ldexp(rs.uniform(1.0, 2.0, n), rs.randint(-545, 531, n))
    odd = np.array([0.0, -0.0, -1e-8, -1e-200, -1e200, np.inf, np.nan, 5e-324, 2.2250738585072014e-308, 1.7976931348623157e308,
                    2.0 ** -450, 2.0 ** 450, 2.0 ** -511, 2.0 ** 511, 2.0 ** -512, 2.0 ** 512, 2.0 ** -537, 2.0 ** -538])
    T[:odd.size] = odd
    return T


def squares_for(rs, P):
    """Candidate squares for threshold squares P >= 0: P (1 +- 2^-40) seen from either side and their neighbours, P, 2 P and
    P / 2 (the rule's edges) and theirs, 2^+-900 and theirs, random squares over the whole exponent range and near P, zero, the
    smallest doubles, the largest, +inf, NaN."""
    n = P.size
    cands = []
    for edge in (P * (1.0 - DELTA), P * (1.0 + DELTA), P / (1.0 - DELTA), P / (1.0 + DELTA), P, 2.0 * P, 0.5 * P):
        cands += around(edge)
    for lim in (SQ_MIN, SQ_MAX):
        cands += around(np.full(n, lim))
    cands.append(np.ldexp(rs.uniform(1.0, 2.0, n), rs.randint(-1074, 1024, n)))
    cands.append(P * np.ldexp(rs.uniform(1.0, 2.0, n), rs.randint(-3, 3, n)))
    for v in (0.0, 5e-324, 1e-323, 1.5e-323, 1.7976931348623157e308, np.inf, np.nan):
        cands.append(np.full(n, v))
    return [np.abs(c) for c in cands]                                 # a sum of squares is never negative


def test_all_clear_gives_the_square_roots_verdict_on_the_tolerance_and_the_floor():
    """"sqrt(s) <= T" (the stopping tests) and "sqrt(s) > FLOOR T" (the growth floor)."""
    rs = np.random.RandomState(40)
    T = thresholds(rs, N)
    with np.errstate(all="ignore"):
        P = np.abs(T * np.abs(T))
        P[~np.isfinite(P)] = 1.0                                      # (squares for an infinite or NaN T: around 1)
        decided_a = decided_c = 0
        for s in squares_for(rs, P):
            root = np.sqrt(s)
            a, c = not_le(s, T), below_floor(s, T)
            assert not (root[a] <= T[a]).any()
            assert not (root[c] > FLOOR * T[c]).any()
            decided_a += int(a.sum())
            decided_c += int(c.sum())
        print("decided", decided_a, decided_c)
        assert decided_a > 5 * N and decided_c > 5 * N                # the rule does decide: not vacuous


def test_all_clear_gives_the_square_roots_verdict_on_tenfold_growth():
    """"sqrt(s) > 10 sqrt(s0)" with s0 the square kept from the previous pass: any double from 0 to +inf (the value before an
    LP's first pass)."""
    rs = np.random.RandomState(41)
    s0 = np.ldexp(rs.uniform(1.0, 2.0, N), rs.randint(-1074, 1024, N))
    odd = np.array([0.0, np.inf, 5e-324, 1e-323, 2.2250738585072014e-308, 1.7976931348623157e308, SQ_MIN, SQ_MAX])
    s0[:odd.size] = odd
    with np.errstate(all="ignore"):
        root0 = np.sqrt(s0)
        P = np.where(np.isfinite(s0), s0, 1.0)
        decided = 0
        for s in squares_for(rs, P) + squares_for(rs, 100.0 * P)[:25]:
            root = np.sqrt(s)
            b = not_grown(s, s0)
            assert not (root[b] > 10.0 * root0[b]).any()
            decided += int(b.sum())
        print("decided", decided)
        assert decided > 5 * N


# ---- the kernels, with and without the exact path ----

def assert_same_bits(a, b):
    for name in BITWISE:
        np.testing.assert_array_equal(getattr(a, name), getattr(b, name), err_msg=name)


GPU_CASES = [
    # id, batch, group shape, full shape, solver options, oracle flags
    ("32x64-full-shape", (32, 64), (32, 96), True, {}, 0),
    ("32x64-generic-shape", (32, 64), (32, 96), False, dict(flags=GENERIC), 0),
    ("16x32-four-groups-per-wave", (16, 32), (16, 48), True, {}, 0),
    ("20x30-padded", (20, 30), (32, 64), False, {}, 0),
    ("32x64-predcorr", (32, 64), (32, 96), False, PC_OPTS, PREDCORR),
]


@pytest.mark.gpu
@pytest.mark.parametrize("case", GPU_CASES, ids=[c[0] for c in GPU_CASES])
def test_exact_norms_flag_changes_no_bit(case):
    _, key, shape, full, opts, oflags = case
    fast = solved(key, **opts)
    exact = solved(key, **dict(opts, flags=opts.get("flags", 0) | EXACT))
    for s in (fast, exact):
        info = s.launch_info()
        assert info["group_shape"] == shape and info["full_shape"] is full, info
    assert_same_bits(fast, exact)
    assert_matches(exact, reference(key, oflags))      # status as the oracle's and 0, iterations within 1 of it, as for `fast`


@pytest.mark.gpu
def test_three_lps():
    """Idle lane groups run the tests along on parked values: they must neither ask for a colder tier nor change a live LP."""
    lp = standard(32, 64)
    b3, c3 = np.ascontiguousarray(lp.b[:3]), np.ascontiguousarray(lp.c[:3])
    fast, exact = solve(lp, b3, c3), solve(lp, b3, c3, flags=EXACT)
    assert_same_bits(fast, exact)
    big = solved((32, 64))
    for name in BITWISE:
        np.testing.assert_array_equal(getattr(fast, name), getattr(big, name)[:3], err_msg=name)


@pytest.mark.gpu
def test_warm_start():
    """A loose cold solve, then the warm one from its result: the first pass of a warm LP starts near the tolerances."""
    import torch
    lp = standard(32, 64)
    got = []
    for flags in (0, EXACT):
        s = solver_registry["hip_dense_primal_normal"](device="cuda:0", autoscale=False, flags=flags)
        lp.init(s)
        s.solve_device(lp.b, lp.c, eps=1e-4)
        buf = s.solve_device(lp.b, lp.c, warm_start=True)
        torch.cuda.synchronize()
        got.append({k: buf[k].cpu().numpy().copy() for k in ("status", "iters", "pobj", "dobj", "x", "y", "z")})
    assert (got[0]["status"] == 0).any()
    for k in got[0]:
        np.testing.assert_array_equal(got[0][k], got[1][k], err_msg=k)


@pytest.mark.gpu
def test_autoscale_per_lp():
    """Every other LP out of band: scaled and unscaled LPs, whose norms differ by decades, side by side in a wave."""
    lp = standard(32, 64)
    b, c = lp.b.copy(), lp.c.copy()
    b[::2] *= 100.0
    c[::2] *= 0.01
    mask = autoscale_mask(b, c)
    assert mask[::2].all() and not mask[1::2].any()
    got = []
    for flags in (0, EXACT):
        s = solver_registry["hip_dense_primal_normal"](device="cuda:0", autoscale="per_lp", flags=flags)
        lp2 = type(lp)(lp.A, b, c, 0.0)
        lp2.init(s)
        lp2.solve(s)
        got.append(s)
    assert (got[0].status == 0).all()
    assert_same_bits(got[0], got[1])


@pytest.mark.gpu
def test_mixed_status_fixture_growth_exits_and_iteration_limit():
    """Every shape of tests/golden/status_cases.npz on the reference's path (hsd=False): infeasible and unbounded LPs leave
    through the tenfold-growth exits (statuses 2 and 4), and under a small max_iter every LP stops at the iteration limit.
    With and without the flag, bit for bit; and on the LPs that are optimal (HiGHS and the oracle agree) status and iteration
    count are the oracle's, as test_hip_parity.py requires of the default solver."""
    seen = set()
    for A, b, c, ref_status, highs, ref_pobj in status_cases():
        elp, fast = solve_arrays(A, b, c, hsd=False)
        _, exact = solve_arrays(A, b, c, hsd=False, flags=EXACT)
        assert fast.launch_info()["group_shape"][0] in (16, 32)
        assert_same_bits(fast, exact)
        seen.update(np.unique(fast.status).tolist())
        r = oracle_on(elp)
        opt = (highs == 0) & (r["status"] == 0)
        print(A.shape, "statuses", np.unique(fast.status, return_counts=True), "optimal by both", int(opt.sum()))
        if opt.any():
            np.testing.assert_array_equal(fast.status[opt], 0)
            np.testing.assert_array_equal(fast.iters[opt], r["iters"][opt])
            assert rel_err(fast.primal_obj[opt], r["pobj"][opt]).max() < 1e-9
        _, fast5 = solve_arrays(A, b, c, hsd=False, max_iter=4)
        _, exact5 = solve_arrays(A, b, c, hsd=False, max_iter=4, flags=EXACT)
        assert_same_bits(fast5, exact5)
        seen.update(np.unique(fast5.status).tolist())
    assert {0, 2, 4, 5} <= seen, seen
