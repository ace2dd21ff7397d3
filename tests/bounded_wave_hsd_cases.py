"""Fixtures of tests/test_bounded_wave_hsd.py (helpers, no tests): the batches the bounded wave kernel's self-dual embedding is
compared on, and their references -- the CPU twin (tests/bounded_hsd_twin.py) and HiGHS -- computed once and left read-only.

B = 64 LPs per size, interleaving optimal / infeasible / mostly-unbounded as ``tw.mixed_batch`` does; every LP has finite,
infinite and zero u.  The dense sizes call ``tw.mixed_batch``; the sparse ones restate its recipe on a masked matrix
(``sparse_mixed_batch``).  The sizes (m', n) are the smallest that reach each distinct path of the kernel:

    (1, 1)      dense   N = 2     no off-diagonal block
    (12, 16)    dense   N = 28    term tables, one 16-row block, one N-vector register
    (17, 48)    dense   N = 65    one row into the second block, one column into the second register
    (40, 130)   10 %    N = 170   term tables with structural zeros, three blocks
    (65, 100)   6 %     N = 165   MR = 2: two row registers per lane
    (33, 160)   dense   N = 193   the dense-image kernel

The seeds were chosen on the CPU by criteria on the references alone (test_fixtures_meet_their_criteria asserts them): the twin's
statuses equal HiGHS's, all three verdicts occur, no pivot meets its floor, the twin needs at most 40 iterations."""
import collections
import functools

import numpy as np

import bounded_hsd_twin as tw

B = 64
MAX_TWIN_ITERS = 40
# what must serve the size: the plan's variant and its (MB, NQ) (csrc/wreg.h: the first shape of the variant's list that covers
# m' rows and N columns; a dense A^ goes to the image once its term tables no longer fit the LDS beside the waves)
Fixture = collections.namedtuple("Fixture", "size density seed variant shape")
FIXTURES = (
    Fixture((1, 1), None, 32, "tables", (1, 4)),
    Fixture((12, 16), None, 11, "tables", (1, 4)),
    Fixture((17, 48), None, 1, "tables", (2, 4)),
    Fixture((40, 130), 0.10, 1, "tables", (3, 4)),
    Fixture((65, 100), 0.06, 2, "tables", (5, 6)),
    Fixture((33, 160), None, 1, "dense image", (3, 4)),
)
BY_SIZE = {f.size: f for f in FIXTURES}
SCALE_B, SCALE_C = 1e4, 1e-3


def sparse_mixed_batch(mp, nd, nb, seed, density):
    """``tw.mixed_batch`` on A = [U(-1, 1) x mask | I]: about ``density`` of the entries of the dense part are structural, every
    row has two at least and every column one.  The infeasible LPs are built from the MASKED row: every column with a negative
    entry there is bounded and b_i = -(10 + sum |A_ij| u_j); their c is the dual feasible one of the optimal LPs."""
    rng = np.random.default_rng(seed)
    N = nd + mp
    mask = rng.random((mp, nd)) < density
    for i in range(mp):
        short = 2 - int(mask[i].sum())
        if short > 0:
            mask[i, rng.choice(np.flatnonzero(~mask[i]), short, replace=False)] = True
    for j in np.flatnonzero(~mask.any(axis=0)):
        mask[rng.integers(mp), j] = True
    A = np.hstack([np.where(mask, rng.uniform(-1, 1, (mp, nd)), 0.0), np.eye(mp)])
    u = rng.uniform(0.5, 3, (nb, N))
    kind = np.arange(nb) % 3
    p_inf = np.where(kind == 2, 0.8, 0.4)[:, None]
    u[rng.random((nb, N)) < p_inf] = np.inf
    u[:, nd:][rng.random((nb, mp)) < 0.4] = 0.0
    u[:, 0] = rng.uniform(0.5, 3, nb); u[:, nd - 1] = np.inf; u[:, N - 1] = 0.0      # all three sorts of column in every LP
    b = 3 * rng.uniform(-1, 1, (nb, mp))
    c = rng.uniform(-1, 1, (nb, N))
    x0 = rng.uniform(0.05, 0.45, (nb, N)) * np.where(u > 0, np.minimum(u, 2.0), 0.0)
    feas = kind != 1
    b[feas] = (x0 @ A.T)[feas]
    y0 = rng.uniform(-1, 1, (nb, mp))
    dual = y0 @ A - rng.uniform(0.1, 1, (nb, N)) + np.where(np.isfinite(u) & (u > 0), rng.uniform(0.1, 1, (nb, N)), 0.0)
    # (the infeasible LPs are dual feasible by construction too: the masked row bounds few columns, and with a random c about a
    # quarter of them were dual infeasible as well -- there the twin's valid ray and HiGHS's 'infeasible' are both right)
    c[kind != 2] = dual[kind != 2]
    for k in np.flatnonzero(kind == 1):
        i = (k // 3) % mp
        neg = A[i] < 0
        u[k, neg & np.isinf(u[k])] = rng.uniform(0.5, 3, int((neg & np.isinf(u[k])).sum()))
        b[k, i] = -(10.0 + (np.abs(A[i]) * np.where(neg, u[k], 0.0)).sum())
    return A, b, c, u


def _frozen(arrays):
    for v in arrays:
        v.setflags(write=False)
    return arrays


@functools.lru_cache(maxsize=None)
def batch(size, variant="plain"):
    """(A, b, c, u) of the fixture of ``size``: 'plain'; 'autoscale': b, u x 1e4 and c x 1e-3 (the same LPs in other units) for
    PYCLLP_FLAG_AUTOSCALE; 'per_lp': every other LP so, for _AUTOSCALE_PER_LP."""
    f = BY_SIZE[size]
    if f.density is None:
        A, b, c, u = tw.mixed_batch(size[0], size[1], B, f.seed)
    else:
        A, b, c, u = sparse_mixed_batch(size[0], size[1], B, f.seed, f.density)
    if variant != "plain":
        sel = slice(None) if variant == "autoscale" else slice(0, None, 2)
        b, c, u = b.copy(), c.copy(), u.copy()
        b[sel] *= SCALE_B; u[sel] *= SCALE_B; c[sel] *= SCALE_C
    return _frozen((A, b, c, u))


@functools.lru_cache(maxsize=None)
def twin(size, variant="plain", k=None, perm=None, take=None):
    """The twin's results on ``batch(size, variant)``; ``k``: max_iter; ``perm``: seed of a row and column permutation under which
    the LPs are solved (results mapped back); ``take``: the first LPs of the batch only."""
    A, b, c, u = batch(size, variant)
    if take is not None:
        b, c, u = b[:take], c[:take], u[:take]
    m, N = A.shape
    rows, cols = np.arange(m), np.arange(N)
    if perm is not None:
        rs = np.random.RandomState(1000 + perm)
        rows, cols = rs.permutation(m), rs.permutation(N)
    opts = {} if k is None else dict(max_iter=k)
    r = tw.solve(np.ascontiguousarray(A[rows][:, cols]), b[:, rows], c[:, cols], u[:, cols],
                 autoscale=variant == "autoscale", per_lp=variant == "per_lp", **opts)
    inv_r, inv_c = np.argsort(rows), np.argsort(cols)
    out = dict(r, x=r["x"][:, inv_c], z=r["z"][:, inv_c], s=r["s"][:, inv_c], y=r["y"][:, inv_r])
    _frozen(tuple(out.values()))
    return out


@functools.lru_cache(maxsize=None)
def highs(size):
    return _frozen(tw.highs_verdicts(*batch(size)))
