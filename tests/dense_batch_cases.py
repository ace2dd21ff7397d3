"""Helpers of tests/test_dense_batch.py (no tests): LP batches in which every LP has its own dense matrix, the oracle run LP by
LP, and the trajectory references with their tolerances (the rule of tests/trajectory.py)."""
import functools

import numpy as np

from pycllp_amd.lp import EqualityLP, SparseMatrix, StandardLP

GROUP_SHAPES = [(16, 32), (16, 48), (16, 64), (32, 64), (32, 96), (32, 128)]
B_EVERY = 37


def dense_structure(m, ncols):
    rows, cols = np.divmod(np.arange(m * ncols), ncols)
    return rows, cols


def standard_batch(m, nd, B, seed, scale=False, b_scale=1.0, c_scale=1.0):
    """Equality form [A_k | I] of max c'x, A_k x <= b, x >= 0 with A_k = 0.1 + U(0, 1) [m, nd] of its own for every LP (times a
    per-LP factor in [0.5, 2] with ``scale``), b, c ~ U[0.5, 1.5) times ``b_scale``, ``c_scale``: feasible and bounded."""
    rs = np.random.RandomState(seed)
    A = 0.1 + rs.rand(B, m, nd)
    if scale:
        A *= (0.5 + 1.5 * rs.rand(B))[:, None, None]
    b = (0.5 + rs.rand(B, m)) * b_scale
    c = (0.5 + rs.rand(B, nd)) * c_scale
    rows, cols = dense_structure(m, nd)
    return _frozen(StandardLP(SparseMatrix(rows, cols, A.reshape(B, -1)), b, c, 0.0).to_equality_form())


def equality_batch(m, N, B, seed):
    """Equality-form LPs WITHOUT an identity tail, A_k = N(0, 1) / sqrt(N) [m, N] of its own for every LP, around a strictly
    feasible primal-dual pair; b and c of max-norm 1 (the construction of test_kernel_variants.equality_lp, per LP)."""
    rs = np.random.RandomState(seed)
    A = rs.randn(B, m, N) / np.sqrt(N)
    x0 = rs.rand(B, N) + 0.1
    y0 = rs.randn(B, m)
    b = np.einsum("kij,kj->ki", A, x0)
    c = np.einsum("kij,ki->kj", A, y0) - (rs.rand(B, N) + 0.1)
    b /= np.abs(b).max(axis=1, keepdims=True)
    c /= np.abs(c).max(axis=1, keepdims=True)
    rows, cols = dense_structure(m, N)
    A_ = SparseMatrix(rows, cols, A.reshape(B, -1))
    A_._shape = (m, N)
    return _frozen(EqualityLP(A_, b, c, 0.0))


def degenerate_batch(m, N, B, seed):
    """The construction of trajectory.degenerate LP by LP, on the matrices of ``equality_batch``: the last row of every A_k
    replaced by its row 3 + 1e-6 noise, b and c around a strictly feasible primal-dual pair of the new matrix."""
    A = matrices(equality_batch(m, N, B, seed)).copy()
    rs = np.random.RandomState(31)
    A[:, -1] = A[:, 3] + 1e-6 * rs.randn(B, N)
    x0, y0 = rs.rand(B, N) + 0.1, rs.randn(B, m)
    b = np.einsum("kij,kj->ki", A, x0)
    c = np.einsum("kij,ki->kj", A, y0) - (rs.rand(B, N) + 0.1)
    b /= np.abs(b).max(axis=1, keepdims=True)
    c /= np.abs(c).max(axis=1, keepdims=True)
    A_ = SparseMatrix(*dense_structure(m, N), A.reshape(B, -1))
    A_._shape = (m, N)
    return _frozen(EqualityLP(A_, b, c, 0.0))


def _frozen(lp):
    for a in (lp.b, lp.c, lp.A.data):
        a.setflags(write=False)
    return lp


def reorder(lp, idx):
    """The LPs ``idx`` of ``lp``, matrices included."""
    A = SparseMatrix(np.asarray(lp.A._rows), np.asarray(lp.A._cols), np.asarray(lp.A.data)[idx])
    A._shape = (lp.nrows, lp.ncols)
    return EqualityLP(A, lp.b[idx].copy(), lp.c[idx].copy(), 0.0)


def matrices(lp):
    """[B, m, n]: every LP's full matrix."""
    from pycllp_amd.solvers.dense_batch import densify_batch
    return densify_batch(lp.A._rows, lp.A._cols, lp.A.data, lp.nrows, lp.ncols)


def smallest_and_full(shape, slack):
    """(m, n of the equality form) of the smallest LP that selects ``shape`` and of the one that fills it exactly, on the
    slack-aware table (n - m dense columns + identity tail) or the general one (n columns, no tail)."""
    mp, np_ = shape
    i = GROUP_SHAPES.index(shape)
    m = 3 if mp == 16 else 17
    if slack:
        below = [s[1] - s[0] for s in GROUP_SHAPES[:i] if s[0] >= m]
        nd = max(below + [4]) + 1
        return (m, m + nd), (mp, np_)
    below = [s[1] for s in GROUP_SHAPES[:i] if s[0] >= m]
    return (m, max(below + [2 * m - 1]) + 1), (mp, np_)


def first_covering(m, n, slack):
    for s in GROUP_SHAPES:
        if slack and m <= s[0] and n - m <= s[1] - s[0]:
            return s
        if not slack and m <= s[0] and n <= s[1]:
            return s
    return None


def make(m, n, slack, B=B_EVERY, seed=None):
    seed = 1000 * m + n if seed is None else seed
    return standard_batch(m, n - m, B, seed) if slack else equality_batch(m, n, B, seed)


def oracle_each(lp, idx=None, **opts):
    """oracle.port.dense_solve LP by LP, each with its own matrix: dict of stacked results for the LPs ``idx`` (default all)."""
    from oracle import port
    idx = range(lp.nproblems) if idx is None else idx
    each = [port.dense_solve(lp.A.todense(k), lp.b[k:k + 1], lp.c[k:k + 1], **opts) for k in idx]
    return {q: np.concatenate([e[q] for e in each]) for q in each[0]}


def assert_matches_oracle(s, r, idx=None):
    """The project's parity bounds: status equal and 0, iterations within 1, objectives 1e-9 relative, x at rtol 1e-5, atol 1e-7."""
    from conftest import rel_err
    idx = np.arange(len(r["status"])) if idx is None else np.asarray(idx)
    assert (r["status"] == 0).all() and (s["status"][idx] == 0).all(), (r["status"], s["status"][idx])
    assert np.abs(s["iters"][idx].astype(int) - r["iters"]).max() <= 1
    assert rel_err(s["pobj"][idx], r["pobj"]).max() < 1e-9 and rel_err(s["dobj"][idx], r["dobj"]).max() < 1e-9
    np.testing.assert_allclose(s["x"][idx], r["x"], rtol=1e-5, atol=1e-7)


# ---- trajectory: the oracle after k iterations, its spread under permutations, the tolerance ---------------------------------
TRAJECTORY_POINTS = {"16-row": (12, 12 + 20, True), "32-row": (24, 24 + 40, True)}      # (m, n, slack)
B_TRAJ = 12


@functools.lru_cache(maxsize=None)
def trajectory_lp(point):
    m, n, slack = TRAJECTORY_POINTS[point]
    return make(m, n, slack, B=B_TRAJ, seed=7000 + m)


def _run_reference(lp, k, perm=None):
    """x, y, z and the objectives OF THAT POINT (c'x, b'y: what the kernel stores at the iteration limit) after k iterations of
    the oracle; ``perm``: seed of a row-and-column permutation under which every LP is solved (results mapped back)."""
    from oracle import port
    m, N = lp.nrows, lp.ncols
    rows, cols = np.arange(m), np.arange(N)
    if perm is not None:
        rs = np.random.RandomState(1000 + perm)
        rows, cols = rs.permutation(m), rs.permutation(N)
    inv_r, inv_c = np.argsort(rows), np.argsort(cols)
    out = {q: [] for q in ("x", "y", "z", "pobj", "dobj", "status", "iters")}
    for i in range(lp.nproblems):
        A = np.ascontiguousarray(lp.A.todense(i)[rows][:, cols])
        r = port.dense_solve(A, lp.b[i:i + 1, rows], lp.c[i:i + 1, cols], max_iter=k)
        x, y, z = r["x"][0][inv_c], r["y"][0][inv_r], r["z"][0][inv_c]
        out["x"].append(x); out["y"].append(y); out["z"].append(z)
        out["pobj"].append(lp.c[i] @ x); out["dobj"].append(lp.b[i] @ y)
        out["status"].append(r["status"][0]); out["iters"].append(r["iters"][0])
    return {q: np.asarray(v) for q, v in out.items()}


@functools.lru_cache(maxsize=None)
def trajectory_reference(point, k):
    return _run_reference(trajectory_lp(point), k)


@functools.lru_cache(maxsize=None)
def trajectory_tolerance(point, k):
    """{quantity: max(FACTOR x the oracle's own spread under NPERM seeded permutations, FLOOR)}, never above CEILING."""
    import trajectory as tj
    ref = trajectory_reference(point, k)
    runs = [_run_reference(trajectory_lp(point), k, perm=p) for p in range(tj.NPERM)]
    tol = {}
    for q in tj.QUANTITIES:
        spread = max(float(tj.deviation(r[q], ref[q]).max()) for r in runs)
        tol[q] = min(max(tj.FACTOR * spread, tj.FLOOR), tj.CEILING)
    return tol
