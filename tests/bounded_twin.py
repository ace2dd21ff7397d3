"""CPU twin of the bounded primal-normal step (csrc/ipm_group_slot.inc, BD), vectorised over LPs.

Test infrastructure only: a numpy restatement of the kernel's arithmetic -- start point, residuals, stop tests, the modified
LDL' with the Nocedal-Wright guard, the x-space refinement and the step -- so that the GPU tests can compare objectives and
iteration counts.  The LP is  maximise c'x  s.t.  A x = b,  0 <= x <= u  (u = +inf: no bound, u = 0: fixed)."""
import numpy as np

GROWTH_FLOOR = 1e3


def ldl_guarded(M, floor, beta2, stats=None):
    """Modified LDL' of every matrix of M [B, m, m]: D_j = max(|M_jj|, floor, theta_j^2 / beta2) (ldl.cl:368).  ``stats``: a
    dict that receives, per matrix, ``floored`` (the pivots with |M_jj| < floor) and ``guard_ratio`` (the largest
    theta_j^2 / (beta2 max(|M_jj|, floor)): above 1 the guard's term is the pivot)."""
    W = M.copy()
    B, m, _ = W.shape
    L = np.broadcast_to(np.eye(m), W.shape).copy()
    D = np.zeros((B, m))
    floored, ratio = np.zeros(B, dtype=np.int64), np.zeros(B)
    for j in range(m):
        col = W[:, j + 1:, j]
        theta = np.abs(col).max(axis=1) if j + 1 < m else np.zeros(B)
        Dj = np.maximum(np.maximum(np.abs(W[:, j, j]), floor), theta * theta / beta2)
        if stats is not None:
            floored += np.abs(W[:, j, j]) < floor
            ratio = np.fmax(ratio, theta * theta / (beta2 * np.maximum(np.abs(W[:, j, j]), floor)))
        lj = col / Dj[:, None]
        W[:, j + 1:, j + 1:] -= lj[:, :, None] * col[:, None, :]
        L[:, j + 1:, j] = lj
        D[:, j] = Dj
    if stats is not None:
        stats["floored"], stats["guard_ratio"] = floored, ratio
    return L, D


def ldl_solve(L, D, r):
    t = np.linalg.solve(L, r[..., None])[..., 0]
    return np.linalg.solve(np.swapaxes(L, 1, 2), (t / D)[..., None])[..., 0]


def solve(A, b, c, u, eps=1e-10, delta=0.02, r=0.9, pivot_floor=1e-6, refine_tol=1e-11, max_iter=200, max_refine=5,
          autoscale=False):
    """dict(x, y, z, s, pobj, dobj, status, iters, nrefs, floored, guard_ratio) for the B LPs (A [m, N] shared; b [B, m];
    c, u [B, N]).  ``nrefs``: refinement passes spent, ``floored``: pivots that met the floor, both summed over the
    iterations an LP was live in; ``guard_ratio``: the largest theta^2 / (beta^2 max(|M_jj|, floor)) of its factorisations."""
    A = np.asarray(A, dtype=np.float64)
    b, c, u = (np.array(v, dtype=np.float64) for v in (b, c, u))
    B, N = c.shape
    m = A.shape[0]
    act = u > 0
    bnd = act & np.isfinite(u)
    sb = np.ones(B); sc = np.ones(B)
    if autoscale:
        sb = np.abs(b).max(axis=1); sb[sb == 0] = 1.0
        sc = np.where(act, np.abs(c), 0.0).max(axis=1); sc[sc == 0] = 1.0
        b = b / sb[:, None]; c = c / sc[:, None]; u = u / sb[:, None]
    uf = np.where(bnd, u, 0.0)
    x = np.where(bnd, np.minimum(1.0, 0.5 * uf), 1.0)
    t = np.where(bnd, uf - x, 1.0)
    z = np.ones((B, N)); s = np.ones((B, N)); y = np.ones((B, m))
    tol_r = eps * (1 + np.linalg.norm(b, axis=1))
    tol_s = eps * (1 + np.linalg.norm(np.where(act, c, 0.0), axis=1))
    tol_u = eps * (1 + np.linalg.norm(uf, axis=1))
    etol = refine_tol * (1 + np.linalg.norm(b, axis=1))
    ncomp = N + m + bnd.sum(axis=1)
    status = np.full(B, 5, dtype=np.int32)
    iters = np.full(B, max_iter, dtype=np.int32)
    out = {k: np.zeros((B, N)) for k in ("x", "z", "s")}
    out["y"] = np.zeros((B, m)); out["pobj"] = np.zeros(B); out["dobj"] = np.zeros(B)
    normr0 = np.full(B, 1e300); norms0 = np.full(B, 1e300)
    live = np.ones(B, dtype=bool)
    nrefs = np.zeros(B, dtype=np.int32); floored = np.zeros(B, dtype=np.int32); guard_ratio = np.zeros(B)

    def store(sel, it):
        v = y @ A
        rr = c - v
        out["x"][sel] = (np.where(act, x, 0.0) * sb[:, None])[sel]
        out["z"][sel] = (np.where(act, z, np.maximum(-rr, 0.0)) * sc[:, None])[sel]
        out["s"][sel] = (np.where(bnd, s, np.where(act, 0.0, np.maximum(rr, 0.0))) * sc[:, None])[sel]
        out["y"][sel] = (y * sc[:, None])[sel]
        out["pobj"][sel] = (np.where(act, c * x, 0.0).sum(1) * sb * sc)[sel]
        out["dobj"][sel] = (((b * y).sum(1) + np.where(bnd, uf * s, 0.0).sum(1)) * sb * sc)[sel]
        iters[sel] = it

    for it in range(max_iter):
        v = y @ A
        sig = np.where(act, c - v + z - np.where(bnd, s, 0.0), 0.0)
        tau = np.where(bnd, (uf - x) - t, 0.0)
        gam = np.where(act, x * z, 0.0).sum(1) + np.where(bnd, s * t, 0.0).sum(1)
        po = np.where(act, c * x, 0.0).sum(1)
        rho = b - np.where(act, x, 0.0) @ A.T
        normr, norms, ntau = (np.linalg.norm(w, axis=1) for w in (rho, sig, tau))
        with np.errstate(invalid="ignore"):
            bad = ~(np.isfinite(normr) & np.isfinite(norms) & np.isfinite(gam) & np.isfinite(ntau))
            opt = ~bad & (normr <= tol_r) & (norms <= tol_s) & (gam <= eps * (1 + np.abs(po))) & (ntau <= tol_u)
            pinf = ~bad & ~opt & (normr > 10 * normr0) & (normr > GROWTH_FLOOR * tol_r)
            dinf = ~bad & ~opt & ~pinf & (norms > 10 * norms0) & (norms > GROWTH_FLOOR * tol_s)
        for flag, st in ((bad, 3), (opt, 0), (pinf, 2), (dinf, 4)):
            sel = live & flag
            status[sel] = st
            store(sel, it)
            live &= ~sel
        if not live.any():
            break
        with np.errstate(all="ignore"):
            mu = delta * gam / ncomp
            d = np.where(bnd, 1.0 / (z / x + s / t), x / z)
            d = np.where(act, d, 0.0)
            tt = np.where(bnd, c - v + mu[:, None] / x - mu[:, None] / t + (s / t) * tau, c - v + mu[:, None] / x)
            tt = np.where(act, tt, 0.0)
            M = np.einsum("ik,bk,jk->bij", A, d, A)
            beta2 = np.abs(np.diagonal(M, axis1=1, axis2=2)).max(axis=1)
            stats = {}
            L, D = ldl_guarded(M, pivot_floor, beta2, stats)
            floored += np.where(live, stats["floored"], 0).astype(np.int32)
            guard_ratio = np.where(live, np.fmax(guard_ratio, stats["guard_ratio"]), guard_ratio)
            dy = ldl_solve(L, D, (d * tt) @ A.T - rho)
            dx = (tt - dy @ A) * d
            for _ in range(max_refine):
                e = rho - dx @ A.T
                need = np.abs(e).max(axis=1) > etol
                if not need.any():
                    break
                nrefs += live & need
                eta = ldl_solve(L, D, np.where(need[:, None], e, 0.0))
                dx = dx + d * (eta @ A)
                dy = dy - eta
            dyb = ~np.isfinite(dy).all(axis=1)
            sel = live & dyb
            status[sel] = 3
            store(sel, it)
            live &= ~sel
            dz = np.where(act, (mu[:, None] - z * dx) / x - z, 0.0)
            dt = np.where(bnd, tau - dx, 0.0)
            ds = np.where(bnd, (mu[:, None] - s * dt) / t - s, 0.0)
            ratio = np.maximum(np.where(act, np.maximum(-dz / z, -dx / x), 0.0),
                               np.where(bnd, np.maximum(-dt / t, -ds / s), 0.0)).max(axis=1)
            theta = np.minimum(r / np.maximum(ratio, 0.0), 1.0)[:, None]
        w = live[:, None]
        y = np.where(w, y + theta * dy, y)
        x = np.where(w & act, x + theta * dx, x)
        z = np.where(w & act, z + theta * dz, z)
        t = np.where(w & bnd, t + theta * dt, t)
        s = np.where(w & bnd, s + theta * ds, s)
        normr0 = np.where(live, normr, normr0); norms0 = np.where(live, norms, norms0)
    store(live, max_iter)
    out["status"], out["iters"] = status, iters
    out["nrefs"], out["floored"], out["guard_ratio"] = nrefs, floored, guard_ratio
    return out
