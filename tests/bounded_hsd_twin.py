"""CPU twin of the bounded homogeneous self-dual step (csrc/ipm_group_bdhsd.inc), vectorised over LPs.

Test infrastructure only: a numpy restatement of the kernel's arithmetic -- start point, residuals, stop tests, the reduced
Newton system with bounds (one LDL', two right-hand sides), the x-space refinement, the two-branch rule for dt, ds and the
step.  The LP is  maximise c'x  s.t.  A x = b,  0 <= x <= u  (u = +inf: no bound, u = 0: fixed).  The system is the exact
Schur complement of the oracle's hsd_one_raw on the explicit expansion, which ``expansion`` builds."""
import numpy as np


def expansion(A, b, c, u):
    """(Ae, be, ce, act, bnd) of ONE LP: Ae = [[A_act, 0], [E_bnd, I]], be = (b; u_bnd), ce = (c_act; 0).  Columns of the
    expansion: the columns that take part (act), then one slack t per bounded column; rows: A's, then one per bound."""
    A = np.asarray(A, dtype=np.float64)
    act = u > 0
    bnd = act & np.isfinite(u)
    m, na, nbd = A.shape[0], int(act.sum()), int(bnd.sum())
    Ae = np.zeros((m + nbd, na + nbd))
    Ae[:m, :na] = A[:, act]
    E = np.zeros((nbd, na))
    E[np.arange(nbd), np.flatnonzero(bnd[act])] = 1.0
    Ae[m:, :na] = E
    Ae[m:, na:] = np.eye(nbd)
    return Ae, np.concatenate([b, u[bnd]]), np.concatenate([c[act], np.zeros(nbd)]), act, bnd


def ldl_floored(M, pf2, stats):
    """Modified LDL' of every matrix of M [B, m, m] with the pivot floor pf2 |M_jj| of column j (its own original diagonal
    entry) and the Nocedal-Wright guard theta_j^2 / beta^2, beta^2 = max |M_jj|.  stats["floored"]: the pivots below their floor."""
    W = M.copy()
    B, m, _ = W.shape
    L = np.broadcast_to(np.eye(m), W.shape).copy()
    D = np.zeros((B, m))
    diag0 = np.abs(np.diagonal(M, axis1=1, axis2=2)).copy()
    beta2 = diag0.max(axis=1)
    floored = np.zeros(B, dtype=np.int64)
    for j in range(m):
        col = W[:, j + 1:, j]
        theta = np.abs(col).max(axis=1) if j + 1 < m else np.zeros(B)
        fl = pf2 * diag0[:, j]
        floored += np.abs(W[:, j, j]) < fl
        Dj = np.maximum(np.maximum(np.abs(W[:, j, j]), fl), theta * theta / beta2)
        lj = col / Dj[:, None]
        W[:, j + 1:, j + 1:] -= lj[:, :, None] * col[:, None, :]
        L[:, j + 1:, j] = lj
        D[:, j] = Dj
    stats["floored"] = floored
    return L, D


def ldl_solve(L, D, r):
    t = np.linalg.solve(L, r[..., None])[..., 0]
    return np.linalg.solve(np.swapaxes(L, 1, 2), (t / D)[..., None])[..., 0]


def out_of_band(mx):
    return (10.0 * mx < 1.0) | ((mx > 10.0) & np.isfinite(mx))


def scale_factors(b, c, u, autoscale=False, per_lp=False):
    """(sb, sc) [B]: what PYCLLP_FLAG_AUTOSCALE divides b, u and c by on load -- max|b| and max|c| over the columns that take
    part (1 where that is 0, or not finite) -- and, under ``per_lp``, only for the LPs out of band; 1 otherwise."""
    b, c, u = (np.asarray(v, dtype=np.float64) for v in (b, c, u))
    B = len(b)
    act = u > 0
    bnd = act & np.isfinite(u)
    sb = np.ones(B); sc = np.ones(B)
    if autoscale or per_lp:
        sb = np.abs(b).max(axis=1)
        sc = np.where(act, np.abs(c), 0.0).max(axis=1)
        scaled = np.ones(B, dtype=bool)
        if per_lp:
            um = np.where(bnd, u, 0.0).max(axis=1)
            scaled = out_of_band(sb) | out_of_band(np.abs(c).max(axis=1)) | ((um > 0) & out_of_band(um))
        sb = np.where(scaled & (sb > 0), sb, 1.0); sc = np.where(scaled & (sc > 0), sc, 1.0)
        sb = np.where(np.isfinite(sb), sb, 1.0)
    return sb, sc


def solve(A, b, c, u, eps=1e-10, delta=0.02, r=0.9, pivot_floor=1e-6, refine_tol=1e-11, max_iter=200, max_refine=20,
          autoscale=False, per_lp=False):
    """dict(x, y, z, s, pobj, dobj, status, iters, tau, floored) for the B LPs (A [m, N] shared; b [B, m]; c, u [B, N]).
    ``floored``: the pivots that met their floor, summed over the iterations an LP was live in.  ``autoscale``: solve with
    b, u / max|b| and c / max|c|; ``per_lp``: only the LPs out of band (autoscale_lp of wave_common.h)."""
    A = np.asarray(A, dtype=np.float64)
    b, c, u = (np.array(v, dtype=np.float64) for v in (b, c, u))
    B, N = c.shape
    m = A.shape[0]
    act = u > 0
    bnd = act & np.isfinite(u)
    sb, sc = scale_factors(b, c, u, autoscale, per_lp)
    b = b / sb[:, None]; c = c / sc[:, None]; u = u / sb[:, None]
    uf = np.where(bnd, u, 0.0)
    x = np.ones((B, N)); z = np.ones((B, N)); t = np.ones((B, N)); s = np.ones((B, N)); y = np.zeros((B, m))
    tau = np.ones(B); kap = np.ones(B)
    eta = 1.0 - delta
    nb = np.sqrt((b * b).sum(1) + (uf * uf).sum(1))
    nc = np.linalg.norm(np.where(act, c, 0.0), axis=1)
    ncomp = act.sum(axis=1) + bnd.sum(axis=1) + 1
    status = np.full(B, 5, dtype=np.int32)
    iters = np.full(B, max_iter, dtype=np.int32)
    out = {k: np.zeros((B, N)) for k in ("x", "z", "s")}
    out["y"] = np.zeros((B, m)); out["pobj"] = np.zeros(B); out["dobj"] = np.zeros(B); out["tau"] = np.ones(B)
    live = np.ones(B, dtype=bool)
    floored = np.zeros(B, dtype=np.int64)
    sbnd = lambda w: np.where(bnd, w, 0.0)

    def store(sel, it, st):
        if not sel.any():
            return
        with np.errstate(all="ignore"):
            rt = np.where((st == 0) | (st == 5), 1.0 / tau, 1.0)[:, None]
            rr = c * tau[:, None] - y @ A
            po = np.where(act, c * x, 0.0).sum(1); du = (b * y).sum(1) + sbnd(uf * s).sum(1)
            out["x"][sel] = (np.where(act, x, 0.0) * rt * sb[:, None])[sel]
            out["z"][sel] = (np.where(act, z, np.maximum(-rr, 0.0)) * rt * sc[:, None])[sel]
            out["s"][sel] = (np.where(bnd, s, np.where(act, 0.0, np.maximum(rr, 0.0))) * rt * sc[:, None])[sel]
            out["y"][sel] = (y * rt * sc[:, None])[sel]
            out["pobj"][sel] = (po * rt[:, 0] * sb * sc)[sel]
            out["dobj"][sel] = (du * rt[:, 0] * sb * sc)[sel]
        out["tau"][sel] = tau[sel]
        status[sel] = st[sel]
        iters[sel] = it

    for it in range(max_iter):
        with np.errstate(all="ignore"):
            v = y @ A
            rho = b * tau[:, None] - np.where(act, x, 0.0) @ A.T
            om = sbnd(uf * tau[:, None] - x - t)
            sig = np.where(act, c * tau[:, None] - v + z - sbnd(s), 0.0)
            gam = np.where(act, x * z, 0.0).sum(1) + sbnd(s * t).sum(1)
            po = np.where(act, c * x, 0.0).sum(1)
            du = (b * y).sum(1) + sbnd(uf * s).sum(1)
            normr = np.sqrt((rho * rho).sum(1) + (om * om).sum(1))
            norms = np.linalg.norm(sig, axis=1)
            bad = ~(np.isfinite(normr) & np.isfinite(norms) & np.isfinite(gam) & np.isfinite(tau) & np.isfinite(kap))
            opt = ~bad & (normr <= eps * (1 + nb) * tau) & (norms <= eps * (1 + nc) * tau) & (gam <= eps * tau * (tau + np.abs(po)))
            p_ray = (po > 0) & (nb * tau + normr <= 100 * eps * po)
            d_ray = (du < 0) & (nc * tau + norms <= 100 * eps * -du)
            ray = ~bad & ~opt & (p_ray | d_ray)
            st = np.where(bad, 3, np.where(opt, 0, np.where(p_ray & d_ray, np.where(-du > po, 2, 4), np.where(p_ray, 4, 2))))
        fin = live & (bad | opt | ray)
        store(fin, it, st)
        live &= ~fin
        if not live.any():
            break
        with np.errstate(all="ignore"):
            mu = (gam + tau * kap) / ncomp
            dmu = (delta * mu)[:, None]
            phi = du - po + kap
            zx = z / x
            stq = sbnd(s / t)
            d = np.where(act, 1.0 / (zx + stq), 0.0)
            w = d * stq
            h = sbnd(t - dmu / s + eta * om)
            r0 = np.where(act, eta * sig + dmu / x - z, 0.0)
            dr = d * r0 + w * h
            dc = d * np.where(act, c, 0.0) + w * uf
            M = np.einsum("ik,bk,jk->bij", A, d, A)
            stats = {}
            L, D = ldl_floored(M, pivot_floor * pivot_floor, stats)
            floored += np.where(live, stats["floored"], 0)
            p = ldl_solve(L, D, dc @ A.T - b)
            q = ldl_solve(L, D, dr @ A.T - eta * rho)
            atp = p @ A; atq = q @ A
            e = np.where(act, c - atp, 0.0)
            uu = d * e + w * uf
            vv = dr - d * atq
            den = (d * e * e).sum(1) + sbnd(zx * w * uf * uf).sum(1) + kap / tau
            num = (eta * phi + (b * q).sum(1) + dmu[:, 0] / tau - kap - (np.where(act, c, 0.0) * vv).sum(1)
                   + sbnd(uf * w * (r0 - atq - zx * h)).sum(1))
            dtau = num / den
            dy = p * dtau[:, None] + q
            dx = uu * dtau[:, None] + vv
            etol = refine_tol * (1 + nb) * np.maximum(tau, kap)
            rhs_e = eta * rho + b * dtau[:, None]
            for _ in range(max_refine):
                ee = rhs_e - dx @ A.T
                need = live & (np.abs(ee).max(axis=1) > etol)
                if not need.any():
                    break
                ec = ldl_solve(L, D, np.where(need[:, None], ee, 0.0))
                dx = dx + d * (ec @ A)
                dy = dy - ec
            atdy = dy @ A
            badstep = ~(np.isfinite(dy).all(axis=1) & np.isfinite(dtau))
            fin = live & badstep
            store(fin, it, np.full(B, 3))
            live &= ~fin
            dkap = dmu[:, 0] / tau - kap - kap / tau * dtau
            dz = np.where(act, (dmu - z * dx) / x - z, 0.0)
            dt1 = eta * om + uf * dtau[:, None] - dx
            ds1 = (dmu - s * dt1) / t - s
            ds2 = dz + eta * sig + c * dtau[:, None] - atdy
            dt2 = dmu / s - t - (t / s) * ds2
            first = t >= s
            dt = sbnd(np.where(first, dt1, dt2)); ds = sbnd(np.where(first, ds1, ds2))
            ratio = np.maximum(np.where(act, np.maximum(-dz / z, -dx / x), 0.0),
                               np.where(bnd, np.maximum(-dt / t, -ds / s), 0.0)).max(axis=1)
            ratio = np.maximum(np.maximum(ratio, np.maximum(-dtau / tau, -dkap / kap)), 0.0)
            theta = np.minimum(r / ratio, 1.0)
        lv = live[:, None]; th = theta[:, None]
        y = np.where(lv, y + th * dy, y)
        x = np.where(lv & act, x + th * dx, x)
        z = np.where(lv & act, z + th * dz, z)
        t = np.where(lv & bnd, t + th * dt, t)
        s = np.where(lv & bnd, s + th * ds, s)
        tau = np.where(live, tau + theta * dtau, tau)
        kap = np.where(live, kap + theta * dkap, kap)
    store(live, max_iter, np.full(B, 5))
    out["status"], out["iters"], out["floored"] = status, iters, floored
    return out


def certificate_ratio(A, b, c, u, res, k, sb=1.0, sc=1.0):
    """Residual of LP k's certificate over its value, from the returned vectors alone: status 2, |A'y - z + s|inf over
    -b'y - u's; status 4, max(|A x|inf, |x_bnd|inf) over c'x.  The bound of the stop rule is 1e-8; inf when the value has
    the wrong sign.  ``sb, sc``: the LP's scale factors under autoscale (``scale_factors``) -- the certificate is then that of
    the LP the kernel solved, b, u / sb and c / sc with x / sb and y, z, s / sc: neither ratio is invariant under the scaling (in
    the caller's units the first is divided by sb, the second by sc), and the stop rule holds in the kernel's."""
    act = u[k] > 0
    bnd = act & np.isfinite(u[k])
    x, y, z, s = res["x"][k] / sb, res["y"][k] / sc, res["z"][k] / sc, res["s"][k] / sc
    if res["status"][k] == 2:
        val = -(b[k] / sb @ y) - (np.where(bnd, u[k] / sb, 0.0) * s).sum()
        resid = np.abs(y @ A - z + s).max()
    elif res["status"][k] == 4:
        val = c[k] / sc @ x
        resid = max(np.abs(A @ x).max(), np.abs(x[bnd]).max() if bnd.any() else 0.0)
    else:
        raise ValueError("LP %d carries no certificate" % k)
    return resid / val if val > 0 else np.inf


# ---- fixtures -------------------------------------------------------------------------------------------------------------
def random_batch(mp, nd, B, seed, p_inf=0.5, feasible=False):
    """The recipe of DESIGN.md section 26: A = [U(-1, 1) | I], u ~ U(0.5, 3) with +inf at probability ``p_inf``, a slack fixed
    (u = 0) at probability 0.4, b ~ 3 U(-1, 1), c ~ U(-1, 1); ``feasible``: A ~ U(0, 1) and b = A x0 with 0 < x0 < u."""
    rng = np.random.default_rng(seed)
    N = nd + mp
    A = np.hstack([rng.uniform(0, 1, (mp, nd)) if feasible else rng.uniform(-1, 1, (mp, nd)), np.eye(mp)])
    u = rng.uniform(0.5, 3, (B, N))
    u[rng.random((B, N)) < p_inf] = np.inf
    u[:, nd:][rng.random((B, mp)) < 0.4] = 0.0
    b = 3 * rng.uniform(-1, 1, (B, mp))
    c = rng.uniform(-1, 1, (B, N))
    if feasible:
        x0 = rng.uniform(0.05, 0.45, (B, N)) * np.where(u > 0, np.minimum(u, 2.0), 0.0)
        b = x0 @ A.T
    return A, b, c, u


def mixed_batch(mp, nd, B, seed):
    """One shared A = [U(-1, 1) | I] and B LPs that interleave the three verdicts: LP 3i is optimal by construction (b = A x0
    with 0 < x0 < u, c = A'y0 - z0 + s0 with z0, s0 > 0), LP 3i + 1 infeasible by construction (row i mod m' asks for less than
    its columns can give: every column with a negative entry there is bounded, b_i = -(10 + sum |A_ij| u_j)), LP 3i + 2 is primal
    feasible with a random c and few bounds (mostly unbounded: MIXED_SEEDS holds seeds where some are).  Every LP mixes finite
    u, +inf and 0 where it has the columns for it."""
    rng = np.random.default_rng(seed)
    N = nd + mp
    A = np.hstack([rng.uniform(-1, 1, (mp, nd)), np.eye(mp)])
    u = rng.uniform(0.5, 3, (B, N))
    kind = np.arange(B) % 3
    p_inf = np.where(kind == 2, 0.8, 0.4)[:, None]
    u[rng.random((B, N)) < p_inf] = np.inf
    u[:, nd:][rng.random((B, mp)) < 0.4] = 0.0
    if nd >= 2:     # all three sorts of column in every LP
        u[:, 0] = rng.uniform(0.5, 3, B); u[:, nd - 1] = np.inf; u[:, N - 1] = 0.0
    b = 3 * rng.uniform(-1, 1, (B, mp))
    c = rng.uniform(-1, 1, (B, N))
    x0 = rng.uniform(0.05, 0.45, (B, N)) * np.where(u > 0, np.minimum(u, 2.0), 0.0)
    feas = kind != 1
    b[feas] = (x0 @ A.T)[feas]
    y0 = rng.uniform(-1, 1, (B, mp))
    dual = y0 @ A - rng.uniform(0.1, 1, (B, N)) + np.where(np.isfinite(u) & (u > 0), rng.uniform(0.1, 1, (B, N)), 0.0)
    c[kind == 0] = dual[kind == 0]
    for k in np.flatnonzero(kind == 1):
        i = (k // 3) % mp
        neg = A[i] < 0
        u[k, neg & np.isinf(u[k])] = rng.uniform(0.5, 3, int((neg & np.isinf(u[k])).sum()))
        b[k, i] = -(10.0 + (np.abs(A[i]) * np.where(neg, u[k], 0.0)).sum())
    return A, b, c, u


# the GPU test's batches: (m', n) -> seed of mixed_batch(m', n, 64, seed) under which HiGHS finds all three verdicts
# (tests/test_bounded_hsd.py checks it); the sizes that select each of the six shapes, then 1 x 1 and the two exact fills
MIXED_SEEDS = {(12, 16): 11, (14, 30): 1, (16, 44): 1, (24, 32): 8, (24, 64): 1, (30, 90): 1, (1, 1): 32, (16, 16): 51, (32, 64): 1}


def highs_verdicts(A, b, c, u):
    """(status, objective) of every LP by HiGHS (scipy.optimize.linprog): 0 optimal, 2 infeasible, 4 unbounded."""
    from scipy.optimize import linprog
    st, obj = np.zeros(len(b), dtype=np.int32), np.full(len(b), np.nan)
    for k in range(len(b)):
        bounds = [(0.0, None if np.isinf(uj) else float(uj)) for uj in u[k]]
        r = linprog(-c[k], A_eq=A, b_eq=b[k], bounds=bounds, method="highs")
        if r.status == 4 or r.status not in (0, 2, 3):      # 'infeasible or unbounded' of the presolve: ask again without it
            r = linprog(-c[k], A_eq=A, b_eq=b[k], bounds=bounds, method="highs", options=dict(presolve=False))
        st[k] = {0: 0, 2: 2, 3: 4}.get(r.status, -1)
        if r.status == 0:
            obj[k] = -r.fun
    return st, obj
