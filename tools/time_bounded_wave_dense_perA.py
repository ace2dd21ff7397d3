#!/usr/bin/env python
"""Upper bounds on per-problem DENSE matrices beyond the lane-group kernels: the wave kernel with an image per wave against the
route such batches had before it and the shared-A bounded dense-image kernel as the ceiling.

    python tools/time_bounded_wave_dense_perA.py [--B 65536] [--Bb 256] [--runs 5] [--paths a,b,c] [--out FILE]
    PYCLLP_HIP_LIB=parent/libpycllp_hip.so python tools/time_bounded_wave_dense_perA.py --paths b   # (b) on another build of the library

Workloads (seeded, feasible by construction, built on the device): section 15's workload (a), 48 rows (16 equality, 16 ranged,
16 '<=') x 128 columns with l = 0 and finite u, dense A, LP k's matrix A times U[0.75, 1.25) entry by entry; and 40 rows (14 / 13
/ 13) x 30 columns of the same kind, where the route before runs.  Timed:
  (a) pycllp_hip_dense_solve_batch_bounded through hip_general_batch_primal_normal(dense_wave=True).solve_device;
  (b) the route before: hip_general_batch_primal_normal with its default options, init() and solve() of the first --Bb LPs --
      'expanded' where it runs, "refused" where the library raises (an expansion beyond 128 rows).  Timed end to end (upload,
      conversion, solve, download: that is the route), between synchronises;
  (c) the shared-A bounded wave kernel on a dense image (pycllp_hip_sparse_solve_bounded) on LP 0's matrix with every LP's b, c,
      u: the ceiling.  (Other LPs than (a)'s, so only its time and iteration count are compared.)
(a) and (c) are device-resident: everything is on the GPU before timing; each is warmed up, then timed with events around the
launch and a synchronise, median of --runs.  A library without the new kernel (a build of the parent commit) serves --paths b only.
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import scipy.sparse as sp
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

from pycllp_amd import _native  # noqa: E402
from pycllp_amd.lp import GeneralLP, SparseMatrix  # noqa: E402
from timing import bounded_outputs, stats, timed, write_lines  # noqa: E402


def workload(neq, nrng, nle, n, B, seed, dev):
    """The batch in the bounded form, on the device: A [B, m, n], b [B, m], c and u [B, n + m]; and what a GeneralLP of its
    first LPs needs (the row bounds a)."""
    g = torch.Generator(device=dev)
    g.manual_seed(seed)
    rnd = lambda *shape: torch.rand(shape, dtype=torch.float64, device=dev, generator=g)     # noqa: E731
    m = neq + nrng + nle
    A = (2.0 * rnd(m, n) - 1.0) * (0.75 + 0.5 * rnd(B, m, n))
    ux = 0.5 + 1.5 * rnd(B, n)
    x0 = (0.2 + 0.6 * rnd(B, n)) * ux
    Ax = torch.bmm(A, x0.unsqueeze(2)).squeeze(2)
    a = torch.full((B, m), -float("inf"), dtype=torch.float64, device=dev)
    b = Ax.clone()
    a[:, :neq] = Ax[:, :neq]
    a[:, neq:neq + nrng] = Ax[:, neq:neq + nrng] - (0.1 + 0.9 * rnd(B, nrng))
    b[:, neq:] = Ax[:, neq:] + (0.1 + 0.9 * rnd(B, m - neq))
    cx = 2.0 * rnd(B, n) - 1.0
    # the bounded form with l = 0: every row kept with +A, slack i in [0, b_i - a_i] (0: equality, +inf: no lower bound)
    c = torch.cat([cx, torch.zeros((B, m), dtype=torch.float64, device=dev)], dim=1)
    u = torch.cat([ux, b - a], dim=1)
    return dict(A=A.contiguous(), a=a, b=b, c=c, u=u, m=m, n=n)


def general_lp(w, Bb):
    """The GeneralLP of the first Bb LPs (host)."""
    m, n = w["m"], w["n"]
    rows, cols = np.divmod(np.arange(m * n), n)
    As = SparseMatrix(rows.astype(np.int64), cols.astype(np.int64), w["A"][:Bb].reshape(Bb, m * n).cpu().numpy())
    As._shape = (m, n)
    h = lambda v: v[:Bb].cpu().numpy()     # noqa: E731
    return GeneralLP(As, h(w["b"]), h(w["c"])[:, :n], a=h(w["a"]), l=np.zeros(n), u=h(w["u"])[:, :n], f=0.0)


def measure(name, w, Bb, runs, paths):
    from pycllp_amd.solvers import solver_registry
    from pycllp_amd.solvers.hip import Handle, solve_opts
    dev = w["A"].device
    B, m, n = int(w["A"].shape[0]), w["m"], w["n"]
    out = dict(workload=name, rows=m, cols=n, native_m=m, native_N=n + m, device=torch.cuda.get_device_name(0),
               library=os.path.relpath(_native.LIB_PATH, ROOT))
    glp = general_lp(w, Bb)
    blp, _ = glp.to_bounded_equality_form()
    # the device-built bounded form is the plugin's own, bit for bit
    out["bounded_form_is_the_plugins"] = all(np.array_equal(w[k][:Bb].cpu().numpy(), v) for k, v in (("b", blp.b), ("c", blp.c), ("u", blp.u)))
    if "a" in paths:
        sa = solver_registry["hip_general_batch_primal_normal"](device=dev, hsd=False, autoscale=False, dense_wave=True)
        glp.init(sa)
        out["bounded_form_is_the_plugins"] &= bool(np.array_equal(sa.bounded_matrices(blp), w["A"][:Bb].cpu().numpy()))
        ra = {}
        ta, tsa = timed(lambda: ra.update(sa.solve_device(w["A"], w["b"], w["c"], w["u"])), runs)
        ia = sa.launch_info()
        out.update(stats("a", B, ta, tsa, ra["status"].cpu().numpy(), ra["iters"].cpu().numpy(), ia), a_kernel=sa.kernel,
                   a_wave_shape=ia.get("wave_shape"), a_group_shape=ia.get("group_shape"))
        del ra
    if "c" in paths:
        A0 = np.ascontiguousarray(blp.A.todense(0))
        h = Handle(sp.csr_matrix(A0), dev, None)
        rc = bounded_outputs(B, m, n + m, dev)
        o = solve_opts({})
        tc, tsc = timed(lambda: h.solve_bounded(None, w["b"], w["c"], w["u"], rc, o), runs)
        ic = h.launch_info()
        out.update(stats("c", B, tc, tsc, rc["status"].cpu().numpy(), rc["iters"].cpu().numpy(), ic), c_wave_shape=ic.get("wave_shape"),
                   c_variant=ic.get("variant"))
        h.free()
        del rc
    if "b" in paths:
        sb = solver_registry["hip_general_batch_primal_normal"](device=dev, hsd=False, autoscale=False)
        try:
            glp.init(sb)
            glp.solve(sb)                                  # warm-up
        except NotImplementedError as e:
            out.update(b="refused", b_message=str(e))
        else:
            ts = []
            for _ in range(runs):
                torch.cuda.synchronize(); t0 = time.perf_counter()
                glp.solve(sb)
                torch.cuda.synchronize(); ts.append(1e3 * (time.perf_counter() - t0))
            tb = float(np.median(ts))
            out.update(b_B=Bb, b_ms=round(tb, 3), b_Mlps=round(Bb / tb / 1e3, 4), b_runs_ms=[round(v, 3) for v in ts],
                       b_optimal=int((sb.status == 0).sum()), b_mean_iters=round(float(np.mean(sb.iters)), 2), b_kernel=sb.kernel)
    for p, q in (("a", "b"), ("a", "c")):
        if p + "_Mlps" in out and q + "_Mlps" in out:
            out["%s_over_%s" % (p, q)] = round(out[p + "_Mlps"] / out[q + "_Mlps"], 3)
    if "a_runs_ms" in out and "b_runs_ms" in out:
        out["every_a_beats_fastest_b"] = bool(B / max(out["a_runs_ms"]) > out["b_B"] / min(out["b_runs_ms"]))
    if "a_over_c" in out:
        out["waves_ratio_a_over_c"] = round(out["a_waves_per_cu"] / out["c_waves_per_cu"], 3)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--B", type=int, default=65536)
    ap.add_argument("--Bb", type=int, default=256)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--paths", default="a,b,c")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    paths = set(args.paths.split(","))
    dev = torch.device("cuda:0")
    lines = []
    for name, shape, seed in (("48x128 dense (16 eq, 16 ranged, 16 le), finite u, per-problem matrices", (16, 16, 16, 128), 1),
                              ("40x30 dense (14 eq, 13 ranged, 13 le), finite u, per-problem matrices", (14, 13, 13, 30), 4)):
        w = workload(*shape, args.B, seed, dev)
        lines.append(json.dumps(measure(name, w, min(args.Bb, args.B), args.runs, paths)))
        print(lines[-1], flush=True)
        del w
        torch.cuda.empty_cache()
    write_lines(lines, args.out)


if __name__ == "__main__":
    main()
