#!/usr/bin/env python
"""Upper bounds on per-problem dense A: the lane-group kernel that has both against the route such batches had before it and
the shared-A bounded kernel as the ceiling.

    python tools/time_bounded_perA.py [--B 65536] [--Bb 8192] [--runs 5] [--paths a,b,c] [--out FILE]
    PYCLLP_HIP_LIB=parent/libpycllp_hip.so python tools/time_bounded_perA.py --paths b     # (b) on another build of the library

Workloads (seeded, feasible by construction; those of tools/time_bounded.py with a matrix per LP): 24 rows (8 equality, 8 ranged,
8 '<='), 64 columns with l = 0 and finite u, and 12 rows (4 / 4 / 4), 32 columns; LP k's matrix is A times U[0.75, 1.25) entry by
entry.  Timed:
  (a) pycllp_hip_dense_solve_batch_bounded through hip_general_batch_primal_normal.solve_device;
  (b) the route these batches had before: hip_general_primal_normal -> 'expanded', i.e. to_standard_form().to_equality_form() on
      hip_dense_primal_normal, which hands per-problem values to the sparse path's kernels.  On --Bb LPs (the first --Bb of the
      batch; the expansion of 65 536 LPs is gigabytes of values); its LPs/s are what the table compares;
  (c) the shared-A bounded kernel (pycllp_hip_dense_solve_bounded) on LP 0's matrix with every LP's b, c, u: the ceiling.  (Other
      LPs than (a)'s, so only its time and iteration count are compared.)
Device-resident: everything is on the GPU before timing; each path is warmed up, then timed with events around the launch and a
synchronise, median of --runs.  A library without the new entry (a build of the parent commit) serves --paths b only.
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

from pycllp_amd import _native  # noqa: E402
from pycllp_amd.lp import GeneralLP, SparseMatrix  # noqa: E402
from timing import bounded_outputs, require_entry, stats, timed, write_lines  # noqa: E402

ENTRY = "pycllp_hip_dense_solve_batch_bounded"


def workload(neq, nrng, nle, n, B, seed):
    rng = np.random.default_rng(seed)
    m = neq + nrng + nle
    A = rng.uniform(-1, 1, (m, n)) * rng.uniform(0.75, 1.25, (B, m, n))
    u = rng.uniform(0.5, 2.0, (B, n))
    x0 = rng.uniform(0.2, 0.8, (B, n)) * u
    Ax = np.einsum("kij,kj->ki", A, x0)
    a = np.full((B, m), -np.inf); b = np.empty((B, m))
    b[:, :neq] = a[:, :neq] = Ax[:, :neq]
    a[:, neq:neq + nrng] = Ax[:, neq:neq + nrng] - rng.uniform(0.1, 1, (B, nrng))
    b[:, neq:] = Ax[:, neq:] + rng.uniform(0.1, 1, (B, m - neq))
    As = SparseMatrix(np.repeat(np.arange(m), n), np.tile(np.arange(n), m), A.reshape(B, -1))
    As._shape = (m, n)
    return GeneralLP(As, b, rng.uniform(-1, 1, (B, n)), a=a, l=np.zeros(n), u=u, f=0.0)


def measure(name, glp, Bb, runs, paths):
    from pycllp_amd.solvers import solver_registry
    from pycllp_amd.solvers.general import subset
    from pycllp_amd.solvers.hip import Handle, solve_opts
    dev = torch.device("cuda:0")
    B = glp.nproblems
    out = dict(workload=name, rows=glp.nrows, cols=glp.ncols, device=torch.cuda.get_device_name(0))
    blp, _ = glp.to_bounded_equality_form()
    out.update(native_m=blp.nrows, native_N=blp.ncols)
    t = lambda v: torch.as_tensor(np.ascontiguousarray(v), dtype=torch.float64, device=dev)   # noqa: E731
    pobj_a = None
    if "a" in paths:
        sa = solver_registry["hip_general_batch_primal_normal"](device=dev, hsd=False, autoscale=False)
        subset(glp, np.arange(2)).init(sa)
        Ad, b, c, u = t(sa.bounded_matrices(blp)), t(blp.b), t(blp.c), t(blp.u)
        ra = {}
        ta, tsa = timed(lambda: ra.update(sa.solve_device(Ad, b, c, u)), runs)
        ia = sa.launch_info()
        st_a, pobj_a = ra["status"].cpu().numpy(), ra["pobj"].cpu().numpy() + blp.f
        out.update(stats("a", B, ta, tsa, st_a, ra["iters"].cpu().numpy(), ia), a_group_shape=ia.get("group_shape"), a_slack=ia.get("slack"))
        del Ad, ra
    if "c" in paths:
        h = Handle(np.ascontiguousarray(blp.A.todense(0)), dev, None)
        b, c, u = t(blp.b), t(blp.c), t(blp.u)
        rc = bounded_outputs(B, blp.nrows, blp.ncols, dev)
        o = solve_opts({})
        tc, tsc = timed(lambda: h.solve_bounded(None, b, c, u, rc, o), runs)
        ic = h.launch_info()
        out.update(stats("c", B, tc, tsc, rc["status"].cpu().numpy(), rc["iters"].cpu().numpy(), ic), c_group_shape=ic.get("group_shape"))
        h.free()
    if "b" in paths:
        sub = subset(glp, np.arange(Bb))
        eq = sub.to_standard_form().to_equality_form()
        sb = solver_registry["hip_dense_primal_normal"](device=dev, hsd=False, autoscale=False, keep_on_device=True)
        eq.init(sb)
        eq.solve(sb)                                      # uploads the per-problem values
        be, ce = sb._dev(eq.b), sb._dev(eq.c)
        rb = {}
        tb, tsb = timed(lambda: rb.update(sb.solve_device(be, ce)), runs)
        ib = sb.launch_info()
        st_b, pobj_b = rb["status"].cpu().numpy(), rb["pobj"].cpu().numpy() + eq.f
        out.update(stats("b", Bb, tb, tsb, st_b, rb["iters"].cpu().numpy(), ib), b_kernel=ib.get("kernel"), b_variant=ib.get("variant"),
                   b_expanded_m=eq.nrows, b_expanded_N=eq.ncols, b_library=os.path.relpath(_native.LIB_PATH, ROOT))
        if pobj_a is not None:
            both = (st_a[:Bb] == 0) & (st_b == 0)
            out.update(max_rel_obj_diff_a_b=float(np.max(np.abs(pobj_a[:Bb] - pobj_b)[both] / np.maximum(1, np.abs(pobj_b[both])))))
    for p, q in (("a", "b"), ("a", "c")):
        if p + "_Mlps" in out and q + "_Mlps" in out:
            out["%s_over_%s" % (p, q)] = round(out[p + "_Mlps"] / out[q + "_Mlps"], 3)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--B", type=int, default=65536)
    ap.add_argument("--Bb", type=int, default=8192)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--paths", default="a,b,c")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    paths = set(args.paths.split(","))
    require_entry(ENTRY, paths)
    lines = []
    for name, shape, seed in (("24x64 (8 eq, 8 ranged, 8 le), finite u, per-problem A", (8, 8, 8, 64), 1),
                              ("12x32 (4 eq, 4 ranged, 4 le), finite u, per-problem A", (4, 4, 4, 32), 2)):
        lines.append(json.dumps(measure(name, workload(*shape, args.B, seed), min(args.Bb, args.B), args.runs, paths)))
        print(lines[-1], flush=True)
    write_lines(lines, args.out)


if __name__ == "__main__":
    main()
