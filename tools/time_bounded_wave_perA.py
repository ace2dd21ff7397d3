#!/usr/bin/env python
"""Upper bounds on per-problem sparse A: the wave kernel that has both against the route such batches had before it and the
shared-A bounded wave kernel as the ceiling.

    python tools/time_bounded_wave_perA.py [--B 65536] [--Bb 256] [--runs 5] [--paths a,b,c] [--out FILE]
    PYCLLP_HIP_LIB=parent/libpycllp_hip.so python tools/time_bounded_wave_perA.py --paths b   # (b) on another build of the library

Workloads (seeded, feasible by construction; tools/time_bounded_wave.py's generator with a set of values per LP): section 15's
(b), 96 rows (32 equality, 32 ranged, 32 '<='), 288 columns with l = 0 and finite u, A 3 % dense, and 48 rows (16 / 16 / 16), 128
columns at 10 %; LP k's values are A times U[0.75, 1.25) entry by entry on the shared structure.  (Section 15's workload (a), 48
x 128 with a DENSE A, stays out of range: the term tables of a dense structure do not fit the LDS, and per-problem values have
no dense-image plan.)  Timed:
  (a) pycllp_hip_sparse_solve_batch_bounded through hip_sparse_general_batch_primal_normal.solve_device;
  (b) the route these batches had before: hip_sparse_general_primal_normal -> 'expanded', i.e.
      to_standard_form().to_equality_form() on hip_dense_primal_normal with hsd=False, which hands per-problem values to the
      sparse path's kernels.  On the first --Bb LPs; "refused" where the library raises (an expansion beyond 128 rows);
  (c) the shared-A bounded wave kernel (pycllp_hip_sparse_solve_bounded) on LP 0's matrix with every LP's b, c, u: the ceiling.
      (Other LPs than (a)'s, so only its time and iteration count are compared.)
Device-resident: everything is on the GPU before timing; each path is warmed up, then timed with events around the launch and a
synchronise, median of --runs.  A library without the new entry (a build of the parent commit) serves --paths b only.
"""
import argparse
import json
import os
import sys

import numpy as np
import scipy.sparse as sp
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

from pycllp_amd import _native  # noqa: E402
from pycllp_amd.lp import GeneralLP, SparseMatrix  # noqa: E402
from timing import bounded_outputs, require_entry, stats, timed, write_lines  # noqa: E402

ENTRY = "pycllp_hip_sparse_solve_batch_bounded"


def workload(neq, nrng, nle, n, B, seed, density):
    rng = np.random.default_rng(seed)
    m = neq + nrng + nle
    A0 = sp.coo_matrix(np.where(rng.uniform(size=(m, n)) < density, rng.uniform(-1, 1, (m, n)), 0.0))
    rows, cols = A0.row.astype(np.int64), A0.col.astype(np.int64)
    data = A0.data * rng.uniform(0.75, 1.25, (B, rows.size))
    u = rng.uniform(0.5, 2.0, (B, n))
    x0 = rng.uniform(0.2, 0.8, (B, n)) * u
    S = sp.csr_matrix((np.ones(rows.size), (rows, np.arange(rows.size))), shape=(m, rows.size))
    Ax = np.asarray((S @ (data * x0[:, cols]).T).T)
    a = np.full((B, m), -np.inf); b = np.empty((B, m))
    b[:, :neq] = a[:, :neq] = Ax[:, :neq]
    a[:, neq:neq + nrng] = Ax[:, neq:neq + nrng] - rng.uniform(0.1, 1, (B, nrng))
    b[:, neq:] = Ax[:, neq:] + rng.uniform(0.1, 1, (B, m - neq))
    As = SparseMatrix(rows, cols, data)
    As._shape = (m, n)
    return GeneralLP(As, b, rng.uniform(-1, 1, (B, n)), a=a, l=np.zeros(n), u=u, f=0.0)


def measure(name, glp, Bb, runs, paths):
    from pycllp_amd.solvers import solver_registry
    from pycllp_amd.solvers.general import subset
    from pycllp_amd.solvers.hip import Handle, solve_opts
    dev = torch.device("cuda:0")
    B = glp.nproblems
    out = dict(workload=name, rows=glp.nrows, cols=glp.ncols, nnz=glp.A.nnzeros, device=torch.cuda.get_device_name(0))
    blp, _ = glp.to_bounded_equality_form()
    out.update(native_m=blp.nrows, native_N=blp.ncols)
    t = lambda v: torch.as_tensor(np.ascontiguousarray(v), dtype=torch.float64, device=dev)   # noqa: E731
    if "a" in paths:
        sa = solver_registry["hip_sparse_general_batch_primal_normal"](device=dev, hsd=False, autoscale=False)
        subset(glp, np.arange(2)).init(sa)
        Ad, b, c, u = t(sa.bounded_values(blp)), t(blp.b), t(blp.c), t(blp.u)
        ra = {}
        ta, tsa = timed(lambda: ra.update(sa.solve_device(Ad, b, c, u)), runs)
        ia = sa.launch_info()
        out.update(stats("a", B, ta, tsa, ra["status"].cpu().numpy(), ra["iters"].cpu().numpy(), ia), a_wave_shape=ia.get("wave_shape"))
        del Ad, ra
    if "c" in paths:
        A0 = blp.A.tocsr(0)
        A0.sum_duplicates(); A0.sort_indices()
        h = Handle(A0, dev, None)
        b, c, u = t(blp.b), t(blp.c), t(blp.u)
        rc = bounded_outputs(B, blp.nrows, blp.ncols, dev)
        o = solve_opts({})
        tc, tsc = timed(lambda: h.solve_bounded(None, b, c, u, rc, o), runs)
        ic = h.launch_info()
        out.update(stats("c", B, tc, tsc, rc["status"].cpu().numpy(), rc["iters"].cpu().numpy(), ic), c_wave_shape=ic.get("wave_shape"))
        h.free()
    if "b" in paths:
        sub = subset(glp, np.arange(Bb))
        eq = sub.to_standard_form().to_equality_form()
        out.update(b_expanded_m=eq.nrows, b_expanded_N=eq.ncols, b_library=os.path.relpath(_native.LIB_PATH, ROOT))
        sb = solver_registry["hip_dense_primal_normal"](device=dev, hsd=False, autoscale=False, keep_on_device=True)
        try:
            eq.init(sb)
            eq.solve(sb)                                  # uploads the per-problem values
        except NotImplementedError as e:
            out.update(b="refused", b_message=str(e))
        else:
            be, ce = sb._dev(eq.b), sb._dev(eq.c)
            rb = {}
            tb, tsb = timed(lambda: rb.update(sb.solve_device(be, ce)), runs)
            ib = sb.launch_info()
            out.update(stats("b", Bb, tb, tsb, rb["status"].cpu().numpy(), rb["iters"].cpu().numpy(), ib), b_kernel=ib.get("kernel"),
                       b_variant=ib.get("variant"))
    for p, q in (("a", "b"), ("a", "c")):
        if p + "_Mlps" in out and q + "_Mlps" in out:
            out["%s_over_%s" % (p, q)] = round(out[p + "_Mlps"] / out[q + "_Mlps"], 3)
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
    require_entry(ENTRY, paths)
    lines = []
    for name, shape, seed, density in (("96x288 (32 eq, 32 ranged, 32 le) at 3 %, finite u, per-problem values", (32, 32, 32, 288), 2, 0.03),
                                       ("48x128 (16 eq, 16 ranged, 16 le) at 10 %, finite u, per-problem values", (16, 16, 16, 128), 3, 0.10)):
        lines.append(json.dumps(measure(name, workload(*shape, args.B, seed, density), min(args.Bb, args.B), args.runs, paths)))
        print(lines[-1], flush=True)
    write_lines(lines, args.out)


if __name__ == "__main__":
    main()
