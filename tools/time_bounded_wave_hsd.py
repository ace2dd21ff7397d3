#!/usr/bin/env python
"""The bounded wave kernel on the homogeneous self-dual embedding against what it replaces.

    python tools/time_bounded_wave_hsd.py [--B 65536] [--B-mixed 8192] [--runs 5] [--sample 256] [--out FILE]

1. The two workloads of tools/time_bounded_wave.py, feasible by construction, device-resident: 65 536 x (48 rows, 128 dense
   columns; m' = 48, N = 176) and 65 536 x (96 x 288 at 3 %; m' = 96, N = 384).  pycllp_hip_sparse_solve_bounded_hsd against
   pycllp_hip_sparse_solve_bounded on one handle in one session, the two arms ALTERNATING -- ms per launch (events, median of
   --runs), mean iterations, waves per workgroup, the ratio.
2. Mixed batches (every third LP infeasible: equality row 0 asks for more than its columns can give), ``solve(lp)`` of
   hip_sparse_general_primal_normal host to host (wall clock, median of --runs): hsd='device' against hsd='auto' at 36 x 40, a
   shape beyond the lane-group range whose expansion fits, with both arms' status counts; hsd='device' alone at 96 x 288, where the
   expansion is refused, with its statuses against HiGHS on the first --sample LPs.
"""
import argparse
import ctypes
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

from pycllp_amd import _native  # noqa: E402
from pycllp_amd.solvers import HipSparseGeneralPrimalNormalSolver  # noqa: E402
from time_bounded_wave import Sparse, workload  # noqa: E402
from timing import BOUNDED_RESULTS, write_lines  # noqa: E402


def kernels(name, glp, runs):
    blp, _ = glp.to_bounded_equality_form()
    S = Sparse(blp)
    P = S.P

    def hsd():
        _native.check(S.L.pycllp_hip_sparse_solve_bounded_hsd(S.h, S.B, P(S.b), P(S.c), P(S.u), *(P(S.out[k]) for k in BOUNDED_RESULTS),
                                                              ctypes.byref(S.o), None), "pycllp_hip_sparse_solve_bounded_hsd")
    arms = (("bounded", S.bounded), ("bounded_hsd", hsd))
    row = dict(workload=name, B=S.B, m=blp.nrows, N=blp.ncols)
    ts = {k: [] for k, _ in arms}
    for _, fn in arms:                                      # warm-up: kernel load, the plan
        fn(); torch.cuda.synchronize()
    for _ in range(runs):                                   # alternating: A B A B ...
        for k, fn in arms:
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(); fn(); e1.record(); torch.cuda.synchronize()
            ts[k].append(e0.elapsed_time(e1))
    ref = None
    for k, fn in arms:                                      # the last word on the outputs: one more launch per arm
        fn(); torch.cuda.synchronize()
        res, pobj = S.results()
        info = S.info()
        st = S.out["status"].cpu().numpy()
        row.update({k + "_ms": round(statistics.median(ts[k]), 3), k + "_runs_ms": [round(v, 3) for v in ts[k]],
                    k + "_optimal": res["optimal"], k + "_mean_iters": res["mean_iters"], k + "_statuses": res["statuses"],
                    k + "_waves_per_workgroup": info["block"] // 64, k + "_grid": info["grid"], k + "_variant": info["kernel"]})
        if ref is None:
            ref, ref_st = pobj, st
        else:
            both = (st == 0) & (ref_st == 0)
            row["max_rel_obj_diff"] = float(np.max(np.abs(pobj - ref)[both] / np.maximum(1, np.abs(ref[both])))) if both.any() else None
    S.free()
    row["hsd_over_bounded"] = round(row["bounded_hsd_ms"] / row["bounded_ms"], 3)
    row["device"] = torch.cuda.get_device_name(0)
    return row


def mixed(glp):
    """``glp`` (finite u, l = 0) with every third LP made infeasible: equality row 0 asks for more than 0 <= x <= u can give."""
    A = glp.A.todense()
    reach = np.maximum(A[0] * glp.u, 0.0).sum(axis=1)
    glp.a[1::3, 0] = glp.b[1::3, 0] = reach[1::3] + 5.0
    return glp


def highs_status(glp, k):
    from scipy.optimize import linprog
    A = glp.A.todense()
    hi, lo = np.isfinite(glp.b[k]), np.isfinite(glp.a[k])
    r = linprog(-glp.c[k], A_ub=np.vstack([A[hi], -A[lo]]), b_ub=np.concatenate([glp.b[k][hi], -glp.a[k][lo]]),
                bounds=list(zip(np.broadcast_to(glp.l, glp.u.shape)[k], glp.u[k])), method="highs")
    return {0: 0, 2: 2, 3: 4}.get(r.status, -1)


def plugins(name, glp, runs, arms, sample=0):
    row = dict(workload=name, B=glp.nproblems)
    status = {}
    for hsd in arms:
        s = HipSparseGeneralPrimalNormalSolver(device="cuda:0", hsd=hsd)
        glp.init(s)
        glp.solve(s)                                    # warm-up: handle, plans, the expansion's second solver
        ts = []
        for _ in range(runs):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            glp.solve(s)
            torch.cuda.synchronize()
            ts.append(1e3 * (time.perf_counter() - t0))
        status[hsd] = np.array(s.status)
        vals, cnt = np.unique(status[hsd], return_counts=True)
        row.update({hsd + "_ms": round(float(np.median(ts)), 2), hsd + "_runs_ms": [round(v, 2) for v in ts],
                    hsd + "_status_counts": {int(v): int(n) for v, n in zip(vals, cnt)}, hsd + "_kernel": s.kernel})
    if len(arms) == 2:
        row["statuses_equal"] = bool(np.array_equal(status[arms[0]], status[arms[1]]))
        row["%s_over_%s" % arms] = round(row[arms[0] + "_ms"] / row[arms[1] + "_ms"], 2)
    if sample:
        n = min(sample, glp.nproblems)
        ref = np.array([highs_status(glp, k) for k in range(n)])
        row.update(highs_sample=n, highs_statuses_equal=bool(np.array_equal(status[arms[-1]][:n], ref)),
                   highs_mismatches=int((status[arms[-1]][:n] != ref).sum()))
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--B", type=int, default=65536)
    ap.add_argument("--B-mixed", type=int, default=8192)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--sample", type=int, default=256)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    lines = []

    def add(row):
        lines.append(json.dumps(row))
        print(lines[-1], flush=True)
        write_lines(lines, args.out)
    add(kernels("(a) 48x128 (16 eq, 16 ranged, 16 le), dense A, finite u", workload(16, 16, 16, 128, args.B, 1), args.runs))
    add(kernels("(b) 96x288 (32 eq, 32 ranged, 32 le), 3 % dense A, finite u", workload(32, 32, 32, 288, args.B, 2, density=0.03),
                args.runs))
    add(plugins("36x40 (12 eq, 12 ranged, 12 le) mixed: every third LP infeasible; the expansion fits",
                mixed(workload(12, 12, 12, 40, args.B_mixed, 3)), args.runs, ("auto", "device")))
    add(plugins("96x288 at 3 % mixed: every third LP infeasible; the expansion is refused",
                mixed(workload(32, 32, 32, 288, args.B_mixed, 4, density=0.03)), args.runs, ("device",), sample=args.sample))


if __name__ == "__main__":
    main()
