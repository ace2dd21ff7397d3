#!/usr/bin/env python
"""Upper bounds on per-problem dense A on the homogeneous self-dual embedding against what it replaces.

    python tools/time_bounded_perA_hsd.py [--B 65536] [--B-mixed 8192] [--runs 5] [--parts kernels,mixed] [--arms device,auto] [--out FILE]
    PYCLLP_HIP_LIB=parent/libpycllp_hip.so python tools/time_bounded_perA_hsd.py --parts mixed --arms auto    # the parent's library

1. kernels: 65 536 feasible LPs of the two workloads of tools/time_bounded_perA.py (24 x 64 and 12 x 32, LP k's matrix A times
   U[0.75, 1.25)), device-resident: pycllp_hip_dense_solve_batch_bounded_hsd against pycllp_hip_dense_solve_batch_bounded through
   ``solve_device`` of one hip_general_batch_primal_normal in one session -- ms per launch (events, median of --runs after a
   warm-up), iterations, optimal count, the ratio.
2. mixed: 8 192 LPs of 24 x 64 with every third one infeasible (equality row 0 asks for more than LP k's own columns can give):
   ``solve(lp)`` host to host (wall clock, --runs runs after a warm-up), ``hsd_device=True`` against ``hsd='auto'``, with both
   arms' status counts.  A library without the new entry (a build of the parent commit) serves --arms auto only.
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

from pycllp_amd import _native  # noqa: E402
from pycllp_amd.solvers import solver_registry  # noqa: E402
from pycllp_amd.solvers.general import subset  # noqa: E402
from time_bounded_perA import workload  # noqa: E402
from timing import timed, write_lines  # noqa: E402

ENTRY = "pycllp_hip_dense_solve_batch_bounded_hsd"
PLUGIN = "hip_general_batch_primal_normal"
WORKLOADS = (("24x64 (8 eq, 8 ranged, 8 le), finite u, per-problem A", (8, 8, 8, 64), 1),
             ("12x32 (4 eq, 4 ranged, 4 le), finite u, per-problem A", (4, 4, 4, 32), 2))


def kernels(name, glp, runs):
    dev = torch.device("cuda:0")
    B = glp.nproblems
    s = solver_registry[PLUGIN](device=dev, hsd=False, autoscale=False)
    subset(glp, np.arange(2)).init(s)
    blp, _ = glp.to_bounded_equality_form()
    t = lambda v: torch.as_tensor(np.ascontiguousarray(v), dtype=torch.float64, device=dev)   # noqa: E731
    Ad, b, c, u = t(s.bounded_matrices(blp)), t(blp.b), t(blp.c), t(blp.u)
    row = dict(workload=name, B=B, m=blp.nrows, N=blp.ncols, device=torch.cuda.get_device_name(0))
    ref = None
    for arm, hsd in (("bounded", False), ("bounded_hsd", True)):
        res = {}
        ms, runs_ms = timed(lambda: res.update(s.solve_device(Ad, b, c, u, hsd=hsd)), runs)
        info = s.launch_info()
        st, it, pobj = res["status"].cpu().numpy(), res["iters"].cpu().numpy(), res["pobj"].cpu().numpy()
        row.update({arm + "_ms": round(ms, 3), arm + "_runs_ms": [round(v, 3) for v in runs_ms], arm + "_Mlps": round(B / ms / 1e3, 3),
                    arm + "_optimal": int((st == 0).sum()), arm + "_mean_iters": round(float(it.mean()), 2),
                    arm + "_max_iters": int(it.max()), arm + "_group_shape": info.get("group_shape"), arm + "_block": info.get("block"),
                    arm + "_grid": info.get("grid")})
        if ref is None:
            ref = (st, pobj)
        else:
            both = (st == 0) & (ref[0] == 0)
            row["max_rel_obj_diff"] = float(np.max(np.abs(pobj - ref[1])[both] / np.maximum(1, np.abs(ref[1][both]))))
    row["hsd_over_bounded"] = round(row["bounded_hsd_ms"] / row["bounded_ms"], 3)
    return row


def mixed(B, seed=3):
    """The feasible 24 x 64 workload with every third LP made infeasible: equality row 0 asks for more than 0 <= x <= u can give
    with LP k's own matrix."""
    glp = workload(8, 8, 8, 64, B, seed)
    A0 = np.asarray(glp.A.data).reshape(B, glp.nrows, glp.ncols)[:, 0, :]
    reach = np.maximum(A0 * glp.u, 0.0).sum(axis=1)
    glp.a[1::3, 0] = glp.b[1::3, 0] = reach[1::3] + 5.0
    return glp


def plugins(glp, runs, arms):
    row = dict(workload="24x64 mixed, per-problem A: every third LP infeasible", B=glp.nproblems,
               library=os.path.relpath(_native.LIB_PATH, ROOT), device=torch.cuda.get_device_name(0))
    status = {}
    for arm in arms:
        s = solver_registry[PLUGIN](device="cuda:0", hsd="auto", **(dict(hsd_device=True) if arm == "device" else {}))
        glp.init(s)
        glp.solve(s)                                    # warm-up: handles, plans, the expansion's second solver
        ts = []
        for _ in range(runs):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            glp.solve(s)
            torch.cuda.synchronize()
            ts.append(1e3 * (time.perf_counter() - t0))
        status[arm] = np.array(s.status)
        vals, cnt = np.unique(status[arm], return_counts=True)
        row.update({arm + "_ms": round(float(np.median(ts)), 2), arm + "_runs_ms": [round(v, 2) for v in ts],
                    arm + "_spread_ms": round(max(ts) - min(ts), 2),
                    arm + "_status_counts": {int(v): int(n) for v, n in zip(vals, cnt)}, arm + "_kernel": s.kernel})
    if len(status) == 2:
        row["statuses_equal"] = bool(np.array_equal(status["auto"], status["device"]))
        row["auto_over_device"] = round(row["auto_ms"] / row["device_ms"], 2)
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--B", type=int, default=65536)
    ap.add_argument("--B-mixed", type=int, default=8192)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--parts", default="kernels,mixed")
    ap.add_argument("--arms", default="device,auto")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    parts, arms = set(args.parts.split(",")), args.arms.split(",")
    if ("kernels" in parts or "device" in arms) and not _native.has_entry(ENTRY):
        sys.exit("%s has no %s: it serves --parts mixed --arms auto only" % (_native.LIB_PATH, ENTRY))
    lines = []
    if "kernels" in parts:
        for name, shape, seed in WORKLOADS:
            lines.append(json.dumps(kernels(name, workload(*shape, args.B, seed), args.runs)))
            print(lines[-1], flush=True)
    if "mixed" in parts:
        lines.append(json.dumps(plugins(mixed(args.B_mixed), args.runs, arms)))
        print(lines[-1], flush=True)
    write_lines(lines, args.out)


if __name__ == "__main__":
    main()
