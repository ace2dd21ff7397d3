#!/usr/bin/env python
"""The bounded kernel on the homogeneous self-dual embedding against what it replaces.

    python tools/time_bounded_hsd.py [--B 65536] [--B-mixed 8192] [--runs 5] [--out FILE]

1. 65 536 x (24 rows, 64 columns), feasible by construction (the workload of tools/time_bounded.py: m' = 24, N = 88 on the
   (32, 96) kernels), device-resident: pycllp_hip_dense_solve_bounded_hsd against pycllp_hip_dense_solve_bounded on one handle in
   one session -- ms per launch (events, median of --runs) and mean iterations.
2. A mixed-sign batch of the same shape (every third LP infeasible: an equality row asks for more than its columns can give):
   ``solve(lp)`` of hip_general_primal_normal with hsd='native' against hsd='auto', host to host (wall clock, median of --runs),
   with both arms' status counts.
"""
import argparse
import ctypes
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
from pycllp_amd.solvers import HipGeneralPrimalNormalSolver  # noqa: E402
from time_bounded import workload  # noqa: E402
from timing import BOUNDED_RESULTS, bounded_outputs, timed, write_lines  # noqa: E402


def kernels(glp, runs):
    dev = torch.device("cuda:0")
    B, L = glp.nproblems, _native.lib()
    blp, _ = glp.to_bounded_equality_form()
    Ah = torch.as_tensor(np.ascontiguousarray(blp.A.todense()), device=dev)
    h = ctypes.c_void_p()
    _native.check(L.pycllp_hip_dense_init(blp.nrows, blp.ncols, ctypes.c_void_p(Ah.data_ptr()), None, ctypes.byref(h)), "init")
    b, c, u = (torch.as_tensor(np.ascontiguousarray(v), dtype=torch.float64, device=dev) for v in (blp.b, blp.c, blp.u))
    o = _native.default_opts()
    P = lambda t: ctypes.c_void_p(t.data_ptr())   # noqa: E731
    row = dict(workload="24x64 (8 eq, 8 ranged, 8 le), finite u, feasible", B=B, m=blp.nrows, N=blp.ncols)
    ref = None
    for name, entry in (("bounded", L.pycllp_hip_dense_solve_bounded), ("bounded_hsd", L.pycllp_hip_dense_solve_bounded_hsd)):
        out = bounded_outputs(B, blp.nrows, blp.ncols, dev)

        def run():
            _native.check(entry(h, B, P(b), P(c), P(u), *(P(out[k]) for k in BOUNDED_RESULTS), ctypes.byref(o), None), name)
        t, ts = timed(run, runs)
        st, it, pobj = out["status"].cpu().numpy(), out["iters"].cpu().numpy(), out["pobj"].cpu().numpy()
        row.update({name + "_ms": round(t, 3), name + "_runs_ms": [round(v, 3) for v in ts], name + "_optimal": int((st == 0).sum()),
                    name + "_mean_iters": round(float(it.mean()), 2), name + "_max_iters": int(it.max())})
        if ref is None:
            ref = pobj
        else:
            both = st == 0
            row["max_rel_obj_diff"] = float(np.max(np.abs(pobj - ref)[both] / np.maximum(1, np.abs(ref[both]))))
    L.pycllp_hip_dense_free(h)
    row["hsd_over_bounded"] = round(row["bounded_hsd_ms"] / row["bounded_ms"], 3)
    row["device"] = torch.cuda.get_device_name(0)
    return row


def mixed(B, seed=3):
    """The feasible workload with every third LP made infeasible: equality row 0 asks for more than 0 <= x <= u can give."""
    glp = workload(8, 8, 8, 64, B, seed)
    A = glp.A.todense()
    reach = np.maximum(A[0] * glp.u, 0.0).sum(axis=1)
    glp.a[1::3, 0] = glp.b[1::3, 0] = reach[1::3] + 5.0
    return glp


def plugins(glp, runs):
    row = dict(workload="24x64 mixed: every third LP infeasible", B=glp.nproblems)
    status = {}
    for hsd in ("auto", "native"):
        s = HipGeneralPrimalNormalSolver(device="cuda:0", hsd=hsd)
        glp.init(s)
        glp.solve(s)                                    # warm-up: handles, plans, the expansion's second solver
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
    row["statuses_equal"] = bool(np.array_equal(status["auto"], status["native"]))
    row["auto_over_native"] = round(row["auto_ms"] / row["native_ms"], 2)
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--B", type=int, default=65536)
    ap.add_argument("--B-mixed", type=int, default=8192)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    lines = [json.dumps(kernels(workload(8, 8, 8, 64, args.B, 1), args.runs)),
             json.dumps(plugins(mixed(args.B_mixed), args.runs))]
    for ln in lines:
        print(ln)
    write_lines(lines, args.out)


if __name__ == "__main__":
    main()
