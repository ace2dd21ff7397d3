#!/usr/bin/env python
"""What PYCLLP_FLAG_AUTOSCALE_PER_LP / ``autoscale='per_lp'`` costs and saves on the headline batch.

    python tools/time_autoscale_per_lp.py [--B 65536] [--runs 5] [--out FILE]

65 536 LPs of (32, 64) (``problems.random_dense_arrays``, equality form N = 96), ``hip_dense_primal_normal``, hsd off.
  (a) the batch as it is -- every LP in band: no flag against the new flag, device-resident.  The price of the maxima and
      of the verdict in the kernel's LP load and store.
  (b) the same batch with 1 % of its LPs scaled out of band (b x 1e3, c x 1e-2): PYCLLP_FLAG_AUTOSCALE for all against
      the new flag, device-resident.
  (c) host to host ``solve(lp)`` of (b): ``autoscale='auto'`` -- which solves the chunks, finds the batch out of band and
      solves them again with the flag -- against ``autoscale='per_lp'``, which runs the pipeline once.  Wall clock.
Each path is warmed up, then timed ``--runs`` times ((a) and (b): events around the launch, the two arms alternating); medians
and every run are reported, one JSON line per comparison."""
import argparse
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

from pycllp_amd import _native, problems  # noqa: E402
from pycllp_amd.lp import SparseMatrix, StandardLP  # noqa: E402
from pycllp_amd.solvers import HipDensePrimalNormalSolver  # noqa: E402
from pycllp_amd.solvers.hip import autoscale_mask  # noqa: E402
from timing import write_lines  # noqa: E402

M, N_STRUCT = 32, 64
B_FACTOR, C_FACTOR = 1e3, 1e-2
WARMUP = 3


def device_pair(name, lp, b, c, flags_a, flags_b, labels, runs):
    s = HipDensePrimalNormalSolver(device="cuda:0", hsd=False, autoscale=False)
    lp.init(s)
    bd, cd = s._dev(b), s._dev(c)
    out = dict(comparison=name, B=int(b.shape[0]), m=M, N=int(c.shape[1]), out_of_band=int(autoscale_mask(b, c).sum()))
    res, ts = {}, {label: [] for label in labels}
    arms = list(zip(labels, (flags_a, flags_b)))
    for _ in range(WARMUP):                                   # (kernel load, plan build, clocks)
        for label, flags in arms:
            res[label] = s.solve_device(bd, cd, flags=flags)
    torch.cuda.synchronize()
    for _ in range(runs):                                     # the two arms alternate
        for label, flags in arms:
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(); res[label] = s.solve_device(bd, cd, flags=flags); e1.record(); torch.cuda.synchronize()
            ts[label].append(e0.elapsed_time(e1))
            if len(ts[label]) == runs:
                st, it = res[label]["status"].cpu().numpy(), res[label]["iters"].cpu().numpy()
                out.update({label + "_ms": round(statistics.median(ts[label]), 3), label + "_runs_ms": [round(v, 3) for v in ts[label]],
                            label + "_optimal": int((st == 0).sum()), label + "_mean_iters": round(float(it.mean()), 2)})
    out["ratio"] = round(out[labels[1] + "_ms"] / out[labels[0] + "_ms"], 4)
    out["device"] = torch.cuda.get_device_name(0)
    return out


def host_pair(lp, runs):
    out = dict(comparison="(c) host to host solve(lp), 1 % out of band: 'auto' against 'per_lp'", B=int(lp.nproblems))
    for mode in ("auto", "per_lp"):
        s = HipDensePrimalNormalSolver(device="cuda:0", hsd=False, autoscale=mode)
        lp.init(s)
        for _ in range(WARMUP):                               # staging buffers, kernel load, clocks
            lp.solve(s)
        ts = []
        for _ in range(runs):
            t0 = time.perf_counter()
            lp.solve(s)
            ts.append(1e3 * (time.perf_counter() - t0))
        out.update({mode + "_ms": round(statistics.median(ts), 3), mode + "_runs_ms": [round(v, 3) for v in ts],
                    mode + "_optimal": int((np.asarray(s.status) == 0).sum())})
    out["ratio"] = round(out["per_lp_ms"] / out["auto_ms"], 4)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--B", type=int, default=65536)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    A, b, c = problems.random_dense_arrays(M, N_STRUCT, args.B)
    lp = StandardLP(SparseMatrix(matrix=A), b, c, 0.0).to_equality_form()
    b0, c0 = np.array(lp.b, dtype=np.float64), np.array(lp.c, dtype=np.float64)
    assert not autoscale_mask(b0, c0).any()
    idx = np.random.RandomState(1).choice(args.B, max(1, args.B // 100), replace=False)
    b1, c1 = b0.copy(), c0.copy()
    b1[idx] *= B_FACTOR
    c1[idx] *= C_FACTOR
    F = _native
    lines = [json.dumps(device_pair("(a) every LP in band: no flag against PER_LP", lp, b0, c0, 0, F.FLAG_AUTOSCALE_PER_LP,
                                    ("flagless", "per_lp"), args.runs)),
             json.dumps(device_pair("(b) 1 % out of band: AUTOSCALE for all against PER_LP", lp, b1, c1, F.FLAG_AUTOSCALE,
                                    F.FLAG_AUTOSCALE_PER_LP, ("autoscale", "per_lp"), args.runs))]
    lp.b, lp.c = b1, c1
    lines.append(json.dumps(host_pair(lp, args.runs)))
    for ln in lines:
        print(ln)
    write_lines(lines, args.out)


if __name__ == "__main__":
    main()
