#!/usr/bin/env python
"""Per-problem dense A beyond the lane-group kernels: the wave kernel with a dense image per wave against the sparse path and the
shared-A ceiling.

    python tools/time_perA_wave.py [--B 16384] [--runs 5] [--shapes 40x40,48x128,100x80] [--out profiles/perA_wave/time_perA_wave.txt]

Workload (seeded, ``pycllp_amd.problems``): standard-form LPs m x n with A, b, c of ``random_dense_arrays(m, n, B, seed=0)`` and
LP k's matrix A times U[0.75, 1.25) entry by entry (``per_problem_values(A, B, seed=7)``); equality form [A_k | I].  Timed:
  (a) pycllp_hip_dense_solve_batch through hip_dense_batch_primal_normal.solve_device (A_k [B, m, n] on the device), which must
      report ``kernel == 'wave per-problem'``;
  (b) the same batch through hip_sparse_primal_normal, as that plugin routes it (which kernel served is recorded; a refusal is
      recorded instead of a time);
  (c) the shared-A dense-image wave kernel (hip_dense_primal_normal) on the same b, c with the one matrix A: the ceiling.
Device-resident: everything is on the GPU before timing; each path is warmed up, then timed with events around the launch and
a synchronise, median of --runs.  ``a_every_run_faster_than_b``: the slowest run of (a) against the fastest of (b).
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

from pycllp_amd import problems  # noqa: E402
from pycllp_amd.lp import EqualityLP, SparseMatrix, StandardLP  # noqa: E402
from pycllp_amd.solvers import solver_registry  # noqa: E402
from timing import timed, write_lines  # noqa: E402


def waves(info):
    return info["block"] // 64


def measure(m, n, B, runs):
    dev = torch.device("cuda:0")
    A, b, c = problems.random_dense_arrays(m, n, B, seed=0)
    rows, cols, data = problems.per_problem_values(sp.csr_matrix(A), B, seed=7)
    assert np.array_equal(rows * n + cols, np.arange(m * n))            # row-major: data.reshape(B, m, n) is the batch
    ce = np.hstack([c, np.zeros((B, m))])
    out = dict(m=m, n=n, N=n + m, B=B, device=torch.cuda.get_device_name(0))

    # (a) the wave kernel with an image per wave
    sa = solver_registry["hip_dense_batch_primal_normal"](device=dev, hsd=False, autoscale=False)
    probe = StandardLP(SparseMatrix(rows, cols, data[:2]), b[:2], c[:2], 0.0).to_equality_form()
    probe.init(sa)
    Ad = torch.as_tensor(data.reshape(B, m, n), device=dev)
    bd, cd = torch.as_tensor(b, device=dev), torch.as_tensor(ce, device=dev)
    ra = {}
    ta, tsa = timed(lambda: ra.update(sa.solve_device(Ad, bd, cd)), runs)
    assert sa.kernel == "wave per-problem", sa.kernel
    ia = sa.launch_info()
    st_a, po_a, it_a = ra["status"].cpu().numpy(), ra["pobj"].cpu().numpy(), ra["iters"].cpu().numpy()
    out.update(a_ms=round(ta, 3), a_Mlps=round(B / ta / 1e3, 4), a_runs_ms=[round(v, 3) for v in tsa], a_optimal=int((st_a == 0).sum()),
               a_mean_iters=round(float(it_a.mean()), 2), a_wave_shape=ia.get("wave_shape"), a_variant=ia.get("variant"),
               a_grid=ia["grid"], a_waves_per_workgroup=waves(ia), a_lds_bytes=ia["lds_bytes"])
    del Ad, ra

    # (c) the shared-A ceiling
    sc = solver_registry["hip_dense_primal_normal"](device=dev, hsd=False, autoscale=False)
    StandardLP(SparseMatrix(matrix=A), b[:2], c[:2], 0.0).to_equality_form().init(sc)
    tc, tsc = timed(lambda: sc.solve_device(bd, cd), runs)
    ic = sc.launch_info()
    out.update(c_ms=round(tc, 3), c_Mlps=round(B / tc / 1e3, 4), c_runs_ms=[round(v, 3) for v in tsc], c_kernel=ic.get("kernel"),
               c_variant=ic.get("variant"), c_wave_shape=ic.get("wave_shape"), c_grid=ic["grid"], c_waves_per_workgroup=waves(ic),
               c_lds_bytes=ic["lds_bytes"])

    # (b) the parent's route: hip_sparse_primal_normal on the per-problem values
    tail = np.arange(m)
    Ae = SparseMatrix(np.r_[rows, tail], np.r_[cols, n + tail], np.hstack([data, np.ones((B, m))]))
    Ae._shape = (m, n + m)
    del data
    lpe = EqualityLP(Ae, b, ce, 0.0)
    sb = solver_registry["hip_sparse_primal_normal"](device=dev, hsd=False, autoscale=False, keep_on_device=True)
    try:
        lpe.init(sb)
        lpe.solve(sb)                                     # uploads the per-problem values
        rb = {}
        tb, tsb = timed(lambda: rb.update(sb.solve_device(bd, cd)), runs)
        ib = sb.launch_info()
        st_b, po_b = rb["status"].cpu().numpy(), rb["pobj"].cpu().numpy()
        both = (st_a == 0) & (st_b == 0)
        out.update(b_ms=round(tb, 3), b_Mlps=round(B / tb / 1e3, 4), b_runs_ms=[round(v, 3) for v in tsb],
                   b_optimal=int((st_b == 0).sum()), b_kernel=ib.get("kernel"), b_variant=ib.get("variant"),
                   b_wave_shape=ib.get("wave_shape"), b_grid=ib["grid"], b_waves_per_workgroup=waves(ib), b_lds_bytes=ib["lds_bytes"],
                   a_over_b=round(tb / ta, 2), a_every_run_faster_than_b=bool(max(tsa) < min(tsb)),
                   max_rel_obj_diff_a_b=float(np.max(np.abs(po_a - po_b)[both] / np.maximum(1, np.abs(po_b[both])))))
    except (NotImplementedError, ValueError) as e:
        out.update(b_refused="%s: %s" % (type(e).__name__, e))
    out.update(a_over_c=round(tc / ta, 3))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--B", type=int, default=16384)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--shapes", default="40x40,48x128,100x80")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    lines = []
    for s in args.shapes.split(","):
        m, n = map(int, s.split("x"))
        lines.append(json.dumps(measure(m, n, args.B, args.runs)))
        print(lines[-1], flush=True)
    write_lines(lines, args.out)


if __name__ == "__main__":
    main()
