#!/usr/bin/env python
"""Native bounded kernel against the expansion path on GeneralLP batches.

    python tools/time_bounded.py [--B 65536] [--runs 5] [--out FILE]

Workloads (seeded, feasible by construction): 24 rows (8 equality, 8 ranged, 8 '<='), 64 columns with l = 0 and finite u --
natively m' = 24, N = 88 on the (32, 96) slack-aware kernel, expanded m = 104, N = 168 -- and 12 rows (4 / 4 / 4), 32 columns
(natively m' = 12 on a 16-row kernel).  Device-resident: the bounded form's b, c, u and the expanded LP's b, c are on the GPU
before timing; each path is warmed up, then timed with events around the launch and a synchronise, median of --runs.
"""
import argparse
import ctypes
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
from pycllp_amd.solvers import HipDensePrimalNormalSolver  # noqa: E402
from timing import BOUNDED_RESULTS, bounded_outputs, timed, write_lines  # noqa: E402


def workload(neq, nrng, nle, n, B, seed):
    rng = np.random.default_rng(seed)
    m = neq + nrng + nle
    A = rng.uniform(-1, 1, (m, n))
    u = rng.uniform(0.5, 2.0, (B, n))
    x0 = rng.uniform(0.2, 0.8, (B, n)) * u
    Ax = x0 @ A.T
    a = np.full((B, m), -np.inf); b = np.empty((B, m))
    b[:, :neq] = a[:, :neq] = Ax[:, :neq]
    a[:, neq:neq + nrng] = Ax[:, neq:neq + nrng] - rng.uniform(0.1, 1, (B, nrng))
    b[:, neq:] = Ax[:, neq:] + rng.uniform(0.1, 1, (B, m - neq))
    return GeneralLP(SparseMatrix(matrix=A), b, rng.uniform(-1, 1, (B, n)), a=a, l=np.zeros(n), u=u, f=0.0)


def measure(name, glp, runs):
    dev = torch.device("cuda:0")
    B = glp.nproblems
    L = _native.lib()
    blp, _ = glp.to_bounded_equality_form()
    Ah = torch.as_tensor(np.ascontiguousarray(blp.A.todense()), device=dev)
    h = ctypes.c_void_p()
    _native.check(L.pycllp_hip_dense_init(blp.nrows, blp.ncols, ctypes.c_void_p(Ah.data_ptr()), None, ctypes.byref(h)), "init")
    f64 = dict(dtype=torch.float64, device=dev)
    b, c, u = (torch.as_tensor(np.ascontiguousarray(v), **f64) for v in (blp.b, blp.c, blp.u))
    out = bounded_outputs(B, blp.nrows, blp.ncols, dev)
    o = _native.default_opts()
    P = lambda t: ctypes.c_void_p(t.data_ptr())   # noqa: E731

    def native():
        _native.check(L.pycllp_hip_dense_solve_bounded(h, B, P(b), P(c), P(u), *(P(out[k]) for k in BOUNDED_RESULTS),
                                                       ctypes.byref(o), None), "solve_bounded")
    t_nat, ts_nat = timed(native, runs)
    st_nat, it_nat = out["status"].cpu().numpy(), out["iters"].cpu().numpy()
    pobj_nat = out["pobj"].cpu().numpy() + blp.f
    L.pycllp_hip_dense_free(h)

    eq = glp.to_standard_form().to_equality_form()
    sol = HipDensePrimalNormalSolver(device=dev, hsd=False, autoscale=False)
    eq.init(sol)
    be, ce = sol._dev(eq.b), sol._dev(eq.c)
    res = {}

    def expanded():
        res.update(sol.solve_device(be, ce))
    t_exp, ts_exp = timed(expanded, runs)
    st_exp = res["status"].cpu().numpy()
    pobj_exp = res["pobj"].cpu().numpy() + eq.f
    agree = float(np.max(np.abs(pobj_nat - pobj_exp) / np.maximum(1, np.abs(pobj_exp))))
    return dict(workload=name, B=B, rows=glp.nrows, cols=glp.ncols, native_m=blp.nrows, native_N=blp.ncols,
                expanded_m=eq.nrows, expanded_N=eq.ncols, native_ms=round(t_nat, 3), expanded_ms=round(t_exp, 3),
                native_Mlps=round(B / t_nat / 1e3, 3), expanded_Mlps=round(B / t_exp / 1e3, 3), speedup=round(t_exp / t_nat, 2),
                native_optimal=int((st_nat == 0).sum()), expanded_optimal=int((st_exp == 0).sum()),
                native_mean_iters=round(float(it_nat.mean()), 2), max_rel_obj_diff=agree,
                native_runs_ms=[round(v, 3) for v in ts_nat], expanded_runs_ms=[round(v, 3) for v in ts_exp],
                device=torch.cuda.get_device_name(0))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--B", type=int, default=65536)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    lines = [json.dumps(measure("24x64 (8 eq, 8 ranged, 8 le), finite u", workload(8, 8, 8, 64, args.B, 1), args.runs)),
             json.dumps(measure("12x32 (4 eq, 4 ranged, 4 le), finite u", workload(4, 4, 4, 32, args.B, 2), args.runs))]
    for ln in lines:
        print(ln)
    write_lines(lines, args.out)


if __name__ == "__main__":
    main()
