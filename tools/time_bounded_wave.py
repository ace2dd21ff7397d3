#!/usr/bin/env python
"""Bounded wave kernel (pycllp_hip_sparse_solve_bounded) against the expansion path and the plain wave
kernel, on GeneralLP batches.

    python tools/time_bounded_wave.py [--B 65536] [--runs 5] [--out FILE]

Workloads (seeded, feasible by construction, l = 0 and finite u on every column):
  (a) 48 rows (16 equality, 16 ranged, 16 '<='), 128 columns, dense A: natively m' = 48, N = 176; expanded m = 208, N = 336
      (the large-LP kernel).  Native against expanded, the expansion timed without and with autoscale (its b is of order 30:
      unscaled, most of its LPs run into the iteration limit).
  (b) 96 rows (32 / 32 / 32), 288 columns, A 3 % dense: natively m' = 96, N = 384; the expansion has more than 256 rows and is
      refused by the library, so native only.
  (c) (a)'s A^ and b with u = +inf on pycllp_hip_sparse_solve (the plain wave kernel on the same plan geometry): time per
      mean iteration against (a)'s native time per mean iteration -- what the bounded phases cost.  The costs are -|c|: with
      (a)'s own costs and no bounds nearly every LP is unbounded and runs to the iteration limit.
Device-resident: every input is on the GPU before timing; each path is warmed up, then timed with events around the launch and
a synchronise, median of --runs.
"""
import argparse
import ctypes
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
from pycllp_amd.solvers import HipDensePrimalNormalSolver  # noqa: E402
from pycllp_amd.solvers.hip import RESULTS  # noqa: E402
from timing import BOUNDED_RESULTS, bounded_outputs, timed, write_lines  # noqa: E402


def workload(neq, nrng, nle, n, B, seed, density=1.0):
    rng = np.random.default_rng(seed)
    m = neq + nrng + nle
    A = rng.uniform(-1, 1, (m, n))
    if density < 1.0:
        A = np.where(rng.uniform(size=(m, n)) < density, A, 0.0)
    u = rng.uniform(0.5, 2.0, (B, n))
    x0 = rng.uniform(0.2, 0.8, (B, n)) * u
    Ax = x0 @ A.T
    a = np.full((B, m), -np.inf); b = np.empty((B, m))
    b[:, :neq] = a[:, :neq] = Ax[:, :neq]
    a[:, neq:neq + nrng] = Ax[:, neq:neq + nrng] - rng.uniform(0.1, 1, (B, nrng))
    b[:, neq:] = Ax[:, neq:] + rng.uniform(0.1, 1, (B, m - neq))
    return GeneralLP(SparseMatrix(matrix=A), b, rng.uniform(-1, 1, (B, n)), a=a, l=np.zeros(n), u=u, f=0.0)


class Sparse:
    """A sparse handle for A^ and device buffers for B LPs."""

    def __init__(self, blp):
        self.dev = torch.device("cuda:0")
        self.L = _native.lib()
        A = sp.csr_matrix(blp.A.tocsr())
        A.sum_duplicates(); A.eliminate_zeros(); A.sort_indices()
        f64 = dict(dtype=torch.float64, device=self.dev)
        self._a = [torch.as_tensor(np.ascontiguousarray(A.data), **f64),
                   torch.as_tensor(A.indptr.astype(np.int32), device=self.dev),
                   torch.as_tensor(A.indices.astype(np.int32), device=self.dev)]
        self.h = ctypes.c_void_p()
        _native.check(self.L.pycllp_hip_sparse_init(A.shape[0], A.shape[1], int(A.nnz), *(self.P(t) for t in self._a), None,
                                                    ctypes.byref(self.h)), "pycllp_hip_sparse_init")
        self.B = blp.nproblems
        self.b, self.c, self.u = (torch.as_tensor(np.ascontiguousarray(v), **f64) for v in (blp.b, blp.c, blp.u))
        self.out = bounded_outputs(self.B, blp.nrows, blp.ncols, self.dev)
        self.o = _native.default_opts()

    def set_c(self, c):
        self.c = torch.as_tensor(np.ascontiguousarray(c), dtype=torch.float64, device=self.dev)

    @staticmethod
    def P(t):
        return ctypes.c_void_p(t.data_ptr())

    def bounded(self):
        P = self.P
        _native.check(self.L.pycllp_hip_sparse_solve_bounded(self.h, self.B, P(self.b), P(self.c), P(self.u),
                                                             *(P(self.out[k]) for k in BOUNDED_RESULTS),
                                                             ctypes.byref(self.o), None), "pycllp_hip_sparse_solve_bounded")

    def plain(self):
        P = self.P
        _native.check(self.L.pycllp_hip_sparse_solve(self.h, self.B, P(self.b), P(self.c), *(P(self.out[k]) for k in RESULTS),
                                                     ctypes.byref(self.o), None), "pycllp_hip_sparse_solve")

    def info(self):
        g, bl, lds, k = (ctypes.c_int() for _ in range(4))
        self.L.pycllp_hip_sparse_launch_info(self.h, *(ctypes.byref(v) for v in (g, bl, lds, k)))
        return dict(grid=g.value, block=bl.value, lds_bytes=lds.value, kernel={1: "tables", 2: "dense image"}.get(k.value, k.value))

    def results(self):
        st, it = self.out["status"].cpu().numpy(), self.out["iters"].cpu().numpy()
        return dict(optimal=int((st == 0).sum()), statuses={int(k): int(v) for k, v in zip(*np.unique(st, return_counts=True))},
                    mean_iters=round(float(it.mean()), 2)), self.out["pobj"].cpu().numpy()

    def free(self):
        self.L.pycllp_hip_sparse_free(self.h)


def native(name, glp, runs, expand=True, plain=False):
    blp, _ = glp.to_bounded_equality_form()
    S = Sparse(blp)
    t_nat, ts_nat = timed(S.bounded, runs)
    res, pobj_nat = S.results()
    st_nat = S.out["status"].cpu().numpy()
    out = dict(workload=name, B=S.B, rows=glp.nrows, cols=glp.ncols, native_m=blp.nrows, native_N=blp.ncols,
               native_ms=round(t_nat, 3), native_Mlps=round(S.B / t_nat / 1e3, 3), native=res, native_launch=S.info(),
               native_runs_ms=[round(v, 3) for v in ts_nat])
    out["native_us_per_iter"] = round(1e3 * t_nat / res["mean_iters"], 3)
    if plain:
        # (c): the same A^ and b, u = +inf, costs -|c| (bounded) on the plain wave kernel
        S.set_c(-np.abs(blp.c))
        t_pl, ts_pl = timed(S.plain, runs)
        rp, _ = S.results()
        out.update(plain_ms=round(t_pl, 3), plain=rp, plain_launch=S.info(), plain_runs_ms=[round(v, 3) for v in ts_pl],
                   plain_us_per_iter=round(1e3 * t_pl / rp["mean_iters"], 3))
        out["bounded_over_plain_per_iter"] = round(out["native_us_per_iter"] / out["plain_us_per_iter"], 3)
    S.free()
    if expand:
        eq = glp.to_standard_form().to_equality_form()
        for tag, scale in (("expanded", False), ("expanded_autoscale", True)):
            sol = HipDensePrimalNormalSolver(device=torch.device("cuda:0"), hsd=False, autoscale=scale)
            eq.init(sol)
            be, ce = sol._dev(eq.b), sol._dev(eq.c)
            r = {}
            t_exp, ts_exp = timed(lambda: r.update(sol.solve_device(be, ce)), runs)
            st_exp = r["status"].cpu().numpy()
            pobj_exp = r["pobj"].cpu().numpy() + eq.f
            ok = (st_exp == 0) & (st_nat == 0)
            out.update({tag + "_ms": round(t_exp, 3), tag + "_Mlps": round(S.B / t_exp / 1e3, 3),
                        tag + "_time_ratio": round(t_exp / t_nat, 2), tag + "_optimal": int((st_exp == 0).sum()),
                        tag + "_mean_iters": round(float(r["iters"].float().mean()), 2),
                        tag + "_runs_ms": [round(v, 3) for v in ts_exp],
                        tag + "_max_rel_obj_diff_both_optimal": float(np.max(
                            (np.abs(pobj_nat + blp.f - pobj_exp) / np.maximum(1, np.abs(pobj_exp)))[ok], initial=0.0))})
        out.update(expanded_m=eq.nrows, expanded_N=eq.ncols)
    out["device"] = torch.cuda.get_device_name(0)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--B", type=int, default=65536)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    lines = [json.dumps(native("(a) 48x128 (16 eq, 16 ranged, 16 le), dense A, finite u", workload(16, 16, 16, 128, args.B, 1),
                               args.runs, expand=True, plain=True)),
             json.dumps(native("(b) 96x288 (32 eq, 32 ranged, 32 le), A 3 % dense, finite u",
                               workload(32, 32, 32, 288, args.B, 2, density=0.03), args.runs, expand=False))]
    for ln in lines:
        print(ln, flush=True)
    write_lines(lines, args.out)


if __name__ == "__main__":
    main()
