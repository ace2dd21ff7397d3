#!/usr/bin/env python
"""What the device-side conversion of GeneralLP batches with per-problem values of A costs and saves.

    python tools/time_general_batch_device.py [--B 65536] [--runs 5] [--parts a,b,c] [--parent-root DIR] [--out FILE]

Workloads: section 17's 24 x 64 dense (tools/time_bounded_perA.py, `hip_general_batch_primal_normal`, the lane-group kernel) and
section 18's 96 x 288 at 3 % (tools/time_bounded_wave_perA.py, `hip_sparse_general_batch_primal_normal`, the wave kernel), seeded
as there.  Median of --runs after one warm-up, one JSON line per workload and part:
  (a) host to host: `glp.init(s); glp.solve(s)`, wall clock around each, on this tree and -- with --parent-root, a checkout of
      the parent commit with its library built -- on that one, each in a process of its own; the ratio, and whether the gain
      exceeds the spread (max - min) of the repetitions.
  (b) device resident: `solve_device_general(Adata, a, b, c, l, u, f)` in the original variables against the bounded solve entry
      alone (`solve_device(A, b, c, u)`) on the pre-converted tensors of the same data, GPU events.  The added time against
      three device-to-device copies (torch.Tensor.copy_) that move the bytes the two conversions move.
  (c) pycllp_hip_general_to_bounded_batch alone: time, bytes, achieved bandwidth, next to the copy that moves its bytes.
A copy of a tensor of X bytes reads X and writes X; "the copy of K bytes of traffic" is the copy of a tensor of K / 2 bytes
(`copy_same_traffic`); the copy of a tensor of all K bytes is reported beside it (`copy_of_tensor`).
"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WORKLOADS = {"24x64 dense": ("time_bounded_perA", (8, 8, 8, 64), {}, "hip_general_batch_primal_normal", "bounded group per-problem"),
             "96x288 3%": ("time_bounded_wave_perA", (32, 32, 32, 288), dict(density=0.03), "hip_sparse_general_batch_primal_normal",
                           "bounded wave per-problem")}


def setup(root):
    sys.path.insert(0, os.path.join(root, "tools"))
    sys.path.insert(0, root)


def workload(name, B):
    module, shape, kw, plugin, kernel = WORKLOADS[name]
    glp = __import__(module).workload(*shape, B, 1, **kw)
    return glp, plugin, kernel


def host_to_host(name, B, runs):
    """Part (a) on the package that is first on sys.path."""
    import pycllp_amd
    from pycllp_amd.solvers import solver_registry
    glp, plugin, kernel = workload(name, B)
    s = solver_registry[plugin](device="cuda:0")
    ti, ts = [], []
    for k in range(runs + 1):                           # (the first ones warm up)
        t0 = time.perf_counter(); glp.init(s); ti.append(time.perf_counter() - t0)
        t0 = time.perf_counter(); glp.solve(s); ts.append(time.perf_counter() - t0)
    assert s.kernel == kernel, s.kernel
    ms = lambda v: round(1e3 * v, 1)     # noqa: E731
    return dict(package=os.path.dirname(os.path.abspath(pycllp_amd.__file__)), conversion=getattr(s, "conversion", "host"),
                init_ms=ms(statistics.median(ti[1:])), init_runs_ms=[ms(t) for t in ti[1:]],
                solve_ms=ms(statistics.median(ts[1:])), solve_runs_ms=[ms(t) for t in ts[1:]], optimal=int((s.status == 0).sum()))


def part_a(name, B, runs, parent_root):
    out = dict(part="a host to host", workload=name, B=B)
    for tag, root in (("parent", parent_root), ("branch", ROOT)):
        if root is None:
            continue
        r = subprocess.run([sys.executable, os.path.abspath(__file__), "--one", name, "--root", root, "--B", str(B), "--runs", str(runs)],
                           capture_output=True, text=True)
        if r.returncode:
            raise SystemExit("part (a) on %s failed:\n%s" % (root, r.stderr[-2000:]))
        out[tag] = json.loads(r.stdout.strip().splitlines()[-1])
    if "parent" in out:
        for k in ("solve", "init"):
            p, b = out["parent"], out["branch"]
            spread = max(max(v[k + "_runs_ms"]) - min(v[k + "_runs_ms"]) for v in (p, b))
            out[k + "_parent_over_branch"] = round(p[k + "_ms"] / b[k + "_ms"], 2)
            out[k + "_gain_ms"], out[k + "_spread_ms"] = round(p[k + "_ms"] - b[k + "_ms"], 1), round(spread, 1)
            out[k + "_faster_by_more_than_spread"] = bool(p[k + "_ms"] - b[k + "_ms"] > spread)
    return out


def conversion_bytes(m, n, mk, nnz, out_len, B):
    """(to_bounded_batch, from_bounded): bytes of the caller's arrays each reads and writes."""
    N = n + mk
    to = B * (8 * (nnz + out_len + 2 * m + 3 * n + 1 + mk + 2 * N + 1) + 4)
    back = B * (8 * (n + 1 + 3 * n + mk + 2 + 3 * n + m + 2) + 4)      # l, f^, x^ z^ s^ [:n], y^, objectives in; x, z, s, y, objectives out
    return to, back


def parts_bc(name, B, runs, parts):
    import torch
    from pycllp_amd.solvers import solver_registry
    from timing import timed
    glp, plugin, kernel = workload(name, B)
    s = solver_registry[plugin](device="cuda:0", autoscale=False, hsd=False)
    glp.init(s)
    assert s.conversion == "device"
    Adata, a, b, c, l, u, f = (s._dev(v) for v in (glp.A.data, glp.a, glp.b, glp.c, glp.l, glp.u, glp.f))
    cv = s._conv
    bl = cv.to_bounded(None, Adata, a, b, c, l, u, f)
    Ah = bl["A"].view(s._values_spec(B)[0])
    to_bytes, back_bytes = conversion_bytes(cv.m, cv.n, cv.mk, cv.nnz, cv.out_len, B)

    def copy_ms(nbytes):
        src = torch.empty(nbytes // 8, dtype=torch.float64, device=s.device).normal_()
        dst = torch.empty_like(src)
        return timed(lambda: dst.copy_(src), runs)[0]

    head = dict(workload=name, B=B, rows=cv.m, cols=cv.n, nnz=cv.nnz, out_len=cv.out_len, native_m=cv.mk, native_N=cv.n + cv.mk,
                kernel=kernel, to_bounded_batch_MB=round(to_bytes / 1e6, 1), from_bounded_MB=round(back_bytes / 1e6, 1),
                device=torch.cuda.get_device_name(0))
    lines = []
    if "b" in parts:
        out, res = {}, {}
        t_solve, ts_solve = timed(lambda: out.update(s.solve_device(Ah, bl["b"], bl["c"], bl["u"])), runs)
        t_dev, ts_dev = timed(lambda: res.update(s.solve_device_general(Adata, a, b, c, l, u, f)), runs)
        same = all(bool((res[k] == out[k]).all()) for k in ("status", "iters"))
        t_same, t_tensor = copy_ms((to_bytes + back_bytes) // 2), copy_ms(to_bytes + back_bytes)
        added = t_dev - t_solve
        lines.append(dict(part="b device resident", **head, solve_bounded_ms=round(t_solve, 3), solve_device_general_ms=round(t_dev, 3),
                          added_ms=round(added, 3), copy_same_traffic_ms=round(t_same, 4), copy_of_tensor_ms=round(t_tensor, 4),
                          added_over_copy_same_traffic=round(added / t_same, 2), added_over_copy_of_tensor=round(added / t_tensor, 2),
                          below_three_copies_of_tensor=bool(added < 3 * t_tensor),
                          below_three_copies_same_traffic=bool(added < 3 * t_same), same_status_and_iters=same,
                          optimal=int((res["status"] == 0).sum()), solve_bounded_runs_ms=[round(v, 3) for v in ts_solve],
                          solve_device_general_runs_ms=[round(v, 3) for v in ts_dev]))
    if "c" in parts:
        t_to, ts_to = timed(lambda: cv.to_bounded(None, Adata, a, b, c, l, u, f), runs)
        lines.append(dict(part="c kernel alone", **head, to_bounded_batch_ms=round(t_to, 4),
                          to_bounded_batch_runs_ms=[round(v, 4) for v in ts_to],
                          to_bounded_batch_GBps=round(to_bytes / t_to / 1e6, 1),
                          copy_same_traffic_ms=round(copy_ms(to_bytes // 2), 4), copy_of_tensor_ms=round(copy_ms(to_bytes), 4)))
    return lines


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--B", type=int, default=65536)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--parts", default="a,b,c")
    ap.add_argument("--parent-root", default=None, help="a checkout of the parent commit with its library built: part (a) runs there too")
    ap.add_argument("--out", default=None)
    ap.add_argument("--one", default=None, help=argparse.SUPPRESS)      # part (a) of one workload on the package under --root
    ap.add_argument("--root", default=ROOT, help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.one:
        setup(args.root)
        print(json.dumps(host_to_host(args.one, args.B, args.runs)))
        return
    parts = set(args.parts.split(","))
    setup(ROOT)
    lines = []
    if "a" in parts:                                    # (first: its child processes start before this one opens the GPU)
        for name in WORKLOADS:
            lines.append(json.dumps(part_a(name, args.B, args.runs, args.parent_root)))
            print(lines[-1], flush=True)
    if parts & {"b", "c"}:
        for name in WORKLOADS:
            for ln in parts_bc(name, args.B, args.runs, parts):
                lines.append(json.dumps(ln))
                print(lines[-1], flush=True)
    if args.out:
        from timing import write_lines
        write_lines(lines, args.out)


if __name__ == "__main__":
    main()
