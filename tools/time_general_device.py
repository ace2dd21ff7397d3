#!/usr/bin/env python
"""What the device-side conversion of GeneralLP batches costs and saves.

    python tools/time_general_device.py [--B 65536] [--runs 5] [--parts a,b,c] [--parent-root DIR] [--out FILE]

Workloads: section 14's 24 x 64 (tools/time_bounded.py, `hip_general_primal_normal`, the lane-group kernel) and section 15's
48 x 128 (tools/time_bounded_wave.py (a), `hip_sparse_general_primal_normal`, the wave kernel), seeded as there.  Median of
--runs after one warm-up, one JSON line per workload and part:
  (a) host to host: `glp.init(s); glp.solve(s)`, wall clock around solve(), on this tree and -- with --parent-root, a checkout
      of the parent commit with its library built -- on that one, each in a process of its own; the ratio.
  (b) device resident: `solve_device(a, b, c, l, u, f)` in the original variables against the bounded solve entry alone on the
      pre-converted bounded form of the same data (the path of tools/time_bounded*.py, the same library and handle), GPU events.
      The added time against three device-to-device copies (torch.Tensor.copy_) that move the bytes the two conversions move.
  (c) each conversion kernel alone next to the copy that moves its bytes.
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
WORKLOADS = {"24x64": ("time_bounded", (8, 8, 8, 64), "hip_general_primal_normal", "bounded group"),
             "48x128": ("time_bounded_wave", (16, 16, 16, 128), "hip_sparse_general_primal_normal", "bounded wave")}


def setup(root):
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    sys.path.insert(0, root)


def workload(name, B):
    module, shape, plugin, kernel = WORKLOADS[name]
    glp = __import__(module).workload(*shape, B, 1)
    return glp, plugin, kernel


def host_to_host(name, B, runs):
    """Part (a) on the package that is first on sys.path."""
    import pycllp_amd
    from pycllp_amd.solvers import solver_registry
    glp, plugin, kernel = workload(name, B)
    s = solver_registry[plugin](device="cuda:0")
    t0 = time.perf_counter(); glp.init(s); t_init = time.perf_counter() - t0
    ts = []
    for k in range(runs + 1):                           # (the first one warms up)
        t0 = time.perf_counter(); glp.solve(s); ts.append(time.perf_counter() - t0)
    assert s.kernel == kernel, s.kernel
    return dict(package=os.path.dirname(os.path.abspath(pycllp_amd.__file__)), init_ms=round(1e3 * t_init, 1),
                solve_ms=round(1e3 * statistics.median(ts[1:]), 1), solve_runs_ms=[round(1e3 * t, 1) for t in ts[1:]],
                optimal=int((s.status == 0).sum()))


def part_a(name, B, runs, parent_root):
    out = dict(part="a host to host", workload=name, B=B)
    for tag, root in (("parent", parent_root), ("branch", ROOT)):
        if root is None:
            continue
        r = subprocess.run([sys.executable, os.path.abspath(__file__), "--one", name, "--root", root, "--B", str(B), "--runs", str(runs)],
                           capture_output=True, text=True, check=True)
        out[tag] = json.loads(r.stdout.strip().splitlines()[-1])
    if "parent" in out:
        out["solve_parent_over_branch"] = round(out["parent"]["solve_ms"] / out["branch"]["solve_ms"], 2)
        out["init_parent_over_branch"] = round(out["parent"]["init_ms"] / out["branch"]["init_ms"], 2)
    return out


def conversion_bytes(m, n, mk, B):
    """(to_bounded, from_bounded): bytes of the caller's arrays each reads and writes."""
    N = n + mk
    to = B * (8 * (2 * m + 3 * n + 1 + mk + 2 * N + 1) + 4)
    back = B * (8 * (n + 1 + 3 * n + mk + 2 + 3 * n + m + 2) + 4)      # l, f^, x^ z^ s^ [:n], y^, objectives in; x, z, s, y, objectives out
    return to, back


def parts_bc(name, B, runs, parts):
    import torch
    from pycllp_amd.solvers import solver_registry
    from pycllp_amd.solvers.hip import bounded_outputs, solve_opts
    from timing import timed
    glp, plugin, kernel = workload(name, B)
    s = solver_registry[plugin](device="cuda:0", autoscale=False, hsd=False)
    glp.init(s)
    a, b, c, l, u, f = (s._dev(v) for v in (glp.a, glp.b, glp.c, glp.l, glp.u, glp.f))
    cv = s._conv
    bl = cv.to_bounded(None, a, b, c, l, u, f)
    out = bounded_outputs(B, cv.mk, cv.n + cv.mk, s.device)
    o = solve_opts(s.options)
    to_bytes, back_bytes = conversion_bytes(cv.m, cv.n, cv.mk, B)

    def copy_ms(nbytes):
        src = torch.empty(nbytes // 8, dtype=torch.float64, device=s.device).normal_()
        dst = torch.empty_like(src)
        return timed(lambda: dst.copy_(src), runs)[0]

    head = dict(workload=name, B=B, rows=cv.m, cols=cv.n, native_m=cv.mk, native_N=cv.n + cv.mk, kernel=kernel,
                to_bounded_MB=round(to_bytes / 1e6, 1), from_bounded_MB=round(back_bytes / 1e6, 1),
                device=torch.cuda.get_device_name(0))
    lines = []
    if "b" in parts:
        t_solve, ts_solve = timed(lambda: s._handle.solve_bounded(None, bl["b"], bl["c"], bl["u"], out, o), runs)
        res = {}
        t_dev, ts_dev = timed(lambda: res.update(s.solve_device(a, b, c, l, u, f)), runs)
        same = all(bool((res[k] == out[k]).all()) for k in ("status", "iters"))
        t_same, t_tensor = copy_ms((to_bytes + back_bytes) // 2), copy_ms(to_bytes + back_bytes)
        added = t_dev - t_solve
        lines.append(dict(part="b device resident", **head, solve_bounded_ms=round(t_solve, 3), solve_device_ms=round(t_dev, 3),
                          added_ms=round(added, 3), copy_same_traffic_ms=round(t_same, 4), copy_of_tensor_ms=round(t_tensor, 4),
                          added_over_copy_same_traffic=round(added / t_same, 2), added_over_copy_of_tensor=round(added / t_tensor, 2),
                          below_three_copies_of_tensor=bool(added < 3 * t_tensor),
                          below_three_copies_same_traffic=bool(added < 3 * t_same), same_status_and_iters=same,
                          optimal=int((res["status"] == 0).sum()), solve_bounded_runs_ms=[round(v, 3) for v in ts_solve],
                          solve_device_runs_ms=[round(v, 3) for v in ts_dev]))
    if "c" in parts:
        t_to = timed(lambda: cv.to_bounded(None, a, b, c, l, u, f), runs)[0]
        t_back = timed(lambda: cv.from_bounded(None, l, bl["f"], bl["invalid"], out), runs)[0]
        lines.append(dict(part="c kernels alone", **head, to_bounded_ms=round(t_to, 4), to_bounded_copy_same_traffic_ms=round(copy_ms(to_bytes // 2), 4),
                          to_bounded_copy_of_tensor_ms=round(copy_ms(to_bytes), 4), to_bounded_GBps=round(to_bytes / t_to / 1e6, 1),
                          from_bounded_ms=round(t_back, 4), from_bounded_copy_same_traffic_ms=round(copy_ms(back_bytes // 2), 4),
                          from_bounded_copy_of_tensor_ms=round(copy_ms(back_bytes), 4), from_bounded_GBps=round(back_bytes / t_back / 1e6, 1)))
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
