"""What the time_*.py tools of this directory share: the event timer, the result keys of one timed path, the outputs of a bounded
solve, the --out writer and the gate for a library that lacks an entry (a build of the parent commit under PYCLLP_HIP_LIB)."""
import ctypes
import os
import statistics

import torch

from pycllp_amd import _native
from pycllp_amd.solvers.hip import BOUNDED_RESULTS, bounded_outputs  # noqa: F401  (the tools allocate through these)


def timed(fn, runs):
    fn(); torch.cuda.synchronize()                        # warm-up (and kernel load, plan build)
    ts = []
    for _ in range(runs):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(); fn(); e1.record(); torch.cuda.synchronize()
        ts.append(e0.elapsed_time(e1))
    return statistics.median(ts), ts


def stats(prefix, B, t, ts, status, iters, info):
    return {prefix + "_B": B, prefix + "_ms": round(t, 3), prefix + "_Mlps": round(B / t / 1e3, 4),
            prefix + "_runs_ms": [round(v, 3) for v in ts], prefix + "_optimal": int((status == 0).sum()),
            prefix + "_mean_iters": round(float(iters.mean()), 2), prefix + "_grid": info["grid"],
            prefix + "_waves_per_cu": info["block"] // 64, prefix + "_lds_bytes": info["lds_bytes"]}


def write_lines(lines, out):
    """The --out file: one JSON line per workload."""
    if out:
        os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
        with open(out, "w") as fh:
            fh.write("\n".join(lines) + "\n")


def require_entry(entry, paths):
    """A library without ``entry`` (a build of the parent commit) serves --paths b only: drop the entry's signature there."""
    if not hasattr(ctypes.CDLL(_native.LIB_PATH), entry):
        if paths != {"b"}:
            raise SystemExit("%s has no %s: it serves --paths b only" % (_native.LIB_PATH, entry))
        _native.SIGNATURES = tuple(s for s in _native.SIGNATURES if s[0] != entry)
