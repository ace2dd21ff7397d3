#!/usr/bin/env python
"""Trajectory parity in figures: for every case of tests/trajectory.py and every k, the reference's spread under permutation, the
tolerance derived from it and the kernel's measured deviation per quantity (the largest over the LPs), plus whether the kernel's
pobj is c'x of the x it returns (its deviation from that; the oracle returns the objectives of the iterate before the last
step).  The source of profiles/r05/trajectory_parity.txt.  GPU box only.  Usage: python tests/dev/trajectory_report.py [id ...]"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
import trajectory as tj  # noqa: E402

print("# case, k: quantity spread / tolerance / kernel deviation [!! = above the tolerance]; pobj-c'x: |pobj - c'x(returned x)|")
for case in tj.CASES:
    if sys.argv[1:] and not any(a in case.id for a in sys.argv[1:]):
        continue
    try:
        got = tj.kernel_results(case)
    except AssertionError as e:
        print("%s: NOT COMPARED -- %s" % (case.id, str(e).splitlines()[0][:200]), flush=True)
        continue
    ref, spread, tol, dev = tj.reference(case.id), tj.spread(case.id), tj.tolerance(case.id), tj.measured(case, got)
    for k in case.ks:
        ok = all((s[k]["status"] == 5).all() and (s[k]["iters"] == k).all() for s in (got, ref))
        cells = ["%s %.0e/%.0e/%.1e%s" % (q, spread[k][q], tol[k][q], dev[k][q], " !!" if dev[k][q] > tol[k][q] else "")
                 for q in tj.quantities(case)]
        if "pobj-c'x" in dev[k]:
            cells.append("pobj-c'x %.1e" % dev[k]["pobj-c'x"])
        print("%-42s k=%d %s  %s" % (case.id, k, "" if ok else "STATUS/ITERS DIFFER", "  ".join(cells)), flush=True)
