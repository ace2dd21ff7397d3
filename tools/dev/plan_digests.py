#!/usr/bin/env python
"""Two builds of the library plan by plan, on the CPU (no GPU needed): pycllp_hip_debug_plan of both over the matrix set of
tests/test_plan_host.py and a seeded random set, one line per (kind, matrix) with return code, scalar fields and digest.

    python tools/dev/plan_digests.py PARENT/libpycllp_hip.so NEW/libpycllp_hip.so OUT.txt            # digests
    python tools/dev/plan_digests.py PARENT/libpycllp_hip.so NEW/libpycllp_hip.so OUT.txt --time     # plan-building time

The parent needs the same entry: profiles/plan_host/README.md says how it was given one.  --time: the largest matrices,
every kind that takes them, REPS alternating repetitions (parent, new, parent, new, ...) of one call each."""
import os
import sys
import time

import numpy as np
import scipy.sparse as sp

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
import test_plan_host as tph  # noqa: E402

REPS = 7


def random_matrix(m, n, density, seed, tail):
    """m x n (the tail's m columns included) with ``density`` of the columns in front of the tail filled, U[0.05, 1) signed."""
    rs = np.random.RandomState(seed)
    nd = n - m if tail else n
    A = sp.random(m, nd, density=density, random_state=rs, format="csr", data_rvs=lambda k: (0.05 + 0.95 * rs.rand(k)) * rs.choice([-1.0, 1.0], k))
    return tph.with_tail(A) if tail else sp.csr_matrix(A)


LARGEST = (("128x512-2.5%", 128, 512, 0.025, True), ("256x1280-2%", 256, 1280, 0.02, True), ("112x384-dense", 112, 384, 1.0, True),
           ("48x384-dense", 48, 384, 1.0, False))


def random_set():
    out, seed = [], 100
    for m, n in ((16, 64), (33, 129), (128, 512), (200, 900)):
        for density in (0.02, 0.3, 1.0):
            for tail in (True, False):
                seed += 1
                out.append(("random-%dx%d-%g-%s" % (m, n, density, "tail" if tail else "general"), random_matrix(m, n, density, seed, tail)))
    return out + [(name, random_matrix(m, n, d, 7, tail)) for name, m, n, d, tail in LARGEST]


def matrix_set():
    """[(name, kinds, matrix)]"""
    out = [(name, [pk], tph.wave_matrix(case)) for name, case, pk in tph.WAVE_POINTS]
    out += [(name, [tph.BIG if case[0] == "big" else tph.BLOCK], tph.structure(tph.twp.make_case(case))) for name, case in tph.WORKGROUP_POINTS]
    for case in tph.dwc.EVERY:
        m, n, tail = tph.dwc.POINTS[case[0]][case[1]]
        out.append((tph.dwc.every_id(case), [tph.DENSE_PA, tph.DENSE_PA_KEEP], tph.structure(tph.dbc.make(m, n, tail, B=2))))
    out += [("edge-" + name, list(range(8)), A) for name, A in sorted(tph.EDGES.items())]
    out += [(name, list(range(8)), A) for name, A in random_set()]
    # (the block kernel's plan: only where pycllp_hip_sparse_init builds one, m <= 128 and n <= 512)
    return [(name, [k for k in kinds if k != tph.BLOCK or (A.shape[0] <= 128 and A.shape[1] <= 512)], A) for name, kinds, A in out]


def line(res):
    """return code, digest, the scalar fields in the order of the plan header (trailing zeros left out)"""
    rc, p, digest = res
    vals = list(p.values())
    while vals and not vals[-1]:
        vals.pop()
    return "%d %016x %s" % (rc, digest, ",".join(map(str, vals)) if rc == 0 else "-")


def digests(parent, new, out):
    n = bad = 0
    with open(out, "w") as f:
        f.write("# kind matrix: return code, digest, scalar fields of the NEW library; '=': the parent's line is the same, character for\n"
                "# character, else the parent's line follows.  Fields, in order (tests/test_plan_host.py):\n")
        for k in (tph.WAVE, tph.BIG, tph.BLOCK):
            f.write("#   %s: %s\n" % ("wave*, dense-pa*" if k == tph.WAVE else tph.KIND_NAMES[k], " ".join(tph.fields_of(k))))
        for name, kinds, A in matrix_set():
            for kind in kinds:
                a, b = line(tph.build_plan(kind, A, path=parent)), line(tph.build_plan(kind, A, path=new))
                n += 1
                bad += a != b
                f.write("%s %s: %s %s\n" % (tph.KIND_NAMES[kind], name[:-len(tph.KIND_NAMES[kind]) - 1] if name.endswith("-" + tph.KIND_NAMES[kind]) else name, b, "=" if a == b else "DIFFERENT\n    parent: " + a))
        f.write("# %d plans, %d different\n" % (n, bad))
    print("%d plans, %d different" % (n, bad))
    return bad


def timings(parent, new, out):
    with open(out, "w") as f:
        f.write("# one call of pycllp_hip_debug_plan, milliseconds; %d alternating repetitions (parent, new, ...)\n" % REPS)
        f.write("# %-12s %-14s %9s %9s %9s   %9s %9s %9s\n" % ("matrix", "kind", "par.min", "par.med", "par.max", "new.min", "new.med", "new.max"))
        for name, m, n, d, tail in LARGEST:
            A = random_matrix(m, n, d, 7, tail)
            for kind in range(8):
                if tph.build_plan(kind, A, path=new)[0] != 0 or (kind == tph.BLOCK and (m > 128 or n > 512)):
                    continue
                t = {parent: [], new: []}
                for _ in range(REPS):
                    for lib in (parent, new):
                        t0 = time.perf_counter()
                        tph.build_plan(kind, A, path=lib)
                        t[lib].append(1e3 * (time.perf_counter() - t0))
                row = [f(t[lib]) for lib in (parent, new) for f in (min, np.median, max)]
                f.write("%-14s %-14s %9.3f %9.3f %9.3f   %9.3f %9.3f %9.3f\n" % ((name, tph.KIND_NAMES[kind]) + tuple(row)))
    print(open(out).read())


if __name__ == "__main__":
    parent, new, out = sys.argv[1:4]
    sys.exit(timings(parent, new, out) if "--time" in sys.argv else digests(parent, new, out))
