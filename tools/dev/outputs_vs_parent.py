"""Outputs of every lane-group kernel family and option on one build of the library, to compare two builds bit for bit:

    PYCLLP_HIP_LIB=<parent library> python tools/dev/outputs_vs_parent.py --dump DIR_A
    PYCLLP_HIP_LIB=<new library>    python tools/dev/outputs_vs_parent.py --dump DIR_B
    python tools/dev/outputs_vs_parent.py --compare DIR_A DIR_B [BENCH_DIR_A BENCH_DIR_B]

--dump solves 37 seeded batches, 26 of 8 192 LPs (one per family and option: plain, HSD, predictor-corrector, guarded path,
refinement, autoscale, the (16, .), (32, 64), (32, 128) shapes, without identity tail, bounded, per-problem A, bounded per-problem
A), the eight shapes of tests/golden/status_cases.npz on the plain path and three batches with a duplicated and a zero row, and writes status, iters, pobj, dobj, x, y, z of each to DIR/<case>.npz, with one line per case (kernel, lane-group shape, LPs
at status 0).  --compare wants equal bytes on every array (and on the <name>.npy files of two `bench.py --dump-outputs`
directories, if given) and exits 1 otherwise.  The library is the one PYCLLP_HIP_LIB names, as everywhere."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
sys.path.insert(0, os.path.join(ROOT, "tests"))

B = 8192
FORCE_GUARD, AUTOSCALE, NO_SLACK = 4, 8, 16
NAMES = ("status", "iters", "primal_obj", "dual_obj", "x", "y", "z")


def dense(m, n, **opts):
    from pycllp_amd import problems
    from pycllp_amd.lp import EqualityLP, SparseMatrix
    A, b, c = problems.random_dense_arrays(m, n, B, seed=100 * m + n)
    Ae, be, ce = problems.equality_arrays(A, b, c)
    return "hip_dense_primal_normal", EqualityLP(SparseMatrix(matrix=Ae), be, ce, 0.0), dict(dict(autoscale=False, hsd=False), **opts)


def per_problem(m, nd):
    import dense_batch_cases as dbc
    return "hip_dense_batch_primal_normal", dbc.standard_batch(m, nd, B, seed=100 * m + nd), dict(hsd=False, autoscale=False)


def bounded(shape, seed):
    import time_bounded
    return "hip_general_primal_normal", time_bounded.workload(*shape, B, seed), dict(hsd=False)


def bounded_per_problem(shape, seed):
    import time_bounded_perA
    return "hip_general_batch_primal_normal", time_bounded_perA.workload(*shape, B, seed), dict(hsd=False, autoscale=False)


def status_case(k):
    """Shape k of tests/golden/status_cases.npz on the plain path: mixed-sign LPs, most of them infeasible or unbounded, whose
    iterates diverge -- pivots of every size and sign, and non-finite values, pass through the sweep."""
    from conftest import status_cases
    from pycllp_amd.lp import SparseMatrix, StandardLP
    A, b, c = status_cases()[k][:3]
    lp = StandardLP(SparseMatrix(matrix=np.asarray(A)), b, c, 0.0).to_equality_form()
    return "hip_dense_primal_normal", lp, dict(autoscale=False, hsd=False)


def singular(m, N):
    """A duplicated and a zero row (tests/test_guard_sign.py): M singular to rounding, pivots <= 0 where the guard does not bite."""
    from test_guard_sign import singular_lp
    return "hip_dense_primal_normal", singular_lp(m, N, 2048, seed=100 * m + N), dict(autoscale=False, hsd=False)


PC = dict(predcorr=True)
CASES = [
    ("dense3 plain 32x64", lambda: dense(32, 64)),
    ("dense3_hsd 32x64", lambda: dense(32, 64, hsd=True)),
    ("dense3_predcorr 32x64", lambda: dense(32, 64, **PC)),
    ("dense3 guard 32x64", lambda: dense(32, 64, flags=FORCE_GUARD)),
    ("dense3 refine 32x64", lambda: dense(32, 64, refine_tol=1e-15)),
    ("dense3 autoscale 32x64", lambda: dense(32, 64, autoscale=True)),
    ("dense2 16x32", lambda: dense(16, 32)),
    ("dense2 hsd 16x32", lambda: dense(16, 32, hsd=True)),
    ("dense2 predcorr 16x32", lambda: dense(16, 32, **PC)),
    ("20x30 (32,64)", lambda: dense(20, 30)),
    ("20x30 hsd (32,64)", lambda: dense(20, 30, hsd=True)),
    ("20x30 predcorr (32,64)", lambda: dense(20, 30, **PC)),
    ("32x96 (32,128)", lambda: dense(32, 96)),
    ("32x96 hsd (32,128)", lambda: dense(32, 96, hsd=True)),
    ("32x96 predcorr (32,128)", lambda: dense(32, 96, **PC)),
    ("32x64 no-slack (32,96)", lambda: dense(32, 64, flags=NO_SLACK)),
    ("32x64 no-slack predcorr (32,96)", lambda: dense(32, 64, flags=NO_SLACK, **PC)),
    ("32x96 no-slack predcorr (32,128)", lambda: dense(32, 96, flags=NO_SLACK, **PC)),
    ("16x48 (16,64)", lambda: dense(16, 48)),
    ("bounded 24x64", lambda: bounded((8, 8, 8, 64), 1)),
    ("bounded 12x32", lambda: bounded((4, 4, 4, 32), 2)),
    ("perA 32x64", lambda: per_problem(32, 64)),
    ("perA 16x32", lambda: per_problem(16, 32)),
    ("perA 24x30", lambda: per_problem(24, 30)),
    ("bounded perA 24x64", lambda: bounded_per_problem((8, 8, 8, 64), 1)),
    ("bounded perA 12x32", lambda: bounded_per_problem((4, 4, 4, 32), 2)),
    # where the hot sweep's redo verdict decides something: non-positive and non-finite pivots
] + [("status cases %d" % k, lambda k=k: status_case(k)) for k in range(8)] + [
    ("singular 32x96", lambda: singular(32, 96)),
    ("singular 24x60 (32,64)", lambda: singular(24, 60)),
    ("singular 12x40 (16,48)", lambda: singular(12, 40)),
]


def same_bits(x, y):
    """np.array_equal on the bytes: a NaN equals the same NaN, -0 does not equal +0"""
    return x.shape == y.shape and x.dtype == y.dtype and x.tobytes() == y.tobytes()


def dump(out):
    from pycllp_amd.solvers import solver_registry
    os.makedirs(out, exist_ok=True)
    for name, make in CASES:
        plugin, lp, opts = make()
        s = solver_registry[plugin](device="cuda:0", **opts)
        lp.init(s)
        lp.solve(s)
        got = {q: np.asarray(getattr(s, q)) for q in NAMES if getattr(s, q, None) is not None}
        np.savez(os.path.join(out, name.replace(" ", "_") + ".npz"), **got)
        info = s.launch_info()
        print(name, getattr(s, "kernel", None), info.get("group_shape"), "optimal", int((np.asarray(s.status) == 0).sum()), flush=True)


def compare(a, b, bench_a=None, bench_b=None):
    bad = 0
    for f in sorted(os.listdir(a)):
        x, y = np.load(os.path.join(a, f)), np.load(os.path.join(b, f))
        diff = [q for q in x.files if q not in y.files or not same_bits(x[q], y[q])]
        bad += len(diff)
        print("%-40s %d arrays  %s" % (f[:-4].replace("_", " "), len(x.files), "bit-identical" if not diff else "DIFFER: %s" % diff))
    if bench_a:
        for f in sorted(os.listdir(bench_a)):
            x, y = np.load(os.path.join(bench_a, f)), np.load(os.path.join(bench_b, f))
            same = same_bits(x, y)
            bad += not same
            print("bench.py --dump-outputs %-20s shape %-16s %s" % (f, x.shape, "bit-identical" if same else "DIFFERS"))
    print("arrays that differ: %d" % bad)
    return bad


if __name__ == "__main__":
    if sys.argv[1] == "--dump":
        dump(sys.argv[2])
    else:
        sys.exit(1 if compare(*sys.argv[2:6]) else 0)
