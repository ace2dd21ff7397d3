"""Full-shape against generic instantiation of the plain slack-aware lane-group kernels, at the six shapes an LP can fill:
python tools/dev/time_full_shapes.py -- one line per shape, 65 536 LPs, device-resident kernel time of the two instantiations of
ONE library (PYCLLP_FLAG_GENERIC_SHAPE keeps the generic one), alternating, median and range of 7 launches each after a warm-up."""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
import numpy as np
import torch
from pycllp_amd import _native, problems
from pycllp_amd.lp import EqualityLP, SparseMatrix
from pycllp_amd.solvers import solver_registry

B = 65536
CASES = [(16, 16, (16, 32)), (16, 32, (16, 48)), (16, 48, (16, 64)), (32, 32, (32, 64)), (32, 64, (32, 96)), (32, 96, (32, 128))]


def timed(s, bd, cd):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record(); s.solve_device(bd, cd); e1.record(); torch.cuda.synchronize()
    return e0.elapsed_time(e1)


for m, n, shape in CASES:
    A, b, c = problems.random_dense_arrays(m, n, B)
    Ae, be, ce = problems.equality_arrays(A, b, c)
    lp = EqualityLP(SparseMatrix(matrix=Ae), be, ce, 0.0)
    bd, cd = torch.as_tensor(be, device="cuda"), torch.as_tensor(ce, device="cuda")
    arms = {}
    for arm, flags in (("generic", _native.FLAG_GENERIC_SHAPE), ("full", 0)):
        s = solver_registry["hip_dense_primal_normal"](autoscale=False, hsd=False, flags=flags)
        lp.init(s)
        buf = s.solve_device(bd, cd); torch.cuda.synchronize()
        info = s.launch_info()
        assert info["group_shape"] == shape and info["full_shape"] is (arm == "full"), info
        arms[arm] = (s, [], int((buf["status"].cpu().numpy() == 0).sum()))
    for _ in range(7):
        for arm in ("generic", "full"):
            arms[arm][1].append(timed(arms[arm][0], bd, cd))
    g, f = arms["generic"][1], arms["full"][1]
    print("%2d x %2d on %-9s generic median %7.4f ms (%7.4f .. %7.4f)  full median %7.4f ms (%7.4f .. %7.4f)  %+5.2f %%  optimal %d / %d" % (
        m, n, shape, np.median(g), min(g), max(g), np.median(f), min(f), max(f), 100.0 * (np.median(f) / np.median(g) - 1.0),
        arms["generic"][2], arms["full"][2]), flush=True)
