"""Device-resident kernel time of the dense lane-group kernels at shapes and options that bench.py has no record for:
python tools/dev/time_group_shapes.py -- one line per case, median and range of 7 launches after a warm-up, 65 536 LPs (the
library named by PYCLLP_HIP_LIB, as everywhere)."""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
import numpy as np
import torch
from pycllp_amd import problems
from pycllp_amd.lp import EqualityLP, SparseMatrix
from pycllp_amd.solvers import solver_registry

B = 65536
NO_SLACK = 16
CASES = [  # name, m, n, options
    ("20x30 predcorr            <32,64,true,true>", 20, 30, dict(predcorr=True, hsd=False)),
    ("20x30 plain               <32,64,true,false>", 20, 30, dict(hsd=False)),
    ("32x64 no-slack plain      <32,96,false,false>", 32, 64, dict(hsd=False, flags=NO_SLACK)),
    ("32x64 no-slack predcorr   <32,96,false,true>", 32, 64, dict(predcorr=True, hsd=False, flags=NO_SLACK)),
    ("20x30 hsd                 hsd<32,64,true>", 20, 30, dict(hsd=True)),
    ("20x30 no-slack hsd        hsd<32,64,false>", 20, 30, dict(hsd=True, flags=NO_SLACK)),
    ("16x48 plain               <16,64,true,false>", 16, 48, dict(hsd=False)),
    ("16x48 predcorr            <16,64,true,true>", 16, 48, dict(predcorr=True, hsd=False)),
    ("16x32 no-slack predcorr   <16,48,false,true>", 16, 32, dict(predcorr=True, hsd=False, flags=NO_SLACK)),
]
for name, m, n, opts in CASES:
    A, b, c = problems.random_dense_arrays(m, n, B)
    Ae, be, ce = problems.equality_arrays(A, b, c)
    lp = EqualityLP(SparseMatrix(matrix=Ae), be, ce, 0.0)
    bd, cd = torch.as_tensor(be, device="cuda"), torch.as_tensor(ce, device="cuda")
    s = solver_registry["hip_dense_primal_normal"](autoscale=False, **opts)
    lp.init(s)
    buf = s.solve_device(bd, cd); torch.cuda.synchronize()
    ts = []
    for _ in range(7):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(); s.solve_device(bd, cd); e1.record(); torch.cuda.synchronize(); ts.append(e0.elapsed_time(e1))
    st = buf["status"].cpu().numpy()
    info = s.launch_info()
    print("%-46s median %7.4f ms  min %7.4f  max %7.4f  optimal %d  shape %s slack %s" % (
        name, np.median(ts), min(ts), max(ts), int((st == 0).sum()), info.get("group_shape"), info.get("slack")), flush=True)
