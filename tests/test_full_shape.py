"""The full-shape instantiations of the slack-aware lane-group kernels (csrc/ipm_group.inc: ipm_group_kernel's FULL; chosen in
csrc/abi_dense.hip for an LP whose m and n -- equality form -- are exactly the (MP, NP) of a compiled shape; the plain step
only: no predictor-corrector or HSD kernel has one).
They drop the per-column padding tests, every one of which is true for such an LP, so they must give the bits of the generic
instantiation, which PYCLLP_FLAG_GENERIC_SHAPE keeps: 32 x 64 fills (32, 96), 16 x 32 fills (16, 48), 32 x 32 fills (32, 64)
and 32 x 96 fills (32, 128).

``launch_info()["full_shape"]`` says which of the two served a launch.  The batches, the oracle's results and the kernel's solves
that test_fused_forward.py also uses are its cached ones."""
import numpy as np
import pytest
import torch

from pycllp_amd import _native, problems
from pycllp_amd.lp import SparseMatrix, StandardLP
from pycllp_amd.solvers import solver_registry
from pycllp_amd.solvers.hip import autoscale_mask
from test_fused_forward import B, BITWISE, PC_OPTS, assert_matches, reference, solve, solved, standard

pytestmark = pytest.mark.gpu
GENERIC = _native.FLAG_GENERIC_SHAPE

# batch (m, n) -> the slack-aware shape (MP, NP) it fills exactly
FILLED = {(32, 64): (32, 96), (16, 32): (16, 48), (32, 32): (32, 64), (32, 96): (32, 128)}


def few(m, n, **opts):
    """Eight LPs of m x n, solved."""
    A, b, c = problems.random_dense_arrays(m, n, 8, seed=7)
    return solve(StandardLP(SparseMatrix(matrix=A), b, c, 0.0).to_equality_form(), **opts)


def test_selection():
    """Full shape iff m == MP and n == NP, and not with PYCLLP_FLAG_GENERIC_SHAPE; one column short falls back."""
    for key in ((32, 64), (16, 32)):
        info = solved(key).launch_info()
        assert info["full_shape"] is True and info["group_shape"] == FILLED[key] and info["slack"] == 1, info
    assert solved((20, 30)).launch_info()["full_shape"] is False
    info = solved((32, 64), flags=GENERIC).launch_info()
    assert info["full_shape"] is False and info["group_shape"] == (32, 96) and info["slack"] == 1, info
    short = few(32, 63)
    info = short.launch_info()
    assert info["full_shape"] is False and info["group_shape"] == (32, 96) and info["slack"] == 1, info
    assert (short.status == 0).all()
    for opts in (PC_OPTS, dict(hsd=True)):      # no full-shape kernel behind these options
        assert solved((32, 64), **opts).launch_info()["full_shape"] is False, opts


def slots_refill(info):
    """More LPs than lane groups in the launch: slots take a second LP from the queue."""
    return B > info["grid"] * (info["block"] // 64) * (64 // info["group_shape"][0])


@pytest.mark.parametrize("pc", [False, True], ids=["plain", "predcorr"])
@pytest.mark.parametrize("key", sorted(FILLED), ids=["%dx%d" % k for k in sorted(FILLED)])
def test_full_equals_generic_bit_for_bit(key, pc):
    """The large batch, in which slots refill from the queue (the 16-row kernels, with four lane groups per wave, on half the
    CUs of the device so that they do), and a batch of 3 LPs, in which the second lane group of a wave is never live.
    predcorr: there is no full-shape predictor-corrector kernel, so these cases pin only that the generic one serves both
    launches and that the flag changes nothing there; they become the real comparison the day such a kernel is built."""
    opts = dict(PC_OPTS) if pc else {}
    if key[0] == 16:
        opts["reserve_cus"] = torch.cuda.get_device_properties(0).multi_processor_count // 2
    full, generic = solved(key, **opts), solved(key, flags=GENERIC, **opts)
    for s, want in ((full, not pc), (generic, False)):
        info = s.launch_info()
        assert info["full_shape"] is want and info["group_shape"] == FILLED[key] and slots_refill(info), info
    assert (full.status == 0).all()
    for name in BITWISE:
        np.testing.assert_array_equal(getattr(full, name), getattr(generic, name), err_msg=name)
    lp = standard(*key)
    b3, c3 = np.ascontiguousarray(lp.b[:3]), np.ascontiguousarray(lp.c[:3])
    opts.pop("reserve_cus", None)
    full3, generic3 = solve(lp, b3, c3, **opts), solve(lp, b3, c3, flags=GENERIC, **opts)
    assert full3.launch_info()["full_shape"] is (not pc) and generic3.launch_info()["full_shape"] is False
    for name in BITWISE:
        np.testing.assert_array_equal(getattr(full3, name), getattr(generic3, name), err_msg=name)
        np.testing.assert_array_equal(getattr(full3, name), getattr(full, name)[:3], err_msg=name)


@pytest.mark.parametrize("key", [(32, 64), (16, 32)], ids=["32x64", "16x32"])
def test_full_matches_the_oracle(key):
    s = solved(key)
    assert s.launch_info()["full_shape"] is True
    assert_matches(s, reference(key, 0))


def test_warm_start_bit_for_bit():
    """PYCLLP_FLAG_WARM_START reads x, y, z under `ok[]` when it loads an LP: a loose cold solve, then the warm one from its
    result, on either instantiation."""
    lp = standard(32, 64)
    got = []
    for flags in (0, GENERIC):
        s = solver_registry["hip_dense_primal_normal"](device="cuda:0", autoscale=False, flags=flags)
        lp.init(s)
        s.solve_device(lp.b, lp.c, eps=1e-4)
        buf = s.solve_device(lp.b, lp.c, warm_start=True)
        torch.cuda.synchronize()
        assert s.launch_info()["full_shape"] is (flags == 0)
        got.append({k: buf[k].cpu().numpy().copy() for k in ("status", "iters", "pobj", "dobj", "x", "y", "z")})
    assert (got[0]["status"] == 0).any()     # (a raw restart, without the plugin's lift, may jam an LP: on both alike)
    for k in got[0]:
        np.testing.assert_array_equal(got[0][k], got[1][k], err_msg=k)


def test_autoscale_per_lp_bit_for_bit():
    """``autoscale='per_lp'`` takes max|c| under `ok[]` at the load and at the store: every other LP out of band."""
    lp = standard(32, 64)
    b, c = lp.b.copy(), lp.c.copy()
    b[::2] *= 100.0
    c[::2] *= 0.01
    mask = autoscale_mask(b, c)
    assert mask[::2].all() and not mask[1::2].any()
    got = []
    for flags in (0, GENERIC):
        s = solver_registry["hip_dense_primal_normal"](device="cuda:0", autoscale="per_lp", flags=flags)
        lp2 = type(lp)(lp.A, b, c, 0.0)
        lp2.init(s)
        lp2.solve(s)
        assert s.launch_info()["full_shape"] is (flags == 0)
        got.append(s)
    assert (got[0].status == 0).all()
    for name in BITWISE:
        np.testing.assert_array_equal(getattr(got[0], name), getattr(got[1], name), err_msg=name)


def test_flag_is_a_no_op_on_a_shape_that_is_not_filled():
    """25 x 30 on (32, 64): the generic instantiation with and without the flag."""
    plain, flagged = solved((25, 30)), solved((25, 30), flags=GENERIC)
    assert plain.launch_info()["full_shape"] is False and flagged.launch_info()["full_shape"] is False
    for name in BITWISE:
        np.testing.assert_array_equal(getattr(plain, name), getattr(flagged, name), err_msg=name)
