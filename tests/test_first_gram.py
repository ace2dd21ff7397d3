"""The Gram matrix of an LP's first iteration, formed once per handle (csrc/ipm_dense.hip first_gram_kernel, read by
csrc/ipm_group.inc GWave::gram_first): without warm start every LP starts at x = z = 1, so the matrix and A x of that pass depend
on A, m and n alone, and the 32-row plain and predictor-corrector lane-group kernels of pycllp_hip_dense_solve copy them from an
image that pycllp_hip_dense_init made with the very device function they would have run.

PYCLLP_FLAG_PER_LP_FIRST_GRAM keeps the product in the kernel, which is the text it had.  Every check here is the default against
that flag, bit for bit (np.array_equal) on x, y, z, the objectives, status and iteration counts: the image holds the bits of the
product, and the A (d t) sums keep their order.

Batches: 6 000 LPs, in which slots refill from the queue (a group on its first pass next to one in mid-solve; the 16-row
kernels on half the CUs so that they do), and 1 and 3 LPs, which leave lane groups idle.  Shapes: full (32 x 64, with and without
its full-shape instantiation), padded rows and columns (29 x 57, 12 x 20), 16 rows (16 x 32), the (32, 128) shapes that keep the
plain sweep (32 x 96), and the general variant's image (32 x 96 without identity tail; 32 x 64 under PYCLLP_FLAG_NO_SLACK_PATH).
The kernels that keep the product -- the 16-row shapes, where the copy buys nothing, and two predictor-corrector kernels with
no register for the path (slack-aware (32, 96), general (32, 128)) -- run here too; for them the flag changes nothing, and
their cases pin that it stays so the day they take the image.  The batches are the cached ones of test_fused_forward.py."""
import numpy as np
import pytest
import torch

from pycllp_amd import _native
from pycllp_amd.solvers import solver_registry
from pycllp_amd.solvers.hip import autoscale_mask
from test_fused_forward import B, BITWISE, FORCE_GUARD, PC_OPTS, equality, standard

pytestmark = pytest.mark.gpu
PER_LP = _native.FLAG_PER_LP_FIRST_GRAM
GENERIC, NO_SLACK = _native.FLAG_GENERIC_SHAPE, _native.FLAG_NO_SLACK_PATH

# id, batch, flags, the kernel that serves it: (MP, NP), slack-aware, full-shape instantiation (plain step only)
SHAPES = [
    ("32x64-full-shape", (32, 64), 0, (32, 96), 1, True),
    ("32x64-generic", (32, 64), GENERIC, (32, 96), 1, False),
    ("29x57-padded", (29, 57), 0, (32, 96), 1, False),
    ("12x20-padded", (12, 20), 0, (16, 48), 1, False),
    ("16x32", (16, 32), 0, (16, 48), 1, True),
    ("32x96-plain-sweep", (32, 96), 0, (32, 128), 1, True),
    ("equality-32x96-general-image", "equality", 0, (32, 96), 0, False),
    ("32x64-no-slack-path-general-image", (32, 64), NO_SLACK, (32, 96), 0, False),
]
MODES = {"plain": {}, "predcorr": dict(predcorr=True), "autoscale": dict(autoscale=True), "autoscale-per-lp": dict(autoscale="per_lp")}


def batch(key):
    return equality() if key == "equality" else standard(*key)


def run(lp, b=None, c=None, autoscale=False, **opts):
    """One solve on a handle of its own; hsd=False: an LP that does not end optimal keeps the result of this kernel."""
    s = solver_registry["hip_dense_primal_normal"](device="cuda:0", autoscale=autoscale, hsd=False, **opts)
    if b is not None:
        lp = type(lp)(lp.A, b, c, 0.0)
    lp.init(s)
    lp.solve(s)
    return s


def assert_same_bits(got, want):
    for name in BITWISE:
        np.testing.assert_array_equal(getattr(got, name), getattr(want, name), err_msg=name)


def both(lp, b=None, c=None, flags=0, **opts):
    """The default and the per-LP product; they must agree bit for bit.  Returns the default's solver."""
    image, per_lp = run(lp, b, c, flags=flags, **opts), run(lp, b, c, flags=flags | PER_LP, **opts)
    assert_same_bits(image, per_lp)
    return image


def half_the_cus():
    return torch.cuda.get_device_properties(0).multi_processor_count // 2


@pytest.mark.parametrize("mode", sorted(MODES))
@pytest.mark.parametrize("shape", SHAPES, ids=[s[0] for s in SHAPES])
def test_image_equals_the_per_lp_product(shape, mode):
    """6 000 LPs: slots refill from the queue, so a group on its first pass shares the wave with one in mid-solve."""
    _, key, flags, group_shape, slack, full = shape
    lp, opts = batch(key), dict(MODES[mode])
    b, c = None, None
    if mode == "autoscale-per-lp":              # every other LP out of band, as in test_full_shape.py
        b, c = lp.b.copy(), lp.c.copy()
        b[::2] *= 100.0
        c[::2] *= 0.01
        mask = autoscale_mask(b, c)
        assert mask[::2].all() and not mask[1::2].any()
    if group_shape[0] == 16:
        opts["reserve_cus"] = half_the_cus()
    s = both(lp, b, c, flags=flags, **opts)
    info = s.launch_info()
    assert info["group_shape"] == group_shape and info["slack"] == slack, info
    assert info["full_shape"] is (full and mode != "predcorr"), info
    assert B > info["grid"] * (info["block"] // 64) * (64 // group_shape[0]), info          # slots refill
    assert (s.status == 0).all(), np.unique(s.status, return_counts=True)


@pytest.mark.parametrize("pc", [False, True], ids=["plain", "predcorr"])
@pytest.mark.parametrize("key", [(32, 64), (29, 57), (12, 20)], ids=["32x64", "29x57", "12x20"])
@pytest.mark.parametrize("nlp", [1, 3])
def test_small_batches_leave_groups_idle(nlp, key, pc):
    lp, opts = batch(key), dict(PC_OPTS) if pc else {}
    opts.pop("hsd", None)
    bs, cs = np.ascontiguousarray(lp.b[:nlp]), np.ascontiguousarray(lp.c[:nlp])
    s = both(lp, bs, cs, **opts)
    assert (s.status == 0).all()
    if key[0] == 12:
        opts["reserve_cus"] = half_the_cus()
    whole = run(lp, **opts)                     # an LP's result does not depend on the batch around it
    for name in BITWISE:
        np.testing.assert_array_equal(getattr(s, name), getattr(whole, name)[:nlp], err_msg=name)


@pytest.mark.parametrize("pc", [False, True], ids=["plain", "predcorr"])
@pytest.mark.parametrize("max_iter", [1, 2])
@pytest.mark.parametrize("key", [(32, 64), (12, 20)], ids=["32x64", "12x20"])
def test_lp_that_ends_on_or_right_after_the_first_pass(key, max_iter, pc):
    opts = dict(predcorr=True) if pc else {}
    if key[0] == 12:
        opts["reserve_cus"] = half_the_cus()
    s = both(batch(key), max_iter=max_iter, **opts)
    assert (s.status == _native.STATUS_ITERATION_LIMIT).all() and (s.iters == max_iter).all(), np.unique(s.status, return_counts=True)


@pytest.mark.parametrize("opts", [{}, dict(predcorr=True)], ids=["plain", "predcorr"])
@pytest.mark.parametrize("key", [(32, 64), (29, 57), (12, 20)], ids=["32x64", "29x57", "12x20"])
def test_forced_guard_path_redoes_the_first_pass_from_the_image(key, opts):
    """PYCLLP_FLAG_FORCE_GUARD_PATH forms M a second time in every pass, the first included; the result is also that of the
    unforced solve (test_fused_forward.py holds those two together)."""
    opts = dict(opts)
    if key[0] == 12:
        opts["reserve_cus"] = half_the_cus()
    forced = both(batch(key), flags=FORCE_GUARD, **opts)
    assert_same_bits(forced, run(batch(key), **opts))


def test_warm_start_takes_the_product_with_and_without_the_flag():
    """A warm start does not begin at x = z = 1: the host hands the kernel no image, and the flag changes nothing.  The cold
    solve in front of it does read the image."""
    lp = standard(32, 64)
    got = []
    for flags in (0, PER_LP):
        s = solver_registry["hip_dense_primal_normal"](device="cuda:0", autoscale=False, flags=flags)
        lp.init(s)
        s.solve_device(lp.b, lp.c, eps=1e-4)
        buf = s.solve_device(lp.b, lp.c, warm_start=True)
        torch.cuda.synchronize()
        got.append({k: buf[k].cpu().numpy().copy() for k in ("status", "iters", "pobj", "dobj", "x", "y", "z")})
    assert (got[0]["status"] == 0).any()
    for k in got[0]:
        np.testing.assert_array_equal(got[0][k], got[1][k], err_msg=k)


def test_the_image_belongs_to_the_handle():
    """Two handles with different A, alive together and solved alternately: each result is that of its own per-LP product."""
    lps = [standard(32, 64), standard(29, 57)]
    solvers = [solver_registry["hip_dense_primal_normal"](device="cuda:0", autoscale=False, hsd=False) for _ in lps]
    for lp, s in zip(lps, solvers):
        lp.init(s)
    want = [run(lp, flags=PER_LP) for lp in lps]
    for _ in range(2):
        for lp, s, w in zip(lps, solvers, want):
            lp.solve(s)
            assert_same_bits(s, w)
