"""Helpers of tests/test_general_device.py and tests/test_general_batch_device.py (no tests): what the tests of the device
conversion with a shared A and with per-problem values of A have in common -- read-only batches, bit equality, the bound on
f^, the stand-in for a bounded solve's outputs and the fake pointer of the argument-check tests."""
import ctypes

import numpy as np
import torch

KINDS5 = ["le", "eq", "rng", "ge", "free"]            # every kind of row: '+' rows, a '-' row, a dropped row
RESULTS = ("x", "y", "z", "s", "status", "iters", "primal_obj", "dual_obj")
DEV = "cuda:0"
P = ctypes.c_void_p(8)         # a fake non-NULL device pointer: every check comes before any HIP call


def frozen(glp):
    for v in (glp.a, glp.b, glp.c, glp.l, glp.u, glp.f, glp.A.data):
        v.setflags(write=False)
    return glp


def bits(v):
    return np.ascontiguousarray(v, dtype=np.float64).view(np.int64)


def same_bits(got, want, what):
    assert got.shape == want.shape and np.array_equal(bits(got), bits(want)), what


def dev(v):
    return None if v is None else torch.as_tensor(np.ascontiguousarray(v), device=DEV)


def fh_bound(glp):
    """2 (n + 1) 2^-53 sum |c_j l_j|: the rounding bound of a dot product of n terms, for two orders of summation."""
    return 2 * (glp.ncols + 1) * 2.0 ** -53 * np.abs(glp.c * glp.l).sum(axis=1)


def fake_solution(blp, seed):
    """Arrays with the shapes of a bounded solve's outputs (the back-conversion does no arithmetic that needs a real one)."""
    rng = np.random.default_rng(seed)
    B, mk, N = blp.nproblems, blp.nrows, blp.ncols
    r = dict(x=rng.uniform(0, 2, (B, N)), y=rng.uniform(-1, 1, (B, mk)), z=rng.uniform(0, 1, (B, N)), s=rng.uniform(0, 1, (B, N)),
             pobj=rng.uniform(-5, 5, B), dobj=rng.uniform(-5, 5, B), status=rng.integers(0, 6, B).astype(np.int32),
             iters=rng.integers(1, 200, B).astype(np.int32))
    r["x"][:, ::3] = 0.0
    r["y"][:, ::2] *= 0.0                                           # signed zeros among them
    return r


def assert_same_results(got, want, keys):
    for k in keys:
        g, w = np.asarray(got[k]), np.asarray(want[k])
        if g.dtype == np.float64:
            same_bits(g, w, k)
        else:
            assert np.array_equal(g, w), k
