"""The five bounded kernels under the numerical options (helpers, no tests): rows in the sense of tests/option_cases.py --
(case, options, base options), the kernel against the CPU twin (tests/bounded_twin.py) at the row's options, tolerances by the
rule of tests/trajectory.py recomputed under those options -- for what the paths of option_cases.py leave out:

  refinement and the pivot floor   degenerate bounded inputs (``trajectory.degenerate_bounded``: two equality rows that differ
                                   by 1e-6, so one pivot per factorisation meets the floor and refinement runs to its cap) on the
                                   three shared-A kernels and the two per-problem-A kernels: the default options, max_refine = 1,
                                   refine_tol = 1e-8 and pivot_floor = 1e-3.  (refine_tol = 1e-6 is met before the first pass on
                                   these inputs and equals max_refine = 0 to the last digit.)
  the per-problem-A kernels        delta = 0.1, r = 0.5 and the eps = 1e-4 stopping row at the smallest trajectory point of
                                   general_batch_cases.py and sparse_general_batch_cases.py
  the forced guard                 PYCLLP_FLAG_FORCE_GUARD_PATH on the two bounded lane-group kernels, on well-conditioned and
                                   degenerate inputs.  The twin's factor is the guarded one, and on these inputs its term never
                                   decides a pivot (``guard_ratio`` <= 0.9), so forced and unforced launch face the same reference.
  the per-problem dense image      delta, r and the stopping row on the wave kernel with an image per wave (not bounded; against
                                   the oracle), a compile of the wave text of its own that is no path of option_cases.py

Every LP of every row must end at the iteration limit (status 5) on both sides: on the wave kernels that is the assertion that
their NUMERICAL exit (the guard would have bitten) stays quiet where the twin's guard does not bite."""
import functools

import numpy as np

import dense_batch_wave_cases as wc
import general_batch_cases as gbc
import option_cases as oc
import sparse_general_batch_cases as sgc
import trajectory as tj

KS, KEY, Row = oc.KS, oc.KEY, oc.Row
GUARD_RATIO = 0.9                    # the largest theta^2 / (beta^2 max(|M_jj|, floor)) a degenerate input may reach

tj.MORE_INPUTS.update({"general-batch": lambda key: gbc.trajectory_lp(key[1]),
                       "sparse-general-batch": lambda key: sgc.trajectory_lp(key[1])})
tj.MORE_BOUNDED.update({"general-batch": lambda key: gbc.trajectory_lp(key[1], True),
                        "sparse-general-batch": lambda key: sgc.trajectory_lp(key[1], True)})


# ---- cases ------------------------------------------------------------------------------------------------------------------
def _degenerate(case):
    return case._replace(id=case.id + "-degenerate", mode="degenerate", ks=KS, key=("degenerate-bounded", case.key))


def _forced(case):
    return case._replace(id=case.id + "-guard", flags=case.flags | tj.GUARD)


@functools.lru_cache(maxsize=None)
def shared_cases():
    """The cold bounded cases of ``trajectory.CASES`` the degenerate inputs are made from: the lane-group point, the smaller
    of the two term-table points and the dense-image point."""
    cold = [c for c in tj.CASES if c.kind == "bounded" and c.mode == "cold"]
    return tuple(min((c for c in cold if c.family == f), key=oc._size) for f in ("slack", "tables", "image"))


@functools.lru_cache(maxsize=None)
def per_problem_cases():
    """The two per-problem-A bounded kernels at the smallest trajectory point of their own test files."""
    point = min(gbc.TRAJECTORY_POINTS, key=lambda p: gbc.TRAJECTORY_POINTS[p][0] ** 2 * sum(gbc.TRAJECTORY_POINTS[p]))
    mk, n = gbc.TRAJECTORY_POINTS[point]
    group = tj.Case("perA-group-%dx%d-bounded" % (mk, n), "perA-group", "bounded", "%dx%d" % (mk, n), "cold", tj.K,
                    ("general-batch", point), gbc.first_covering(mk, n), 0, None, "")
    point = min(sgc.TRAJECTORY_POINTS, key=lambda p: sgc.POINTS[p][0] ** 2 * sum(sgc.POINTS[p][:2]))
    mk, n, _, shape, _ = sgc.POINTS[point]
    wave = tj.Case("perA-wave-%dx%d-bounded" % (mk, n), "perA-wave", "bounded", "%dx%d" % (mk, n), "cold", tj.K,
                   ("sparse-general-batch", point), shape, 0, None, "")
    return tj.register(group), tj.register(wave)


@functools.lru_cache(maxsize=None)
def degenerate_cases():
    return tuple(tj.register(_degenerate(c)) for c in shared_cases() + per_problem_cases())


def lane_group_cases():
    """The cases of the two bounded lane-group kernels (the wave kernels have no guarded factor and refuse the flag): the
    well-conditioned inputs, then the degenerate ones."""
    return [c for c in shared_cases() + per_problem_cases() + degenerate_cases() if c.family in ("slack", "perA-group")]


# ---- rows -------------------------------------------------------------------------------------------------------------------
NO_REFINEMENT = KEY(dict(max_refine=0))
# the default options are a row too: the reference it must differ from is the one without refinement
ON_DEGENERATE = (("default", {}, NO_REFINEMENT), ("max_refine", dict(max_refine=1), KEY({})),
                 ("refine_tol", dict(refine_tol=1e-8), KEY({})), ("pivot_floor", dict(pivot_floor=1e-3), KEY({})))


@functools.lru_cache(maxsize=None)
def option_rows():
    """Refinement and the floor on the five degenerate inputs; delta and r on the two per-problem-A kernels."""
    rows = [Row("%s:%s" % (c.id, name), c, KEY(opts), base) for c in degenerate_cases() for name, opts, base in ON_DEGENERATE]
    rows += [Row("%s:%s" % (c.id, name), c, KEY(opts), KEY({})) for c in per_problem_cases() for name, opts in oc.ON_EVERY_PATH]
    assert len({r.id for r in rows}) == len(rows) and {rid for rid, _ in dropped()} <= {r.id for r in rows}
    return tuple(rows)


@functools.lru_cache(maxsize=None)
def guard_rows():
    """The forced guard at the default options: k = 1, 2, 4, 8 on the well-conditioned inputs, k = 1, 2, 4 on the degenerate ones.
    ``base`` names nothing the flag must move: the twin has one factor, the guarded one."""
    return tuple(Row("%s:guard" % c.id, tj.register(_forced(c)), KEY({}), None) for c in lane_group_cases())


def unforced(case):
    """The case a forced-guard case is the twin of: the same LPs, options and reference without the flag."""
    assert case.flags & tj.GUARD and case.id.endswith("-guard")
    return tj.BY_ID[case.id[:-len("-guard")]]


@functools.lru_cache(maxsize=None)
def dropped():
    """{(row id, k): reason}: the points at which an option does not move the twin's x by twice the tolerance (see
    option_cases.dropped)."""
    return {}


def row_ks(row):
    ks = tuple(k for k in row.case.ks if (row.id, k) not in dropped())
    if row in option_rows():
        ks = tuple(k for k in ks if k in KS)
    if len(ks) < 2:
        raise ValueError("row %s is left with fewer than two k" % row.id)
    return ks


# ---- the per-problem dense-image wave kernel: not bounded, and in no row of option_cases.py ------------
tj.MORE_INPUTS["dense-batch-wave"] = lambda key: wc.trajectory_lp()


@functools.lru_cache(maxsize=None)
def image_per_problem_case():
    m, N, tail = wc.TRAJECTORY_POINT
    assert tail
    return tj.register(tj.Case("perA-image-%dx%d-plain" % (m, N - m), "perA-image", "plain", "%dx%d" % (m, N - m), "cold", KS,
                               ("dense-batch-wave",), wc.plan(m, N, tail)[0], 0, None, ""))


@functools.lru_cache(maxsize=None)
def image_per_problem_rows():
    c = image_per_problem_case()
    return tuple(Row("%s:%s" % (c.id, name), c, KEY(opts), KEY({})) for name, opts in oc.ON_EVERY_PATH)


def image_per_problem_results(case, ks, **opts):
    """``trajectory.kernel_results`` for the per-problem dense-image wave kernel, through its plugin's device entry."""
    import torch
    from pycllp_amd.solvers import solver_registry
    from pycllp_amd.solvers.dense_batch import densify_batch
    lp, P = tj.inputs(case.key), tj.problem(case.key, False)
    s = solver_registry["hip_dense_batch_primal_normal"](device="cuda:0", hsd=False, autoscale=False)
    lp.init(s)
    A = densify_batch(lp.A._rows, lp.A._cols, lp.A.data, lp.nrows, s.a_cols)
    out = {}
    for k in ks:
        g = s.solve_device(A, lp.b, lp.c, max_iter=k, **opts)
        torch.cuda.synchronize()
        info = s.launch_info()
        assert s.kernel == "wave per-problem", s.kernel
        assert info.get("kernel") == "wave" and info.get("variant") == "dense image" and info.get("wave_shape") == case.where, info
        out[k] = {q: g[q].cpu().numpy() for q in ("x", "y", "z", "pobj", "dobj", "status", "iters")}
        out[k]["aty"] = tj.a_transpose_y(P, out[k]["y"])
    return out


# ---- the GPU side -----------------------------------------------------------------------------------------------------------
def same_bits(a, b, ks, quantities):
    return all(np.array_equal(a[k][q], b[k][q]) for k in ks for q in quantities)
