"""Non-finite data (helpers, no tests): one LP of a batch carries a NaN or an Inf -- what becomes of it, and of the others.

Every solve kernel ends an LP whose arithmetic stops being finite with PYCLLP_STATUS_NUMERICAL, and the
oracle (oracle/ipm_dense_ref.c) and tests/bounded_twin.py restate those guards.  A ROW is one (kernel family, kind) at the
family's smallest point of tests/trajectory.py (its cold rows: ``key``, ``where``, ``flags``, ``solver_options``), or one of the
three per-problem entries that have no trajectory row, at a point of their own test files.  ``Setup(row, B)`` generates the
healthy batch with the row's own generator at B LPs and holds the arrays as the entry takes them; ``poisoned`` writes the POISONS
into copies, one per poisoned LP; ``reference`` runs the oracle / the twin on chosen LPs of such a batch; ``Gpu`` launches the
entry on sentinel-filled outputs with four compute units resident, so that every slot takes several LPs in turn; ``check`` holds
the kernel's results against its clean run of the same batch (bit for bit, every healthy LP) and against the reference.

Placement (``placement``).  The lane-group kernels hand out slots group-major: with W = grid x waves per workgroup, LP i and
LP i + W start in one wavefront.  LP p < W and LP W + q (q != p) are poisoned, so LP W + p and LP q each run beside a poisoned
LP from the first instruction on; further poisoned LPs enter used slots (index >= slots), and the last LP of the batch is one.
The other kernels: LP 1, LP slots + 1 (first refill), the last LP, and further ones in between.  A poisoned LP ends at iteration
0, so the next occupant of its slot is a healthy LP, and every healthy LP is compared.

Mid-run exits (``MIDRUN``).  The cases above stop at iteration 0.  An LP that goes non-finite LATER was searched for with the
references alone: finite data, b of one LP times 10^k (k = 80 .. 150, no autoscale), kept where the reference ends with status
3 at iters >= 2 and keeps status and iters under the NPERM seeded permutations of ``trajectory.run_reference``.  See ``MIDRUN``
for what the search found per kind."""
import collections
import os

import numpy as np
import scipy.sparse as sp

import bounded_twin
import dense_batch_cases as dbc
import footprint as fp
import general_batch_cases as gbc
import sparse_general_batch_cases as sgbc
import test_kernel_variants as tkv
import test_workgroup_kernel_plans as twp
import trajectory as tj
from conftest import rel_err
from pycllp_amd.lp import EqualityLP

NAN, INF = float("nan"), float("inf")
WARM_FLAG, AUTOSCALE_FLAG = tj.WARM, tj.AUTOSCALE
SAMPLE = 64                                  # healthy LPs held against the reference, at most
RESERVE_LEAVES = 4                           # compute units a launch keeps (reserve_cus = multi_processor_count - 4)
MAX_POISONED = 8

# family, kind, the entry of include/pycllp_hip.h that solves it, the trajectory case it takes its point from (None: ``point``
# names one of the entry's own test files)
Row = collections.namedtuple("Row", "id family kind entry case point")

# the per-problem entries without a trajectory row: entry -> (family, kind, point of its own test file)
PER_PROBLEM_ENTRIES = {
    "pycllp_hip_dense_solve_batch": ("perA-dense", "plain", (20, 60, True)),            # dbc.make(m, n, slack)
    "pycllp_hip_dense_solve_batch_bounded": ("perA-dense", "bounded", (12, 16)),        # gbc.make(m', n)
    "pycllp_hip_sparse_solve_batch_bounded": ("perA-sparse", "bounded", "P2"),          # sgbc.make(point)
}


def build_rows():
    cold = [c for c in tj.CASES if c.mode == "cold"]
    rows = []

    def take(family, kinds, at):
        for kind in kinds:
            found = [c for c in cold if c.family == family and c.kind == kind and at(c)]
            assert len(found) == 1, (family, kind, [c.id for c in found])
            c = found[0]
            if kind == "bounded":
                entry = "pycllp_hip_dense_solve_bounded" if family == "slack" else "pycllp_hip_sparse_solve_bounded"
            else:
                dense = family in ("slack", "group") or (family == "big" and c.where[2] == "mfma")      # (trajectory.kernel_results)
                entry = "pycllp_hip_%s_solve%s" % ("dense" if dense else "sparse", "_batch" if kind.startswith("pa") else "")
            rows.append(Row(c.id, family, kind, entry, c, c.point))

    take("slack", ("plain", "hsd", "pc"), lambda c: c.point == "16x32")
    take("slack", ("guard",), lambda c: c.point == "32x64")
    take("slack", ("bounded",), lambda c: c.point == "24x30")
    take("group", ("plain", "hsd", "pc"), lambda c: c.point == "17x33")
    take("tables", ("plain", "hsd", "pc", "pa", "pa-hsd", "pa-pc", "bounded"), lambda c: c.key[0] == "variants")   # ragged (3, 4)
    take("image", ("plain", "hsd", "pc"), lambda c: c.point == "40x100")
    take("image", ("bounded",), lambda c: True)
    take("block", ("plain", "hsd", "pa", "pa-hsd"), lambda c: c.point.startswith("lds-paired"))
    take("block", ("plain",), lambda c: c.point.startswith("l2"))
    for gram in twp.GRAMS:                   # the smallest point per Gram path with the factor in LDS
        take("big", ("plain", "hsd", "pc"), lambda c: c.where[2] == gram and c.where[1][0] == "L")
    for entry, (family, kind, point) in PER_PROBLEM_ENTRIES.items():
        rows.append(Row("%s-%s" % (family, kind), family, kind, entry, None, point))
    return rows


ROWS = build_rows()
BY_ID = {r.id: r for r in ROWS}
assert len(BY_ID) == len(ROWS)
# a start point with a NaN in x and an Inf in z (PYCLLP_FLAG_WARM_START): rows of their own on these two
WARM_ROWS = ("slack-16x32-plain", "tables-33x193-plain")

# Mid-run exits: row id -> (index of the LP in the row's batch at MIDRUN_B LPs, factor on its b).  Found with the references alone
# (module docstring): under PREDCORR the oracle ends such an LP with status 3 after 15 .. 30 iterations (b x 1e80 and larger:
# the growth test's status 2 below that), with the same iteration count for every factor from 1e80 to 1e150 and under all NPERM
# permutations -- one case on the lane-group kernel, one on the wave kernel.  No case exists for the other kinds and they are left
# out: with plain and hsd the oracle, and with bounded the twin, end such LPs with status 2, 4 or 5 and never with 3 (b, c, u or
# both times 1e20 .. 1e150; from 1e160 on |c|^2 overflows and they stop at iteration 0, which the rows above cover).
MIDRUN_B = 8
MIDRUN = {"slack-16x32-pc": (2, 1e100), "tables-33x193-pc": (1, 1e100)}


# ---- the healthy batch ------------------------------------------------------------------------------------------------------
def _regenerated(mod, case, B):
    """``mod.make_case(case)`` at B LPs: the generator of tests/test_kernel_variants.py or test_workgroup_kernel_plans.py
    draws ``mod.batch(...)`` LPs and keeps them in ``mod._CACHE``; both are set aside for this one call."""
    saved = mod.batch, mod._CACHE
    mod.batch, mod._CACHE = (lambda *a: B), {}
    try:
        return mod.make_case(case)
    finally:
        mod.batch, mod._CACHE = saved


def healthy_lp(row, B):
    """The row's batch at B LPs: an EqualityLP, or a GeneralLP (bounded kinds)."""
    if row.case is None:
        if row.entry == "pycllp_hip_dense_solve_batch":
            return dbc.make(*row.point, B=B)
        if row.entry == "pycllp_hip_dense_solve_batch_bounded":
            return gbc.make(*row.point, B=B)
        return sgbc.make(row.point, B=B)
    key = row.case.key
    if key[0] == "variants":
        return _regenerated(tkv, key[1], B)
    if key[0] == "plans":
        return _regenerated(twp, key[1], B)
    assert key[0] in ("standard", "equality", "bounded-dense", "bounded-image") and key[3] in (tj.B, tj.B_BIG), key
    return tj.inputs(key[:3] + (B,) + key[4:])


def csr_order(A):
    """(perm, indptr, indices): the CSR order of a SparseMatrix's structure, as the plugins hand per-problem values over."""
    rows, cols = np.asarray(A._rows), np.asarray(A._cols)
    perm = np.lexsort((cols, rows))
    counts = np.zeros(A.nrows + 1, dtype=np.int64)
    np.add.at(counts, rows + 1, 1)
    return perm, np.cumsum(counts).astype(np.int32), cols[perm].astype(np.int32)


class Setup(object):
    """The healthy batch of ``row`` at B LPs as its entry takes it: ``arrays`` = dict(b [B, m], c [B, N][, u [B, N]][, A: the
    per-problem array]) in the (bounded) equality form's variables, ``tail`` (the last m columns are the identity), and the
    dense matrix of LP k (``matrix``) for the references."""

    def __init__(self, row, B):
        self.row, self.B = row, B
        self.bounded = row.kind == "bounded"
        self.lp = lp = healthy_lp(row, B)
        assert lp.nproblems == B, (row.id, lp.nproblems, B)
        if self.bounded:
            self.blp, self.bmap = lp.to_bounded_equality_form()
            form = self.blp
            self.arrays = dict(b=form.b.copy(), c=form.c.copy(), u=form.u.copy())
        else:
            form = lp
            self.arrays = dict(b=np.array(lp.b), c=np.array(lp.c))
        self.form = form
        self.m, self.N = int(form.nrows), int(form.ncols)
        self.shared = form.A.nproblems == 1
        self.A0 = np.asarray(form.A.todense(0) if not self.shared else form.A.todense(), dtype=np.float64).reshape(self.m, self.N)
        self.tail = self.N > self.m and np.array_equal(self.A0[:, self.N - self.m:], np.eye(self.m))
        self.layout = None
        if not self.shared:
            if row.entry in ("pycllp_hip_dense_solve_batch", "pycllp_hip_dense_solve_batch_bounded"):
                # dense [B, m, a_cols]: the identity tail is implied
                assert self.tail
                self.layout, self.a_cols = "dense", self.N - self.m
                self.arrays["A"] = dbc.matrices(form)[:, :, :self.a_cols].copy()
            else:
                self.layout = "csr"
                self.perm, self.indptr, self.indices = csr_order(form.A)
                self.arrays["A"] = np.ascontiguousarray(np.asarray(form.A.data, dtype=np.float64)[:, self.perm])

    def matrix(self, arrays, k):
        if self.shared:
            return self.A0
        if self.layout == "dense":
            return np.hstack([arrays["A"][k], np.eye(self.m)])
        return sp.csr_matrix((arrays["A"][k], self.indices, self.indptr), shape=(self.m, self.N)).toarray()

    def structural(self):
        return self.N - self.m if self.tail else self.N


# ---- the poisons ------------------------------------------------------------------------------------------------------------
def poisons(setup):
    """[(name, array, where, value)]: ``where`` 'last' / 'first' (a row of b), 'structural' / 'slack' (a column of c that takes
    part: u > 0 in a bounded LP), 'value' (a stored value of the LP's own matrix)."""
    out = [("NaN in the last row of b", "b", "last", NAN), ("+Inf in b", "b", "first", INF),
           ("NaN in c of a structural column", "c", "structural", NAN)]
    if setup.tail:
        out.append(("NaN in c of a slack column", "c", "slack", NAN))
    out.append(("-Inf in c", "c", "structural", -INF))
    if not setup.shared:
        out.append(("NaN in a value of A", "A", "value", NAN))
    return out


def _column(setup, arrays, k, where):
    nd = setup.structural()
    cols = range(nd - 1, -1, -1) if where == "structural" else range(setup.N - 1, nd - 1, -1)
    for j in cols:
        if not setup.bounded or arrays["u"][k, j] > 0:
            return j
    raise AssertionError("LP %d of %s has no %s column that takes part" % (k, setup.row.id, where))


def poisoned(setup, indices):
    """(arrays with the POISONS written into copies -- poison i into LP indices[i] --, [(LP, what)])."""
    arrays = {q: v.copy() for q, v in setup.arrays.items()}
    what = []
    todo = poisons(setup)
    assert len(indices) >= len(todo) and len(todo) <= MAX_POISONED, (setup.row.id, indices)
    for k, (name, array, where, value) in zip(indices, todo):
        if array == "b":
            arrays["b"][k, setup.m - 1 if where == "last" else 0] = value
        elif array == "c":
            arrays["c"][k, _column(setup, arrays, k, where)] = value
        elif setup.layout == "dense":
            arrays["A"][k, setup.m - 1, setup.a_cols - 1] = value
        else:
            arrays["A"][k, arrays["A"].shape[1] // 2] = value
        what.append((int(k), name))
    return arrays, what


def poisoned_start(setup, indices):
    """(x0, y0, z0) of ``trajectory.warm_point`` with a NaN in x of LP indices[0] and an Inf in z of LP indices[1]."""
    x0, y0, z0 = tj.warm_point(setup.B, setup.m, setup.N)
    x0[indices[0], 0] = NAN
    z0[indices[1], setup.N - 1] = INF
    return (x0, y0, z0), [(int(indices[0]), "NaN in x0"), (int(indices[1]), "Inf in z0")]


# ---- placement --------------------------------------------------------------------------------------------------------------
def slots_of(info):
    """(slots, W): LPs in flight of the launch ``info`` describes; W = wavefronts of a lane-group launch, else None."""
    waves = info["grid"] * (info["block"] // 64)
    if "group_shape" in info:
        return waves * (64 // info["group_shape"][0]), waves
    if info.get("kernel") == "wave":
        return waves, None
    return info["grid"], None


def placement(info, B, n):
    """(the n LPs to poison, the healthy wave neighbours among the others) for a launch of B >= 3 slots LPs."""
    slots, W = slots_of(info)
    assert B >= 3 * slots and slots >= 2, (B, slots, info)
    if W is not None:
        assert 3 <= W and 2 * W <= slots, info
        p, q = 1, 2
        idx = [p, W + q, slots + 1, B - 1, slots + W + 3, 2 * slots + 5, 2 * slots + W, 5 % W + 3]
        near = [W + p, q]
    else:
        idx = [1, slots + 1, B - 1, 2 * slots + 1, slots + 3, 2 * slots, 3, slots + 4]
        near = [0, 2] if slots > 2 else [0]          # (by index only: these kernels share no wavefront)
    idx = idx[:n]
    assert len(set(idx)) == n and max(idx) < B and not set(idx) & set(near), (idx, near, B, slots)
    return idx, near


def sample_of(B, poisoned_idx, near, info, limit=SAMPLE):
    """At most ``limit`` healthy LPs for the reference: the wave neighbours, the LP after each poisoned one, the tail of the
    batch, and seeded others."""
    slots, _ = slots_of(info)
    bad = set(poisoned_idx)
    first = list(near) + [k + 1 for k in poisoned_idx if k + 1 < B] + list(range(B - 8, B)) + [slots, slots + 2]
    rest = list(np.random.RandomState(5).permutation(B))
    out = []
    for k in first + rest:
        k = int(k)
        if 0 <= k < B and k not in bad and k not in out:
            out.append(k)
        if len(out) == limit:
            break
    return sorted(out)


# ---- the references ---------------------------------------------------------------------------------------------------------
def oracle_flags(row):
    return tj.ORACLE_FLAGS.get(row.kind, 0)


def reference(setup, arrays, idx, autoscale=False, start=None, **opts):
    """The reference's results (x, y, z[, s], pobj, dobj, status, iters) for the LPs ``idx`` of the batch ``arrays``."""
    from oracle import port
    idx = np.asarray(idx, dtype=int)
    b, c = arrays["b"][idx], arrays["c"][idx]
    if setup.bounded:
        u = arrays["u"][idx]
        with np.errstate(all="ignore"):
            if setup.shared:
                return bounded_twin.solve(setup.A0, b, c, u, autoscale=autoscale, **opts)
            each = [bounded_twin.solve(setup.matrix(arrays, k), b[i:i + 1], c[i:i + 1], u[i:i + 1], autoscale=autoscale, **opts)
                    for i, k in enumerate(idx)]
            return {q: np.concatenate([e[q] for e in each]) for q in gbc.OUTPUTS}
    flags = oracle_flags(setup.row) | (AUTOSCALE_FLAG if autoscale else 0) | (WARM_FLAG if start is not None else 0)
    st = {} if start is None else dict(x0=start[0][idx], y0=start[1][idx], z0=start[2][idx])
    if setup.shared:
        return port.dense_solve(setup.A0, b, c, nthreads=8, flags=flags, **st, **opts)
    each = [port.dense_solve(setup.matrix(arrays, k), b[i:i + 1], c[i:i + 1], flags=flags,
                             **{q: v[i:i + 1] for q, v in st.items()}, **opts) for i, k in enumerate(idx)]
    return {q: np.concatenate([e[q] for e in each]) for q in each[0]}


def outputs_of(setup):
    return fp.BOUNDED_OUT if setup.bounded else fp.SOLVE_OUT


# ---- the assertions ---------------------------------------------------------------------------------------------------------
def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.int64) if a.dtype == np.float64 else a


def unwritten(a):
    return bits(a) == (fp._SENT64_I if a.dtype == np.float64 else fp.SENT32)


def check(names, got, clean, ref, ref_idx, bad_idx):
    """``got`` / ``clean``: the kernel's results of the poisoned / the clean batch (every LP); ``ref``: the reference's results of
    the LPs ``ref_idx`` of the poisoned batch (the poisoned LPs ``bad_idx`` among them).  Returns the number of healthy LPs,
    all of which carry the bits of the clean run."""
    B = got["status"].shape[0]
    ref_idx, bad_idx = [int(k) for k in ref_idx], [int(k) for k in bad_idx]
    at = {k: i for i, k in enumerate(ref_idx)}
    assert set(bad_idx) <= set(at)
    # every output of every LP is written
    for q in names:
        miss = unwritten(got[q])
        assert not miss.any(), "output %r not written for LP %d" % (q, int(np.argwhere(miss)[0][0]))
    # a poisoned LP
    for k in bad_idx:
        i = at[k]
        assert ref["status"][i] == 3, "the reference ends poisoned LP %d with status %d" % (k, ref["status"][i])
        assert got["status"][k] == ref["status"][i], "poisoned LP %d: status %d, the reference's %d (iters %d / %d)" % (
            k, got["status"][k], ref["status"][i], got["iters"][k], ref["iters"][i])
        assert abs(int(got["iters"][k]) - int(ref["iters"][i])) <= 1, "poisoned LP %d: iters %d, the reference's %d" % (
            k, got["iters"][k], ref["iters"][i])
        for q in ("x", "y", "z"):
            fin = np.isfinite(ref[q][i])
            np.testing.assert_allclose(got[q][k][fin], ref[q][i][fin], rtol=1e-5, atol=1e-6,
                                       err_msg="poisoned LP %d: %s where the reference's is finite" % (k, q))
    # a healthy LP: the bits of the clean run, every output, every LP
    healthy = np.setdiff1d(np.arange(B), bad_idx)
    for q in names:
        same = bits(got[q])[healthy] == bits(clean[q])[healthy]
        same = same if same.ndim == 1 else same.all(axis=1)
        assert same.all(), "healthy LP %d: %s differs from the clean run of the same batch" % (int(healthy[np.argmin(same)]), q)
    # ... and the reference's verdict on the sample
    hs = [k for k in ref_idx if k not in bad_idx]
    gi, ri = np.asarray(hs, dtype=int), np.asarray([at[k] for k in hs], dtype=int)
    assert np.array_equal(got["status"][gi], ref["status"][ri]), (got["status"][gi], ref["status"][ri])
    assert np.abs(got["iters"][gi].astype(int) - ref["iters"][ri]).max() <= 1, (got["iters"][gi], ref["iters"][ri])
    for q in ("pobj", "dobj"):
        e = rel_err(got[q][gi], ref[q][ri])
        assert e.max() <= 1e-9, "healthy LP %d: %s off by %.2e against the reference" % (hs[int(e.argmax())], q, e.max())
    return int(healthy.size)


def midrun_lp(rid):
    """(the row's batch at MIDRUN_B LPs, index of the mid-run LP in it, factor on its b)."""
    k, factor = MIDRUN[rid]
    return Setup(BY_ID[rid], MIDRUN_B), k, factor


def _midrun_input(key):
    setup, k, factor = midrun_lp(key[1])
    return EqualityLP(setup.form.A, setup.arrays["b"][k:k + 1] * factor, setup.arrays["c"][k:k + 1].copy(), 0.0)


tj.MORE_INPUTS["nonfinite-midrun"] = _midrun_input


def midrun_case(rid):
    """The mid-run LP of row ``rid`` as a case ``trajectory.run_reference`` takes (its permutations included)."""
    c = BY_ID[rid].case
    return tj.register(tj.Case(rid + "-midrun", c.family, c.kind, c.point, "cold", (200,), ("nonfinite-midrun", rid), c.where,
                               c.flags, None, ""))


def served_text(info):
    if "group_shape" in info:
        return "lane groups %dx%d%s" % (info["group_shape"] + (" slack" if info.get("slack") else "",))
    if info.get("kernel") == "wave":
        return "wave %s %dx%d" % ((info["variant"],) + info["wave_shape"])
    if info.get("kernel") == "big":
        return "big %s %dx%d factor in %s" % ((info["variant"],) + info["big_shape"] + ("LDS" if info["factor_in_lds"] else "L2",))
    return "block, A in %s" % ("LDS" if info.get("a_in_lds") else "L2")


def record(line):
    path = os.environ.get("PYCLLP_NONFINITE_RECORD")
    if path:
        with open(path, "a") as f:
            f.write(line + "\n")


# ---- the GPU ----------------------------------------------------------------------------------------------------------------
def reserve():
    import torch
    return max(torch.cuda.get_device_properties(0).multi_processor_count - RESERVE_LEAVES, 0)


def assert_served(row, info, setup):
    """``trajectory.assert_served`` for a launch through the entry itself: the compiled shape (lane groups, wave kernel) or
    the plan (block and large-LP kernel; their grid follows the resident compute units here, not the batch).  The per-problem
    entries: the kernel of their own test files."""
    if row.case is None:
        if row.family == "perA-dense":
            want = (dbc.first_covering(setup.m, setup.N, True) if not setup.bounded else
                    gbc.first_covering(setup.m, setup.N - setup.m))
            assert info.get("group_shape") == want and info.get("slack") == 1, info
        else:
            assert (info.get("variant"), info.get("kernel")) == ("tables", "wave"), info
            assert info.get("wave_shape") == sgbc.POINTS[row.point][3], info
        return
    case = row.case
    if case.where is None:
        assert info.get("kernel") == "block" and "wave_shape" not in info, info
    elif case.family in ("block", "big"):
        twp.assert_served_by(info, case.where, setup.form)
    else:
        tkv.assert_served_by(info, (case.family, case.where))


class Gpu(object):
    """The row's handle (made the way its plugin makes it) and one launch of its entry on sentinel-filled outputs."""

    def __init__(self, setup):
        import torch
        from pycllp_amd.solvers import solver_registry
        from pycllp_amd.solvers.hip import Handle
        self.setup, row = setup, setup.row
        self.device = torch.device("cuda:0")
        self.flags = 0
        common = dict(device="cuda:0", reserve_cus=reserve())
        if row.case is None:
            name = {"pycllp_hip_dense_solve_batch": "hip_dense_batch_primal_normal",
                    "pycllp_hip_dense_solve_batch_bounded": "hip_general_batch_primal_normal",
                    "pycllp_hip_sparse_solve_batch_bounded": "hip_sparse_general_batch_primal_normal"}[row.entry]
            s = solver_registry[name](hsd=False, autoscale=False, **common)
            setup.lp.init(s)
            assert s._handle is not None, "the entry does not serve %s" % row.id
            if row.entry == "pycllp_hip_dense_solve_batch":
                assert s.a_cols == setup.a_cols
                self.flags = s._flags
            elif setup.layout == "csr":
                assert np.array_equal(s._perm, setup.perm)
            self.handle, self.options = s._handle, s.options
        elif setup.bounded:
            cls = solver_registry["hip_general_primal_normal" if row.family == "slack" else "hip_sparse_general_primal_normal"]
            assert cls.native_fits(setup.lp, setup.blp)
            self.handle = Handle(cls._bounded_matrix(setup.blp.A)[0], self.device, None)
            self.options = dict(reserve_cus=reserve())
        else:
            name = "hip_dense_primal_normal" if row.entry.startswith("pycllp_hip_dense") else "hip_sparse_primal_normal"
            s = solver_registry[name](**dict(tj.solver_options(row.case), **common))
            setup.lp.init(s)
            if not setup.shared:
                assert np.array_equal(s._a_perm, setup.perm)
            self.handle, self.options = s._handle, s.options
        self._keep = None

    def launch(self, arrays, autoscale=False, start=None, **overrides):
        """(results as numpy, launch_info) of one launch on ``arrays``; ``start``: (x0, y0, z0) of a warm start."""
        import torch
        from pycllp_amd.solvers.hip import solve_opts
        setup, h, dev = self.setup, self.handle, self.device
        B, m, N = setup.B, setup.m, setup.N
        shapes = dict(x=(B, N), y=(B, m), z=(B, N), s=(B, N), pobj=(B,), dobj=(B,), status=(B,), iters=(B,))
        out = {}
        for q in outputs_of(setup):
            if q in fp.I32_ARRAYS:
                out[q] = torch.full(shapes[q], fp.SENT32, dtype=torch.int32, device=dev)
            else:
                out[q] = torch.full(shapes[q], fp._SENT64_I, dtype=torch.int64, device=dev).view(torch.float64)
        if start is not None:
            for q, v in zip(("x", "y", "z"), start):
                out[q].copy_(torch.as_tensor(v, device=dev))
        t = {q: torch.as_tensor(np.ascontiguousarray(v), device=dev) for q, v in arrays.items()}
        o = solve_opts(self.options, self.flags | (AUTOSCALE_FLAG if autoscale else 0) | (WARM_FLAG if start is not None else 0),
                       **overrides)
        entry = setup.row.entry
        if entry == "pycllp_hip_dense_solve_batch":
            h.solve_batch_dense(None, t["A"], t["b"], t["c"], out, o)
        elif entry == "pycllp_hip_dense_solve_batch_bounded":
            h.solve_batch_bounded(None, t["A"], t["b"], t["c"], t["u"], out, o)
        elif setup.bounded:
            h.solve_bounded(None, t["b"], t["c"], t["u"], out, o, values=t.get("A"))
        else:
            h.solve(None, t["b"], t["c"], out, o, t.get("A"))
        torch.cuda.synchronize()
        self._keep = t
        return {q: v.cpu().numpy() for q, v in out.items()}, h.launch_info()


def sized(row, guess):
    """(setup, gpu, clean results, info) at the smallest B >= 3 slots found from ``guess`` on: the launch plan follows B, so the
    clean run is launched, its slots read, and B grown until every slot is refilled at least twice."""
    B = guess
    for _ in range(4):
        setup = Setup(row, B)
        gpu = Gpu(setup)
        clean, info = gpu.launch(setup.arrays)
        slots, _ = slots_of(info)
        if B >= 3 * slots:
            return setup, gpu, clean, info
        B = 3 * slots + 5
    raise AssertionError("%s: no B >= 3 slots (%d LPs, %d slots)" % (row.id, B, slots))


def first_guess(row):
    """B for four resident compute units by the launch rules (ipm_dense.hip plan_group with host.h small_batch_wpb: eight waves per workgroup, 64 / MP
    lane groups per wave; the wave kernel: four waves per workgroup and up to two workgroups per compute unit; block and
    large-LP kernel: up to four workgroups per compute unit); ``sized`` corrects it from ``launch_info()``."""
    if row.family in ("slack", "group", "perA-dense"):
        return 3 * RESERVE_LEAVES * 8 * 4 + 5
    return 3 * RESERVE_LEAVES * 4 + 5
