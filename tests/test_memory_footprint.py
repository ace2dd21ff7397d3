"""Where every solve entry writes (tests/footprint.py): guard bands around every array, inputs unchanged, optional outputs as NULL,
two alignments, at B = 3 (most slots of the only wave or workgroup stay parked) and at a B that makes every slot of one compute
unit take several LPs in turn.

CPU: the arena's own checks bite on five bad fake entries, and the case table covers every store site and every entry.
GPU: per store site and kind one ragged point (test_kernel_variants.ragged_point and its NEAREST exceptions), each first asserting
from ``launch_info()`` which kernel served it; the reference call is held against the CPU reference of the family's own test at
that test's tolerances, every arena call against the reference call bit for bit.

PYCLLP_FOOTPRINT_RECORD=<file>: every GPU case appends the kernel that served it, B, the slots and the outcome (the record under
profiles/memory_footprint/ was written this way)."""
import os
import types

import numpy as np
import pytest
import scipy.sparse as sp
import torch

import footprint as fp
import test_kernel_variants as tkv
from conftest import rel_err
from pycllp_amd.lp import EqualityLP, SparseMatrix

F64, I32 = fp.F64, fp.I32
FLAG_FORCE_GUARD, FLAG_AUTOSCALE, FLAG_NO_SLACK, FLAG_HSD, FLAG_BLOCK, FLAG_PC = 4, 8, 16, 32, 64, 128
E_BADARG = -1


# ---- CPU: the helper bites --------------------------------------------------------------------------------------------------
def fake_specs(B=3, m=2, n=5):
    rs = np.random.RandomState(0)
    return [fp.inp("b", rs.rand(B, m)), fp.inp("c", rs.rand(B, n)), fp.out("x", (B, n)), fp.out("y", (B, m)), fp.out("z", (B, n)),
            fp.out("pobj", (B,)), fp.out("dobj", (B,)), fp.out("status", (B,), I32), fp.out("iters", (B,), I32)]


def fake_good(a):
    """A well-behaved entry on CPU tensors: writes every output it was given, reads the inputs."""
    s = float(a["b"].sum() + a["c"].sum())
    for k in fp.SOLVE_OUT:
        if a[k] is not None:
            a[k].fill_(0 if k in fp.I32_ARRAYS else s)


def beyond(t, k):
    """The element k places past the end of t (k < 0: before its start) in t's storage."""
    off = t.storage_offset() + (t.numel() - 1 + k if k > 0 else k)
    return t.as_strided((1,), (1,), off)


def fake_past_x(a):
    fake_good(a)
    beyond(a["x"], 1).fill_(1.0)


def fake_before_y(a):
    fake_good(a)
    beyond(a["y"], -1).fill_(1.0)


def fake_hole_in_z(a):
    z = a["z"].clone()
    fake_good(a)
    a["z"][1, 3] = z[1, 3]


def fake_scales_b(a):
    fake_good(a)
    a["b"].mul_(2.0)


def fake_writes_null_iters(arena):
    def entry(a):
        fake_good(a)
        arena.views["iters"].fill_(7)
    return entry


@pytest.mark.parametrize("placement", ["aligned", "natural"])
def test_arena_layout(placement):
    ar = fp.Arena(fake_specs(), placement)
    base, end = ar.buf.data_ptr(), 0
    for s in ar.specs:
        addr = base + ar.offset[s.name]
        if placement == "aligned":
            assert addr % 256 == 0
        else:
            assert addr % 16 == 8 if s.dtype == F64 else addr % 8 == 4
        assert ar.offset[s.name] - end >= fp.GUARD, s.name
        end = ar.offset[s.name] + s.nbytes
        assert ar.views[s.name].data_ptr() == addr and tuple(ar.views[s.name].shape) == s.shape
    assert ar.buf.numel() - end >= fp.GUARD
    assert fp.GUARD >= 1280 * 8          # one padded row of the widest kernel
    x = np.array([fp.SENT64], dtype=np.uint64).view(np.float64)[0]
    assert np.isnan(x) and (fp.SENT64 >> 51) & 1 and not 0 <= fp.SENT32 <= 1 << 20
    assert ar.result("x").view(np.uint64).tolist() == [[fp.SENT64] * 5] * 3 and (ar.result("iters") == fp.SENT32).all()


@pytest.mark.parametrize("placement", ["aligned", "natural"])
def test_well_behaved_fake_passes(placement):
    for null in ((), ("iters",), ("y", "z", "pobj", "dobj", "iters")):
        ar = fp.Arena(fake_specs(), placement, null=null)
        assert [k for k, v in ar.arrays().items() if v is None] == [k for k in fp.SOLVE_OUT if k in null]
        fake_good(ar.arrays())
        ar.check()
        assert sorted(ar.results()) == sorted(set(fp.SOLVE_OUT) - set(null))
    ar = fp.Arena(fake_specs(), placement)
    ar.check(outputs_written=False)         # a refused call: nothing written
    pl = fp.Plain(fake_specs())
    fake_good(pl.arrays())
    pl.check()


@pytest.mark.parametrize("placement", ["aligned", "natural"])
@pytest.mark.parametrize("fake,message", [
    (fake_past_x, r"guard band of 'x' overwritten at element 15 "),
    (fake_before_y, r"guard band of 'y' overwritten at element -1 "),
    (fake_hole_in_z, r"output 'z' not written at element 8 "),
    (fake_scales_b, r"input 'b' changed at element 0 "),
    ("null iters", r"output 'iters' passed as NULL was written at element 0 "),
], ids=["past-x", "before-y", "hole-in-z", "scales-b", "writes-null-iters"])
def test_bad_fakes_are_caught(fake, message, placement):
    ar = fp.Arena(fake_specs(), placement, null=("iters",) if fake == "null iters" else ())
    (fake_writes_null_iters(ar) if fake == "null iters" else fake)(ar.arrays())
    with pytest.raises(AssertionError, match=message):
        ar.check()
    if fake != "null iters":                 # a refused call that wrote after all is caught too
        ar = fp.Arena(fake_specs(), placement)
        fake_good(ar.arrays())
        with pytest.raises(AssertionError, match="of a refused call was written"):
            ar.check(outputs_written=False)


# ---- problems as raw arrays -------------------------------------------------------------------------------------------------
class Raw(object):
    """B LPs in the arrays the entries take.  ``A``: the shared [m, N] matrix, or None with per-problem values ``data [B, nnz]``
    on the coordinate structure ``rows, cols``; ``u``: upper bounds of a bounded form or None."""

    def __init__(self, m, N, b, c, A=None, rows=None, cols=None, data=None, u=None):
        self.m, self.N, self.A, self.rows, self.cols, self.data, self.b, self.c, self.u = m, N, A, rows, cols, data, b, c, u
        self.B = int(b.shape[0])

    def take(self, B):
        """B LPs: these in turn, from the second round on with b (and u) and c each scaled by a factor of their own in
        [0.9, 1) -- feasible and bounded as they are."""
        idx = np.arange(B) % self.B
        rs = np.random.RandomState(5)
        tb = np.where(np.arange(B) < self.B, 1.0, 0.9 + 0.1 * rs.rand(B))[:, None]
        tc = np.where(np.arange(B) < self.B, 1.0, 0.9 + 0.1 * rs.rand(B))[:, None]
        return Raw(self.m, self.N, self.b[idx] * tb, self.c[idx] * tc, self.A, self.rows, self.cols,
                   None if self.data is None else self.data[idx], None if self.u is None else self.u[idx] * tb)

    def dense(self, k):
        if self.A is not None:
            return self.A
        out = np.zeros((self.m, self.N))
        np.add.at(out, (self.rows, self.cols), self.data[k])
        return out

    def lp(self):
        if self.A is not None:
            return EqualityLP(SparseMatrix(matrix=self.A), self.b, self.c, 0.0)
        A = SparseMatrix(self.rows.copy(), self.cols.copy(), self.data)
        A._shape = (self.m, self.N)
        return EqualityLP(A, self.b, self.c, 0.0)

    def csr(self):
        """(scipy CSR of the structure with LP 0's values, the permutation of ``data``'s columns into its order)"""
        if self.A is not None:
            A = sp.csr_matrix(self.A)
            A.sum_duplicates(); A.eliminate_zeros(); A.sort_indices()
            return A, None
        perm = np.lexsort((self.cols, self.rows))
        ptr = np.zeros(self.m + 1, dtype=np.int64)
        np.add.at(ptr, self.rows + 1, 1)
        return sp.csr_matrix((self.data[0][perm], self.cols[perm], np.cumsum(ptr)), shape=(self.m, self.N)), perm


def raw_of(lp):
    """An EqualityLP or BoundedEqualityLP as ``Raw``."""
    u = getattr(lp, "u", None)
    if lp.A.nproblems > 1:
        return Raw(lp.nrows, lp.ncols, np.array(lp.b), np.array(lp.c), rows=np.asarray(lp.A._rows), cols=np.asarray(lp.A._cols),
                   data=np.array(lp.A.data), u=None if u is None else np.array(u))
    return Raw(lp.nrows, lp.ncols, np.array(lp.b), np.array(lp.c), A=np.asarray(lp.A.todense(), dtype=np.float64),
               u=None if u is None else np.array(u))


def variant_case(family, shape, kind, point="ragged"):
    hit = [c for c in tkv.CASES if c[:4] == (family, shape, kind, point)]
    assert len(hit) == 1, (family, shape, kind, point)
    return hit[0]


def from_variants(family, shape, kind, point="ragged"):
    """The LPs of test_kernel_variants' case (its point rules and NEAREST exceptions) as ``Raw``."""
    case = variant_case(family, shape, kind, point)
    lp = tkv.make_case(case[:2] + ("plain",) + case[3:] if kind == "newton" else case)
    if kind == "bounded":
        lp = lp.to_bounded_equality_form()[0]
    raw = raw_of(lp)
    assert (raw.m, raw.N) == (case[4], case[5])
    return raw


def smallest_lp():
    """(1, 2): one row, one column and its slack."""
    rs = np.random.RandomState(12)
    B = 8
    return Raw(1, 2, 0.5 + rs.rand(B, 1), np.hstack([0.5 + rs.rand(B, 1), np.zeros((B, 1))]), A=np.array([[0.75, 1.0]]))


def dense_per_problem(m, N, slack):
    import dense_batch_cases as dbc
    return raw_of(dbc.make(m, N, slack, B=24))


def bounded_per_problem_dense(mk, n):
    import general_batch_cases as gbc
    return raw_of(gbc.make(mk, n, B=24).to_bounded_equality_form()[0])


def bounded_per_problem_sparse(mk, n, density):
    import general_batch_cases as gbc
    import sparse_general_batch_cases as sgbc
    from test_sparse_general_solver import make_sparse_general
    base = make_sparse_general(mk, n, 24, 500 + mk, density, fixed=2, mixed_u=True, kinds=gbc.kinds(mk))
    return raw_of(sgbc.per_problem(base, 501 + mk, gbc.kinds(mk), 2).to_bounded_equality_form()[0])


def block_lp(m, n, per_col, B=12):
    """A sparse standard-form LP of the block kernel's tests (test_workgroup_kernel_plans.column_structure)."""
    import test_workgroup_kernel_plans as wkp
    rs = np.random.RandomState(21)
    A = wkp.column_structure(m, n, per_col, 21).toarray()
    return Raw(m, m + n, 0.5 + rs.rand(B, m), np.hstack([0.5 + rs.rand(B, n), np.zeros((B, m))]), A=np.hstack([A, np.eye(m)]))


def block_per_problem(m, n, per_col, B=12):
    from pycllp_amd import problems
    raw = block_lp(m, n, per_col, B)
    A = sp.csr_matrix(raw.A[:, :n])
    rows, cols, data = problems.per_problem_values(A, B, seed=23)
    rows, cols = np.concatenate([rows, np.arange(m)]), np.concatenate([cols, n + np.arange(m)])
    return Raw(m, m + n, raw.b, raw.c, rows=rows, cols=cols, data=np.hstack([data, np.ones((B, m))]))


def deferred_batch():
    """Per-problem values on one sparse structure whose rows 0 and 1 share their columns; in LP 1 row 1 repeats row 0 (and its
    right-hand side), as test_rank_deficient_constraints duplicates rows: the wave kernel's unguarded LDL' meets a zero pivot
    there.  Whether it hands that LP to the block kernel is the kernel's business -- it defers when the Nocedal-Wright guard
    would have bitten, u^2 / D > beta^2, and after an EXACT duplicate the column under the floored pivot is rounding noise, so
    the guard stays quiet and the wave kernel keeps the LP (measured on MI355X: LP 1 does not carry the block kernel's bits).
    The case is therefore one of store_lp and asserts that: LP 1 does NOT carry the block kernel's bits, every output is
    written, no status -1 is left.  A change of the deferral rule shows up as a failure here.  The 'deferred-all' cases are
    those in which the block kernel stores behind the wave kernel."""
    rs = np.random.RandomState(3)
    m, n, B = 7, 14, 9
    mask = rs.rand(m, n) < 0.5
    mask[1] = mask[0] = True
    rows, cols = np.nonzero(mask)
    data = 0.1 + rs.rand(B, rows.size)
    b = 0.5 + rs.rand(B, m)
    data[1][rows == 1] = data[1][rows == 0]
    b[1, 1] = b[1, 0]
    rows, cols = np.concatenate([rows, np.arange(m)]), np.concatenate([cols, n + np.arange(m)])
    return Raw(m, m + n, b, np.hstack([0.5 + rs.rand(B, n), np.zeros((B, m))]), rows=rows, cols=cols,
               data=np.hstack([data, np.ones((B, m))]))


def dense_big(m, n, B=5):
    from pycllp_amd import problems
    A, b, c = problems.random_dense_arrays(m, n, B, seed=m + n)
    return Raw(m, m + n, b, np.hstack([c, np.zeros((B, m))]), A=np.hstack([A, np.eye(m)]))


def sparse_big(m, n, per_col, B=5):
    return block_lp(m, n, per_col, B)


# ---- the case table -----------------------------------------------------------------------------------------------------------
class Case(object):
    """One store site x kind: ``entry`` on the LPs of ``problem()`` (a ``Raw``) with ``flags``; ``handle``: 'dense' or 'sparse';
    ``kind``: 'solve', 'bounded' or 'newton'; ``expect``: what ``launch_info()`` must report (see ``assert_served``)."""

    def __init__(self, id, site, entry, problem, expect, flags=0, oracle_flags=0, deferred=None, rank_deficient=None):
        self.id, self.site, self.entry, self.problem, self.expect, self.flags = id, site, entry, problem, expect, flags
        self.oracle_flags, self.deferred, self.rank_deficient = oracle_flags, deferred, rank_deficient
        self.handle = entry.split("_")[0]
        self.kind = "newton" if entry.endswith("newton") else ("bounded" if "bounded" in entry else "solve")
        self.per_problem = "batch" in entry


G, GS = (32, 96), (32, 96)          # the lane-group shape of the ragged points: m = 17, one past the 16-row kernels
W = (3, 4)                          # the wave shape: m = 33, N = 193


def group(shape, slack):
    return ("group", shape, 1 if slack else 0)


CASES = [
    # ipm_group.inc finalize
    Case("group-plain-general", "ipm_group.inc", "dense_solve", lambda: from_variants("group", G, "plain"), group(G, 0), FLAG_NO_SLACK),
    Case("group-pc-general", "ipm_group.inc", "dense_solve", lambda: from_variants("group", G, "pc"), group(G, 0),
         FLAG_NO_SLACK | FLAG_PC, FLAG_PC),
    Case("group-plain-slack", "ipm_group.inc", "dense_solve", lambda: from_variants("slack", GS, "plain"), group(GS, 1)),
    Case("group-pc-slack", "ipm_group.inc", "dense_solve", lambda: from_variants("slack", GS, "pc"), group(GS, 1), FLAG_PC, FLAG_PC),
    Case("group-guard-slack", "ipm_group.inc", "dense_solve", lambda: from_variants("slack", GS, "plain"), group(GS, 1),
         FLAG_FORCE_GUARD),
    Case("group-plain-1x2", "ipm_group.inc", "dense_solve", lambda: from_variants("group", (16, 32), "plain"), group((16, 32), 0),
         FLAG_NO_SLACK),
    # ipm_group_hsd.inc
    Case("group-hsd-general", "ipm_group_hsd.inc", "dense_solve", lambda: from_variants("group", G, "hsd"), group(G, 0),
         FLAG_NO_SLACK | FLAG_HSD, FLAG_HSD),
    Case("group-hsd-slack", "ipm_group_hsd.inc", "dense_solve", lambda: from_variants("slack", GS, "hsd"), group(GS, 1), FLAG_HSD,
         FLAG_HSD),
    # ipm_group_slot_body.inc
    Case("slot-bounded", "ipm_group_slot_body.inc", "dense_solve_bounded", lambda: from_variants("slack", GS, "bounded"), group(GS, 1)),
    Case("slot-perA-slack", "ipm_group_slot_body.inc", "dense_solve_batch", lambda: dense_per_problem(17, 66, True), group(GS, 1)),
    Case("slot-perA-general", "ipm_group_slot_body.inc", "dense_solve_batch", lambda: dense_per_problem(17, 65, False), group(G, 0),
         FLAG_NO_SLACK),
    Case("slot-perA-bounded", "ipm_group_slot_body.inc", "dense_solve_batch_bounded", lambda: bounded_per_problem_dense(17, 49),
         group(GS, 1), FLAG_AUTOSCALE),
    # lane-group Newton
    Case("group-newton", "lane-group Newton", "dense_newton", lambda: from_variants("group", G, "newton"), group(G, 0)),
    Case("group-newton-1x2", "lane-group Newton", "dense_newton", lambda: from_variants("group", (16, 32), "newton"),
         group((16, 32), 0)),
    # store_lp (wreg_wave.h)
    Case("wave-tables-plain", "store_lp", "sparse_solve", lambda: from_variants("tables", W, "plain"), ("wave", "tables", W)),
    Case("wave-tables-hsd", "store_lp", "sparse_solve", lambda: from_variants("tables", W, "hsd"), ("wave", "tables", W), FLAG_HSD,
         FLAG_HSD),
    Case("wave-tables-pc", "store_lp", "sparse_solve", lambda: from_variants("tables", W, "pc"), ("wave", "tables", W), FLAG_PC, FLAG_PC),
    Case("wave-image-plain", "store_lp", "sparse_solve", lambda: from_variants("image", W, "plain"), ("wave", "dense image", W)),
    Case("wave-image-hsd", "store_lp", "sparse_solve", lambda: from_variants("image", W, "hsd"), ("wave", "dense image", W), FLAG_HSD,
         FLAG_HSD),
    Case("wave-image-pc", "store_lp", "sparse_solve", lambda: from_variants("image", W, "pc"), ("wave", "dense image", W), FLAG_PC,
         FLAG_PC),
    Case("wave-perA", "store_lp", "sparse_solve_batch", lambda: from_variants("tables", W, "pa"), ("wave", "tables", W)),
    Case("wave-plain-1x2", "store_lp", "sparse_solve", smallest_lp, ("wave", "tables", (1, 4))),
    Case("wave-rank-deficient", "store_lp", "sparse_solve_batch", deferred_batch, ("wave", "tables", (1, 4)), rank_deficient=[1]),
    # ipm_wreg_bounded.inc
    Case("wave-bounded", "ipm_wreg_bounded.inc", "sparse_solve_bounded", lambda: from_variants("tables", W, "bounded"),
         ("wave", "tables", W)),
    Case("wave-perA-bounded", "ipm_wreg_bounded.inc", "sparse_solve_batch_bounded", lambda: bounded_per_problem_sparse(33, 160, 0.08),
         ("wave", "tables", W), FLAG_AUTOSCALE),
    # ipm_wreg_newton.inc
    Case("wave-newton", "ipm_wreg_newton.inc", "sparse_newton", lambda: from_variants("tables", W, "newton"), ("wave", "tables", W)),
    # ipm_block.inc
    Case("block-plain", "ipm_block.inc", "sparse_solve", lambda: block_lp(17, 240, 3), ("block",), FLAG_BLOCK),
    Case("block-hsd", "ipm_block.inc", "sparse_solve", lambda: block_lp(17, 240, 3), ("block",), FLAG_BLOCK | FLAG_HSD, FLAG_HSD),
    Case("block-perA", "ipm_block.inc", "sparse_solve_batch", lambda: block_per_problem(17, 240, 3), ("block",), FLAG_BLOCK),
    Case("block-perA-hsd", "ipm_block.inc", "sparse_solve_batch", lambda: block_per_problem(17, 240, 3), ("block",),
         FLAG_BLOCK | FLAG_HSD, FLAG_HSD),
    Case("block-newton", "ipm_block.inc", "sparse_newton", lambda: block_lp(17, 240, 3), ("block",), FLAG_BLOCK),
    # ipm_block.inc behind the wave kernel
    Case("deferred-all-257", "ipm_block.inc (deferred LPs)", "sparse_solve", lambda: block_lp(17, 240, 3), ("wave", "tables", (5, 6)),
         FLAG_FORCE_GUARD, deferred=True),
    Case("deferred-all-257-perA", "ipm_block.inc (deferred LPs)", "sparse_solve_batch", lambda: block_per_problem(17, 240, 3),
         ("wave", "tables", (5, 6)), FLAG_FORCE_GUARD, deferred=True),
    Case("deferred-all", "ipm_block.inc (deferred LPs)", "sparse_solve", lambda: from_variants("tables", W, "plain"),
         ("wave", "tables", W), FLAG_FORCE_GUARD, deferred=True),
    Case("deferred-all-perA", "ipm_block.inc (deferred LPs)", "sparse_solve_batch", lambda: from_variants("tables", W, "pa"),
         ("wave", "tables", W), FLAG_FORCE_GUARD, deferred=True),
    # ipm_big.hip
    Case("big-dense-plain", "ipm_big.hip", "dense_solve", lambda: dense_big(129, 40), ("big",)),
    Case("big-dense-hsd", "ipm_big.hip", "dense_solve", lambda: dense_big(129, 40), ("big",), FLAG_HSD, FLAG_HSD),
    Case("big-sparse-plain", "ipm_big.hip", "sparse_solve", lambda: sparse_big(40, 473, 4), ("big",)),
    Case("big-sparse-hsd", "ipm_big.hip", "sparse_solve", lambda: sparse_big(40, 473, 4), ("big",), FLAG_HSD, FLAG_HSD),
    Case("big-dense-newton", "ipm_big.hip", "dense_newton", lambda: dense_big(129, 40), ("big",)),
    Case("big-sparse-newton", "ipm_big.hip", "sparse_newton", lambda: sparse_big(40, 473, 4), ("big",)),
]
BATCHES = ("B=3", "hand-over")
LDL_N = (1, 63, 65, 128)
LDL_CASES = [(e, n, mod) for e in ("ldl", "ldl_solve") for n in LDL_N for mod in (0, 1)] + [("forward_backward_ldl", n, 0) for n in LDL_N]
# the store sites of the issue's table -> the entries that must reach each
SITES = {
    "ipm_group.inc": {"dense_solve"}, "ipm_group_hsd.inc": {"dense_solve"},
    "ipm_group_slot_body.inc": {"dense_solve_bounded", "dense_solve_batch", "dense_solve_batch_bounded"},
    "lane-group Newton": {"dense_newton"}, "store_lp": {"sparse_solve", "sparse_solve_batch"},
    "ipm_wreg_bounded.inc": {"sparse_solve_bounded", "sparse_solve_batch_bounded"}, "ipm_wreg_newton.inc": {"sparse_newton"},
    "ipm_block.inc": {"sparse_solve", "sparse_solve_batch", "sparse_newton"},
    "ipm_block.inc (deferred LPs)": {"sparse_solve_batch"},
    "ipm_big.hip": {"dense_solve", "sparse_solve", "dense_newton", "sparse_newton"},
}


def test_case_table_covers_every_store_site_and_entry():
    for site, entries in SITES.items():
        assert entries <= {c.entry for c in CASES if c.site == site}, site
    assert {c.site for c in CASES} == set(SITES)
    assert {c.entry for c in CASES} | {e for e, _, _ in LDL_CASES} == set(fp.ENTRIES)
    assert len({c.id for c in CASES}) == len(CASES)
    ids = {c.id: c for c in CASES}
    # kinds of the table: both lane-group tables per path, the guard path, both per-problem tables, both wave variants per path
    for k in ("plain", "pc"):
        assert ids["group-%s-general" % k].expect[2] == 0 and ids["group-%s-slack" % k].expect[2] == 1
    assert ids["group-guard-slack"].flags & FLAG_FORCE_GUARD and ids["slot-perA-general"].flags & FLAG_NO_SLACK
    for c in CASES:
        assert c.handle in ("dense", "sparse") and not (c.flags & FLAG_HSD and c.flags & FLAG_PC)
        assert (c.oracle_flags != 0) == bool(c.flags & (FLAG_HSD | FLAG_PC)), c.id


def test_ragged_points_are_one_past_the_previous_padding_step():
    assert tkv.ragged_point("group", G) == (17, 65) and tkv.ragged_point("slack", GS) == (17, 66)
    assert tkv.ragged_point("tables", W) == (33, 193) == tkv.ragged_point("image", W) and variant_case("group", (16, 32), "plain")[4:6] == (1, 2)
    for c in CASES:
        if c.site.startswith("ipm_block.inc") or c.site == "ipm_big.hip" or c.rank_deficient:
            continue
        raw = c.problem()
        if c.expect[0] == "group":
            fam = "slack" if c.expect[2] else "group"
            assert tkv.first_covering(fam, tkv.GROUP_SHAPES, raw.m, raw.N) == c.expect[1], c.id
            assert (raw.m, raw.N) in (tkv.ragged_point(fam, c.expect[1]), (1, 2)), c.id
        else:
            fam = "image" if c.expect[1] == "dense image" else "tables"
            assert tkv.first_covering(fam, tkv.SHAPES[fam], raw.m, raw.N) == c.expect[2], c.id
            assert (raw.m, raw.N) in (tkv.ragged_point(fam, c.expect[2]), (1, 2)), c.id
    # the workgroup kernels: one column past the block kernel's 256 threads (its second column register holds one live column),
    # directly and behind the wave kernel; one row past 128 and one column past 512 on the large-LP kernel
    for c in CASES:
        if c.site == "ipm_block.inc" or c.id.startswith("deferred-all-257"):
            assert c.problem().N == 257 and c.problem().m == 17, c.id
    assert sum(c.id.startswith("deferred-all-257") for c in CASES) == 2
    assert dense_big(129, 40).m == 129 and sparse_big(40, 473, 4).N == 513


# ---- GPU: one call of a case ------------------------------------------------------------------------------------------------
def out_shape(name, entry, B, m, N):
    if entry == "ldl":
        return (B, N * (N + 1) // 2) if name == "L" else (B, N)
    if name in ("x", "z", "s"):
        return (B, N)
    if name in ("y", "dy"):
        return (B, m)
    return (B,)


def specs_of(entry, ins, B, m, N):
    outs = fp.OUTPUTS[entry]
    return [fp.out(k, out_shape(k, entry, B, m, N), I32 if k in fp.I32_ARRAYS else F64) if k in outs else fp.inp(k, ins[k])
            for k in fp.ENTRIES[entry][2]]


class Run(object):
    """A case at one batch size: handle, inputs, options; ``call`` runs the entry once on a ``Plain`` or an ``Arena``."""

    def __init__(self, case, raw, reserve=0):
        from pycllp_amd import _native
        from pycllp_amd.solvers.hip import Handle
        self.case, self.raw, self.B = case, raw, raw.B
        self.dev = torch.device("cuda", 0)
        self.scalars, ins = {}, dict(b=raw.b, c=raw.c)
        if case.handle == "dense":
            self.handle = Handle(np.ascontiguousarray(raw.dense(0)), self.dev, None)
            if case.per_problem:
                slack = not (case.flags & FLAG_NO_SLACK)
                a_cols = raw.N - raw.m if slack else raw.N
                ins["A"] = np.stack([raw.dense(k)[:, :a_cols] for k in range(raw.B)])
                self.scalars["a_cols"] = a_cols
        else:
            A, perm = raw.csr()
            self.handle = Handle(A, self.dev, None)
            if case.per_problem:
                ins["A"] = raw.data[:, perm]
        if raw.u is not None:
            ins["u"] = raw.u
        if case.kind == "newton":
            rs = np.random.RandomState(7)
            B = raw.B
            ins = dict(x=0.5 + rs.rand(B, raw.N), z=0.5 + rs.rand(B, raw.N), y=rs.rand(B, raw.m), b=rs.rand(B, raw.m), c=rs.rand(B, raw.N))
            self.scalars["mu"] = 1.0
        self.ins = ins
        self.opts = dict(flags=case.flags, reserve_cus=reserve)
        self._native = _native

    def specs(self):
        return specs_of(self.case.entry, self.ins, self.B, self.raw.m, self.raw.N)

    def call(self, placement=None, null=(), **opts):
        mem = fp.Plain(self.specs(), self.dev) if placement is None else fp.Arena(self.specs(), placement, self.dev, null=null)
        o = self._native.default_opts(**dict(self.opts, **opts))
        rc = fp.call(self.case.entry, mem.arrays(), self.B, handle=self.handle, opts=o, **self.scalars)
        assert rc == 0, (rc, self._native.lib().pycllp_hip_last_error())
        mem.check()
        return mem.results()

    def slots(self):
        info = self.handle.launch_info()
        if "group_shape" in info:
            return info["grid"] * (info["block"] // 64) * (64 // info["group_shape"][0])
        if info.get("kernel") == "wave":
            return info["grid"] * (info["block"] // 64)
        return info["grid"]


def assert_served(info, expect):
    if expect[0] == "group":
        assert info.get("group_shape") == expect[1] and info.get("slack") == expect[2], info
        assert (info["m_pad"], info["n_pad"]) == expect[1] and "wave_shape" not in info and "kernel" not in info, info
    elif expect[0] == "wave":
        assert info.get("kernel") == "wave" and info.get("variant") == expect[1] and info.get("wave_shape") == expect[2], info
        assert "group_shape" not in info, info
    else:
        assert info.get("kernel") == expect[0] and "wave_shape" not in info and "group_shape" not in info, info
        if expect[0] == "big":
            assert "big_shape" in info, info
        else:
            assert "a_in_lds" in info, info


def as_solver(res):
    return types.SimpleNamespace(status=res["status"], iters=res["iters"], primal_obj=res["pobj"], dual_obj=res["dobj"],
                                 x=res["x"], y=res["y"], z=res["z"])


def verify(case, raw, ins, res):
    """The reference call against the CPU reference of the family's own test, at that test's tolerances."""
    from oracle import port
    B = raw.B
    if case.kind == "newton":
        A = raw.dense(0)
        for i in list(range(min(B, 12))) + list(range(max(B - 4, 12), B)):          # (the first and the last states of a long batch)
            ref = port.solve_primal_normal(A, ins["x"][i], ins["z"][i], ins["y"][i], ins["b"][i], ins["c"][i], 1.0)
            np.testing.assert_allclose(res["dy"][i], ref, rtol=1e-7, atol=1e-9)
            np.testing.assert_allclose(res["dy"][i], port.newton_step_known_answer(A, ins["x"][i], ins["z"][i], ins["y"][i],
                                                                                  ins["b"][i], ins["c"][i], 1.0), rtol=1e-5, atol=1e-5)
        assert (res["nrefine"] >= 0).all() and (res["nrefine"] <= 5).all()
        return
    if case.kind == "bounded":
        import bounded_twin
        sel = np.unique(np.linspace(0, B - 1, min(B, 8)).astype(int))
        auto = bool(case.flags & FLAG_AUTOSCALE)
        tw = [bounded_twin.solve(raw.dense(k), raw.b[k:k + 1], raw.c[k:k + 1], raw.u[k:k + 1], autoscale=auto) for k in sel]
        tw = {q: np.concatenate([t[q] for t in tw]) for q in ("x", "pobj", "dobj", "status", "iters")}
        assert (res["status"] == 0).all() and (tw["status"] == 0).all(), (res["status"], tw["status"])
        assert np.abs(res["iters"][sel] - tw["iters"]).max() <= 1, (res["iters"][sel], tw["iters"])
        assert rel_err(res["pobj"][sel], tw["pobj"]).max() <= 1e-9 and rel_err(res["dobj"][sel], tw["dobj"]).max() <= 1e-9
        n = raw.N - raw.m
        np.testing.assert_allclose(res["x"][sel, :n], tw["x"][:, :n], rtol=1e-5, atol=1e-6)
        return
    lp = raw.lp()
    if case.rank_deficient:
        # the bounds of test_rank_deficient_constraints
        r = tkv.oracle_each(lp, case.oracle_flags)
        assert (res["status"] == 0).all() and (r["status"] == 0).all() and res["iters"].max() < 40, (res["status"], res["iters"])
        assert rel_err(res["pobj"], r["pobj"]).max() < 1e-8
        return
    if case.per_problem:
        r = tkv.oracle_each(lp, case.oracle_flags)
    else:
        r = port.dense_solve(raw.A, raw.b, raw.c, nthreads=8, flags=case.oracle_flags)
    tkv.assert_matches(as_solver(res), r, lp)


def same_bits(got, ref, names, what):
    for k in names:
        assert np.array_equal(got[k].view(np.uint8), ref[k].view(np.uint8)), \
            "%s: %s differs from the reference call at %d" % (what, k, int(np.flatnonzero((got[k] != ref[k]).reshape(-1))[0]))


def record(line):
    path = os.environ.get("PYCLLP_FOOTPRINT_RECORD")
    if path:
        with open(path, "a") as f:
            f.write(line + "\n")


def one_cu():
    return torch.cuda.get_device_properties(0).multi_processor_count - 1


def hand_over_run(case, base):
    """The case at a B larger than the slots of its launch with one compute unit resident (where the entry honours
    ``reserve_cus``; B follows ``launch_info()`` of a first launch either way)."""
    B = 2 * base.B + 1
    for _ in range(8):
        run = Run(case, base.take(B), reserve=one_cu())
        ref = run.call()
        slots = run.slots()
        if B > 2 * slots:
            return run, ref, slots
        B = max(2 * slots + 3, 4 * B)            # (a grid that still grows with B: in steps)
    raise AssertionError("no B beyond the slots of %s: %d LPs, %d slots" % (case.id, B, slots))


@pytest.mark.gpu
@pytest.mark.parametrize("batch", BATCHES)
@pytest.mark.parametrize("case", CASES, ids=[c.id for c in CASES])
def test_footprint(case, batch):
    base = case.problem()
    if batch == "B=3":
        run = Run(case, base.take(3))
        ref = run.call()
        slots = run.slots()
    else:
        run, ref, slots = hand_over_run(case, base)
        assert run.B > slots, (run.B, slots)
    info = run.handle.launch_info()
    assert_served(info, case.expect)
    outs, optional = fp.OUTPUTS[case.entry], fp.ENTRIES[case.entry][3]
    verify(case, run.raw, run.ins, ref)
    if case.kind != "newton":
        assert not (ref["status"] == -1).any()
    # every output: both placements
    for placement in ("aligned", "natural"):
        same_bits(run.call(placement), ref, outs, placement)
    # NULL outputs: all at once, then z, y (and s) alone
    kept = [k for k in outs if k not in optional]
    same_bits(run.call("natural", null=optional), ref, kept, "all optional outputs NULL")
    for k in [k for k in ("z", "y", "s") if k in optional]:
        same_bits(run.call("aligned", null=(k,)), ref, [q for q in outs if q != k], "%s NULL" % k)
    note = ""
    if case.deferred or case.rank_deficient:
        # what the wave kernel defers carries the block kernel's bits (the two kernels agree to rounding only)
        blk = Run(case, run.raw, reserve=run.opts["reserve_cus"])
        r2 = blk.call(flags=case.flags | FLAG_BLOCK)
        assert blk.handle.launch_info()["kernel"] == "block"
        if case.deferred:                   # PYCLLP_FLAG_FORCE_GUARD_PATH: the wave kernel defers every LP
            same_bits(ref, r2, outs, "deferred LPs against the block kernel")
        else:                               # the exact duplicate does not make the guard bite: the wave kernel keeps the LP
            for k in [k for k in range(run.B) if k % base.B in case.rank_deficient]:
                assert not np.array_equal(ref["x"][k], r2["x"][k]), "LP %d carries the block kernel's bits: it was deferred" % k
            note = " (rank-deficient LPs kept by the wave kernel)"
    # the early exit: every LP at the iteration limit
    if case.kind != "newton":
        lim = run.call("aligned", max_iter=3)
        assert (lim["status"] == 5).all() and (lim["iters"] == 3).all(), (lim["status"], lim["iters"])
    assert_served(run.handle.launch_info(), case.expect)
    record("%-24s | %-28s | %-26s | B=%-5d slots=%-5d grid=%-4d block=%-4d | ok%s"
           % (case.id, case.site, case.entry, run.B, slots, info["grid"], info["block"], note))


# ---- every status writes every output ---------------------------------------------------------------------------------------
# (family, handle, m, n of the standard form, non-zeros per column, flags): LP 2 infeasible, LP 4 unbounded
MIXED = [("group", "dense", 12, 20, None, 0), ("wave", "sparse", 24, 60, 3, 0), ("block", "sparse", 24, 60, 3, FLAG_BLOCK),
         ("big", "dense", 160, 60, None, 0)]


@pytest.mark.gpu
@pytest.mark.parametrize("hsd", [False, True], ids=["plain", "hsd"])
@pytest.mark.parametrize("mixed", MIXED, ids=[c[0] for c in MIXED])
def test_every_status_writes_every_output(mixed, hsd):
    """A batch with an infeasible and an unbounded LP between optimal ones (test_workgroup_kernel_plans.mixed_batch): whatever
    the status, x, y, z, both objectives, the status and the iteration count are written, and nothing else."""
    import test_workgroup_kernel_plans as wkp
    from oracle import port
    family, handle, m, n, nz, flags = mixed
    raw = raw_of(wkp.mixed_batch(m, n, nz, 11))
    flags |= FLAG_HSD if hsd else 0
    case = Case("mixed-" + family, family, handle + "_solve", None, None, flags)
    run = Run(case, raw)
    ref = run.call()
    info = run.handle.launch_info()
    assert ("group_shape" in info) if family == "group" else info.get("kernel") == family, info
    r = port.dense_solve(raw.A, raw.b, raw.c, nthreads=8, flags=FLAG_HSD if hsd else 0)
    assert r["status"][2] != 0 and r["status"][4] != 0 and (np.delete(r["status"], [2, 4]) == 0).all(), r["status"]
    if hsd:
        assert list(r["status"]) == [0, 0, 2, 0, 4, 0, 0]
    np.testing.assert_array_equal(ref["status"], r["status"])
    ok = r["status"] == 0                   # the optimal LPs at the parity bounds of test_kernel_variants.assert_matches
    assert np.abs(ref["iters"][ok].astype(int) - r["iters"][ok]).max() <= 1, (ref["iters"], r["iters"])
    assert rel_err(ref["pobj"][ok], r["pobj"][ok]).max() <= 1e-9 and rel_err(ref["dobj"][ok], r["dobj"][ok]).max() <= 1e-9
    np.testing.assert_allclose(ref["x"][ok], r["x"][ok], rtol=1e-5, atol=1e-6)
    for placement in ("aligned", "natural"):
        same_bits(run.call(placement), ref, fp.SOLVE_OUT, placement)
    same_bits(run.call("natural", null=fp.ENTRIES[case.entry][3]), ref, ("x", "status"), "all optional outputs NULL")
    record("%-24s | %-28s | %-26s | B=%-5d statuses=%s | ok" % ("mixed-%s-%s" % (family, "hsd" if hsd else "plain"), "every status",
                                                               case.entry, raw.B, [int(v) for v in ref["status"]]))


# ---- the LDL' entries -------------------------------------------------------------------------------------------------------
def spd_batch(n, B, seed):
    rs = np.random.RandomState(seed)
    X = rs.rand(B, n, 8) - 0.5
    return X @ X.transpose(0, 2, 1) + n * np.eye(n)


def ldl_slots(entry, modified):
    """Matrices in flight per launch: ldl_solve_wreg_kernel runs four per workgroup on one workgroup per compute unit, the
    ldl_batched.inc kernels one per workgroup on at most 4096 workgroups.  These entries have no handle and no launch_info():
    the figures restate the launch rules of the sources, which test_ldl_launch_rules_are_those_of_the_sources holds against
    their text, and the record says 'by the sources' rule', not 'observed'."""
    if entry == "ldl_solve" and not modified:
        return 4 * torch.cuda.get_device_properties(0).multi_processor_count
    return 4096


def test_ldl_launch_rules_are_those_of_the_sources():
    """What ldl_slots restates: min(B, 4096) workgroups in the three launches of ldl_batched.inc's kernels, min(CUs, (B + 3) / 4)
    workgroups of four waves in ldl_solve_wreg_kernel's."""
    block = open(os.path.join(tkv.CSRC, "ipm_block.hip")).read()
    wreg = open(os.path.join(tkv.CSRC, "ipm_wreg.hip")).read()
    assert block.count("blocks = B < 4096 ? B : 4096;") == 3
    for kernel in ("ldl_batched_kernel", "ldl_solve_batched_kernel", "forward_backward_ldl_kernel"):
        assert "hipLaunchKernelGGL(%s, dim3((unsigned)blocks)" % kernel in block, kernel
    launch = wreg[wreg.index("hipError_t wreg_launch_ldl_solve"):]
    assert "long grid = std::min((long)num_cu, (B + 3) / 4);" in launch[:launch.index("hipLaunchKernelGGL")]
    assert "hipLaunchKernelGGL((ldl_solve_wreg_kernel<8>), dim3((unsigned)grid), dim3(256)" in launch


@pytest.mark.gpu
@pytest.mark.parametrize("batch", BATCHES)
@pytest.mark.parametrize("entry,n,modified", LDL_CASES, ids=["%s-n%d-%s" % (e, n, "modified" if mod else "plain") for e, n, mod in LDL_CASES])
def test_ldl_footprint(entry, n, modified, batch):
    from oracle import port
    from pycllp_amd import _native
    slots = ldl_slots(entry, modified)
    B = 3 if batch == "B=3" else slots + 3
    assert batch == "B=3" or B > slots
    A = spd_batch(n, B, n)
    beta, delta = float(np.sqrt(A.max())), 1e-6
    rs = np.random.RandomState(n + 1)
    sample = sorted(set(range(min(B, 3))) | {B - 1})
    if entry == "ldl":
        ins = dict(A=A)
    elif entry == "ldl_solve":
        ins = dict(A=A, rhs=rs.rand(B, n))
    else:
        L = np.tril(rs.rand(B, n, n) - 0.5, -1) / n + np.eye(n)
        ti = np.tril_indices(n)
        ins = dict(L=L[:, ti[0], ti[1]], D=0.5 + rs.rand(B, n), b=rs.rand(B, n))
    scalars = dict(n=n, modified=modified, beta=beta, delta=delta)
    dev = torch.device("cuda", 0)

    def call(mem):
        rc = fp.call(entry, mem.arrays(), B, **scalars)
        assert rc == 0, (rc, _native.lib().pycllp_hip_last_error())
        mem.check()
        return mem.results()

    ref = call(fp.Plain(specs_of(entry, ins, B, n, n), dev))
    for i in sample:                       # the tolerances of test_ldl_kernels_against_oracle_and_cholesky / test_ldl_solves_against_numpy
        if entry == "ldl":
            Lo, Do = port.ldl(A[i], modified=bool(modified), beta=beta, delta=delta) if modified else port.ldl(A[i])
            np.testing.assert_allclose(ref["D"][i], Do, rtol=1e-6, atol=1e-7)
            np.testing.assert_allclose(ref["L"][i], Lo[np.tril_indices(n)], rtol=1e-6, atol=1e-7)
        elif entry == "ldl_solve":
            np.testing.assert_allclose(ref["x"][i], np.linalg.solve(A[i], ins["rhs"][i]), rtol=1e-9, atol=1e-12)
        else:
            M = (L[i] * ins["D"][i]) @ L[i].T
            np.testing.assert_allclose(ref["x"][i], np.linalg.solve(M, ins["b"][i]), rtol=1e-9, atol=1e-12)
    for placement in ("aligned", "natural"):
        same_bits(call(fp.Arena(specs_of(entry, ins, B, n, n), placement, dev)), ref, fp.OUTPUTS[entry], placement)
    site = "ldl_solve_wreg_kernel" if entry == "ldl_solve" and not modified else "ldl_batched.inc"
    record("%-24s | %-28s | %-26s | B=%-5d slots=%-5d (by the sources' rule) | ok" % ("%s-n%d-%s" % (entry, n, "modified" if modified else "plain"), site,
                                                              entry, B, slots))


# ---- a deferred LP where no block kernel stands behind the wave kernel -----------------------------------------------------------
def wave_only_batch(B=5):
    """Per-problem values on a structure that the wave kernel's per-problem plan takes and the block kernel does not: m = 128,
    N = 512, 3 344 non-zeros -- with A's arrays the block kernel's workgroup would need 164 336 B of LDS (block_plan: None),
    while the structure tables beside ONE wave area with the LP's values fit.  To stay inside both, the structure keeps the
    Gram terms few and their table records full: 16 groups of 8 rows (two per 16-row block) x 32 columns, a column holding 7
    (17 of a group's columns) or 6 of its group's rows."""
    rows, cols = [], []
    for g in range(16):
        for j in range(32):
            omit = {j % 8} if j < 17 else {(j - 17) % 8, ((j - 17) % 8 + 1 + (j - 17) // 8) % 8}
            for r in sorted(set(range(8)) - omit):
                rows.append(8 * g + r)
                cols.append(32 * g + j)
    rows, cols = np.array(rows), np.array(cols)
    # every LP around a strictly feasible primal-dual pair of its own matrix, b and c of max-norm 1 (test_kernel_variants.equality_lp)
    rs = np.random.RandomState(41)
    data = (0.1 + 0.9 * rs.rand(B, rows.size)) * rs.choice([-1.0, 1.0], (B, rows.size))
    x0, y0, z0 = rs.rand(B, 512) + 0.1, rs.randn(B, 128), rs.rand(B, 512) + 0.1
    b, c = np.zeros((B, 128)), -z0
    for k in range(B):
        np.add.at(b[k], rows, data[k] * x0[k, cols])
        np.add.at(c[k], cols, data[k] * y0[k, rows])
    b /= np.abs(b).max(axis=1, keepdims=True)
    c /= np.abs(c).max(axis=1, keepdims=True)
    return Raw(128, 512, b, c, rows=rows, cols=cols, data=data)


def test_wave_only_structure_is_beyond_the_block_kernel():
    import test_workgroup_kernel_plans as wkp
    raw = wave_only_batch()
    A, perm = raw.csr()
    assert A.nnz == raw.rows.size == 3344 and A.shape == (128, 512) and sorted(perm) == list(range(3344))
    assert wkp.block_plan(128, 512, A.nnz, pa=True) is None            # lds_with_a == 0: per-problem values have no block kernel
    assert wkp.block_plan(128, 512, A.nnz - 21, pa=True) is not None   # (and 21 entries fewer would have one)
    assert tkv.first_covering("tables", tkv.WAVE_TAB_SHAPES, 128, 512) == (8, 8)


UNTOUCHED = ("x", "y", "z", "pobj", "dobj", "iters")


@pytest.mark.gpu
def test_deferred_lp_without_a_block_kernel_ends_numerical_and_keeps_its_outputs():
    """The exception the header states: per-problem values on a structure that only the wave kernel serves.  An LP it defers
    (here every LP: PYCLLP_FLAG_FORCE_GUARD_PATH; without the flag the same batch solves to the oracle's optimum) ends PYCLLP_STATUS_NUMERICAL, and status is ALL it gets: x, y, z, pobj, dobj
    and iters stay as the caller left them.  Guard bands and inputs intact at both placements, B = 3 and beyond the slots."""
    E_UNSUPPORTED = -2
    case = Case("wave-only-perA", "deferred_to_numerical_kernel", "sparse_solve_batch", None, ("wave", "tables", (8, 8)), FLAG_FORCE_GUARD)
    # unforced, the batch is an ordinary solve on the per-problem wave plan: nothing is deferred, every output against the oracle
    free = Case("wave-only-perA-unforced", "store_lp", case.entry, None, case.expect)
    run = Run(free, wave_only_batch().take(3))
    ref = run.call()
    assert_served(run.handle.launch_info(), free.expect)
    verify(free, run.raw, run.ins, ref)
    same_bits(run.call("natural"), ref, fp.SOLVE_OUT, "natural")
    record("%-24s | %-28s | %-26s | B=%-5d slots=%-5d | ok" % (free.id, free.site, free.entry, run.B, run.slots()))
    for B, reserve in ((3, 0), (9, one_cu())):
        run = Run(case, wave_only_batch().take(B), reserve=reserve)
        o = run._native.default_opts(**run.opts)
        mems = [fp.Plain(run.specs(), run.dev), fp.Arena(run.specs(), "aligned", run.dev), fp.Arena(run.specs(), "natural", run.dev),
                fp.Arena(run.specs(), "natural", run.dev, null=fp.ENTRIES[case.entry][3])]
        for mem in mems:
            rc = fp.call(case.entry, mem.arrays(), B, handle=run.handle, opts=o)
            assert rc == 0, (rc, run._native.lib().pycllp_hip_last_error())
            mem.check(untouched=UNTOUCHED)
            assert (mem.result("status") == 3).all(), mem.result("status")
        info = run.handle.launch_info()
        assert_served(info, case.expect)
        slots = run.slots()
        assert B == 3 or B > slots, (B, slots)
        # no block kernel for these values: asked for by flag, the entry declines before it launches anything
        mem = fp.Arena(run.specs(), "aligned", run.dev)
        rc = fp.call(case.entry, mem.arrays(), B, handle=run.handle, opts=run._native.default_opts(flags=FLAG_BLOCK))
        assert rc == E_UNSUPPORTED, rc
        mem.check(outputs_written=False)
        record("%-24s | %-28s | %-26s | B=%-5d slots=%-5d grid=%-4d block=%-4d | ok: status 3, other outputs untouched"
               % (case.id, case.site, case.entry, B, slots, info["grid"], info["block"]))


# ---- refused calls touch nothing ----------------------------------------------------------------------------------------------
REFUSED = [
    ("dense_solve", lambda: from_variants("slack", GS, "plain"), dict(flags=FLAG_HSD | FLAG_PC), {}),
    ("dense_solve_bounded", lambda: from_variants("slack", GS, "bounded"), dict(flags=FLAG_HSD), {}),
    ("dense_solve_batch", lambda: dense_per_problem(17, 66, True), dict(flags=0), dict(a_cols=66)),
    ("dense_solve_batch_bounded", lambda: bounded_per_problem_dense(17, 49), dict(flags=0), dict(a_cols=66)),
    ("sparse_solve", lambda: from_variants("tables", W, "plain"), dict(flags=FLAG_HSD | FLAG_PC), {}),
    ("sparse_solve_batch", lambda: from_variants("tables", W, "pa"), dict(flags=FLAG_HSD | FLAG_PC), {}),
    ("sparse_solve_bounded", lambda: from_variants("tables", W, "bounded"), dict(flags=FLAG_BLOCK), {}),
    ("sparse_solve_batch_bounded", lambda: bounded_per_problem_sparse(33, 160, 0.08), dict(flags=FLAG_BLOCK), {}),
]


@pytest.mark.gpu
@pytest.mark.parametrize("entry,problem,opts,scalars", REFUSED, ids=[r[0] for r in REFUSED])
def test_refused_call_touches_nothing(entry, problem, opts, scalars):
    """A flag combination the header lists as PYCLLP_E_BADARG, or an a_cols other than the handle's: the return code, and every
    output, guard band and input of a real arena as before the call."""
    case = Case("refused", None, entry, None, None, 0)
    run = Run(case, problem().take(3))
    for placement in ("aligned", "natural"):
        mem = fp.Arena(run.specs(), placement, run.dev)
        o = run._native.default_opts(**opts)
        rc = fp.call(entry, mem.arrays(), run.B, handle=run.handle, opts=o, **dict(run.scalars, **scalars))
        assert rc == E_BADARG, rc
        mem.check(outputs_written=False)
    run.call("aligned")                     # and the handle still serves a good call


# ---- the launch ring ----------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("family", ["dense", "sparse"])
def test_ring_wrap(family):
    """130 solves back to back on one handle, no sync in between, alternating two streams, each into arena outputs of its own:
    two full turns of the handle's 64 launch counters (the wave kernel takes two per solve).  All results carry the bits of the
    first and every guard band is intact."""
    from pycllp_amd import problems
    if family == "dense":
        A, b, c = problems.random_dense_arrays(16, 16, 5, seed=4)
        raw = Raw(16, 32, b, np.hstack([c, np.zeros((5, 16))]), A=np.hstack([A, np.eye(16)]))
        case = Case("ring-dense", None, "dense_solve", None, group((16, 32), 1))
    else:
        raw = from_variants("tables", W, "plain").take(5)
        case = Case("ring-sparse", None, "sparse_solve", None, ("wave", "tables", W))
    run = Run(case, raw)
    ref = run.call()
    assert_served(run.handle.launch_info(), case.expect)
    assert (ref["status"] == 0).all()
    o = run._native.default_opts(**run.opts)
    streams = [torch.cuda.Stream(run.dev), torch.cuda.Stream(run.dev)]
    arenas = [fp.Arena(run.specs(), ("aligned", "natural")[i % 2], run.dev) for i in range(130)]
    torch.cuda.synchronize()
    for i, mem in enumerate(arenas):
        rc = fp.call(case.entry, mem.arrays(), run.B, handle=run.handle, opts=o, stream=streams[i % 2])
        assert rc == 0, (i, rc)
    torch.cuda.synchronize()
    for i, mem in enumerate(arenas):
        mem.check()
        same_bits(mem.results(), ref, fp.SOLVE_OUT, "solve %d" % i)
    record("%-24s | %-28s | %-26s | B=%-5d launches=130 | ok" % (case.id, "launch ring", case.entry, run.B))
