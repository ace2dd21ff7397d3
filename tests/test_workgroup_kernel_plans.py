"""Every compiled instantiation and LDS plan of the two workgroup-per-LP kernels against the CPU references, in the scheme of
test_kernel_variants.py: the large-LP kernel ``ipm_big_kernel<WGPC, BNC>`` (csrc/ipm_big.hip; BIG_SHAPES) and the block kernel
(csrc/ipm_block.inc), the guarded fallback behind every plan of the wavefront-per-LP kernel.

Large-LP kernel.  A CELL is (factor storage, WGPC, BNC): the blocks of the factor in LDS ('L') or in the L2 workspace ('W'),
workgroups per CU, N-vector registers per thread.  The host decides all three from (MB, N) -- MB 16-row blocks, N columns of
the equality form -- and the rules are restated below (big_lds_doubles, big_plan).  Every reachable cell is solved on both Gram
paths (matrix cores on a dense image, term list) and in every kind at two points: FULL, N = 256 BNC with the most 16-row blocks
the cell has there, every row live; RAGGED, N = 256 BNC_prev + 1 (one live column in the last register) with the fewest blocks
the cell has there and one live row in the last of them.

Block kernel.  One instantiation, three LDS plans: A's CSR / CSC copy in LDS with room for a second workgroup ('lds-paired'),
A read through L2 ('l2'), A in LDS and the workgroup alone on its CU ('lds-alone').  FULL: N = 512 (both column registers of a
thread full) and m a multiple of 8; RAGGED: N = 257 and m = 8 k + 1 (m-vectors are padded to 8 rows).

CPU: the rules hold against the sources, the table covers exactly the reachable cells x Gram paths x kinds, every point lands in
its cell.  GPU: every case first asserts what served it (``launch_info()``), then compares with its reference; one point per
cell and plan is solved a second time on a grid of one CU's worth of workgroups, where every workgroup takes several LPs in turn,
and must give the same bits."""
import os
import re

import numpy as np
import pytest
import scipy.sparse as sp

from conftest import check_certificates
from pycllp_amd import problems
from pycllp_amd.lp import EqualityLP, SparseMatrix, StandardLP
from test_kernel_variants import (CSRC, MAX_LDS, ORACLE_FLAGS, WAVE_DA_SHAPES, WAVE_TAB_SHAPES, assert_matches, equality_lp,
                                  first_covering, image_waves, newton_matches, oracle_each, tables_cannot_fit)

# ---- the sources' constants, as this file knows them (test_constants_and_shape_list_of_the_sources holds them) ---------------
BIG_SHAPES = [(3, 2), (2, 2), (3, 3), (2, 3), (3, 5), (2, 5)]        # (WGPC, BNC) in the order the selection walks them
BT, BIG_MAX_M, BIG_MAX_N = 256, 256, 1280
BLK_T, BLK_MAX_M, BLK_MAX_N = 256, 128, 512
BIG_MAX_TERMS = 1 << 24
BNCS = sorted({s[1] for s in BIG_SHAPES})
FLAG_BLOCK_KERNEL = 64

BIG_KINDS = ("plain", "hsd", "pc", "newton")
GRAMS = ("mfma", "terms")
# block kernel: kinds per plan.  Per-problem values of A force A's arrays into LDS (sparse_solve_impl: lds_with_a), so 'l2' has no
# 'pa' kinds; without them base <= half the LDS at every m <= 128, N <= 512, so only they reach 'lds-alone'
# (test_block_plan_rule_and_reachable_plans).  No predictor-corrector on this kernel (test_block_kernel_refuses_predcorr).
BLOCK_KINDS = {"lds-paired": ("plain", "hsd", "newton", "pa", "pa-hsd"), "l2": ("plain", "hsd", "newton"),
               "lds-alone": ("pa", "pa-hsd")}


# ---- restatements of the plan rules ---------------------------------------------------------------------------------------
def big_lds_doubles(MB, n, m_in_lds):
    """big.h big_lds_doubles: the factor blocks (when in LDS), W_K, two N-vectors, nine m-vectors, tile, wsA, red."""
    MP, NPv = 16 * MB, (n + 7) & ~7
    return (MB * (MB + 1) // 2 * 256 if m_in_lds else 0) + MB * 256 + 2 * NPv + 9 * MP + 272 + 256 + 32


def big_plan(MB, N):
    """(cell, lds_bytes, workgroups per CU the LDS allows) of big_host_plan (big_plan.h) / big_select: the factor in LDS only when two
    workgroups still fit a CU with it; three workgroups per CU where the LDS allows, else two, else one; the first BNC with
    N <= 256 BNC."""
    in_lds = 2 * 8 * big_lds_doubles(MB, N, True) <= MAX_LDS
    lds = 8 * big_lds_doubles(MB, N, in_lds)
    per_cu = 3 if 3 * lds <= MAX_LDS else (2 if 2 * lds <= MAX_LDS else 1)
    bnc = next(k for k in BNCS if N <= k * BT)
    return ("L" if in_lds else "W", per_cu, bnc), lds, per_cu


def reachable(m, N):
    """An LP the large-LP kernel serves: within its caps, with a column to spare, and past what the wavefront-per-LP and block
    kernels take first (pycllp_hip_sparse_init: m <= BLK_MAX_M and N <= BLK_MAX_N)."""
    return 1 <= m <= BIG_MAX_M and m < N <= BIG_MAX_N and (m > BLK_MAX_M or N > BLK_MAX_N)


def cell_blocks(cell, N):
    """The block counts MB at which column count N lies in ``cell`` with a reachable m of one live row in the last block."""
    return [MB for MB in range(1, BIG_MAX_M // 16 + 1) if big_plan(MB, N)[0] == cell and reachable(16 * (MB - 1) + 1, N)]


def reachable_cells():
    return {big_plan(MB, N)[0] for N in range(2, BIG_MAX_N + 1) for MB in range(1, BIG_MAX_M // 16 + 1)
            if reachable(16 * (MB - 1) + 1, N)}


def gram_is_dense(A, tail):
    """big_plan_create: the Gram matrix on the matrix cores when the term list would be longer than an eighth of the dense
    product's MP^2 nd multiply-adds (nd: the columns before the identity tail).  ``A``: scipy sparse, equality form."""
    m, N = A.shape
    lens = np.diff(sp.csc_matrix(A).indptr).astype(np.int64)
    MP, nd = 16 * ((m + 15) // 16), (N - m if tail else N)
    return int((lens * (lens + 1) // 2).sum()) > 0.125 * MP * MP * nd


def gram_terms(A):
    lens = np.diff(sp.csc_matrix(A).indptr).astype(np.int64)
    return int((lens * (lens + 1) // 2).sum())


def block_plan(m, n, nnz, pa=False):
    """(plan, a_in_lds, lds_bytes, workgroups per CU) of pycllp_hip_sparse_init's LDS plan and sparse_solve_impl's launch; None
    where per-problem values do not fit the LDS."""
    mp8 = (m + 7) & ~7
    base = 8 * (m * (m + 1) // 2 + 1 + 2 * (n + 1) + 7 * mp8 + 8)
    with_a = base + 8 * 2 * nnz + 4 * (2 * nnz + m + n + 2) + 16
    half = MAX_LDS // 2
    a = True if with_a <= half else (False if base <= half else with_a <= MAX_LDS)
    if pa:
        if with_a > MAX_LDS:
            return None
        a = True
    lds = with_a if a else base
    per_cu = 4 if MAX_LDS // lds >= 4 else (2 if MAX_LDS // lds >= 2 else 1)
    plan = "l2" if not a else ("lds-paired" if per_cu >= 2 else "lds-alone")
    return plan, a, lds, per_cu


# ---- the case table ---------------------------------------------------------------------------------------------------------
CELLS = [("W", 3, 2), ("W", 2, 2), ("L", 3, 3), ("L", 2, 3), ("W", 3, 3), ("W", 2, 3), ("L", 3, 5), ("L", 2, 5), ("W", 3, 5),
         ("W", 2, 5)]

# Points that cannot be reached, with the nearest one that can and why: (cell, point[, gram]) -> (m, N, note).
# test_nearest_points_are_the_nearest holds them against the rules.
_BNC2 = ("BNC = 2 is N <= 512, which this kernel serves only for m > 128, and an LP has a column to spare (N > m): N = 1 cannot "
         "be reached; the smallest N at which the cell has a point, the fewest blocks the cell has there, one live row in the last")
_MFMA1 = ("a dense A of m <= 7 rows in one block takes the term list (m (m + 1) / 2 <= MP^2 / 8 per column): the fewest rows "
          "whose Gram goes to the matrix cores, m = 8")
NEAREST = {
    (("W", 3, 2), "ragged"): (129, 130, _BNC2),
    (("W", 2, 2), "ragged"): (225, 226, _BNC2),
    (("L", 3, 3), "ragged", "mfma"): (8, 513, _MFMA1),
    (("L", 3, 5), "ragged", "mfma"): (8, 769, _MFMA1),
}


def cell_name(cell):
    return "%s%dx%d" % cell


def big_full_point(cell):
    N = BT * cell[2]
    return 16 * max(cell_blocks(cell, N)), N


def big_ragged_point(cell):
    """None where N = 256 BNC_prev + 1 holds no point of the cell."""
    N = BT * max([k for k in BNCS if k < cell[2]], default=0) + 1
    mbs = cell_blocks(cell, N)
    return (16 * (min(mbs) - 1) + 1, N) if mbs else None


# block kernel: (m, N, columns' non-zeros) per plan and point; dense = None.  test_block_points_land_in_their_plan holds the
# plan of the matrix that make_block_case builds against block_plan.
BLOCK_POINTS = {
    ("lds-paired", "full"): (96, 512, 2), ("lds-paired", "ragged"): (97, 257, 3),
    ("l2", "full"): (128, 512, None), ("l2", "ragged"): (121, 257, None),
    ("lds-alone", "full"): (128, 512, 4), ("lds-alone", "ragged"): (121, 257, 6),
}


def build_cases():
    """[(family, cell or plan, gram, kind, point, m, N, note)]"""
    out = []
    for cell in CELLS:
        for gram in GRAMS:
            for point, exact in (("full", big_full_point(cell)), ("ragged", big_ragged_point(cell))):
                note = ""
                for key in ((cell, point, gram), (cell, point)):
                    if key in NEAREST:
                        exact, note = NEAREST[key][:2], NEAREST[key][2]
                        break
                for kind in BIG_KINDS:
                    out.append(("big", cell, gram, kind, point, exact[0], exact[1], note))
    for plan, kinds in BLOCK_KINDS.items():
        for point in ("full", "ragged"):
            m, N, _ = BLOCK_POINTS[(plan, point)]
            for kind in kinds:
                out.append(("block", plan, None, kind, point, m, N, ""))
    return out


CASES = build_cases()


def case_id(c):
    if c[0] == "big":
        return "big-%s-%s-%s-%s" % (cell_name(c[1]), c[2], c[3], c[4])
    return "block-%s-%s-%s" % (c[1], c[3], c[4])


def batch(m, N):
    """LPs per case, odd; 7 at the largest sizes: the CPU reference costs ~ m^2 N per iteration and LP."""
    cost = m * m * N
    return 7 if cost > 2e7 else (13 if cost > 2e6 else 19)


def column_structure(m, n, per_col, seed, signed=False):
    """A sparse m x n matrix with ``per_col`` non-zeros in every column at random rows, U[0.05, 1) (signed: times +-1)."""
    rs = np.random.RandomState(seed)
    k = min(m, per_col)
    rows = np.concatenate([rs.choice(m, k, replace=False) for _ in range(n)])
    cols = np.repeat(np.arange(n), k)
    vals = 0.05 + 0.95 * rs.rand(n * k)
    if signed:
        vals *= rs.choice([-1.0, 1.0], n * k)
    return sp.csr_matrix((vals, (rows, cols)), shape=(m, n))


def per_col(m):
    """Non-zeros per column of a term-list case: an eighth of the rows, at least 3 -- entries of M with several terms, far
    below the MP / 2 per column at which the Gram goes to the matrix cores."""
    return max(3, m // 8)


def sparse_equality_lp(m, N, B, per_col_, seed):
    """A sparse EqualityLP without an identity tail around a strictly feasible primal-dual pair (as equality_lp)."""
    A = sp.lil_matrix(column_structure(m, N, per_col_, seed, signed=True))
    rs = np.random.RandomState(seed + 1)
    for i in np.where(np.diff(sp.csr_matrix(A).indptr) == 0)[0]:          # no empty row
        A[int(i), int(rs.randint(N))] = 1.0
    A = sp.csr_matrix(A)
    x0 = rs.rand(B, N) + 0.1
    y0 = rs.randn(B, m)
    b = (A @ x0.T).T
    c = (A.T @ y0.T).T - (rs.rand(B, N) + 0.1)
    b /= np.abs(b).max(axis=1, keepdims=True)
    c /= np.abs(c).max(axis=1, keepdims=True)
    return EqualityLP(SparseMatrix(matrix=A.toarray()), b, c, 0.0)


def big_form(case):
    """'standard' (identity tail) or 'equality' (no tail), alternating over cells, Gram paths and points; 'standard' where the
    equality form would be nearly square (N < 2 m: a feasible set of few dimensions)."""
    _, cell, gram, _, point, m, N, _ = case
    alt = (CELLS.index(cell) + (gram == "terms") + (point == "ragged")) % 2
    return "equality" if alt and N >= 2 * m else "standard"


# Seed rule: a point's batch comes from seed 7000 + 100 * (index of its cell) + 10 * (Gram path) + (ragged) + 1000 * bump,
# bump = the first of 0, 1, 2, ... at which the reference ends every LP of the batch optimal in every kind; bumps other than 0:
SEED_BUMP = {}

_CACHE = {}


def case_seed(case):
    _, cell, gram, _, point = case[:5]
    if case[0] == "big":
        base = 7000 + 100 * CELLS.index(cell) + 10 * GRAMS.index(gram) + (point == "ragged")
    else:
        base = 9000 + 100 * list(BLOCK_KINDS).index(cell) + (point == "ragged")
    return base + 1000 * SEED_BUMP.get((case[0], cell, gram, point), 0)


def make_big_case(case):
    _, cell, gram, _, point, m, N, _ = case
    key = ("big", cell, gram, point)
    if key not in _CACHE:
        B, seed, form = batch(m, N), case_seed(case), big_form(case)
        if form == "equality":
            lp = equality_lp(m, N, B, seed) if gram == "mfma" else sparse_equality_lp(m, N, B, per_col(m), seed)
        elif gram == "mfma":
            A, b, c = problems.random_dense_arrays(m, N - m, B, seed=seed)
            lp = StandardLP(SparseMatrix(matrix=A), b, c, 0.0).to_equality_form()
        else:
            A = column_structure(m, N - m, per_col(m), seed)
            rs = np.random.RandomState(seed + 1)
            b, c = 0.5 + rs.rand(B, m), 0.5 + rs.rand(B, N - m)
            lp = StandardLP(SparseMatrix(matrix=A.toarray()), b, c, 0.0).to_equality_form()
        _CACHE[key] = lp
    return _CACHE[key]


def make_block_case(case):
    _, plan, _, kind, point, m, N, _ = case
    pa = kind.startswith("pa")
    key = ("block", plan, point, pa)
    if key not in _CACHE:
        B, seed, nz = batch(m, N), case_seed(case), BLOCK_POINTS[(plan, point)][2]
        n = N - m
        if nz is None:
            A, b, c = problems.random_dense_arrays(m, n, B, seed=seed)
            lp = StandardLP(SparseMatrix(matrix=A), b, c, 0.0).to_equality_form()
        else:
            A = column_structure(m, n, nz, seed)
            rs = np.random.RandomState(seed + 1)
            b, c = 0.5 + rs.rand(B, m), 0.5 + rs.rand(B, n)
            if pa:
                rows, cols, data = problems.per_problem_values(A, B, seed=seed + 2)
                lp = StandardLP(SparseMatrix(rows, cols, data), b, c, 0.0).to_equality_form()
            else:
                lp = StandardLP(SparseMatrix(matrix=A.toarray()), b, c, 0.0).to_equality_form()
        _CACHE[key] = lp
    return _CACHE[key]


def make_case(case):
    return make_big_case(case) if case[0] == "big" else make_block_case(case)


def structure_of(lp):
    """The equality form's matrix as the handle sees its structure (problem 0's values of a per-problem A)."""
    return sp.csr_matrix(np.asarray(lp.A.todense(0) if lp.A.nproblems > 1 else lp.A.todense()))


def default_is_block(m, N):
    """A dense standard-form A that neither plan of the wavefront-per-LP kernel takes (no dense-image shape covers it or its
    image beside one wave area exceeds the LDS, and its term tables exceed it too): the block kernel serves it without
    PYCLLP_FLAG_BLOCK_KERNEL."""
    img, tab = first_covering("image", WAVE_DA_SHAPES, m, N), first_covering("tables", WAVE_TAB_SHAPES, m, N)
    return not (img and image_waves(m, N, True, img, False)) and (tab is None or tables_cannot_fit(m, N, True, tab, False))


# ---- CPU ------------------------------------------------------------------------------------------------------------------
def _src(name):
    return open(os.path.join(CSRC, name)).read()


def test_constants_and_shape_list_of_the_sources():
    big, bigh, blk, plan = _src("ipm_big.hip"), _src("big.h"), _src("block.h"), _src("big_plan.h")
    line = re.search(r"#define BIG_SHAPES\(X\)(.*)", big).group(1)
    assert [(int(a), int(b)) for a, b in re.findall(r"X\((\d+),\s*(\d+)\)", line)] == BIG_SHAPES
    assert int(re.search(r"constexpr int BT = (\d+);", big).group(1)) == BT
    assert int(re.search(r"constexpr int BIG_MAX_M = (\d+);", bigh).group(1)) == BIG_MAX_M
    assert int(re.search(r"constexpr int BIG_MAX_N = (\d+);", bigh).group(1)) == BIG_MAX_N
    assert [int(re.search(r"#define %s (\d+)" % k, blk).group(1)) for k in ("BLK_T", "BLK_MAX_M", "BLK_MAX_N")] == \
        [BLK_T, BLK_MAX_M, BLK_MAX_N]
    assert max(BNCS) * BT == BIG_MAX_N and BLK_MAX_N == 2 * BLK_T
    # the selection: the first shape with WGPC = the workgroups per CU the LDS allows and n <= BNC * BT; the term cap
    assert re.search(r"v\.wgpc == per_cu && n <= v\.bnc \* BT", big)
    # (the plan's rules: big_plan.h; gram_terms of plan_host.h refuses once more than the cap were visited)
    assert re.search(r"const size_t max_terms = \(size_t\)1 << 24;", plan) and BIG_MAX_TERMS == 1 << 24
    assert re.search(r"if \(!gram_terms<true>\(n, csc, max_terms,[^\n]*\n\s*return 1;", plan)
    assert re.search(r"if \(\+\+count > cap\) return false;", _src("plan_host.h"))
    assert re.search(r"T\.dense = n_terms > 0\.125 \* \(double\)MP \* MP \* nd", plan)
    assert {(w, k) for w in (2, 3) for k in BNCS} == set(BIG_SHAPES)


def test_case_table_covers_exactly_the_reachable_cells():
    cells = reachable_cells()
    assert cells == set(CELLS) and len(CELLS) == 10
    want = {(cell, g, k, p) for cell in cells for g in GRAMS for k in BIG_KINDS for p in ("full", "ragged")}
    have = [c[1:5] for c in CASES if c[0] == "big"]
    assert len(have) == len(set(have)) and set(have) == want
    wantb = {(plan, k, p) for plan, kinds in BLOCK_KINDS.items() for k in kinds for p in ("full", "ragged")}
    haveb = [(c[1], c[3], c[4]) for c in CASES if c[0] == "block"]
    assert len(haveb) == len(set(haveb)) and set(haveb) == wantb
    n_big = len(CELLS) * len(GRAMS) * len(BIG_KINDS)
    n_block = sum(len(k) for k in BLOCK_KINDS.values())
    assert (n_big, n_block) == (80, 10) and len(CASES) == 2 * (n_big + n_block)


def test_no_reachable_size_leaves_one_workgroup_per_cu():
    """... so ipm_big_kernel has no instantiation for it: every plan runs two or three workgroups per CU, and the factor sits
    in LDS only for m <= 96."""
    for MB in range(1, BIG_MAX_M // 16 + 1):
        for N in range(1, BIG_MAX_N + 1):
            cell, lds, per_cu = big_plan(MB, N)
            assert per_cu in (2, 3) and 2 * lds <= MAX_LDS, (MB, N)
            assert (cell[1], cell[2]) in BIG_SHAPES
            assert cell[0] == "W" or MB <= 6, (MB, N)
    assert big_plan(6, 513)[0][0] == "L" and big_plan(7, 2)[0][0] == "W"


def test_every_point_lands_in_its_cell():
    for case in CASES:
        family, cell, gram, kind, point, m, N, note = case
        if family != "big":
            continue
        assert reachable(m, N), case_id(case)
        assert big_plan((m + 15) // 16, N)[0] == cell, case_id(case)
        exact = big_full_point(cell) if point == "full" else big_ragged_point(cell)
        assert (m, N) == exact or (cell, point) in NEAREST or (cell, point, gram) in NEAREST, case_id(case)
        if point == "full":
            assert m % 16 == 0 and N == BT * cell[2]                     # every row live, every column register full
        else:
            assert (N - 1) % BT == 0 or (cell, point) in NEAREST          # one live column in the last register
            assert (m - 1) % 16 == 0 or (cell, point, gram) in NEAREST    # one live row in the last block
        lp = make_case(case)
        A, tail = structure_of(lp), big_form(case) == "standard"
        assert (lp.nrows, lp.ncols) == (m, N) == A.shape
        if tail:
            assert (A[:, N - m:] != sp.identity(m)).nnz == 0
        assert gram_is_dense(A, tail) == (gram == "mfma"), case_id(case)
        assert gram == "mfma" or gram_terms(A) <= BIG_MAX_TERMS
    forms = {(c[2], big_form(c)) for c in CASES if c[0] == "big"}
    assert forms == {(g, f) for g in GRAMS for f in ("standard", "equality")}


def test_nearest_points_are_the_nearest():
    for key, (m, N, _) in NEAREST.items():
        cell, point = key[0], key[1]
        assert point == "ragged"
        if len(key) == 2:
            # no point of the cell at N = 1 ... and none at any N below the one taken; there, the fewest blocks
            assert big_ragged_point(cell) is None
            assert not any(cell_blocks(cell, NN) for NN in range(1, N))
            assert m == 16 * (min(cell_blocks(cell, N)) - 1) + 1
        else:
            # the exact point exists but its Gram takes the term list, as does every m below the one taken
            em, eN = big_ragged_point(cell)
            assert eN == N and em == 1 and big_plan(1, N)[0] == cell
            for mm in range(1, m + 1):
                A = sp.csr_matrix(np.hstack([np.ones((mm, N - mm)), np.eye(mm)]))
                assert gram_is_dense(A, True) == (mm == m), mm
                assert gram_is_dense(sp.csr_matrix(np.ones((mm, N))), False) == (mm == m), mm


def test_block_plan_rule_and_reachable_plans():
    """Without per-problem values `base` never passes half the LDS (m <= 128, N <= 512), so the rule's third branch -- A in LDS,
    the workgroup alone -- is reached by per-problem values only, which force A into LDS at any size that fits."""
    for m in range(1, BLK_MAX_M + 1):
        mp8 = (m + 7) & ~7
        base = 8 * (m * (m + 1) // 2 + 1 + 2 * (BLK_MAX_N + 1) + 7 * mp8 + 8)
        assert base <= MAX_LDS // 2
    plans = set()
    for m in (1, 40, 96, 128):
        for n in (m + 1, 257, 512):
            for nnz in (m, 3 * n, 2000, 4000, m * n):
                plans.add(block_plan(m, n, nnz)[0])
                assert block_plan(m, n, nnz)[3] >= 2
    assert plans == {"lds-paired", "l2"}
    assert block_plan(128, 512, 1500, pa=True)[0] == "lds-alone" and block_plan(128, 512, 128 * 384, pa=True) is None


def test_block_points_land_in_their_plan():
    for case in CASES:
        family, plan, _, kind, point, m, N, _ = case
        if family != "block":
            continue
        lp = make_case(case)
        A = structure_of(lp)
        assert A.shape == (m, N) and m <= BLK_MAX_M and N <= BLK_MAX_N
        got = block_plan(m, N, A.nnz, pa=kind.startswith("pa"))
        assert got is not None and got[0] == plan, (case_id(case), got)
        assert N == (512 if point == "full" else 257) and m % 8 == (0 if point == "full" else 1)
        if plan == "l2":
            assert default_is_block(m, N)


def test_case_inputs_keep_autoscale_off():
    from pycllp_amd.solvers.hip import autoscale_wanted
    for case in CASES:
        if case[3] == "newton":
            continue
        lp = make_case(case)
        assert not autoscale_wanted(lp.b, lp.c), case_id(case)


# ---- GPU ------------------------------------------------------------------------------------------------------------------
def solver_for(case, **extra):
    from pycllp_amd.solvers import solver_registry
    family, gram, kind = case[0], case[2], case[3]
    opts = dict(hsd=kind.endswith("hsd"), predcorr=kind == "pc", autoscale=False, **extra)
    if family == "big":
        name = "hip_dense_primal_normal" if gram == "mfma" else "hip_sparse_primal_normal"
    else:
        name = "hip_sparse_primal_normal"
        if case[1] != "l2":
            opts["flags"] = FLAG_BLOCK_KERNEL           # ('l2': dense, m > 112 -- the block kernel is the default there)
    return solver_registry[name](device="cuda:0", **opts)


def assert_served_by(info, case, lp, grid=None):
    family, m, N = case[0], case[5], case[6]
    assert "wave_shape" not in info and "group_shape" not in info, info
    if family == "big":
        cell, lds, _ = big_plan((m + 15) // 16, N)
        assert cell == case[1]
        assert info.get("kernel") == "big" and info["variant"] == ("MFMA Gram" if case[2] == "mfma" else "term list"), info
        assert info.get("big_shape") == (cell[1], cell[2]) and info.get("factor_in_lds") == (cell[0] == "L"), info
        assert "a_in_lds" not in info and info["lds_bytes"] == lds and info["block"] == BT, info
    else:
        plan, a, lds, _ = block_plan(m, N, structure_of(lp).nnz, pa=case[3].startswith("pa"))
        assert plan == case[1]
        assert info.get("kernel") == "block" and info["variant"] == "block", info
        assert info.get("a_in_lds") == a and "big_shape" not in info and "factor_in_lds" not in info, info
        assert info["lds_bytes"] == lds and info["block"] == BLK_T, info
    if grid is not None:
        assert info["grid"] == grid, info


@pytest.mark.gpu
@pytest.mark.parametrize("case", CASES, ids=[case_id(c) for c in CASES])
def test_plan_matches_its_reference(case):
    from test_hip_parity import oracle_on
    kind = case[3]
    lp = make_case(case)
    s = solver_for(case)
    if kind == "newton":
        return newton_matches(s, lp, batch(case[5], case[6]), lambda info: assert_served_by(info, case, lp))
    lp.init(s)
    lp.solve(s)
    assert_served_by(s.launch_info(), case, lp, grid=lp.nproblems)
    r = oracle_each(lp, ORACLE_FLAGS[kind]) if kind.startswith("pa") else oracle_on(lp, auto=False, flags=ORACLE_FLAGS[kind])
    assert_matches(s, r, lp)


def one_cu_worth(case):
    """(workgroups per CU of the case's plan, reserve_cus that leaves one CU)"""
    import torch
    m, N = case[5], case[6]
    if case[0] == "big":
        per_cu = big_plan((m + 15) // 16, N)[2]
    else:
        per_cu = block_plan(m, N, structure_of(make_case(case)).nnz, pa=case[3].startswith("pa"))[3]
    return per_cu, torch.cuda.get_device_properties(0).multi_processor_count - 1


def widen(lp, B):
    """The LP batch grown to B LPs (B <= 2 nproblems) on the shared A: the added ones are the first ones with b and c each
    scaled by a factor of their own in [0.9, 1) -- feasible and bounded as they are, in either form."""
    rs = np.random.RandomState(5)
    k = B - lp.nproblems
    b = np.vstack([lp.b, lp.b[:k] * (0.9 + 0.1 * rs.rand(k, 1))])
    c = np.vstack([lp.c, lp.c[:k] * (0.9 + 0.1 * rs.rand(k, 1))])
    return EqualityLP(lp.A, b, c, 0.0)


RESULT_ARRAYS = ("x", "y", "z", "primal_obj", "dual_obj", "status", "iters")

# one point per cell (Gram paths and kinds in turn) and per block plan
SECOND_LP_CASES = [c for c in CASES if c[4] == "full" and (
    (c[0] == "big" and c[2] == GRAMS[CELLS.index(c[1]) % 2] and c[3] == ("plain", "hsd", "pc")[CELLS.index(c[1]) % 3])
    or (c[0] == "block" and c[3] == {"lds-paired": "hsd", "l2": "plain", "lds-alone": "pa"}[c[1]]))]


def test_second_lp_cases_cover_every_cell_and_plan():
    assert [c[1] for c in SECOND_LP_CASES if c[0] == "big"] == CELLS
    assert [c[1] for c in SECOND_LP_CASES if c[0] == "block"] == list(BLOCK_KINDS)
    assert {c[2] for c in SECOND_LP_CASES if c[0] == "big"} == set(GRAMS)


@pytest.mark.gpu
@pytest.mark.parametrize("case", SECOND_LP_CASES, ids=[case_id(c) for c in SECOND_LP_CASES])
def test_second_lp_of_a_workgroup_gives_the_same_bits(case):
    """The batch on the default grid (one LP per workgroup) and on one CU's worth of workgroups, where every workgroup takes at
    least three LPs in turn from the queue: whatever an LP leaves in LDS, the workspace or registers must not reach the next."""
    per_cu, reserve = one_cu_worth(case)
    lp = make_case(case)
    B = 3 * per_cu + 1 + (per_cu % 2)                # odd
    if case[3].startswith("pa"):
        assert lp.nproblems >= B
        rows, cols = np.asarray(lp.A._rows), np.asarray(lp.A._cols)
        lp = EqualityLP(SparseMatrix(rows, cols, np.asarray(lp.A.data)[:B]), lp.b[:B], lp.c[:B], 0.0)
    else:
        lp = widen(lp, B) if B > lp.nproblems else EqualityLP(lp.A, lp.b[:B], lp.c[:B], 0.0)
    runs = []
    for extra, grid in ((dict(), B), (dict(reserve_cus=reserve), per_cu)):
        s = solver_for(case, **extra)
        lp.init(s)
        lp.solve(s)
        assert_served_by(s.launch_info(), case, make_case(case), grid=grid)
        runs.append({k: np.array(getattr(s, k)) for k in RESULT_ARRAYS})
    assert B >= 3 * per_cu + 1 and (runs[0]["status"] == 0).all()
    for k in RESULT_ARRAYS:
        np.testing.assert_array_equal(runs[0][k], runs[1][k], err_msg=k)


def mixed_batch(m, n, nz, seed):
    """Seven LPs on one A (standard form, m x n; ``nz`` non-zeros per column, None = dense): LP 2 infeasible (a row a'x <= -1
    with a >= 0, not all zero), LP 4 unbounded (column 5 of A is structurally there but 1e-300: no row bounds it, and only LP 4
    gains from it), the others optimal -- built as test_large_lp_newton_step_and_statuses builds them."""
    rs = np.random.RandomState(seed)
    A = rs.rand(m, n) if nz is None else column_structure(m, n, nz, seed).toarray()
    A[:, 5] = 0.0
    A[0, 5] = 1e-300
    b, c = 0.5 + rs.rand(7, m), 0.5 + rs.rand(7, n)
    c[:, 5] = -c[:, 5]
    c[4, 5] = 1.0
    row = int(np.argmax((A[:, :5] > 0).sum(axis=1) + (A[:, 6:] > 0).sum(axis=1)))
    b[2, row] = -1.0
    return StandardLP(SparseMatrix(matrix=A), b, c, 0.0).to_equality_form()


# (kernel, cell or plan, plugin, m, n of the standard form, non-zeros per column, flags)
MIXED = [("big", ("W", 3, 2), "hip_dense_primal_normal", 160, 60, None, 0),
         ("big", ("L", 3, 3), "hip_dense_primal_normal", 60, 640, None, 0),
         ("big", ("L", 2, 5), "hip_sparse_primal_normal", 80, 1000, 8, 0),
         ("block", "l2", "hip_sparse_primal_normal", 121, 136, None, 0),
         ("block", "lds-paired", "hip_sparse_primal_normal", 90, 200, 3, FLAG_BLOCK_KERNEL)]


def test_mixed_batches_land_in_their_plans():
    for family, where, name, m, n, nz, flags in MIXED:
        A = structure_of(mixed_batch(m, n, nz, 11))
        if family == "big":
            assert reachable(m, m + n) and big_plan((m + 15) // 16, m + n)[0] == where
            assert gram_is_dense(A, True) == (name == "hip_dense_primal_normal")
        else:
            assert block_plan(m, m + n, A.nnz)[0] == where
            assert flags or default_is_block(m, m + n)


@pytest.mark.gpu
@pytest.mark.parametrize("mixed", MIXED, ids=["%s-%s" % (c[0], c[1] if c[0] == "block" else cell_name(c[1])) for c in MIXED])
def test_non_optimal_exits_leave_nothing_behind(mixed):
    """hsd=True on a batch where an infeasible and an unbounded LP sit between optimal ones: the reference's statuses, the
    certificates, and the same bits whether the LPs run one per workgroup, all through one CU's worth of workgroups (each takes
    several in turn, optimal ones after non-optimal ones), or each alone."""
    import torch
    from pycllp_amd.solvers import solver_registry
    from test_hip_parity import oracle_on
    family, where, name, m, n, nz, flags = mixed
    lp = mixed_batch(m, n, nz, 11)
    N, B = m + n, lp.nproblems
    if family == "big":
        per_cu = big_plan((m + 15) // 16, N)[2]
    else:
        per_cu = block_plan(m, N, structure_of(lp).nnz)[3]
    reserve = torch.cuda.get_device_properties(0).multi_processor_count - 1
    runs = []
    for extra, grid in ((dict(), B), (dict(reserve_cus=reserve), min(per_cu, B))):
        s = solver_registry[name](device="cuda:0", hsd=True, autoscale=False, flags=flags, **extra)
        lp.init(s)
        lp.solve(s)
        info = s.launch_info()
        assert info["kernel"] == family and info["grid"] == grid, info
        if family == "big":
            assert (info["factor_in_lds"], info["big_shape"]) == (where[0] == "L", where[1:]), info
        else:
            assert info["a_in_lds"] == (where != "l2"), info
        runs.append({k: np.array(getattr(s, k)) for k in RESULT_ARRAYS})
    r = oracle_on(lp, auto=False, flags=32)
    np.testing.assert_array_equal(runs[0]["status"], r["status"])
    assert list(r["status"]) == [0, 0, 2, 0, 4, 0, 0]
    check_certificates(np.asarray(lp.A.todense()), lp.b, lp.c, runs[0])
    ok = r["status"] == 0
    np.testing.assert_allclose(runs[0]["primal_obj"][ok], r["pobj"][ok], rtol=1e-9, atol=1e-9)
    for k in RESULT_ARRAYS:
        np.testing.assert_array_equal(runs[0][k], runs[1][k], err_msg=k)
    for i in range(B):                                   # each LP alone, on a handle of its own
        one = EqualityLP(lp.A, lp.b[i:i + 1], lp.c[i:i + 1], 0.0)
        s = solver_registry[name](device="cuda:0", hsd=True, autoscale=False, flags=flags)
        one.init(s)
        one.solve(s)
        for k in RESULT_ARRAYS:
            np.testing.assert_array_equal(np.array(getattr(s, k))[0], runs[0][k][i], err_msg="%s of LP %d" % (k, i))


@pytest.mark.gpu
def test_block_kernel_refuses_predcorr():
    """No predictor-corrector on the block kernel: by flag, and where it is the default (dense, m > 112)."""
    from pycllp_amd.solvers import solver_registry
    for case in (c for c in CASES if c[0] == "block" and c[3] == "plain" and c[4] == "ragged"):
        lp = make_case(case)
        flags = FLAG_BLOCK_KERNEL if case[1] != "l2" else 0
        s = solver_registry["hip_sparse_primal_normal"](device="cuda:0", predcorr=True, hsd=False, autoscale=False, flags=flags)
        lp.init(s)
        with pytest.raises(NotImplementedError):
            lp.solve(s)
