"""Every compiled instantiation of the wavefront-per-LP kernel (csrc/ipm_wreg_*.hip; shape lists WREG_TAB_SHAPES and
WREG_DA_SHAPES of csrc/wreg.h) and of the lane-group kernels (GROUP_SHAPES of csrc/group_pa.h) against the CPU references.

Each shape is solved at two points of the region it serves first: FULL, its corner (every row and lane live), and RAGGED, one
row past the previous 16-row block and one column past the previous 64-column register (the last block and the last register
hold one live row / column; lane groups: one past the previous shape's MP and NP).  CPU: the case table covers exactly
{shape x kind} of the lists in the sources, and the first-covering rule puts every point on its shape.  GPU: every case first
asserts the instantiation that served it (``launch_info()``), then compares with its reference."""
import os
import re
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest

import bounded_twin
from conftest import ROOT, rel_err
from pycllp_amd import problems
from pycllp_amd.lp import EqualityLP, GeneralLP, SparseMatrix, StandardLP
from test_general_solver import check_kkt, make_general
from test_sparse_general_solver import make_sparse_general

CSRC = os.path.join(ROOT, "pycllp_amd", "csrc")

# ---- the shape lists, as this file knows them (the CPU tests hold them against the sources) ---------------------------------
WAVE_TAB_SHAPES = [(1, 4), (2, 4), (3, 4), (4, 2), (4, 4), (5, 6), (6, 6), (7, 6), (8, 4), (8, 6), (8, 8)]
WAVE_DA_SHAPES = [(1, 4), (2, 4), (3, 4), (4, 2), (4, 4), (5, 4), (6, 4), (7, 4), (8, 4), (8, 6)]
GROUP_SHAPES = [(16, 32), (16, 48), (16, 64), (32, 64), (32, 96), (32, 128)]

# kinds per family: the launcher tables of csrc/wreg.h (kWTab, kWPA, kWPC, kWPCPA, kWBD / kWDA, kWPCDA, kWBDDA) and the
# Variant / SlackVariant tables of csrc/ipm_dense.hip (declared in csrc/dense_tab.h; the C ABI that uses them is csrc/abi_dense.hip)
KINDS = {
    "tables": ("plain", "hsd", "newton", "pc", "pa", "pa-hsd", "pa-pc", "bounded"),
    "image": ("plain", "hsd", "newton", "pc", "bounded"),
    "group": ("plain", "hsd", "pc", "newton"),
    "slack": ("plain", "hsd", "pc", "bounded"),
}
SHAPES = {"tables": WAVE_TAB_SHAPES, "image": WAVE_DA_SHAPES, "group": GROUP_SHAPES, "slack": GROUP_SHAPES}
MAX_LDS = 160 * 1024

# Points a kind cannot reach, with the nearest one it can and why: (family, shape, point[, kind]) -> (m, N, note); m counts
# the kept rows of a bounded case.  test_nearest_points_are_the_nearest holds them against the plan rules.
_DA86 = ("m > 112 rows: the image beside one wave area exceeds 160 KB of LDS (such LPs run on the block kernel); the most rows "
         "whose image fits, at N = %d%s")
NEAREST = {
    ("image", (1, 4), "ragged"): (12, 193, "a single row has no Gram term, so its term tables always fit: the dense image "
                                           "needs m >= 12 at N = 193 (tables_cannot_fit)"),
    ("image", (8, 6), "full"): (48, 384, _DA86 % (384, "")),
    ("image", (8, 6), "ragged"): (97, 257, _DA86 % (257, ", one live row in the last live block")),
    ("image", (8, 6), "full", "bounded"): (40, 384, _DA86 % (384, " (t and s make the wave area larger)")),
    ("image", (8, 6), "ragged", "bounded"): (81, 257, _DA86 % (257, ", one live row in the last live block")),
    ("group", (16, 32), "ragged"): (1, 2, "N = 1 is no LP with a column to spare: m = 1, N = 2"),
}
# bounded cases whose size leaves out some of: fixed columns, columns without a bound, every row kind
BOUNDED_NOTES = {1: "one kept row: row kinds '<=' and free only", 2: "n = 1: no fixed column"}


def full_point(family, shape):
    if family in ("tables", "image"):
        return 16 * shape[0], 64 * shape[1]
    return shape


def _prev(values, v):
    return max([w for w in values if w < v], default=0)


def ragged_point(family, shape):
    if family in ("tables", "image"):
        return 16 * (shape[0] - 1) + 1, 64 * (shape[1] - 1) + 1
    mp, np_ = shape
    m = _prev({s[0] for s in GROUP_SHAPES}, mp) + 1
    if family == "group":
        return m, _prev({s[1] for s in GROUP_SHAPES}, np_) + 1
    # slack kernels: the analogue on the dense columns N - m (capacity NP - MP)
    return m, m + _prev({s[1] - s[0] for s in GROUP_SHAPES}, np_ - mp) + 1


def build_cases():
    """[(family, shape, kind, point, m, N, note)]: every shape x kind at its full and ragged point."""
    out = []
    for family, shapes in SHAPES.items():
        for shape in shapes:
            for kind in KINDS[family]:
                for point, (m, N) in (("full", full_point(family, shape)), ("ragged", ragged_point(family, shape))):
                    note = ""
                    for key in ((family, shape, point, kind), (family, shape, point)):
                        if key in NEAREST:
                            m, N, note = NEAREST[key]
                            break
                    if kind == "bounded":
                        n = N - m
                        note = "; ".join([note] + [v for k, v in BOUNDED_NOTES.items() if (m if k == 1 else n) == 1]).strip("; ")
                    out.append((family, shape, kind, point, m, N, note))
    return out


CASES = build_cases()


def case_id(c):
    return "%s-%s-%dx%d-%s" % (c[0], c[2], c[1][0], c[1][1], c[3])


# ---- restatements of the plan rules ---------------------------------------------------------------------------------------
def source_list(fname, macro):
    text = open(os.path.join(CSRC, fname)).read()
    if macro == "GROUP_SHAPES":          # the default branch (the others are development builds of one shape)
        line = re.search(r"#else\s*\n#define GROUP_SHAPES\(X\)(.*)", text).group(1)
    else:
        line = re.search(r"#define %s\(X\)(.*)" % macro, text).group(1)
    return [(int(a), int(b)) for a, b in re.findall(r"X\((\d+),\s*(\d+)\)", line)]


def first_covering(family, shapes, m, N):
    for s in shapes:
        if family in ("tables", "image"):
            if m <= 16 * s[0] and N <= 64 * s[1]:
                return s
        elif family == "group":
            if m <= s[0] and N <= s[1]:
                return s
        elif m <= s[0] and N - m <= s[1] - s[0]:
            return s
    return None


def wave_doubles(mb, nq, bounded):
    """LDS doubles of one wave's area (wreg.h WGeo::WAVE_D, + t and s of the bounded kernel)."""
    stage = max(192 * nq, 768) + 272
    return stage + 64 * nq + 5 * 16 * mb + 144 * mb + (2 * 64 * nq if bounded else 0)


def image_waves(m, N, tail, shape, bounded):
    """Waves per workgroup of the dense-image plan (wreg_plan.h wreg_image_plan), 0 when the image does not fit."""
    nd = N - m if tail else N
    img = 8 * ((m + 7) // 8 * 8) * (((max(nd, 1) + 15) // 16) * 16 + 1)
    return max([w for w in (1, 2, 3, 4) if img + 16 + 8 * w * wave_doubles(*shape, bounded) <= MAX_LDS], default=0)


def tables_cannot_fit(m, N, tail, shape, bounded):
    """A lower bound of the term-table plan's LDS for a dense A exceeds the LDS: CSR values, the Gram terms (weight + column /
    destination) and the fewest wave areas the plan may take (4; the bounded plan goes down to 1)."""
    nd = N - m if tail else N
    nnz = m * nd + (m if tail else 0)
    terms = nd * m * (m - 1) // 2
    return 8 * nnz + 12 * terms + 8 * (1 if bounded else 4) * wave_doubles(*shape, bounded) > MAX_LDS


def image_form(case):
    """'standard' (identity tail kept out of the image) or 'equality' (no tail): alternating over shapes and points where the
    image of the equality form fits, else 'standard'.  Bounded forms always have the tail."""
    family, shape, kind, point, m, N, _ = case
    if kind == "bounded":
        return "standard"
    alt = (WAVE_DA_SHAPES.index(shape) + (point == "ragged")) % 2
    return "equality" if alt and image_waves(m, N, False, shape, False) else "standard"


# ---- CPU ------------------------------------------------------------------------------------------------------------------
def test_case_table_covers_every_shape_and_kind_of_the_sources():
    lists = {"tables": source_list("wreg.h", "WREG_TAB_SHAPES"), "image": source_list("wreg.h", "WREG_DA_SHAPES"),
             "group": source_list("group_pa.h", "GROUP_SHAPES"), "slack": source_list("group_pa.h", "GROUP_SHAPES")}
    for family, shapes in lists.items():
        assert shapes == SHAPES[family], (family, shapes)
        want = {(s, k, p) for s in shapes for k in KINDS[family] for p in ("full", "ragged")}
        have = [(c[1], c[2], c[3]) for c in CASES if c[0] == family]
        assert len(have) == len(set(have)) and set(have) == want, family
    n_wave = sum(len(lists[f]) * len(KINDS[f]) for f in ("tables", "image"))
    n_group = sum(len(lists[f]) * len(KINDS[f]) for f in ("group", "slack"))
    assert (n_wave, n_group) == (138, 48)


def test_every_point_is_served_first_by_its_shape():
    for family, shape, kind, point, m, N, note in CASES:
        assert first_covering(family, SHAPES[family], m, N) == shape, (family, shape, kind, point, m, N)
        exact = (full_point if point == "full" else ragged_point)(family, shape)
        assert (m, N) == exact or (family, shape, point) in NEAREST
        if point == "ragged" and family in ("tables", "image"):
            assert (N - 1) % 64 == 0                                          # one live column in the last register
            assert (m - 1) % 16 == 0 or (family, shape, point) in NEAREST      # one live row in the last block
        assert N > m


def test_dense_image_points_fit_the_image_and_not_the_tables():
    for case in CASES:
        family, shape, kind, point, m, N, _ = case
        if family != "image":
            continue
        tail = image_form(case) == "standard"
        assert image_waves(m, N, tail, shape, kind == "bounded") >= 1, case_id(case)
        assert tables_cannot_fit(m, N, tail, shape, kind == "bounded"), case_id(case)
    # the nearest point is the nearest: one row fewer and the tables may fit
    m, N, _ = NEAREST[("image", (1, 4), "ragged")]
    assert not tables_cannot_fit(m - 1, N, True, (1, 4), True)


def test_nearest_points_are_the_nearest():
    """The exact point of every dense-image entry of NEAREST reaches no dense-image plan, and neither does one row more than
    the point taken (16 on a ragged point)."""
    for key, (m, N, _) in NEAREST.items():
        if key[0] != "image":
            continue
        shape, point = key[1], key[2]
        # the kinds the entry serves: bounded (t and s per wave) or not
        served = [True] if key[3:] == ("bounded",) else [False] if key + ("bounded",) in NEAREST else [False, True]

        def reachable(mm, NN, bounded):
            return any(image_waves(mm, NN, tail, shape, bounded) and tables_cannot_fit(mm, NN, tail, shape, bounded)
                       for tail in (True, False) if NN > mm)
        em, eN = (full_point if point == "full" else ragged_point)("image", shape)
        nearer = m + (16 if point == "ragged" else 1) if em > m else m - 1
        assert all(reachable(m, N, bd) for bd in served), key
        assert not any(reachable(em, eN, bd) for bd in served), key
        assert not all(reachable(nearer, N, bd) for bd in served), key


def test_case_inputs_keep_autoscale_off():
    from pycllp_amd.solvers.hip import autoscale_wanted
    for case in CASES:
        if case[2] == "newton":
            continue
        lp = make_case(case)
        if case[2] == "bounded":
            blp, _ = lp.to_bounded_equality_form()
            assert blp.nrows == case[4] and blp.ncols == case[5], case_id(case)
            assert not autoscale_wanted(blp.b, blp.c, blp.u), case_id(case)
            if case[4] > 1:
                assert (blp.u == 0).any() and np.isinf(blp.u).any(), case_id(case)
        else:
            assert (lp.nrows, lp.ncols) == (case[4], case[5]), case_id(case)
            assert not autoscale_wanted(lp.b, lp.c), case_id(case)


# ---- case inputs ----------------------------------------------------------------------------------------------------------
def batch(m):
    """LPs per case: not a multiple of the waves per workgroup; fewer at the largest shapes (the CPU references dominate)."""
    return 19 if m > 96 else 37


def equality_lp(m, N, B, seed):
    """A dense EqualityLP without an identity tail around a strictly feasible primal-dual pair, b and c of max-norm 1."""
    rs = np.random.RandomState(seed)
    A = rs.randn(m, N) / np.sqrt(N)
    x0 = rs.rand(B, N) + 0.1
    y0 = rs.randn(B, m)
    b = x0 @ A.T
    c = y0 @ A - (rs.rand(B, N) + 0.1)
    b /= np.abs(b).max(axis=1, keepdims=True)
    c /= np.abs(c).max(axis=1, keepdims=True)
    return EqualityLP(SparseMatrix(matrix=A), b, c, 0.0)


def bounded_kinds(mk):
    """mk kept rows -- row 0 '<=', then '=', ranged, '<=', '>=' in turn -- and a row without bounds after every fourth."""
    kinds = []
    for i in range(mk):
        kinds.append("le" if i == 0 else ("eq", "rng", "le", "ge")[(i - 1) % 4])
        if i % 4 == 0:
            kinds.append("free")
    return kinds


def banded(glp):
    """The same LPs with rows of A (and their bounds) scaled so that the bounded form's right-hand sides stay within 2, and c
    of max-norm 1."""
    A = glp.A.todense()
    Al = glp.l @ A.T
    with np.errstate(invalid="ignore"):
        r = np.maximum(np.where(np.isfinite(glp.b), np.abs(glp.b - Al), 0.0).max(axis=0),
                       np.where(np.isfinite(glp.a), np.abs(glp.a - Al), 0.0).max(axis=0))
    s = 2.0 / np.maximum(r, 2.0)
    c = glp.c / np.abs(glp.c).max(axis=1, keepdims=True)
    return GeneralLP(SparseMatrix(matrix=A * s[:, None]), glp.b * s[None, :], c, a=glp.a * s[None, :], l=glp.l, u=glp.u, f=glp.f)


def table_density(m, N):
    """Sparse enough for the term tables beside four wave areas: above N = 384 those take 128 KB of the 160 KB."""
    return 0.004 if N > 384 else max(0.02, min(0.2, 2.0 / m))


def table_structure(m, n, seed):
    return problems.random_sparse_arrays(m, n, 1, density=table_density(m, m + n), seed=seed)[0]


_CACHE = {}


def make_case(case):
    """The LP batch of a case (shared by the kinds that solve the same LPs)."""
    family, shape, kind, point, m, N, _ = case
    seed = 1000 * shape[0] + 10 * shape[1] + (point == "ragged")
    B = batch(m)
    if kind == "bounded":
        key = (family, shape, point, "bounded")
        if key not in _CACHE:
            kinds, n = bounded_kinds(m), N - m
            fixed = min(2, n - 1)
            if family == "tables":
                glp = make_sparse_general(len(kinds), n, B, seed, density=table_density(m, N), fixed=fixed, mixed_u=True,
                                          kinds=kinds)
            else:
                glp = make_general(len(kinds), n, B, seed, kinds=kinds, fixed=fixed, mixed_u=True)
            _CACHE[key] = banded(glp)
        return _CACHE[key]
    pa = kind.startswith("pa")
    key = (family, shape, point, pa)
    if key not in _CACHE:
        n = N - m
        if family == "tables":
            A = table_structure(m, n, seed)
            rs = np.random.RandomState(seed + 1)
            b, c = 0.5 + rs.rand(B, m), 0.5 + rs.rand(B, n)
            if pa:
                rows, cols, data = problems.per_problem_values(A, B, seed=seed + 2)
                lp = StandardLP(SparseMatrix(rows, cols, data), b, c, 0.0).to_equality_form()
            else:
                lp = StandardLP(SparseMatrix(matrix=A), b, c, 0.0).to_equality_form()
        elif family == "image":
            if image_form(case) == "equality":
                lp = equality_lp(m, N, B, seed)
            else:
                A, b, c = problems.random_dense_arrays(m, n, B, seed=seed)
                lp = StandardLP(SparseMatrix(matrix=A), b, c, 0.0).to_equality_form()
        elif point == "ragged" and family == "group":
            lp = equality_lp(m, N, B, seed)                      # the general kernels: no identity tail
        else:
            A, b, c = problems.random_dense_arrays(m, n, B, seed=seed)
            lp = StandardLP(SparseMatrix(matrix=A), b, c, 0.0).to_equality_form()
        _CACHE[key] = lp
    return _CACHE[key]


# ---- GPU ------------------------------------------------------------------------------------------------------------------
ORACLE_FLAGS = {"plain": 0, "hsd": 32, "pc": 128, "pa": 0, "pa-hsd": 32, "pa-pc": 128}


def solver_for(case):
    from pycllp_amd.solvers import solver_registry
    family, kind = case[0], case[2]
    if kind == "bounded":
        name = "hip_general_primal_normal" if family == "slack" else "hip_sparse_general_primal_normal"
        return solver_registry[name](device="cuda:0", hsd=False)
    name = "hip_dense_primal_normal" if family in ("group", "slack") else "hip_sparse_primal_normal"
    opts = dict(hsd=kind.endswith("hsd"), predcorr=kind.endswith("pc"), autoscale=False)
    if family == "group":
        opts["flags"] = 16                        # PYCLLP_FLAG_NO_SLACK_PATH: the general kernels on an identity tail too
    return solver_registry[name](device="cuda:0", **opts)


def assert_served_by(info, case):
    family, shape = case[0], case[1]
    if family in ("tables", "image"):
        assert info.get("kernel") == "wave" and info.get("wave_shape") == shape, info
        assert info["variant"] == ("tables" if family == "tables" else "dense image"), info
        assert "group_shape" not in info and "slack" not in info, info
    else:
        assert info.get("group_shape") == shape and info.get("slack") == (1 if family == "slack" else 0), info
        assert (info["m_pad"], info["n_pad"]) == shape and "wave_shape" not in info and "kernel" not in info, info


def oracle_each(lp, flags):
    """The oracle on every LP with its own matrix (per-problem values of A)."""
    from oracle import port
    B = lp.nproblems
    with ThreadPoolExecutor(8) as ex:
        rs = list(ex.map(lambda k: port.dense_solve(lp.A.todense(k), lp.b[k:k + 1], lp.c[k:k + 1], flags=flags), range(B)))
    return {key: np.concatenate([r[key] for r in rs]) for key in rs[0]}


def assert_matches(s, r, lp):
    """Statuses, iterations, objectives and x against the reference ``r``, then the residuals of the returned vectors."""
    np.testing.assert_array_equal(s.status, r["status"])
    assert (s.status == 0).all()
    assert np.abs(s.iters.astype(int) - r["iters"]).max() <= 1, (s.iters, r["iters"])
    assert rel_err(s.primal_obj, r["pobj"]).max() <= 1e-9 and rel_err(s.dual_obj, r["dobj"]).max() <= 1e-9
    np.testing.assert_allclose(s.x, r["x"], rtol=1e-5, atol=1e-6)
    for k in range(lp.nproblems):
        A = lp.A.todense(k if lp.A.nproblems > 1 else 0)
        x, y, z, b, c = s.x[k], s.y[k], s.z[k], lp.b[k], lp.c[k]
        assert x.min() >= 0 and z.min() >= 0, k
        assert np.abs(A @ x - b).max() <= 1e-7 * (1 + np.abs(b).max()), k
        assert np.abs(A.T @ y - z - c).max() <= 1e-7 * (1 + np.abs(c).max()), k
        assert abs(c @ x - b @ y) <= 1e-7 * (1 + abs(c @ x)), k


def newton_matches(s, lp, B, served):
    """The stand-alone Newton step of solver ``s`` on B random interior states of ``lp``'s matrix against the oracle's step and
    the known-answer formula; ``served(launch_info)`` asserts what ran."""
    from oracle import port
    lp.init(s)
    A = lp.A.todense()
    m, N = A.shape
    rs = np.random.RandomState(7)
    x, z = 0.5 + rs.rand(B, N), 0.5 + rs.rand(B, N)
    y, b, c = rs.rand(B, m), rs.rand(B, m), rs.rand(B, N)
    dy = s.newton_step(x, z, y, b, c, 1.0)
    served(s.launch_info())
    for i in range(B):
        np.testing.assert_allclose(dy[i], port.solve_primal_normal(A, x[i], z[i], y[i], b[i], c[i], 1.0), rtol=1e-7, atol=1e-9)
        np.testing.assert_allclose(dy[i], port.newton_step_known_answer(A, x[i], z[i], y[i], b[i], c[i], 1.0), rtol=1e-5, atol=1e-5)


def run_newton(case):
    lp = make_case(case[:2] + ("plain",) + case[3:])
    newton_matches(solver_for(case), lp, batch(lp.nrows), lambda info: assert_served_by(info, case))


def run_bounded(case):
    glp = make_case(case)
    s = solver_for(case)
    glp.init(s)
    glp.solve(s)
    assert s.kernel == ("bounded group" if case[0] == "slack" else "bounded wave")
    assert_served_by(s.launch_info(), case)
    assert (s.status == 0).all(), np.unique(s.status, return_counts=True)
    blp, _ = glp.to_bounded_equality_form()
    sel = np.arange(min(glp.nproblems, 16 if blp.ncols <= 256 else 6))
    tw = bounded_twin.solve(blp.A.todense(), blp.b[sel], blp.c[sel], blp.u[sel])
    assert (tw["status"] == 0).all()
    assert np.abs(s.iters[sel] - tw["iters"]).max() <= 1, (s.iters[sel], tw["iters"])
    assert rel_err(s.primal_obj[sel], tw["pobj"] + blp.f[sel]).max() <= 1e-9
    assert rel_err(s.dual_obj[sel], tw["dobj"] + blp.f[sel]).max() <= 1e-9
    np.testing.assert_allclose(s.x[sel], glp.l[sel] + tw["x"][:, :glp.ncols], rtol=1e-5, atol=1e-6)
    check_kkt(glp, s)


@pytest.mark.gpu
@pytest.mark.parametrize("case", CASES, ids=[case_id(c) for c in CASES])
def test_instantiation_matches_its_reference(case):
    from test_hip_parity import oracle_on
    kind = case[2]
    if kind == "newton":
        return run_newton(case)
    if kind == "bounded":
        return run_bounded(case)
    lp = make_case(case)
    s = solver_for(case)
    lp.init(s)
    lp.solve(s)
    assert_served_by(s.launch_info(), case)
    r = oracle_each(lp, ORACLE_FLAGS[kind]) if kind.startswith("pa") else oracle_on(lp, auto=False, flags=ORACLE_FLAGS[kind])
    assert_matches(s, r, lp)
