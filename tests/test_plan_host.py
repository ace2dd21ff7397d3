"""The plans of the wave, block and large-LP kernels as the host builds them (csrc/wreg_plan.h, block_plan.h, big_plan.h on the
passes of plan_host.h), without a GPU: ``pycllp_hip_debug_plan`` runs a creator's pure part on host CSR arrays and reports its
return code, the plan's scalar fields and a digest of its tables.

The restatements of the plan rules in test_kernel_variants.py, test_workgroup_kernel_plans.py and dense_batch_wave_cases.py are
held here against the running code, on the matrices their GPU tests build; then the edge cases and refusals at the smallest sizes
where they occur; and on every plan built, the invariants of its LDS layout: offsets that are multiples of 16, sections that do
not overlap and end inside lds_bytes, wave areas of wpb x wave_doubles doubles."""
import ctypes

import numpy as np
import pytest
import scipy.sparse as sp

import dense_batch_cases as dbc
import dense_batch_wave_cases as dwc
import test_kernel_variants as tkv
import test_workgroup_kernel_plans as twp

MAX_LDS = tkv.MAX_LDS
BLOCK, WAVE, WAVE_PA, WAVE_BD, WAVE_BDPA, DENSE_PA, DENSE_PA_KEEP, BIG = range(8)
KIND_NAMES = ("block", "wave", "wave-pa", "wave-bd", "wave-bdpa", "dense-pa", "dense-pa-keep", "big")
NSCALARS = 32          # PLAN_NSCALARS of csrc/plan_host.h
# the scalar fields in the order the plan headers document them (wreg_plan_report, big_plan_report, block_plan_report)
WAVE_FIELDS = ("mb", "nq", "wpb", "lds_bytes", "wave_doubles", "nd", "as", "img_rows", "rmax", "ctot", "n_lev", "n_term", "nnzp",
               "variant", "pa", "bd", "o_csr_val", "o_ec_val", "o_t_w", "o_wave", "o_lev", "o_meta", "o_csr_col", "o_csr_ptr",
               "o_csr_len", "o_ec_row", "o_colmap", "o_t_cd", "o_ec_src", "o_t_ab", "o_img")
BIG_FIELDS = ("MB", "dense", "m_in_lds", "lds_bytes", "n_ent", "ks", "ws_doubles", "nd", "imgR", "n_sl")
BLOCK_FIELDS = ("a_in_lds", "lds", "lds_with_a", "n_entries", "n_terms")
META_N = 32


def fields_of(kind):
    return BLOCK_FIELDS if kind == BLOCK else (BIG_FIELDS if kind == BIG else WAVE_FIELDS)


_LIBS = {}


def entry(path=None):
    """``pycllp_hip_debug_plan`` of the library that build() made (or of another build of it, for comparisons)."""
    from pycllp_amd import _native
    path = path or _native.LIB_PATH
    if path not in _LIBS:
        f = ctypes.CDLL(path).pycllp_hip_debug_plan
        f.restype = ctypes.c_int
        f.argtypes = [ctypes.c_int] * 4 + [ctypes.c_void_p] * 3 + [ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p]
        _LIBS[path] = f
    return _LIBS[path]


def build_plan(kind, A, max_lds=MAX_LDS, path=None):
    """(return code, {field: value}, digest) of the plan of ``kind`` for the scipy CSR matrix ``A`` (entries as stored)."""
    A = sp.csr_matrix(A)
    val = np.ascontiguousarray(A.data, dtype=np.float64)
    ptr = np.ascontiguousarray(A.indptr, dtype=np.int32)
    col = np.ascontiguousarray(A.indices, dtype=np.int32)
    scalars = np.zeros(NSCALARS, dtype=np.int64)
    digest = np.zeros(1, dtype=np.uint64)
    rc = entry(path)(kind, A.shape[0], A.shape[1], len(val), val.ctypes.data, ptr.ctypes.data, col.ctypes.data, max_lds,
                     scalars.ctypes.data, digest.ctypes.data)
    return rc, dict(zip(fields_of(kind), (int(v) for v in scalars))), int(digest[0])


# ---- the invariants of a plan's LDS layout ----------------------------------------------------------------------------------
def wave_sections(p, nnz):
    """{offset field: bytes} of the LDS sections a wave-kernel plan lays out, from its scalar fields."""
    waves = 8 * p["wpb"] * p["wave_doubles"]
    if p["variant"] == 2:
        return {"o_wave": waves} if p["pa"] else {"o_img": 8 * p["img_rows"] * p["as"], "o_wave": waves}
    ell, terms, mpl = 64 * max(p["ctot"], 1), max(p["n_term"], 1), 64 * ((16 * p["mb"] + 63) // 64)
    sec = {"o_wave": waves, "o_lev": 4 * (p["n_lev"] + 1), "o_t_cd": 4 * terms, "o_colmap": 4 * 64 * p["nq"], "o_meta": 4 * META_N,
           "o_csr_col": 2 * nnz, "o_csr_ptr": 2 * mpl, "o_csr_len": 2 * mpl, "o_ec_row": 2 * ell}
    if p["pa"]:
        sec.update({"o_t_ab": 4 * terms, "o_ec_src": 2 * ell})
    else:
        sec.update({"o_csr_val": 8 * nnz, "o_ec_val": 8 * ell, "o_t_w": 8 * terms})
    return sec


def check_wave_invariants(p, nnz, what):
    assert all(p[f] % 16 == 0 for f in WAVE_FIELDS if f.startswith("o_")), what
    assert 1 <= p["wpb"] <= 4 and p["lds_bytes"] <= MAX_LDS and p["lds_bytes"] % 8 == 0, what
    spans = sorted((p[f], p[f] + size) for f, size in wave_sections(p, nnz).items() if size)
    assert all(a[1] <= b[0] for a, b in zip(spans, spans[1:])), (what, spans)
    assert spans[0][0] >= 0 and spans[-1][1] <= p["lds_bytes"], (what, spans)
    assert 16 * p["mb"] <= 128 and (max(192 * p["nq"], 768) + 272) + 144 * p["mb"] <= 65535, what


def checked(kind, A, what, max_lds=MAX_LDS):
    rc, p, digest = build_plan(kind, A, max_lds)
    if rc == 0 and kind not in (BLOCK, BIG):
        check_wave_invariants(p, sp.csr_matrix(A).nnz, what)
    if rc == 0 and kind == BIG:
        assert p["lds_bytes"] % 8 == 0 and 2 * p["lds_bytes"] <= max_lds, what
    if rc == 0 and kind == BLOCK:
        assert p["lds"] <= max_lds and p["lds_with_a"] <= max_lds, what
    return rc, p, digest


def structure(lp):
    return twp.structure_of(lp)


# ---- the wave kernel's variants: every case of test_kernel_variants.CASES on tables or an image -------------------------------
def wave_points():
    """[(id, case, plan kind)] of the distinct matrices and plan kinds among the wave cases."""
    seen, out = set(), []
    for case in tkv.CASES:
        family, shape, kind, point = case[:4]
        if family not in ("tables", "image"):
            continue
        pk = WAVE_BD if kind == "bounded" else (WAVE_PA if kind.startswith("pa") else WAVE)
        if (family, shape, point, pk) not in seen:
            seen.add((family, shape, point, pk))
            out.append(("%s-%dx%d-%s-%s" % (family, shape[0], shape[1], point, KIND_NAMES[pk]), case, pk))
    return out


WAVE_POINTS = wave_points()


def wave_matrix(case):
    lp = tkv.make_case(case)
    if case[2] == "bounded":
        lp = lp.to_bounded_equality_form()[0]
    return structure(lp)


@pytest.mark.parametrize("name,case,pk", WAVE_POINTS, ids=[w[0] for w in WAVE_POINTS])
def test_wave_variant_of_every_case(name, case, pk):
    family, shape, kind, point, m, N, _ = case
    A = wave_matrix(case)
    assert A.shape == (m, N)
    bounded = pk == WAVE_BD
    rc, p, _ = checked(pk, A, name)
    assert rc == 0 and (p["mb"], p["nq"]) == shape, (rc, p)
    assert p["wave_doubles"] - p["nnzp"] == tkv.wave_doubles(shape[0], shape[1], bounded) and p["lds_bytes"] <= MAX_LDS
    assert (p["pa"], p["bd"]) == (int(pk == WAVE_PA), int(bounded))
    if family == "image":
        tail = tkv.image_form(case) == "standard"
        # the creator tries the term tables first: it reaches the image only where they refuse (return code 1)
        assert tkv.tables_cannot_fit(m, N, tail, shape, bounded) and p["variant"] == 2
        assert p["wpb"] == tkv.image_waves(m, N, tail, shape, bounded)
        assert p["nd"] == (N - m if tail else N)
    else:
        assert p["variant"] == 1 and (p["wpb"] == 4 or pk != WAVE)
        assert p["nnzp"] == ((A.nnz + 2) & ~1 if pk == WAVE_PA else 0)


def test_compiled_shapes_keep_16_bit_destinations():
    """stage_d + MB WL <= 65535 at every compiled shape: the refusal of wreg_tables_plan for it cannot occur."""
    for mb, nq in tkv.WAVE_TAB_SHAPES + tkv.WAVE_DA_SHAPES:
        assert max(192 * nq, 768) + 272 + 144 * mb <= 65535


# ---- the workgroup-per-LP kernels: every case of test_workgroup_kernel_plans.CASES ------------------------------------------
def workgroup_points():
    seen, out = set(), []
    for case in twp.CASES:
        key = (case[0], case[1], case[2], case[4], case[0] == "block" and case[3].startswith("pa"))
        if key not in seen:
            seen.add(key)
            out.append((twp.case_id(case), case))
    return out


WORKGROUP_POINTS = workgroup_points()


@pytest.mark.parametrize("name,case", WORKGROUP_POINTS, ids=[w[0] for w in WORKGROUP_POINTS])
def test_workgroup_plan_of_every_case(name, case):
    family, cell, gram, kind, point, m, N, _ = case
    A = structure(twp.make_case(case))
    assert A.shape == (m, N)
    if family == "big":
        rc, p, _ = checked(BIG, A, name)
        want, lds, _ = twp.big_plan((m + 15) // 16, N)
        assert rc == 0 and ("L" if p["m_in_lds"] else "W", p["lds_bytes"]) == (want[0], lds), (rc, p)
        assert p["MB"] == (m + 15) // 16 and p["ws_doubles"] == (0 if p["m_in_lds"] else p["MB"] * (p["MB"] + 1) // 2 * 256)
        tail = twp.big_form(case) == "standard"
        assert p["dense"] == int(gram == "mfma") == int(twp.gram_is_dense(A, tail))
        assert p["nd"] == ((N - m if tail else N) if p["dense"] else 0) and (p["n_ent"] > 0) == (not p["dense"])
    else:
        rc, p, _ = checked(BLOCK, A, name)
        plan, a, lds, _ = twp.block_plan(m, N, A.nnz)
        assert rc == 0 and (p["a_in_lds"], p["lds"]) == (int(a), lds), (rc, p)
        with_a = twp.block_plan(m, N, A.nnz, pa=True)
        assert p["lds_with_a"] == (with_a[2] if with_a else 0)
        assert (plan if not kind.startswith("pa") else with_a[0]) == cell
        assert p["n_terms"] == twp.gram_terms(A)


# ---- per-problem dense matrices: the points of dense_batch_wave_cases --------------------------------------------------------
@pytest.mark.parametrize("case", dwc.EVERY, ids=[dwc.every_id(c) for c in dwc.EVERY])
def test_dense_image_per_wave_of_every_point(case):
    shape, which = case
    m, n, tail = dwc.POINTS[shape][which]
    A = structure(dbc.make(m, n, tail, B=2))
    for kind, implied in ((DENSE_PA, tail), (DENSE_PA_KEEP, False)):
        want = dwc.plan(m, n, implied)
        rc, p, _ = checked(kind, A, dwc.every_id(case))
        assert rc == (0 if want[2] else 1), (kind, rc, want)
        if rc == 0:
            assert (p["mb"], p["nq"]) == want[0] == shape and p["wpb"] == want[2] and p["lds_bytes"] == want[2] * want[1]
            assert p["nd"] == (n - m if implied else n) and (p["variant"], p["pa"]) == (2, 1)


# ---- edge cases and refusals -----------------------------------------------------------------------------------------------
def with_tail(A):
    return sp.hstack([sp.csr_matrix(A), sp.identity(A.shape[0], format="csr")], format="csr")


def edge_matrices():
    """{name: CSR matrix}: the smallest sizes at which a builder takes another path."""
    rs = np.random.RandomState(5)
    hollow = np.array([[1.0, 0.0, 2.0, 0.0], [0.0, 0.0, 0.0, 0.0], [3.0, 0.0, 0.0, 4.0]])       # an empty row, an empty column
    tail = with_tail(rs.rand(3, 4) + 0.1)
    off = tail.copy().tolil()
    off[1, 4 + 1] = 1.0 + 2.0 ** -52
    # the tail's entry of row 2 twice: a CSR with a duplicate entry, as stored
    dup = sp.csr_matrix((np.append(tail.data, 1.0), np.append(tail.indices, 6), np.append(tail.indptr[:-1], tail.nnz + 1)),
                        shape=tail.shape)
    return {
        "m1": sp.csr_matrix(rs.rand(1, 5) + 0.1), "n1": sp.csr_matrix(rs.rand(3, 1) + 0.1), "1x1": sp.csr_matrix([[2.0]]),
        "hollow": sp.csr_matrix(hollow), "empty": sp.csr_matrix((4, 6)), "tail": tail, "tail-off-by-an-ulp": sp.csr_matrix(off),
        "tail-duplicate": dup,
    }


EDGES = edge_matrices()


def column_terms(A):
    """Gram terms with the diagonal's: len (len + 1) / 2 per column, over the entries as stored."""
    lens = np.bincount(A.indices, minlength=A.shape[1]).astype(np.int64)
    return int((lens * (lens + 1) // 2).sum())


@pytest.mark.parametrize("name", sorted(EDGES))
def test_edge_matrices_on_every_kind(name):
    A = EDGES[name]
    m, n = A.shape
    for kind in range(8):
        rc, p, _ = checked(kind, A, (name, KIND_NAMES[kind]))
        assert rc == 0, (KIND_NAMES[kind], rc)
        if kind in (WAVE, WAVE_PA, WAVE_BD, WAVE_BDPA):
            assert p["variant"] == 1 and (p["mb"], p["nq"]) == (1, 4) and p["rmax"] == int(np.diff(A.indptr).max())
            assert (p["n_term"] > 0) == (column_terms(A) > A.nnz)          # a term: two entries of one column
        if kind == BLOCK:
            assert p["n_terms"] == column_terms(A) and p["a_in_lds"] == 1
        if kind == BIG:
            assert p["MB"] == 1 and p["m_in_lds"] == 1


def test_identity_tail_is_exact():
    """Only a tail that is exactly the identity is kept out of a dense image: one value off by an ulp, or one entry stored
    twice, and every column goes in."""
    m, n = EDGES["tail"].shape
    for name, nd in (("tail", n - m), ("tail-off-by-an-ulp", n), ("tail-duplicate", n)):
        assert build_plan(DENSE_PA, EDGES[name])[1]["nd"] == nd, name
        assert build_plan(DENSE_PA_KEEP, EDGES[name])[1]["nd"] == n, name


def test_table_plan_stops_below_65535_entries():
    """16-bit CSR indices, with 65535 = the zero entry of a padded slot: nnz = 65535 is refused by the plans on tables (return
    code 1), nnz = 65534 is not refused for that -- a dense 128 x 512 matrix less one and two entries, whose Gram terms stay
    below the cap of 2^22, on structure-only tables with no limit on the LDS."""
    for nnz, refused in ((65535, True), (65534, False)):
        A = np.ones((128, 512))
        A.ravel()[nnz:] = 0.0
        A = sp.csr_matrix(A)
        assert A.nnz == nnz and twp.gram_terms(A) - nnz <= 1 << 22
        assert build_plan(WAVE_PA, A, max_lds=2 ** 31 - 1)[0] == (1 if refused else 0), nnz


def test_refusals_keep_their_return_codes():
    rs = np.random.RandomState(9)
    assert build_plan(BIG, sp.csr_matrix(rs.rand(257, 300)))[0] == 1          # beyond BIG_MAX_M
    assert build_plan(BIG, sp.csr_matrix(rs.rand(4, 1281)))[0] == 1           # beyond BIG_MAX_N
    assert build_plan(WAVE, sp.csr_matrix(rs.rand(129, 200)))[0] == 1         # no shape covers 129 rows
    assert build_plan(DENSE_PA, sp.csr_matrix(rs.rand(100, 385)))[0] == 1     # kWDAPA has no (8, 6)
    dense = sp.csr_matrix(rs.rand(128, 512))
    assert build_plan(WAVE, dense)[0] == 1 and build_plan(DENSE_PA, dense)[0] == 1      # neither tables nor an image fit
    assert build_plan(BLOCK, dense)[0] == 0
    assert build_plan(BLOCK, dense, max_lds=64 * 1024)[0] == 2                # BLOCK_PLAN_NO_LDS
    assert build_plan(BIG, sp.csr_matrix(rs.rand(256, 1280)), max_lds=32 * 1024)[0] == 1
    assert entry()(8, 1, 1, 0, None, None, None, MAX_LDS, None, None) == -1
