"""CPU: host-side logic -- LP containers, plugin registry, generators, loud failure without a GPU."""
import numpy as np
import pytest
import torch

from conftest import golden
from pycllp_amd import problems, solvers
from pycllp_amd.lp import SparseMatrix, EqualityLP, StandardLP
from pycllp_amd.solvers import solver_registry, BaseSolver


def test_registry_semantics():
    # pycllp/solvers/__init__.py:6-11: classes with a name are registered at creation, name=None are not
    assert solver_registry["hip_dense_primal_normal"] is solvers.HipDensePrimalNormalSolver

    class _Anon(BaseSolver):
        pass

    class _Named(BaseSolver):
        name = "unit_test_solver"

    try:
        assert "unit_test_solver" in solver_registry and solver_registry["unit_test_solver"] is _Named
        assert _Anon not in solver_registry.values()
        with pytest.raises(NotImplementedError):
            _Named().init(None)
        with pytest.raises(NotImplementedError):
            _Named().solve(None)
    finally:
        solver_registry.pop("unit_test_solver", None)


def test_lp_container_broadcasting_and_errors():
    A = SparseMatrix(matrix=np.array([[1.0, 2.0, 0.0], [0.0, 1.0, 3.0]]))
    assert (A.nrows, A.ncols, A.nnzeros, A.nproblems) == (2, 3, 4, 1)
    lp = EqualityLP(A, np.ones((5, 2)), np.array([1.0, 2.0, 3.0]), 0.5)      # lp.py:338-352
    assert lp.b.shape == (5, 2) and lp.c.shape == (5, 3) and lp.f.shape == (5,) and lp.nproblems == 5
    assert (lp.c == [1.0, 2.0, 3.0]).all() and (lp.f == 0.5).all()
    lp1 = EqualityLP(A, np.ones(2), np.ones(3), 0.0)
    assert lp1.b.shape == (1, 2) and lp1.nproblems == 1
    with pytest.raises(ValueError):
        EqualityLP(A, np.ones((5, 2)), np.ones((4, 3)), 0.0)
    with pytest.raises(ValueError):
        EqualityLP(A, None, np.ones(3), 0.0)
    with pytest.raises(ValueError):
        SparseMatrix(rows=[0, 1], cols=[0], data=[1.0, 2.0])
    vals, iA, kA = A.tocsc_arrays()                                         # lp.py:289-299
    assert vals.shape == (1, 4) and list(kA) == [0, 1, 3, 4] and list(iA) == [0, 0, 1, 1]
    assert list(vals[0]) == [1.0, 2.0, 1.0, 3.0]


def test_to_equality_form_appends_unit_slacks():
    lp, xopt = problems.vanderbei_2_9()
    elp = lp.to_equality_form()                                             # lp.py:551-567
    assert isinstance(lp, StandardLP) and (elp.nrows, elp.ncols) == (3, 6)
    dense = elp.A.todense()
    np.testing.assert_array_equal(dense[:, 3:], np.eye(3))
    np.testing.assert_array_equal(dense[:, :3], lp.A.todense())
    np.testing.assert_array_equal(elp.c[:, 3:], 0.0)
    assert lp.ncols == 3   # original untouched
    Ae, b, ce = problems.equality_arrays(lp.A.todense(), lp.b, lp.c)
    np.testing.assert_array_equal(Ae, dense)
    np.testing.assert_array_equal(ce, elp.c)


def test_generator_is_deterministic_and_matches_golden_checksum():
    g = golden("config_32x64.npz")
    A, b, c = problems.random_dense_arrays(32, 64, int(g["nobj"]), seed=0)
    np.testing.assert_array_equal([A.sum(), b.sum(), c.sum()], g["input_checksum"])
    A2, b2, c2 = problems.random_dense_arrays(32, 64, 16, seed=0, shard=3)
    np.testing.assert_array_equal(A, A2)                     # shards share A
    assert not np.allclose(b[:16], b2)
    assert b.min() >= 0.5 and b.max() < 1.5 and c.min() >= 0.5 and c.max() < 1.5


def test_textbook_problem_data():
    g = golden("vanderbei.npz")
    lp, xopt = problems.vanderbei_2_9()
    np.testing.assert_array_equal(lp.A.todense(), g["v29_A"])
    lp2, xopt2 = problems.vanderbei_2_10()
    assert isinstance(lp2, EqualityLP) and not isinstance(lp2, StandardLP)
    np.testing.assert_array_equal(lp2.A.todense(), g["v210_A"])


@pytest.mark.skipif(torch.cuda.is_available(), reason="checks the no-GPU failure mode")
def test_solver_fails_loudly_without_gpu():
    lp, _ = problems.vanderbei_2_9()
    elp = lp.to_equality_form()
    s = solvers.HipDensePrimalNormalSolver()
    with pytest.raises(RuntimeError, match="no ROCm device"):
        elp.init(s)
    with pytest.raises(RuntimeError):
        s.solve_device(np.ones((1, 3)), np.ones((1, 6)))
    with pytest.raises(TypeError):
        solvers.HipDensePrimalNormalSolver(not_an_option=1)


def test_plugin_option_semantics_without_gpu():
    """The constructor options of all four plugins (no GPU needed): the spellings of hsd and autoscale, how FLAG_HSD and
    FLAG_AUTOSCALE in ``flags`` are absorbed, the combinations that are refused, and the bounded plugins' rejections."""
    from pycllp_amd import _native
    flags = lambda s: int(s.options.get("flags", 0))      # noqa: E731
    for cls in (solvers.HipDensePrimalNormalSolver, solvers.HipSparsePrimalNormalSolver):
        assert cls().hsd == "auto" and cls().autoscale == "auto" and flags(cls()) == 0
        for v in (True, 1, np.True_, np.int64(1)):
            s = cls(hsd=v)
            assert s.hsd is True and flags(s) == _native.FLAG_HSD
            s = cls(autoscale=v)
            assert s.autoscale is True and flags(s) == _native.FLAG_AUTOSCALE
        for v in (False, 0, np.False_):
            s = cls(hsd=v, autoscale=v)
            assert s.hsd is False and s.autoscale is False and flags(s) == 0
        assert cls(autoscale=None).autoscale is False
        s = cls(flags=_native.FLAG_HSD)
        assert s.hsd is True and flags(s) == _native.FLAG_HSD
        s = cls(autoscale=False, flags=_native.FLAG_AUTOSCALE)
        assert s.autoscale is True and flags(s) == _native.FLAG_AUTOSCALE
        s = cls(predcorr=True, hsd=False, flags=_native.FLAG_FORCE_GUARD_PATH)
        assert s.hsd is False and flags(s) == _native.FLAG_PREDCORR | _native.FLAG_FORCE_GUARD_PATH
        assert cls(predcorr=True).hsd == "auto" and flags(cls(predcorr=True)) == _native.FLAG_PREDCORR
        s = cls(warm_start=1, warm_lift=0)
        assert s.warm_start is True and s.warm_lift == 0.0 and flags(s) == 0
        s = cls(max_iter=50, eps=1e-9)
        assert (s.options["max_iter"], s.options["eps"], flags(s)) == (50, 1e-9, 0)
        for kw in (dict(hsd="yes"), dict(hsd=None), dict(hsd=1.5), dict(autoscale="sometimes"),
                   dict(predcorr=True, hsd=True), dict(predcorr=1, hsd=np.True_),
                   dict(warm_lift=-1e-3), dict(warm_lift=float("nan"))):
            with pytest.raises(ValueError):
                cls(**kw)
        with pytest.raises(TypeError):
            cls(not_an_option=1)
    for cls in (solvers.HipGeneralPrimalNormalSolver, solvers.HipSparseGeneralPrimalNormalSolver):
        assert cls().hsd == "auto" and cls().autoscale == "auto" and cls(hsd=False).hsd is False
        for v in (True, 1, np.True_):
            assert cls(autoscale=v).autoscale is True
        for v in (False, 0, np.False_, None):
            assert cls(autoscale=v).autoscale is False
        assert cls(autoscale=False, flags=_native.FLAG_AUTOSCALE).autoscale is True
        assert cls(max_iter=50).options["max_iter"] == 50
        for kw in (dict(hsd=True), dict(hsd=1), dict(hsd=np.True_), dict(hsd="yes"), dict(hsd=None),
                   dict(predcorr=True), dict(warm_start=True), dict(autoscale="sometimes"),
                   dict(flags=_native.FLAG_HSD), dict(flags=_native.FLAG_PREDCORR), dict(flags=_native.FLAG_WARM_START),
                   dict(flags=_native.FLAG_WAVE_KERNEL), dict(flags=_native.FLAG_NO_SLACK_PATH)):
            with pytest.raises(ValueError):
                cls(**kw)
        with pytest.raises(TypeError):
            cls(not_an_option=1)
        with pytest.raises(TypeError):
            cls(warm_lift=0.0)         # an option of the dense plugins only
    for flag in (_native.FLAG_BLOCK_KERNEL, _native.FLAG_FORCE_GUARD_PATH):
        solvers.HipGeneralPrimalNormalSolver(flags=flag)
        with pytest.raises(ValueError):
            solvers.HipSparseGeneralPrimalNormalSolver(flags=flag)


def test_product_does_not_import_the_oracle():
    import os
    import re
    from conftest import ROOT
    for dirpath, _, files in os.walk(os.path.join(ROOT, "pycllp_amd")):
        for f in files:
            if f.endswith((".py", ".hip", ".h", ".cpp")):
                text = open(os.path.join(dirpath, f)).read()
                assert not re.search(r"^\s*(from|import)\s+oracle", text, flags=re.M), f
                assert "liboracle" not in text and "libhsd_ref" not in text, f


def test_packed_result_layout_round_trip_through_unpack():
    """The result arrays of a solve are views into one packed byte buffer (what the multi-GPU gather ships): the layout
    must be aligned, non-overlapping, have the gathered arrays as a contiguous prefix, and unpack() must invert it."""
    import torch
    from pycllp_amd.solvers.hip import HipDensePrimalNormalSolver, unpack
    s = HipDensePrimalNormalSolver()
    s.m, s.n = 5, 13
    for B in (0, 1, 7, 1000):
        lay = s._pack_layout(B)
        spans = sorted((off, off + nb, name) for name, (off, nb, dt, shape) in
                       ((k, v) for k, v in lay.items() if not k.startswith("_")))
        for (a0, a1, _), (b0, b1, _) in zip(spans[:-1], spans[1:]):
            assert a1 <= b0
        assert all(off % 256 == 0 for off, _, _ in spans)
        assert lay["x"][0] + lay["x"][1] <= lay["_gather_bytes"] <= lay["z"][0] <= lay["_total_bytes"]
        packed = torch.zeros(max(lay["_total_bytes"], 256), dtype=torch.uint8)
        views = unpack(packed, lay, names=("pobj", "dobj", "status", "iters", "y", "x", "z"))
        assert views["x"].shape == (B, 13) and views["y"].shape == (B, 5) and views["status"].dtype == torch.int32
        if B:
            views["x"][:] = 1.5; views["status"][:] = 7; views["z"][:] = -2.0
            again = unpack(packed[:lay["_gather_bytes"]].clone(), lay)      # what a peer would receive
            assert float(again["x"].sum()) == 1.5 * B * 13 and int(again["status"].sum()) == 7 * B


def _surface_cases():
    import scipy.sparse as sp
    from conftest import golden
    from pycllp_amd import lp as our_lp
    g = golden("reference_lp_surface.npz")
    for key in [str(k) for k in g["keys"]]:
        A = our_lp.SparseMatrix(matrix=sp.coo_matrix(g[key + "_in_A"]))
        f = float(g[key + "_in_f"])
        if str(g[key + "_in_kind"]) == "standard":
            lp = our_lp.StandardLP(A, g[key + "_in_b"], g[key + "_in_c"], f).to_equality_form()
        else:
            lp = our_lp.EqualityLP(A, g[key + "_in_b"], g[key + "_in_c"], f)
        yield key, g, lp


def test_lp_containers_show_the_surface_recorded_from_the_reference_objects():
    """tests/golden/reference_lp_surface.npz holds what REFERENCE-built LP objects (pycllp/lp.py) exposed to
    HipDensePrimalNormalSolver.consume for a set of raw inputs (tools/check_reference_boundary.py, build container):
    this package's own containers must expose the same values for the same inputs."""
    from pycllp_amd.solvers.hip import HipDensePrimalNormalSolver
    n = 0
    for key, g, lp in _surface_cases():
        s = HipDensePrimalNormalSolver.consume(lp)
        assert [s["m"], s["n"], s["nproblems"]] == list(g[key + "_shape"])
        for k in ("A", "b", "c", "f"):
            np.testing.assert_array_equal(s[k], g[key + "_" + k])
        n += 1
    assert n == 4


def test_general_lp_to_standard_form_matches_the_reference_fixtures():
    """tests/golden/general_lp.npz: StandardLPs the REFERENCE's GeneralLP.to_standard_form (pycllp/lp.py:725-792) returned for
    the case of its own tests/test_lp.py:236-250 and two more (tools/gen_lp_fixtures.py, build container)."""
    import scipy.sparse as sp
    from conftest import golden
    from pycllp_amd.lp import GeneralLP
    g = golden("general_lp.npz")
    for key in [str(k) for k in g["keys"]]:
        lp = GeneralLP(SparseMatrix(matrix=sp.coo_matrix(g[key + "_A"])), b=g[key + "_b"], c=g[key + "_c"], a=g[key + "_a"],
                       l=g[key + "_l"], f=0.0)
        slp = lp.to_standard_form()
        np.testing.assert_allclose(slp.A.todense(), g[key + "_std_A"], rtol=0, atol=1e-15)
        np.testing.assert_allclose(slp.b, g[key + "_std_b"], rtol=1e-15, atol=1e-15)
        np.testing.assert_allclose(slp.c, g[key + "_std_c"], rtol=0, atol=0)
        np.testing.assert_allclose(slp.f, g[key + "_std_f"], rtol=1e-15, atol=1e-15)
    with pytest.raises(ValueError):
        GeneralLP(SparseMatrix(matrix=sp.coo_matrix(np.eye(2))), b=[1.0, 1.0], c=[1.0, 1.0], l=[-np.inf, 0.0], f=0.0).to_standard_form()


def test_general_lp_bound_infinite_for_some_problems_only_raises_like_the_reference():
    """a row / upper bound that is infinite for some problems of the batch and finite for others makes
    the reference's remove_unbounded raise ValueError (pycllp/lp.py:518-523); a stand-in bound of 1e30 would wreck that LP's
    tolerances.  A bound that is infinite for EVERY problem is dropped (lp.py:515-517)."""
    import scipy.sparse as sp
    from pycllp_amd.lp import GeneralLP
    rs = np.random.RandomState(5)
    A = sp.coo_matrix(rs.rand(4, 5))
    b = 1.0 + rs.rand(3, 4); c = rs.rand(3, 5)
    bm = b.copy(); bm[2, 1] = np.inf
    with pytest.raises(ValueError):
        GeneralLP(SparseMatrix(matrix=A), b=bm, c=c, f=0.0).to_standard_form()
    um = np.full((3, 5), np.inf); um[0, 2] = 4.0
    with pytest.raises(ValueError):
        GeneralLP(SparseMatrix(matrix=A), b=b, c=c, u=um, f=0.0).to_standard_form()
    am = np.full((3, 4), -np.inf); am[1, 0] = 0.1
    with pytest.raises(ValueError):
        GeneralLP(SparseMatrix(matrix=A), b=b, c=c, a=am, f=0.0).to_standard_form()
    ball = b.copy(); ball[:, 1] = np.inf          # unbounded for every problem: the row goes
    slp = GeneralLP(SparseMatrix(matrix=A), b=ball, c=c, f=0.0).to_standard_form()
    assert slp.nrows == 3 and np.isfinite(slp.b).all()
    np.testing.assert_array_equal(slp.A.todense(), A.toarray()[[0, 2, 3]])


def test_per_problem_values_of_A_in_the_containers():
    """SparseMatrix.data[nproblems, nnz] (pycllp/lp.py:16-54): one set of values per problem is accepted (the reference's
    LP classes refuse it, lp.py:335-336), carried through to_equality_form, and a mismatch raises."""
    rs = np.random.RandomState(0)
    rows, cols = np.array([0, 0, 1, 1, 1]), np.array([0, 2, 0, 1, 2])
    data = rs.rand(4, 5)
    lp = StandardLP(SparseMatrix(rows, cols, data), rs.rand(4, 2), rs.rand(4, 3), 0.0)
    elp = lp.to_equality_form()
    assert elp.A.nproblems == 4 and elp.ncols == 5 and elp.nrows == 2
    for k in range(4):
        D = elp.A.todense(k)
        assert D[0, 0] == data[k, 0] and D[1, 1] == data[k, 3] and D[0, 3] == 1.0 and D[1, 4] == 1.0
    with pytest.raises(ValueError):
        StandardLP(SparseMatrix(rows, cols, data), rs.rand(3, 2), rs.rand(3, 3), 0.0)


def test_sparse_generator_terminates_on_narrow_matrices():
    """The >= 3 non-zeros per row rule of the config-5 generator is capped by the number of columns (n = 2 used to loop
    forever: found by tests/dev/fuzz_gpu.py)."""
    from pycllp_amd import problems
    A, b, c = problems.random_sparse_arrays(7, 2, 3, density=1.0, seed=1)
    assert A.shape == (7, 2) and (np.diff(A.indptr) == 2).all() and b.shape == (3, 7) and c.shape == (3, 2)


@pytest.mark.parametrize("bad", [np.nan, np.inf, -np.inf], ids=["nan", "+inf", "-inf"])
@pytest.mark.parametrize("array", ["b", "c"])
def test_autoscale_auto_leaves_lps_with_non_finite_data_out_of_the_band_test(array, bad):
    """``autoscale_wanted``: an LP whose max|b| or max|c| is not finite ends with status 3 whatever the scaling and must not
    decide the arithmetic of the others -- in an in-band batch the answer stays False, in an out-of-band batch True; numpy
    and torch arguments agree (the rule ``_solve_host`` applies on the device is the torch one)."""
    from pycllp_amd.solvers.hip import autoscale_wanted
    rs = np.random.RandomState(3)
    b, c = 0.5 + rs.rand(7, 5), 0.5 + rs.rand(7, 9)
    u = np.where(rs.rand(7, 9) < 0.5, np.inf, 1.0 + rs.rand(7, 9))
    both = lambda b_, c_, u_=None: (autoscale_wanted(b_, c_, u_),
                                    autoscale_wanted(torch.as_tensor(b_), torch.as_tensor(c_), None if u_ is None else torch.as_tensor(u_)))
    assert both(b, c) == (False, False) and both(b, c, u) == (False, False)
    sick = dict(b=b.copy(), c=c.copy())
    sick[array][2, 1] = bad
    assert both(sick["b"], sick["c"]) == (False, False)
    assert both(sick["b"], sick["c"], u) == (False, False)
    # the same entry in an out-of-band batch: another LP's data decides, as without the entry
    for far in (dict(b=b * 1e3, c=c), dict(b=b, c=c * 1e-3)):
        assert both(far["b"], far["c"]) == (True, True)
        sick = dict(b=far["b"].copy(), c=far["c"].copy())
        sick[array][2, 1] = bad
        assert both(sick["b"], sick["c"]) == (True, True)
    # ... and where the sick LP is the only one out of band, the batch stays on the reference's arithmetic
    lone = dict(b=b.copy(), c=c.copy())
    lone[array][2] *= 1e3
    assert both(lone["b"], lone["c"]) == (True, True)
    lone[array][2, 1] = bad
    assert both(lone["b"], lone["c"]) == (False, False)
    # upper bounds: u = +inf is "no bound", a NaN or a negative u is "not > 0" (fixed): neither counts, as before
    u2 = u.copy()
    u2[0, 0], u2[1, 1] = np.nan, -1.0
    assert both(b, c, u2) == (False, False)
    assert both(b, c, np.where(np.isfinite(u), u * 1e3, u)) == (True, True)
