"""GeminalJastrow without a GPU: the NumPy statement of the closed form (tests/geminal_ref.py) reproduces every array the reference
wrote to g48_geminal.npz, its Laplacian agrees with a finite difference of its own ratio, the parameter derivative contracts back to
the value, and the library and the package export the feature."""

import numpy as np
import pytest

import helpers
import geminal_ref
from pyqmc_amd import _ffi

GEMINAL_SYMBOLS = ["pqa_geminal_set", "pqa_geminal_recompute", "pqa_geminal_value", "pqa_geminal_eval", "pqa_geminal_testvalue_many",
                   "pqa_geminal_update", "pqa_geminal_pgradient", "pqa_geminal_get_state"]


@pytest.fixture(scope="module")
def g():
    return helpers.golden(geminal_ref.GOLDEN)


def ref_of(g, name):
    ref = geminal_ref.GeminalRef(geminal_ref.case_mol(name), g[name + "_gcoeff"])
    return ref, ref.recompute(g[name + "_configs"])


@pytest.mark.parametrize("name", list(geminal_ref.CASES))
def test_numpy_statement_reproduces_the_reference(g, name):
    p = name + "_"
    W, electrons, many, keep = geminal_ref.CASES[name]
    ref, val = ref_of(g, name)
    assert ref.nao == {"a": 23, "b": 184, "c": 26}[name] and len(val) == W
    ksl = slice(None) if keep is None else slice(0, keep)
    fsl = slice(None) if keep is None else slice(None, None, 8)
    err = {"value": helpers.relerr(val, g[p + "value"]), "ao_val": helpers.relerr(ref.A[ksl], g[p + "ao_val"])}
    assert [int(e) for e in g[p + "electrons"]] == list(electrons) and [int(e) for e in g[p + "many"]] == list(many)
    for e in electrons:
        q = p + f"e{e}_"
        newpos, aux, mask, accept = g[q + "newpos"], g[q + "aux"], g[q + "mask"], g[q + "accept"]
        gr, v = ref.gradient_value(e, newpos)
        err[q + "gv_grad"], err[q + "gv_val"] = helpers.relerr(gr, g[q + "gv_grad"]), helpers.relerr(v, g[q + "gv_val"])
        err[q + "grad"] = helpers.relerr(ref.gradient(e, newpos), g[q + "grad"])
        gr, lap = ref.gradient_laplacian(e, newpos)
        err[q + "gl_grad"], err[q + "gl_lap"] = helpers.relerr(gr, g[q + "gl_grad"]), helpers.relerr(lap, g[q + "gl_lap"])
        err[q + "testvalue"] = helpers.relerr(ref.testvalue(e, newpos), g[q + "testvalue"])
        err[q + "testvalue_mask"] = helpers.relerr(ref.testvalue(e, newpos, mask), g[q + "testvalue_mask"])
        err[q + "testvalue_aux"] = helpers.relerr(ref.testvalue(e, aux), g[q + "testvalue_aux"])
        err[q + "testvalue_aux_mask"] = helpers.relerr(ref.testvalue(e, aux, mask), g[q + "testvalue_aux_mask"])
        err[q + "testvalue_many"] = helpers.relerr(ref.testvalue_many(many, newpos), g[q + "testvalue_many"])
        err[q + "testvalue_many_mask"] = helpers.relerr(ref.testvalue_many(many, newpos, mask), g[q + "testvalue_many_mask"])
        assert g[q + "testvalue_aux"].shape == (W, 5) and g[q + "testvalue_mask"].shape == (int(mask.sum()),)
        assert g[q + "testvalue_many"].shape == (W, 3)
        ref.update(e, newpos, accept)
        err[q + "post_value"] = helpers.relerr(ref.value(), g[q + "post_value"])
    err["final_ao_moved"] = helpers.relerr(ref.A[fsl][:, list(electrons), :], g[p + "final_ao_moved"])
    pg = ref.pgradient()["gcoeff"]
    assert pg.shape == (W, ref.nao * (ref.nao + 1) // 2)
    err["pgrad_gcoeff"] = helpers.relerr(pg[ksl], g[p + "pgrad_gcoeff"])
    print(name, {k: f"{v:.1e}" for k, v in err.items()})
    assert max(err.values()) < 1e-12, {k: v for k, v in err.items() if v >= 1e-12}


@pytest.mark.parametrize("name", list(geminal_ref.CASES))
def test_goldens_exercise_the_factor(g, name):
    """The reference's default gcoeff = 0 would leave every ratio exactly 1: these cases do not, and stay inside (1e-2, 1e2)."""
    p = name + "_"
    assert np.max(np.abs(g[p + "value"])) > 0.1 and g[p + "sigma"][0] > 0
    for e in g[p + "electrons"]:
        for k in ("gv_val", "testvalue", "testvalue_mask", "testvalue_aux", "testvalue_aux_mask", "testvalue_many", "testvalue_many_mask"):
            r = g[p + f"e{e}_" + k]
            assert r.min() > 1e-2 and r.max() < 1e2
        assert np.max(np.abs(g[p + f"e{e}_testvalue"] - 1)) > 0.01 and np.max(np.abs(g[p + f"e{e}_gl_lap"])) > 0.01


@pytest.mark.parametrize("name", ["a", "b"])
def test_laplacian_against_finite_difference_of_the_ratio(g, name):
    """lap Psi / Psi at q from the central second difference of R(q) = Psi(e -> q) / Psi with h = 1e-3, on the open cases: the periodic
    AOs drop lattice images at the reference's cut-offs (orbital value 1e-2 there), so they jump, and a stencil that straddles a
    cut-off measures the jump, not a derivative.  The truncation of the second difference is h^2 / 12 times the fourth derivative of R along the axis, which is estimated per walker and axis by the central fourth difference
    of R at d = 2e-2 (rounding 16 eps / d^4 = 2e-8, below the derivative itself by orders); the bound allows twice that estimate, for
    the variation of the fourth derivative over the stencil, plus the second difference's own rounding, 4 eps R / h^2 per axis."""
    p = name + "_"
    ref, _ = ref_of(g, name)
    h, d, eps = 1e-3, 2e-2, np.finfo(float).eps
    for e in g[p + "electrons"]:
        e = int(e)
        q = g[p + f"e{e}_newpos"]
        _, lap = ref.gradient_laplacian(e, q)
        r0 = ref.testvalue(e, q)
        fd, bound = np.zeros(len(q)), np.zeros(len(q))
        for a in range(3):
            dq = np.zeros(3)
            dq[a] = 1.0
            R = lambda s: ref.testvalue(e, q + s * dq)  # noqa: E731
            fd += (R(h) + R(-h) - 2 * r0) / h**2
            d4 = (R(2 * d) - 4 * R(d) + 6 * r0 - 4 * R(-d) + R(-2 * d)) / d**4
            bound += 2 * h**2 / 12 * np.abs(d4) + 4 * eps * r0 / h**2
        err = np.abs(fd / r0 - lap)
        print(name, e, "max |finite difference - laplacian|", err.max(), "bound", (bound / r0).min(), "..", (bound / r0).max())
        assert np.max(np.abs(lap)) > 0.05
        assert np.all(err < bound / r0), (err.max(), (bound / r0).max())


def test_gradient_against_finite_difference_of_the_ratio(g):
    ref, _ = ref_of(g, "a")
    e, h = int(g["a_electrons"][0]), 1e-5
    q = g[f"a_e{e}_newpos"]
    grad = ref.gradient(e, q)
    r0 = ref.testvalue(e, q)
    for a in range(3):
        dq = np.zeros(3)
        dq[a] = h
        fd = (ref.testvalue(e, q + dq) - ref.testvalue(e, q - dq)) / (2 * h * r0)
        # truncation h^2 / 6 |R'''| / R with third derivatives of these Gaussians times |h_e| below 1e3: 2e-8; rounding eps / h = 2e-11
        assert np.max(np.abs(fd - grad[a])) < 1e-7


@pytest.mark.parametrize("name", list(geminal_ref.CASES))
def test_parameter_derivative_contracts_to_the_value(g, name):
    """log Psi is linear in gcoeff: sum_{m<=n} p_mn d log Psi / d p_mn = log Psi (a sum of nao (nao + 1) / 2 products: 1e-12)."""
    ref, val = ref_of(g, name)
    assert helpers.relerr(ref.pgradient()["gcoeff"] @ g[name + "_gcoeff"], val) < 1e-12


def test_update_then_value_is_a_recompute(g):
    ref, _ = ref_of(g, "a")
    for e in g["a_electrons"]:
        ref.update(int(e), g[f"a_e{e}_newpos"], g[f"a_e{e}_accept"])
    again = geminal_ref.GeminalRef(geminal_ref.case_mol("a"), g["a_gcoeff"])
    assert helpers.relerr(again.recompute(ref.x), ref.value()) < 1e-14
    assert helpers.relerr(again.A, ref.A) == 0.0


def test_wrong_parameter_count_raises():
    with pytest.raises(ValueError, match="Wrong number of parameters"):
        geminal_ref.GeminalRef(geminal_ref.case_mol("a"), np.zeros(23 * 23))


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as ge

    ge.build()
    return _ffi.lib()


def test_library_exports_the_geminal_entry_points(lib):
    assert sorted(n for n in _ffi.header_symbols() if n.startswith("pqa_geminal_")) == sorted(GEMINAL_SYMBOLS)
    for n in GEMINAL_SYMBOLS:
        assert hasattr(lib, n) and n in _ffi._PROTOTYPES, n


def test_the_unit_is_built():
    import __graft_entry__ as ge

    assert "pqa_geminal" in ge.UNITS


def test_geminaljastrow_is_exported():
    import pyqmc_amd as pa
    from pyqmc_amd import geminal

    assert pa.GeminalJastrow is geminal.GeminalJastrow
    assert not hasattr(pa.GeminalJastrow, "_dev") and hasattr(pa.GeminalJastrow, "testvalue_many")
