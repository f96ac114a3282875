"""GPSJastrow without a GPU: the NumPy statement of the formulas (tests/gps_ref.py) reproduces every array the reference wrote to
g47_gps.npz, its Laplacian agrees with a finite difference of its own ratio, the library exports the pqa_gps_* entry points and
the factor fails loudly when no GPU is visible."""

import numpy as np
import pytest

import helpers
import gps_ref
from pyqmc_amd import _ffi

GPS_SYMBOLS = ["pqa_gps_set", "pqa_gps_recompute", "pqa_gps_value", "pqa_gps_eval", "pqa_gps_update", "pqa_gps_pgradient", "pqa_gps_get_state"]


@pytest.fixture(scope="module")
def g():
    return helpers.golden(gps_ref.GOLDEN)


def ref_of(g, name):
    p = name + "_"
    lat = g[p + "lattice"] if p + "lattice" in g.files else None
    ref = gps_ref.GpsRef(g[p + "Xsupport"], g[p + "alpha"], g[p + "f"][0], lat)
    return ref, ref.recompute(g[p + "configs"])


@pytest.mark.parametrize("name", list(gps_ref.CASES))
def test_numpy_statement_reproduces_the_reference(g, name):
    p = name + "_"
    ref, val = ref_of(g, name)
    keep = slice(0, 4) if name == "b" else slice(None)
    err = {"value": helpers.relerr(val, g[p + "value"]), "e_cs": helpers.relerr(ref.e[keep], g[p + "e_cs"])}
    electrons = [int(e) for e in g[p + "electrons"]]
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
        assert g[q + "testvalue_aux"].shape == (len(newpos), 5) and g[q + "testvalue_mask"].shape == (int(mask.sum()),)
        ref.update(e, newpos, accept)
        err[q + "post_value"] = helpers.relerr(ref.value(), g[q + "post_value"])
    err["final_e_cs_moved"] = helpers.relerr(ref.e[:, :, electrons, :], g[p + "final_e_cs_moved"])
    for k, v in ref.pgradient().items():
        assert v.shape == g[p + "pgrad_" + k].shape
        err["pgrad_" + k] = helpers.relerr(v, g[p + "pgrad_" + k])
    print(name, {k: f"{v:.1e}" for k, v in err.items()})
    assert max(err.values()) < 1e-12, {k: v for k, v in err.items() if v >= 1e-12}


@pytest.mark.parametrize("name", list(gps_ref.CASES))
def test_goldens_exercise_the_factor(g, name):
    """The default f = 100 would leave every ratio exactly 1: these cases do not."""
    p = name + "_"
    assert np.max(np.abs(g[p + "value"])) > 0.1
    for e in g[p + "electrons"]:
        assert np.max(np.abs(g[p + f"e{e}_testvalue"] - 1)) > 0.01 and np.max(np.abs(g[p + f"e{e}_gl_lap"])) > 0.01


@pytest.mark.parametrize("name", list(gps_ref.CASES))
def test_laplacian_against_finite_difference_of_the_ratio(g, name):
    """lap Psi / Psi at q from the central second difference of R(q) = Psi(e -> q) / Psi.  With h = 1e-3 the truncation is
    h^2 / 12 times a fourth derivative of a sum of Gaussians of width f <= 1 (their fourth derivatives are below 12 f^2 per unit
    weight; sum |alpha| (S - o) of these cases stays below 10), i.e. below 1e-5, and rounding is 4 eps R / h^2 = 1e-9."""
    p = name + "_"
    ref, _ = ref_of(g, name)
    h = 1e-3
    worst = 0.0
    for e in g[p + "electrons"]:
        e = int(e)
        q = g[p + f"e{e}_newpos"]
        _, lap = ref.gradient_laplacian(e, q)
        r0 = ref.testvalue(e, q)
        fd = np.zeros(len(q))
        for a in range(3):
            dq = np.zeros(3)
            dq[a] = h
            fd += (ref.testvalue(e, q + dq) + ref.testvalue(e, q - dq) - 2 * r0) / h**2
        fd /= r0
        worst = max(worst, float(np.max(np.abs(fd - lap))))
        assert np.max(np.abs(lap)) > 0.05
    print(name, "max |finite difference - laplacian|", worst)
    assert worst < 1e-5


def test_gradient_against_finite_difference_of_the_ratio(g):
    ref, _ = ref_of(g, "c")
    e, h = int(g["c_electrons"][0]), 1e-5
    q = g[f"c_e{e}_newpos"]
    grad = ref.gradient(e, q)
    r0 = ref.testvalue(e, q)
    for a in range(3):
        dq = np.zeros(3)
        dq[a] = h
        fd = (ref.testvalue(e, q + dq) - ref.testvalue(e, q - dq)) / (2 * h * r0)
        assert np.max(np.abs(fd - grad[a])) < 1e-8  # truncation h^2 / 6 |f'''| ~ 1e-10, rounding eps / h = 1e-11


def test_update_then_value_is_a_recompute(g):
    ref, _ = ref_of(g, "a")
    for e in g["a_electrons"]:
        ref.update(int(e), g[f"a_e{e}_newpos"], g[f"a_e{e}_accept"])
    again = gps_ref.GpsRef(ref.X, ref.alpha, ref.f)
    assert helpers.relerr(again.recompute(ref.x), ref.value()) < 1e-14
    assert helpers.relerr(again.e, ref.e) == 0.0


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as ge

    ge.build()
    return _ffi.lib()


def test_library_exports_the_gps_entry_points(lib):
    assert sorted(n for n in _ffi.header_symbols() if n.startswith("pqa_gps_")) == sorted(GPS_SYMBOLS)
    for n in GPS_SYMBOLS:
        assert hasattr(lib, n) and n in _ffi._PROTOTYPES, n


def test_gpsjastrow_is_exported():
    import pyqmc_amd as pa
    from pyqmc_amd import gps

    assert pa.GPSJastrow is gps.GPSJastrow
    assert not hasattr(pa.GPSJastrow, "_dev") and not hasattr(pa.GPSJastrow, "testvalue_many")


def test_no_gpu_means_loud_failure(lib, g):
    if lib.pqa_device_count() > 0:
        pytest.skip("a GPU is visible")
    import pyqmc_amd as pa

    with pytest.raises(_ffi.PqaError):
        pa.GPSJastrow(gps_ref.case_mol("a"), g["a_Xsupport"], f=0.5)
