"""GPSJastrow on the device (pqa_gps.hip) against the reference's golden vectors (g47_gps.npz, cases a, b, c of tests/gps_ref.py),
the update / ratio / recompute triangle, parameters, copies, the product with Slater and JastrowSpin, and no side effect on another
wave function of the device.

Metric and bound: helpers.relerr < 1e-10, as tests/test_gpu_tbdm_fused.py: fp64 sums of at most 2 x 33 positive Gaussians times 64
electrons, no cancellation beyond what appears there."""

import copy
import pickle

import numpy as np
import pytest

import gps_ref
from pyqmc_amd import _ffi, systems
from pyqmc_amd.configs import OpenConfigs, OpenElectron, PeriodicConfigs
from tests import helpers

pytestmark = pytest.mark.gpu

TOL = 1e-10


@pytest.fixture(scope="module")
def g():
    return helpers.golden(gps_ref.GOLDEN)


def _configs(g, name, x=None):
    x = np.array(g[name + "_configs"] if x is None else x)
    return PeriodicConfigs(x, g[name + "_lattice"]) if name == "c" else OpenConfigs(x)


def _wf(g, name, **over):
    import pyqmc_amd as pa

    p = name + "_"
    wf = pa.GPSJastrow(gps_ref.case_mol(name), over.get("X", g[p + "Xsupport"]), f=over.get("f", g[p + "f"][0]))
    wf.parameters["alpha"] = over.get("alpha", g[p + "alpha"])
    return wf


def _check(err):
    bad = {k: v for k, v in err.items() if not v < TOL}
    assert not bad, bad


@pytest.mark.parametrize("name", list(gps_ref.CASES))
def test_golden_arrays(g, name):
    p = name + "_"
    wf = _wf(g, name)
    configs = _configs(g, name)
    W = len(configs.configs)
    sign, val = wf.recompute(configs)
    assert np.array_equal(sign, np.ones(W)) and wf.dtype is float
    keep = slice(0, 4) if name == "b" else slice(None)
    err = {"value": helpers.relerr(val, g[p + "value"]), "e_cs": helpers.relerr(wf._get_state()[0][keep], g[p + "e_cs"])}
    electrons = [int(e) for e in g[p + "electrons"]]
    for e in electrons:
        q = p + f"e{e}_"
        mask, accept = g[q + "mask"], g[q + "accept"]
        ep, ea = configs.make_irreducible(e, g[q + "newpos"]), configs.make_irreducible(e, g[q + "aux"])
        gr, v, saved = wf.gradient_value(e, ep)
        assert np.array_equal(saved, np.array([1])) and gr.shape == (3, W)
        err[q + "gv_grad"], err[q + "gv_val"] = helpers.relerr(gr, g[q + "gv_grad"]), helpers.relerr(v, g[q + "gv_val"])
        err[q + "grad"] = helpers.relerr(wf.gradient(e, ep), g[q + "grad"])
        gr, lap = wf.gradient_laplacian(e, ep)
        err[q + "gl_grad"], err[q + "gl_lap"] = helpers.relerr(gr, g[q + "gl_grad"]), helpers.relerr(lap, g[q + "gl_lap"])
        tv, saved = wf.testvalue(e, ep)
        assert np.array_equal(saved, np.array([1]))
        err[q + "testvalue"] = helpers.relerr(tv, g[q + "testvalue"])
        err[q + "testvalue_mask"] = helpers.relerr(wf.testvalue(e, ep, mask)[0], g[q + "testvalue_mask"])
        err[q + "testvalue_aux"] = helpers.relerr(wf.testvalue(e, ea)[0], g[q + "testvalue_aux"])
        err[q + "testvalue_aux_mask"] = helpers.relerr(wf.testvalue(e, ea, mask)[0], g[q + "testvalue_aux_mask"])
        # one auxiliary point per walker, an all-False mask, a single True
        one = configs.make_irreducible(e, g[q + "aux"][:, :1])
        r1 = wf.testvalue(e, one)[0]
        assert r1.shape == (W, 1)
        err[q + "testvalue_aux_npt1"] = helpers.relerr(r1, g[q + "testvalue_aux"][:, :1])
        none = np.zeros(W, dtype=bool)
        assert wf.testvalue(e, ep, none)[0].shape == (0,) and wf.testvalue(e, ea, none)[0].shape == (0, 5)
        single = none.copy()
        single[W // 2] = True
        err[q + "testvalue_single"] = helpers.relerr(wf.testvalue(e, ep, single)[0], g[q + "testvalue"][W // 2 : W // 2 + 1])
        err[q + "testvalue_aux_single"] = helpers.relerr(wf.testvalue(e, ea, single)[0], g[q + "testvalue_aux"][W // 2 : W // 2 + 1])
        wf.updateinternals(e, ep, configs, mask=accept)
        configs.move(e, ep, accept)
        err[q + "post_value"] = helpers.relerr(wf.value()[1], g[q + "post_value"])
    e_cs, x = wf._get_state()
    assert np.array_equal(x, configs.configs)
    err["final_e_cs_moved"] = helpers.relerr(e_cs[:, :, electrons, :], g[p + "final_e_cs_moved"])
    pg = wf.pgradient()
    assert sorted(pg) == ["Xsupport", "alpha", "f"]
    for k, v in pg.items():
        assert v.shape == g[p + "pgrad_" + k].shape
        err["pgrad_" + k] = helpers.relerr(v, g[p + "pgrad_" + k])
    print(name, {k: f"{v:.1e}" for k, v in err.items()})
    _check(err)


@pytest.mark.parametrize("name", ["a", "c"])
def test_single_walker(g, name):
    p = name + "_"
    wf = _wf(g, name)
    configs = _configs(g, name, g[p + "configs"][:1])
    e = int(g[p + "electrons"][0])
    q = p + f"e{e}_"
    err = {"value": helpers.relerr(wf.recompute(configs)[1], g[p + "value"][:1])}
    ep = configs.make_irreducible(e, g[q + "newpos"][:1])
    gr, lap = wf.gradient_laplacian(e, ep)
    err["gl_grad"], err["gl_lap"] = helpers.relerr(gr, g[q + "gl_grad"][:, :1]), helpers.relerr(lap, g[q + "gl_lap"][:1])
    err["testvalue_aux"] = helpers.relerr(wf.testvalue(e, configs.make_irreducible(e, g[q + "aux"][:1]))[0], g[q + "testvalue_aux"][:1])
    wf.updateinternals(e, ep, configs)
    assert wf.pgradient()["f"].shape == (1, 1)
    _check(err)


def test_update_ratio_recompute_triangle(g):
    """testwf.test_updateinternals on case b: two sweeps of masked moves of all 64 electrons."""
    wf = _wf(g, "b")
    configs = _configs(g, "b")
    W, N, _ = configs.configs.shape
    rng = np.random.default_rng(8)
    _, v0 = wf.recompute(configs)
    logratio = np.zeros(W)
    for _ in range(2):
        for e in range(N):
            ep = OpenElectron(configs.configs[:, e] + 0.5 * rng.standard_normal((W, 3)), configs.dist)
            mask = rng.random(W) > 0.4
            logratio[mask] += np.log(wf.testvalue(e, ep, mask)[0])
            wf.updateinternals(e, ep, configs, mask=mask)
            configs.move(e, ep, mask)
    _, v1 = wf.value()
    e_cs, x = wf._get_state()
    assert np.array_equal(x, configs.configs)
    fresh = _wf(g, "b")
    _, v2 = fresh.recompute(configs)
    err = {"ratio product": helpers.relerr(logratio, v1 - v0), "value": helpers.relerr(v1, v2),
           "e_cs": helpers.relerr(e_cs, fresh._get_state()[0])}
    print(err)
    assert np.max(np.abs(v1 - v0)) > 0.1
    _check(err)


def test_parameters(g):
    wf = _wf(g, "a")
    configs = _configs(g, "a")
    _, v = wf.recompute(configs)
    assert set(wf.parameters) == {"Xsupport", "alpha", "f"} and wf.parameters["f"].shape == (1,)
    wf.parameters["alpha"] = 2 * g["a_alpha"]  # log Psi is linear in alpha: no recompute needed
    assert helpers.relerr(wf.value()[1], 2 * v) < TOL
    for key, bad in (("alpha", np.zeros(5)), ("Xsupport", np.zeros((6, 3, 2))), ("f", np.zeros(2))):
        with pytest.raises(ValueError):
            wf.parameters[key] = bad
    # Xsupport / f take effect on the stored Gaussians at the next recompute
    X2, f2 = g["a_Xsupport"] + 0.1, 0.7
    wf.parameters["Xsupport"] = X2
    wf.parameters["f"] = np.array([f2])
    assert helpers.relerr(wf.value()[1], 2 * v) < TOL
    other = _wf(g, "a", X=X2, f=f2, alpha=2 * g["a_alpha"])
    _, vo = other.recompute(configs)
    assert helpers.relerr(wf.recompute(configs)[1], vo) < TOL and np.max(np.abs(vo - 2 * v)) > 1e-3
    ref = gps_ref.GpsRef(X2, 2 * g["a_alpha"], f2)
    assert helpers.relerr(vo, ref.recompute(configs.configs)) < TOL
    import pyqmc_amd as pa

    d = pa.GPSJastrow(gps_ref.case_mol("a"), g["a_Xsupport"])  # defaults of the reference: alpha zeros, f an array of one
    assert np.array_equal(d.parameters["alpha"], np.zeros(6)) and np.array_equal(d.parameters["f"], [100.0])
    assert np.array_equal(d.recompute(configs)[1], np.zeros(len(v)))


def test_errors_name_what_is_missing(g):
    import pyqmc_amd as pa

    wf = _wf(g, "a")
    with pytest.raises(_ffi.PqaError, match="pqa_gps_recompute"):
        wf._gps.call("pqa_gps_value", _ffi.ptr(np.empty(4)))
    bare = pa.DeviceWF(gps_ref.case_mol("a"))
    with pytest.raises(_ffi.PqaError, match="pqa_gps_set"):
        bare.call("pqa_gps_recompute", _ffi.ptr(np.zeros((2, 8, 3))), 2, _ffi.ptr(np.empty(2)))
    wf.recompute(_configs(g, "a"))
    with pytest.raises(_ffi.PqaError, match="electron index"):
        wf.gradient(8, OpenElectron(np.zeros((24, 3))))


@pytest.mark.parametrize("how", ["copy", "pickle"])
def test_copies_are_independent(g, how):
    wf = _wf(g, "a")
    configs = _configs(g, "a")
    _, v = wf.recompute(configs)
    twin = copy.copy(wf) if how == "copy" else pickle.loads(pickle.dumps(wf))
    assert twin._gps is not wf._gps and twin._gps._h.value != wf._gps._h.value
    for k in wf.parameters:
        assert np.array_equal(twin.parameters[k], wf.parameters[k])
    assert helpers.relerr(twin.value()[1], v) < TOL
    e = int(g["a_electrons"][0])
    ep = OpenElectron(g[f"a_e{e}_newpos"])
    assert helpers.relerr(twin.testvalue(e, ep)[0], g[f"a_e{e}_testvalue"]) < TOL
    twin.updateinternals(e, ep, configs)
    assert np.max(np.abs(twin.value()[1] - v)) > 1e-3
    assert np.array_equal(wf.value()[1], v)
    twin.parameters["alpha"] = np.zeros(6)
    assert np.array_equal(wf.value()[1], v) and np.array_equal(wf.parameters["alpha"], g["a_alpha"])


def test_product_with_slater_and_jastrow(g):
    import pyqmc_amd as pa
    from pyqmc_amd.wf import readonly_device

    mol = systems.water()
    sj = helpers.gpu_wf(mol, systems.random_mf(mol))
    sl, ja = sj.wf_factors
    gp = _wf(g, "a")
    wf = pa.MultiplyWF(sl, ja, gp)
    configs = _configs(g, "a")
    W = len(configs.configs)
    sign, logv = wf.recompute(configs)
    parts = [f.value() for f in (sl, ja, gp)]
    assert helpers.relerr(logv, sum(p[1] for p in parts)) < TOL and np.array_equal(sign, np.prod([p[0] for p in parts], axis=0))
    assert np.max(np.abs(parts[2][1])) > 0.1
    e = 5
    ep = OpenElectron(g["a_e5_newpos"])
    gs, ls = zip(*[f.gradient_laplacian(e, ep) for f in (sl, ja, gp)])
    cross = sum(np.sum(gs[i] * gs[j], axis=0) for i in range(3) for j in range(i + 1, 3))
    gr, lap = wf.gradient_laplacian(e, ep)
    assert helpers.relerr(gr, sum(gs)) < TOL and helpers.relerr(lap, sum(ls) + 2 * cross) < TOL
    assert helpers.relerr(wf.testvalue(e, ep)[0], np.prod([f.testvalue(e, ep)[0] for f in (sl, ja, gp)], axis=0)) < TOL
    # the product takes the per-factor protocol route, the fused drivers and estimators refuse it
    assert wf.fused_device() is None and readonly_device(wf) is None
    import sys

    assert sys.modules["pyqmc_amd.vmc"].device_of(wf) is None and sys.modules["pyqmc_amd.vmc"].device_of(gp) is None
    with pytest.raises(NotImplementedError, match="lives on one device handle"):
        pa.vmc_worker(wf, configs, 0.3, 1, {})
    np.random.seed(3)
    blk, configs = helpers.protocol_vmc_worker(wf, configs, 0.3, 1, {})
    assert 0.1 < blk["acceptance"] < 1.0
    _, v_run = wf.value()
    _, v_new = wf.recompute(configs)
    assert helpers.relerr(v_run, v_new) < TOL
    assert len(wf.pgradient()["wf3alpha"]) == W


def test_unit_disturbs_nothing(g):
    """A Slater x JastrowSpin wave function gives bitwise the same recompute and energy before and after a GPSJastrow is created and
    exercised on the same device."""
    mol = systems.water()
    sj = helpers.gpu_wf(mol, systems.random_mf(mol))
    configs = _configs(g, "a")
    dev = sj.fused_device()

    def both():
        s, v = sj.recompute(configs)
        return s.copy(), v.copy(), dev.energy(seed=5).copy()

    before = both()
    gp = _wf(g, "a")
    gp.recompute(configs)
    e = 1
    ep = OpenElectron(g["a_e1_newpos"])
    gp.gradient_value(e, ep)
    gp.testvalue(e, OpenElectron(g["a_e1_aux"]), g["a_e1_mask"])
    gp.updateinternals(e, ep, configs, mask=g["a_e1_accept"])
    gp.pgradient()
    after = both()
    for a, b in zip(before, after):
        assert np.array_equal(a, b)
    del gp
    for a, b in zip(before, both()):
        assert np.array_equal(a, b)
