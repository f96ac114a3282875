"""Variance optimisation on the device: pqa_variance against the reference's costs (g45) on both routes and its Nelder-Mead run,
its ke against pqa_correlated's on open, periodic and chunked handles, its gradient against central differences and the NumPy
restatement, the handle left as it was with repeatable bits, route selection, and optvariance with jac=True end to end."""

import importlib

import numpy as np
import pytest

import pyqmc_amd as pa
from pyqmc_amd import pbc, systems
from pyqmc_amd.configs import OpenConfigs, PeriodicConfigs
from tests import helpers
from tests.test_optvariance_cpu import numpy_variance

ov = importlib.import_module("pyqmc_amd.optvariance")

pytestmark = pytest.mark.gpu


def _sets(wf, K, seed, scale=0.05):
    rng = np.random.default_rng(seed)
    a0, b0 = np.asarray(wf.parameters["wf2acoeff"]), np.asarray(wf.parameters["wf2bcoeff"])
    return (np.stack([a0 + scale * rng.standard_normal(a0.shape) for _ in range(K)]),
            np.stack([b0 + scale * rng.standard_normal(b0.shape) for _ in range(K)]))


def _fixed_energy(g):
    return lambda coords, wf: {"total": g["enref_total"], "ke": g["enref_ke"]}


def test_g45_costs_both_routes(monkeypatch):
    g = helpers.golden("g45_optvariance")
    mol = systems.water()
    wf = helpers.gpu_wf(mol, systems.random_mf(mol))
    configs = OpenConfigs(g["configs"].copy())
    params = ["wf2acoeff", "wf2bcoeff"]
    assert ov.optvariance_route(wf, params) == "fused"
    x0, shapes = ov.flatten(wf, params)
    assert np.array_equal(x0, g["cost_x"][0])
    eoff = g["enref_total"] - g["enref_ke"]
    wf.recompute(configs)
    cost, cost_jac = ov._fused_cost(wf, params, shapes, eoff)
    fused = np.array([cost(x) for x in g["cost_x"]])
    assert helpers.relerr(fused, g["cost"]) < 1e-10, (fused, g["cost"])
    assert helpers.relerr([cost_jac(x)[0] for x in g["cost_x"]], g["cost"]) < 1e-10
    enacc = pa.EnergyAccumulator(mol)
    proto = ov._protocol_cost(enacc, wf, configs, params, shapes, eoff)
    got = np.array([proto(x) for x in g["cost_x"]])
    assert helpers.relerr(got, g["cost"]) < 1e-10, (got, g["cost"])


def test_g45_nelder_mead_fused():
    g = helpers.golden("g45_optvariance")
    mol = systems.water()
    wf = helpers.gpu_wf(mol, systems.random_mf(mol))
    configs = OpenConfigs(g["configs"].copy())
    assert np.array_equal(wf.parameters["wf2bcoeff"], g["nm_x0"])
    fun, out = pa.optvariance(_fixed_energy(g), wf, configs, params=["wf2bcoeff"], method="Nelder-Mead",
                              options={"maxiter": int(g["nm_maxiter"])})
    assert out is wf
    assert abs(fun - g["nm_fun"]) < 1e-8 * abs(g["nm_fun"])
    assert np.abs(wf.parameters["wf2bcoeff"] - g["nm_bcoeff"]).max() < 1e-8


def _ke_check(wf, configs, K, seed, grad):
    wf.recompute(configs)
    dev = wf.fused_device()
    acoeff, bcoeff = _sets(wf, K, seed)
    eoff = np.random.default_rng(seed + 1).standard_normal(dev.W)
    var, dvar, ke = dev.variance(acoeff, bcoeff, eoff, grad=grad, ke=True)
    _, en = dev.correlated(acoeff, bcoeff, 10.0, seed=seed)
    assert helpers.relerr(ke, en[:, 0, :]) < 1e-12, helpers.relerr(ke, en[:, 0, :])
    E = eoff + ke
    assert np.abs(var - E.var(axis=1)).max() < 1e-10 * E.var(axis=1).max()
    return var, dvar, ke


def test_ke_matches_correlated_water():
    mol = systems.water()
    wf = helpers.gpu_wf(mol, systems.random_mf(mol))
    configs = OpenConfigs(systems.initial_guess(mol, 256, rng=np.random.default_rng(1)).configs.copy())
    for grad in (False, True):
        _ke_check(wf, configs, 5, 11, grad)


def test_ke_matches_correlated_cluster_and_cell():
    mol = systems.water_cluster()
    wf = helpers.gpu_wf(mol, systems.random_mf(mol))
    _ke_check(wf, OpenConfigs(systems.initial_guess(mol, 2048, rng=np.random.default_rng(2)).configs.copy()), 3, 12, True)
    sup, wfc = helpers.gpu_pbc_wf("k222")
    x = systems.initial_guess(sup, 128, rng=np.random.default_rng(3)).configs.copy()
    _ke_check(wfc, PeriodicConfigs(x, sup.lattice_vectors()), 3, 13, True)


def test_chunked_65536_cluster():
    """(H2O)8 at 65 536 walkers: with K = 3 and the gradient the derivatives exceed one 256 MiB chunk."""
    mol = systems.water_cluster()
    wf = helpers.gpu_wf(mol, systems.random_mf(mol))
    configs = OpenConfigs(systems.initial_guess(mol, 65536, rng=np.random.default_rng(4)).configs.copy())
    dev = wf.fused_device()
    P = wf.parameters["wf2acoeff"].size + wf.parameters["wf2bcoeff"].size
    assert 3 * 65536 * P * 8 > 256 << 20
    var, dvar, ke = _ke_check(wf, configs, 3, 14, True)
    # the chunked reduction against the single-chunk one of each set alone (K = 1 fits one chunk)
    acoeff, bcoeff = _sets(wf, 3, 14)
    eoff = np.random.default_rng(15).standard_normal(dev.W)
    for k in range(3):
        v1, d1, _ = dev.variance(acoeff[k : k + 1], bcoeff[k : k + 1], eoff, grad=True)
        assert abs(v1[0] - var[k]) < 1e-12 * var[k]
        assert helpers.relerr(d1[0], dvar[k]) < 1e-11


def test_gradient_central_differences_and_numpy():
    g = helpers.golden("g45_optvariance")
    mol = systems.water()
    mf = systems.random_mf(mol)
    wf = helpers.gpu_wf(mol, mf)
    configs = OpenConfigs(g["configs"].copy())
    wf.recompute(configs)
    dev = wf.fused_device()
    eoff = g["enref_total"] - g["enref_ke"]
    acoeff, bcoeff = _sets(wf, 1, 21)
    var, dvar, ke = dev.variance(acoeff, bcoeff, eoff, grad=True, ke=True)
    c = np.concatenate([acoeff[0].ravel(), bcoeff[0].ravel()])
    Pa = acoeff[0].size
    h = 1e-5

    def v(c):
        return dev.variance(c[:Pa].reshape(acoeff.shape), c[Pa:].reshape(bcoeff.shape), eoff)[0][0]

    fd = np.array([(v(c + h * e) - v(c - h * e)) / (2 * h) for e in np.eye(c.size)])
    assert helpers.relerr(dvar[0], fd) < 1e-6, helpers.relerr(dvar[0], fd)
    nv, nd, nk = numpy_variance(helpers.oracle_wf(mol, mf), configs, acoeff[0], bcoeff[0], eoff)
    assert helpers.relerr(ke[0], nk) < 1e-11 and abs(var[0] - nv) < 1e-10 * nv
    assert helpers.relerr(dvar[0], nd) < 1e-9, helpers.relerr(dvar[0], nd)


def test_read_only_and_repeatable():
    mol = systems.water()
    wf = helpers.gpu_wf(mol, systems.random_mf(mol))
    dev = wf.fused_device()
    configs = OpenConfigs(systems.initial_guess(mol, 512, rng=np.random.default_rng(5)).configs.copy())
    wf.recompute(configs)
    dev.vmc_sweeps(0.3, 2, seed=9, energy=False)  # (state after a fused sweep)
    sl, ja = wf.wf_factors
    a0, b0 = np.asarray(ja.parameters["acoeff"]), np.asarray(ja.parameters["bcoeff"])
    before = (wf.value()[1], dev.configs(), sl._get_state(0), sl._get_state(1))
    own = dev.correlated(a0[None], b0[None], 10.0, seed=3)
    acoeff, bcoeff = _sets(wf, 4, 6)
    eoff = np.random.default_rng(6).standard_normal(dev.W)
    r1 = dev.variance(acoeff, bcoeff, eoff, grad=True, ke=True)
    r2 = dev.variance(acoeff, bcoeff, eoff, grad=True, ke=True)
    assert all(np.array_equal(x, y) for x, y in zip(r1, r2))
    after = (wf.value()[1], dev.configs(), sl._get_state(0), sl._get_state(1))
    assert np.array_equal(before[0], after[0]) and np.array_equal(before[1], after[1])
    for s in (2, 3):
        assert all(np.array_equal(x, y) for x, y in zip(before[s], after[s]))
    again = dev.correlated(a0[None], b0[None], 10.0, seed=3)
    assert np.array_equal(own[0], again[0]) and np.array_equal(own[1], again[1])
    p = np.empty(a0.size)
    dev.call("pqa_get_param", b"acoeff", pa._ffi.ptr(p), p.size)
    assert np.array_equal(p.reshape(a0.shape), a0)


def test_routes():
    mol = systems.water()
    mf = systems.random_mf(mol)
    wf = helpers.gpu_wf(mol, mf)
    assert ov.optvariance_route(wf, ["wf2acoeff", "wf2bcoeff"]) == "fused"
    assert ov.optvariance_route(wf, ["wf2bcoeff"]) == "fused"
    assert ov.optvariance_route(wf, None) == "protocol"
    assert ov.optvariance_route(wf, ["wf2bcoeff", "wf1mo_coeff_alpha"]) == "protocol"
    assert ov.optvariance_route(wf, ["wf1det_coeff"]) == "protocol"
    mfd = systems.random_mf(mol, nvirt=6)
    wfd = helpers.gpu_wf(mol, mfd, determinants=systems.random_determinants(mol, mfd, 4))
    assert ov.optvariance_route(wfd, ["wf2bcoeff"]) == "protocol"
    wf3 = pa.generate_wf(mol, mf, jastrow3=True)
    assert ov.optvariance_route(wf3, ["wf2bcoeff"]) == "protocol"
    c3 = pbc.get_supercell(systems.diamond_primitive(), np.array([[-1.0, 1, 1], [1, -1, 1], [1, 1, -1]]))
    wfc = pa.generate_wf(c3, pbc.random_kmf(c3, complex_coeff=True, twist=(0.25, 0.1, -0.3)))
    assert ov.optvariance_route(wfc, ["wf2bcoeff"]) == "protocol"
    configs = OpenConfigs(systems.initial_guess(mol, 64, rng=np.random.default_rng(8)).configs.copy())
    wf.recompute(configs)
    with pytest.raises(ValueError, match="jac=True"):
        pa.optvariance(pa.EnergyAccumulator(mol), wf, configs, params=["wf2bcoeff", "wf1mo_coeff_alpha"], jac=True, method="BFGS")
    with pytest.raises(pa._ffi.PqaError, match="pqa_variance"):
        wfd.recompute(configs)
        a, b = _sets(wfd, 1, 1)
        wfd.fused_device().variance(a, b, np.zeros(64))


def test_optvariance_bfgs_jac_water():
    mol = systems.water()
    wf = pa.generate_wf(mol, systems.model_mf(mol))
    configs = pa.initial_guess(mol, 1024, rng=np.random.default_rng(31))
    pa.vmc(wf, configs, nblocks=2, nsteps_per_block=10, tstep=0.3, verbose=False)
    rng = np.random.default_rng(32)
    wf.parameters["wf2acoeff"] = wf.parameters["wf2acoeff"] + 0.1 * rng.standard_normal(wf.parameters["wf2acoeff"].shape)
    wf.parameters["wf2bcoeff"] = wf.parameters["wf2bcoeff"] + 0.1 * rng.standard_normal(wf.parameters["wf2bcoeff"].shape)
    params = ["wf2acoeff", "wf2bcoeff"]
    wf.recompute(configs)
    enacc = pa.EnergyAccumulator(mol)
    en = enacc(configs, wf)
    start = np.var(en["total"])
    fun, wf = pa.optvariance(enacc, wf, configs, params=params, jac=True, method="BFGS", options={"maxiter": 30})
    print("variance", start, "->", fun)
    assert fun < 0.9 * start
    # the handle's state is a fresh recompute at the returned parameters
    dev = wf.fused_device()
    twin = pa.generate_wf(mol, systems.model_mf(mol))
    for k in params:
        twin.parameters[k] = wf.parameters[k]
    lt = twin.recompute(configs)[1]
    assert np.array_equal(dev.configs(), configs.configs)
    assert np.abs(wf.value()[1] - lt).max() < 1e-12 * max(1.0, np.abs(lt).max())
    e2 = twin.fused_device().energy(10.0, seed=5)
    assert helpers.relerr(dev.energy(10.0, seed=5), e2) < 1e-12
