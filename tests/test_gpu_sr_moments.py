"""Stochastic-reconfiguration moments from the resident state (pqa_sr_moments) against the protocol route (pgradient, energy, pqa_gram)
on the same walkers and energy draws: tile and slice tails, the regularisation branch against NumPy, more than one tile each way and
the mirrored triangle, several slices, the handle left as it was, gradient-VMC blocks on open and periodic handles, and the scope.

Tolerance: both routes use the same per-walker numbers and differ in summation order only (~ W 2^-53), checked at the 1e-9 that
test_gpu_linemin.py::test_routes sets for its two routes; two device calls give the same bits."""

import copy
import importlib

import numpy as np
import pytest

import pyqmc_amd as pa
from pyqmc_amd import pbc, systems
from pyqmc_amd import wf as pwf
from pyqmc_amd.accumulators import gradient_generator, nodal_regularization, sr_columns, sr_route
from pyqmc_amd.configs import OpenConfigs, PeriodicConfigs
from tests import helpers

pytestmark = pytest.mark.gpu

TOL = 1e-9
pvmc = importlib.import_module("pyqmc_amd.vmc")


def _water(ndet=1, jastrow3=False):
    mol = systems.water()
    if ndet > 1:
        mf = systems.random_mf(mol, nvirt=6)
        return mol, helpers.gpu_wf(mol, mf, determinants=systems.random_determinants(mol, mf, ndet))
    if jastrow3:
        wf = pa.generate_wf(mol, systems.random_mf(mol), jastrow3=True)
        wf.parameters["wf2acoeff"], wf.parameters["wf2bcoeff"] = helpers.jastrow_params(mol)
        wf.parameters["wf3ccoeff"] = 0.02 * np.random.default_rng(12).standard_normal(np.shape(wf.parameters["wf3ccoeff"]))
        return mol, wf
    return mol, helpers.gpu_wf(mol, systems.random_mf(mol))


def _walkers(mol, W, seed):
    return OpenConfigs(systems.initial_guess(mol, W, rng=np.random.default_rng(seed)).configs.copy())


def _pair(mol, wf, seed=100):
    """The same accumulator once per route, with the same energy key sequence."""
    out = []
    for route in ("device", "protocol"):
        sr = gradient_generator(mol, wf, pwf.default_to_opt(wf), route=route)
        sr.enacc.seed = seed
        out.append(sr)
    return out


def _agree(d, p):
    assert sorted(d) == sorted(p)
    for k in p:
        err = helpers.relerr(d[k], p[k])
        print(k, err)
        assert np.shape(d[k]) == np.shape(p[k]) and err < TOL, (k, err)


def test_tile_and_slice_tails():
    mol, wf = _water(ndet=4)
    configs = _walkers(mol, 200, 1)  # 3 * 64 + 8 walkers
    wf.recompute(configs)
    sd, sp = _pair(mol, wf)
    assert sd.transform.nparams % 16 != 0 and "wf1det_coeff" in sd.transform.to_opt
    _agree(sd.avg(configs, wf), sp.avg(configs, wf))
    assert sd.last_route == "device" and sp.last_route == "protocol"
    wts = 0.5 + np.random.default_rng(2).random(200)
    _agree(sd.avg(configs, wf, weights=wts), sp.avg(configs, wf, weights=wts))
    assert sd.last_route == "device" and sp.last_route == "protocol"
    auto = gradient_generator(mol, wf, pwf.default_to_opt(wf))
    assert sr_route(wf, auto)[0] == "device"


def test_against_numpy_and_regularisation_branch():
    mol, wf = _water(ndet=4)
    W = 200
    configs = _walkers(mol, W, 3)
    wf.recompute(configs)
    dev = wf.fused_device()
    en = dev.energy(10.0, seed=77)
    cut = float(np.median(en[4]) ** -0.5)
    near, f = nodal_regularization(en[4], cut)
    assert near.any() and (~near).any()
    tr = gradient_generator(mol, wf, pwf.default_to_opt(wf)).transform
    src, pos = sr_columns(tr)
    mean, mom, enw = dev.sr_moments(src, pos, cut, seed=77, per_walker=True)
    assert np.array_equal(enw.T, en)
    dp = tr.serialize_gradients(wf.pgradient())
    ref = np.concatenate((dp, enw[:, 5:6], np.ones((W, 1))), axis=1).T @ (f[:, None] * dp / W)
    for name, a, b in (("dpidpj", mom[:-2], ref[:-2]), ("dpH", mom[-2], ref[-2]), ("dppsi", mom[-1], ref[-1]), ("means", mean, en.mean(axis=1))):
        err = helpers.relerr(a, b)
        print(name, err)
        assert err < TOL, (name, err)
    # the weight really acts: the unregularised moments differ
    assert helpers.relerr(dev.sr_moments(src, pos, 1e-3, seed=77)[1][-1], ref[-1]) > 1e-3


def test_many_tiles_and_mirror():
    mol, wf = _water(jastrow3=True)
    configs = _walkers(mol, 96, 4)
    wf.recompute(configs)
    sd, sp = _pair(mol, wf)
    assert sd.transform.nparams > 32 and "wf3ccoeff" in sd.transform.to_opt
    d, p = sd.avg(configs, wf), sp.avg(configs, wf)
    _agree(d, p)
    assert np.array_equal(d["dpidpj"], d["dpidpj"].T)


def test_several_slices_and_determinism():
    mol, wf = _water()
    configs = _walkers(mol, 4096, 5)
    wf.recompute(configs)
    sd, sp = _pair(mol, wf)
    d = sd.avg(configs, wf)
    _agree(d, sp.avg(configs, wf))
    sd.enacc._calls = 0  # (the same energy key again)
    d2 = sd.avg(configs, wf)
    assert all(np.array_equal(d[k], d2[k]) for k in d)


def test_state_untouched():
    mol, wf = _water()
    dev = wf.fused_device()
    configs = _walkers(mol, 512, 6)
    wf.recompute(configs)
    twin = copy.deepcopy(wf)  # (rebuilt from the same walkers: the same state)
    for d in (dev, twin.fused_device()):
        d.vmc_sweeps(0.3, 2, seed=9, energy=False)  # (state after a fused sweep: layouts and stale sums as a driver leaves them)
    sl = wf.wf_factors[0]
    before = (wf.value()[1], dev.configs(), sl._get_state(0), sl._get_state(1))
    src, pos = sr_columns(gradient_generator(mol, wf, pwf.default_to_opt(wf)).transform)
    dev.sr_moments(src, pos, 1e-3, seed=21)
    after = (wf.value()[1], dev.configs(), sl._get_state(0), sl._get_state(1))
    assert np.array_equal(before[0], after[0]) and np.array_equal(before[1], after[1])
    for s in (2, 3):
        assert all(np.array_equal(x, y) for x, y in zip(before[s], after[s]))
    # a VMC trajectory after the call is the one the untouched twin makes
    r1 = dev.vmc_sweeps(0.3, 3, seed=33)
    r2 = twin.fused_device().vmc_sweeps(0.3, 3, seed=33)
    assert np.array_equal(r1[0], r2[0]) and np.array_equal(r1[1], r2[1])
    assert np.array_equal(dev.configs(), twin.fused_device().configs())


def _blocks(mol, wf, start, nsteps, monkeypatch):
    """One vmc_worker block per route from the same walkers, random state and energy keys -> {route: (block, configs, fetches)}."""
    out = {}
    fetch = pvmc._fetch
    for sr in _pair(mol, wf):
        calls = []
        monkeypatch.setattr(pvmc, "_fetch", lambda dev, configs: (calls.append(1), fetch(dev, configs))[1])
        np.random.seed(11)
        cfg = copy.deepcopy(start)
        blk, cfg = pa.vmc_worker(wf, cfg, 0.3, nsteps, {"pgrad": sr}, seed=5)
        monkeypatch.setattr(pvmc, "_fetch", fetch)
        out[sr.route] = (blk, cfg, len(calls))
        assert sr.last_route == sr.route
    bd, bp = out["device"][0], out["protocol"][0]
    assert sorted(bd) == sorted(bp) and {"pgraddpidpj", "pgradtotal", "acceptance", "move time", "accumulator time"} <= set(bd)
    for k in bp:
        if "time" not in k:
            err = helpers.relerr(bd[k], bp[k])
            print(k, err)
            assert err < TOL, (k, err)
    assert np.array_equal(out["device"][1].configs, out["protocol"][1].configs)
    return out


def test_block_open(monkeypatch):
    mol, wf = _water()
    out = _blocks(mol, wf, _walkers(mol, 256, 7), 3, monkeypatch)
    assert out["device"][2] == 1 and out["protocol"][2] == 3
    assert np.array_equal(out["device"][1].configs, wf.fused_device().configs())


def test_block_periodic(monkeypatch):
    sup, wf = helpers.gpu_pbc_wf("fcc2cubic")
    assert not wf.fused_device().cplx
    x = systems.initial_guess(sup, 64, rng=np.random.default_rng(8)).configs.copy()
    out = _blocks(sup, wf, PeriodicConfigs(x, sup.lattice_vectors()), 2, monkeypatch)
    assert np.array_equal(out["device"][1].wrap, out["protocol"][1].wrap)
    assert out["device"][2] == 2 and out["protocol"][2] == 2  # (periodic containers carry every sweep's wrap counters)


def test_scope():
    c3 = pbc.get_supercell(systems.diamond_primitive(), np.array([[-1.0, 1, 1], [1, -1, 1], [1, 1, -1]]))
    wfc = pa.generate_wf(c3, pbc.random_kmf(c3, complex_coeff=True, twist=(0.25, 0.1, -0.3)))
    sr = gradient_generator(c3, wfc, pwf.default_to_opt(wfc))
    assert sr.resolve_route(wfc) == "protocol" and "complex" in sr_route(wfc, sr)[1]
    with pytest.raises(NotImplementedError, match="complex"):
        gradient_generator(c3, wfc, pwf.default_to_opt(wfc), route="device")
    mol, wf = _water()
    orb = gradient_generator(mol, wf, pwf.default_to_opt(wf, optimize_orbitals=True))
    assert orb.resolve_route(wf) == "protocol" and "mo_coeff" in sr_route(wf, orb)[1]
    # the library refuses what the Python side would not send: a column of a factor the handle lacks, a position out of range
    dev = wf.fused_device()
    wf.recompute(_walkers(mol, 64, 9))
    for src, pos in (([3], [0]), ([2], [12]), ([4], [0])):
        with pytest.raises(pa._ffi.PqaError, match="pqa_sr_moments"):
            dev.sr_moments(src, pos, 1e-3)
