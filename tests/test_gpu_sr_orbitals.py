"""Orbital-coefficient columns of the SR moments from the resident state (pqa_sr_moments_orb, k_sr_orb) against the protocol route
(pgradient with k_pgrad_mo, energy, pqa_gram) on the same walkers and energy key; the per-walker matrix dp_walker against
serialize_gradients(wf.pgradient()) and, on g18's state, against the reference's own gradients.

Bound: helpers.relerr < 1e-9 for every key of avg and for dp_walker, the bound of test_gpu_sr_moments.py (from
test_gpu_linemin.py::test_routes): the routes share the per-walker inputs and differ in summation order.  Every figure is printed
before it is asserted.  Shapes are the smallest that reach each tail of k_sr_orb: the AO-tile tail (23 = 16 + 7), k tails on either
spin, one and two orbital tiles, several determinants with unoccupied orbitals, a sparse column map, several walker chunks."""

import ast
import copy
import importlib

import numpy as np
import pytest

import pyqmc_amd as pa
from pyqmc_amd import pbc, systems
from pyqmc_amd import wf as pwf
from pyqmc_amd.accumulators import gradient_generator, sr_columns_orb, sr_route
from pyqmc_amd.configs import OpenConfigs, PeriodicConfigs
from tests import helpers

pytestmark = pytest.mark.gpu

TOL = 1e-9
pvmc = importlib.import_module("pyqmc_amd.vmc")


def _mol53():
    sym, xyz = zip(*systems._WATER)
    return systems.Mol(sym, xyz, nelec=(5, 3))


def _walkers(mol, W, seed):
    return OpenConfigs(systems.initial_guess(mol, W, rng=np.random.default_rng(seed)).configs.copy())


def _pair(mol, wf, to_opt=None, seed=100):
    """The same accumulator once per route, with the same energy key sequence."""
    out = []
    for route in ("device", "protocol"):
        sr = gradient_generator(mol, wf, to_opt or pwf.default_to_opt(wf, optimize_orbitals=True), route=route)
        sr.enacc.seed = seed
        out.append(sr)
    return out


def _agree(d, p):
    assert sorted(d) == sorted(p)
    for k in p:
        err = helpers.relerr(d[k], p[k])
        print(k, np.shape(p[k]), err)
        assert np.shape(d[k]) == np.shape(p[k]) and err < TOL, (k, err)


def _dp(wf, transform, **kw):
    """dp_walker of the device call and the protocol route's serialised derivatives."""
    src, pos = sr_columns_orb(transform)
    out = wf.fused_device().sr_moments_orb(src, pos, 1e-3, seed=5, dp_walker=True, **kw)
    return out[-1], transform.serialize_gradients(wf.pgradient()), out


def _check(mol, wf, W, seed, weights=False, to_opt=None):
    configs = _walkers(mol, W, seed)
    wf.recompute(configs)
    sd, sp = _pair(mol, wf, to_opt)
    assert {"wf1mo_coeff_alpha", "wf1mo_coeff_beta"} <= set(sd.transform.to_opt)
    wts = 0.5 + np.random.default_rng(seed + 1).random(W) if weights else None
    d, p = sd.avg(configs, wf, weights=wts), sp.avg(configs, wf, weights=wts)
    assert sd.last_route == "device" and sp.last_route == "protocol"
    _agree(d, p)
    dp, ref, _ = _dp(wf, sd.transform)
    err = helpers.relerr(dp, ref)
    print("dp_walker", dp.shape, err)
    assert dp.shape == ref.shape and err < TOL, err
    return d, dp


def test_water_single_determinant():
    """23 AOs (a-tile tail), 4 + 4 electrons (one k-step), 4 orbitals (one orbital tile), weights."""
    mol = systems.water()
    wf = helpers.gpu_wf(mol, systems.random_mf(mol))
    d, dp = _check(mol, wf, 70, 1, weights=True)
    assert dp.shape[1] == d["dpidpj"].shape[0] > 2 * 23 * 4


def test_unequal_spins():
    """nelec = (5, 3): k tails on both spins, 5 and 3 orbitals."""
    mol = _mol53()
    _check(mol, helpers.gpu_wf(mol, systems.random_mf(mol)), 70, 2)


def test_all_electron_general_basis():
    """24 AOs, 5 + 5 electrons, no ECP pass."""
    mol = systems.water_general()
    wf = pa.generate_wf(mol, systems.random_mf(mol))  # (its default Jastrow basis starts with the ion cusp: keep those entries)
    rng = np.random.default_rng(11)
    a, b = np.array(wf.parameters["wf2acoeff"]), np.array(wf.parameters["wf2bcoeff"])
    a[:, 1:, :] = 0.05 * rng.standard_normal(a[:, 1:, :].shape)
    b[1:] = 0.05 * rng.standard_normal(b[1:].shape)
    wf.parameters["wf2acoeff"], wf.parameters["wf2bcoeff"] = a, b
    assert wf.fused_device().nao == 24 and wf.fused_device().nelec == (5, 5) and wf.fused_device().necp == 0
    _check(mol, wf, 40, 3)


def test_multideterminant_against_the_reference():
    """g18's state (12 determinants with 6 virtuals, three-body factor, g18's walkers): dp_walker against the reference's own
    gradients; beta orbital 6 is occupied in no determinant: its columns are exactly zero."""
    g = helpers.golden("g18_testvalue_many")
    g7 = helpers.golden("g7_jastrow3_multidet")
    mol = systems.water()
    wf = helpers.gpu_wf3(mol, systems.random_mf(mol, nvirt=6), ast.literal_eval(str(g7["det_json"])))
    configs = OpenConfigs(g["h2o_configs"].copy())
    wf.recompute(configs)
    sd, sp = _pair(mol, wf)
    assert set(sd.transform.to_opt) == {"wf1det_coeff", "wf1mo_coeff_alpha", "wf1mo_coeff_beta", "wf2acoeff", "wf2bcoeff", "wf3ccoeff"}
    _agree(sd.avg(configs, wf), sp.avg(configs, wf))
    dp, ours, _ = _dp(wf, sd.transform)
    ref = sd.transform.serialize_gradients({k: g["h2o_pgrad_" + k] for k in g["h2o_pgrad_keys"].tolist()})
    for name, r in (("reference", ref), ("protocol", ours)):
        err = helpers.relerr(dp, r)
        print("dp_walker against the", name, dp.shape, err)
        assert err < TOL, (name, err)
    dev = wf.fused_device()
    free = sorted(set(range(dev.nmo[1])) - set(np.unique(dev.det_occup[1]).tolist()))
    assert free == [6]
    src, pos = sr_columns_orb(sd.transform)
    cols = np.flatnonzero((src == 5) & (pos % dev.nmo[1] == 6))
    assert len(cols) == dev.nao and np.all(dp[:, cols] == 0.0) and np.all(ref[:, cols] == 0.0)


def test_two_orbital_tiles_sparse_selection():
    """(H2O)5 in a row: 115 AOs (8 AO tiles with a tail), 20 + 20 electrons and orbitals (two orbital tiles, 5 k-steps); the Jastrow
    coefficients and a seeded ~10 % of each orbital matrix."""
    mol = systems.water_cluster(5, 1, 1)
    wf = helpers.gpu_wf(mol, systems.random_mf(mol))
    to_opt = pwf.default_to_opt(wf, optimize_orbitals=True)
    rng = np.random.default_rng(17)
    for k in ("wf1mo_coeff_alpha", "wf1mo_coeff_beta"):
        assert to_opt[k].shape == (115, 20)
        to_opt[k] = rng.random(to_opt[k].shape) < 0.1
    d, _ = _check(mol, wf, 48, 4, to_opt=to_opt)
    P = d["dpidpj"].shape[0]
    print("P", P)
    assert 300 < P < 1000
    assert np.array_equal(d["dpidpj"], d["dpidpj"].T)


def test_walker_chunks_and_determinism():
    mol = systems.water()
    wf = helpers.gpu_wf(mol, systems.random_mf(mol))
    configs = _walkers(mol, 70, 6)
    wf.recompute(configs)
    tr = gradient_generator(mol, wf, pwf.default_to_opt(wf, optimize_orbitals=True), route="device").transform
    dp1, ref, one = _dp(wf, tr)
    dp3, _, three = _dp(wf, tr, walker_chunk=24)  # 24 + 24 + 22
    assert np.array_equal(dp1, dp3)
    for name, a, b in (("means", three[0], one[0]), ("moments", three[1], one[1])):
        err = helpers.relerr(a, b)
        print(name, err)
        assert err < TOL, (name, err)
    assert np.array_equal(three[0], one[0])  # (the means do not depend on the chunks)
    # two calls, same key: the same bits, for either chunking
    again1, again3 = _dp(wf, tr)[2], _dp(wf, tr, walker_chunk=24)[2]
    assert all(np.array_equal(x, y) for x, y in zip(one, again1)) and all(np.array_equal(x, y) for x, y in zip(three, again3))
    # without an orbital source the new entry gives the old entry's bits
    plain = gradient_generator(mol, wf, pwf.default_to_opt(wf)).transform
    src, pos = sr_columns_orb(plain)
    dev = wf.fused_device()
    old, new = dev.sr_moments(src, pos, 1e-3, seed=5), dev.sr_moments_orb(src, pos, 1e-3, seed=5)
    assert all(np.array_equal(x, y) for x, y in zip(old, new))


def test_three_entries_one_driver():
    """The 200-walker (3 x 64 + 8), 4-determinant water case of test_gpu_sr_moments.py, P no multiple of 16, with and without weights:
    pqa_sr_moments_orb with sources 0 - 2 only gives pqa_sr_moments' bits, and pqa_sr_moments_c with an empty tail gives them as real
    parts, with imaginary parts that are exactly zero."""
    mol = systems.water()
    mf = systems.random_mf(mol, nvirt=6)
    wf = helpers.gpu_wf(mol, mf, determinants=systems.random_determinants(mol, mf, 4))
    wf.recompute(_walkers(mol, 200, 1))
    dev = wf.fused_device()
    src, pos = sr_columns_orb(gradient_generator(mol, wf, pwf.default_to_opt(wf)).transform)
    assert len(src) % 16 != 0 and set(src.tolist()) == {0, 1, 2}
    for wts in (None, 0.5 + np.random.default_rng(2).random(200)):
        mean, mom = dev.sr_moments(src, pos, 1e-3, weights=wts, seed=5)
        orb = dev.sr_moments_orb(src, pos, 1e-3, weights=wts, seed=5)
        meanc, momc = dev.sr_moments_c(src, pos, [], 1e-3, weights=wts, seed=5)
        assert np.array_equal(orb[0], mean) and np.array_equal(orb[1], mom)
        assert momc.shape == mom.shape and meanc.shape == mean.shape
        assert np.array_equal(momc.real, mom) and np.array_equal(meanc.real, mean)
        assert np.all(momc.imag == 0) and np.all(meanc.imag == 0)


def test_state_untouched():
    mol = systems.water()
    wf = helpers.gpu_wf(mol, systems.random_mf(mol))
    dev = wf.fused_device()
    configs = _walkers(mol, 512, 7)
    wf.recompute(configs)
    twin = copy.deepcopy(wf)  # (rebuilt from the same walkers: the same state)
    for d in (dev, twin.fused_device()):
        d.vmc_sweeps(0.3, 2, seed=9, energy=False)  # (state after a fused sweep: layouts and stale sums as a driver leaves them)
    sl = wf.wf_factors[0]
    before = (wf.value()[1], dev.configs(), sl._get_state(0), sl._get_state(1))
    src, pos = sr_columns_orb(gradient_generator(mol, wf, pwf.default_to_opt(wf, optimize_orbitals=True), route="device").transform)
    dev.sr_moments_orb(src, pos, 1e-3, seed=21)
    after = (wf.value()[1], dev.configs(), sl._get_state(0), sl._get_state(1))
    assert np.array_equal(before[0], after[0]) and np.array_equal(before[1], after[1])
    for s in (2, 3):
        assert all(np.array_equal(x, y) for x, y in zip(before[s], after[s]))
    # a VMC trajectory after the call is the one the untouched twin makes
    r1 = dev.vmc_sweeps(0.3, 3, seed=33)
    r2 = twin.fused_device().vmc_sweeps(0.3, 3, seed=33)
    assert np.array_equal(r1[0], r2[0]) and np.array_equal(r1[1], r2[1])
    assert np.array_equal(dev.configs(), twin.fused_device().configs())


def test_block(monkeypatch):
    """One vmc_worker block of 3 sweeps per route from the same walkers, random state and energy keys: the device route keeps the walkers
    resident (one fetch against three)."""
    mol = systems.water()
    wf = helpers.gpu_wf(mol, systems.random_mf(mol))
    start = _walkers(mol, 256, 8)
    out = {}
    fetch = pvmc._fetch
    for sr in _pair(mol, wf):
        calls = []
        monkeypatch.setattr(pvmc, "_fetch", lambda dev, configs: (calls.append(1), fetch(dev, configs))[1])
        np.random.seed(11)
        blk, cfg = pa.vmc_worker(wf, copy.deepcopy(start), 0.3, 3, {"pgrad": sr}, seed=5)
        monkeypatch.setattr(pvmc, "_fetch", fetch)
        out[sr.route] = (blk, cfg, len(calls))
        assert sr.last_route == sr.route
    bd, bp = out["device"][0], out["protocol"][0]
    assert sorted(bd) == sorted(bp) and {"pgraddpidpj", "pgraddpH", "pgraddppsi", "pgradtotal", "acceptance"} <= set(bd)
    for k in bp:
        if "time" not in k:
            err = helpers.relerr(bd[k], bp[k])
            print(k, err)
            assert err < TOL, (k, err)
    assert np.array_equal(out["device"][1].configs, out["protocol"][1].configs)
    assert out["device"][2] == 1 and out["protocol"][2] == 3


def test_scope():
    mol = systems.water()
    wf = helpers.gpu_wf(mol, systems.random_mf(mol))
    orbitals = pwf.default_to_opt(wf, optimize_orbitals=True)
    # not asked for: the protocol route, as before
    auto = gradient_generator(mol, wf, orbitals)
    assert auto.resolve_route(wf) == "protocol" and "mo_coeff" in sr_route(wf, auto)[1] and "route='device'" in sr_route(wf, auto)[1]
    assert gradient_generator(mol, wf, orbitals, route="device").resolve_route(wf) == "device"
    # the library: a position outside (nao, nmo), a column named twice, the old entry keeps refusing source 4
    dev = wf.fused_device()
    wf.recompute(_walkers(mol, 64, 9))
    for src, pos in (([4], [dev.nao * dev.nmo[0]]), ([5], [-1]), ([4, 4], [3, 3]), ([6], [0])):
        with pytest.raises(pa._ffi.PqaError, match="pqa_sr_moments_orb"):
            dev.sr_moments_orb(src, pos, 1e-3)
    with pytest.raises(pa._ffi.PqaError, match="pqa_sr_moments"):
        dev.sr_moments([4], [0], 1e-3)
    # a periodic Gamma cell (real orbitals, per-k parameter layout): Python refuses, and so does the library itself
    sup, pwfn = helpers.gpu_pbc_wf("fcc2cubic")
    pdev = pwfn.fused_device()
    assert not pdev.cplx
    with pytest.raises(NotImplementedError, match="unfold_mo_gradient"):
        gradient_generator(sup, pwfn, pwf.default_to_opt(pwfn, optimize_orbitals=True), route="device")
    assert gradient_generator(sup, pwfn, pwf.default_to_opt(pwfn, optimize_orbitals=True)).resolve_route(pwfn) == "protocol"
    pwfn.recompute(PeriodicConfigs(systems.initial_guess(sup, 16, rng=np.random.default_rng(8)).configs.copy(), sup.lattice_vectors()))
    with pytest.raises(NotImplementedError, match="periodic"):
        pdev.sr_moments_orb([4], [0], 1e-3)
    src, pos = np.array([4], dtype=np.int32), np.array([0], dtype=np.int32)
    mean, mom = np.empty(6), np.empty((3, 1))
    ptr = pa._ffi.ptr
    with pytest.raises(pa._ffi.PqaError, match="periodic cell"):
        pdev.call("pqa_sr_moments_orb", 1, ptr(src), ptr(pos), 1e-3, None, 10.0, None, None, 0, 0, ptr(mean), ptr(mom), None, None)
    # a complex cell
    c3 = pbc.get_supercell(systems.diamond_primitive(), np.array([[-1.0, 1, 1], [1, -1, 1], [1, 1, -1]]))
    wfc = pa.generate_wf(c3, pbc.random_kmf(c3, complex_coeff=True, twist=(0.25, 0.1, -0.3)))
    with pytest.raises(NotImplementedError, match="complex"):
        gradient_generator(c3, wfc, pwf.default_to_opt(wfc, optimize_orbitals=True), route="device")
    with pytest.raises(NotImplementedError, match="complex"):
        wfc.fused_device().sr_moments_orb([4], [0], 1e-3)
