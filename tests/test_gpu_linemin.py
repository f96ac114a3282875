"""Line minimisation on the device: pqa_correlated against the per-set sequence it replaces (set, recompute, energy) on open,
periodic and > 32-per-spin handles, K = 1 at the handle's own coefficients, the handle left as it was, the reference's values
(g43 b, c) with its draws replayed, route selection and agreement of the routes, and line_minimization end to end with a
restart from its file."""

import copy

import numpy as np
import pytest

import pyqmc_amd as pa
from pyqmc_amd import linemin, pbc, systems
from pyqmc_amd import wf as pwf
from pyqmc_amd.accumulators import gradient_generator
from pyqmc_amd.configs import OpenConfigs, PeriodicConfigs
from tests import helpers

pytestmark = pytest.mark.gpu

TOL = 1e-10


def _container(mol, x):
    return PeriodicConfigs(x, mol.lattice_vectors()) if hasattr(mol, "a") else OpenConfigs(x)


def _sets(wf, K, seed):
    rng = np.random.default_rng(seed)
    a0, b0 = np.asarray(wf.parameters["wf2acoeff"]), np.asarray(wf.parameters["wf2bcoeff"])
    return (np.stack([a0 + 0.05 * rng.standard_normal(a0.shape) for _ in range(K)]),
            np.stack([b0 + 0.05 * rng.standard_normal(b0.shape) for _ in range(K)]))


def _per_set(wf, configs, acoeff, bcoeff, seed):
    """The sequence pqa_correlated stands in for, on a copy of wf."""
    w = copy.deepcopy(wf)
    dev = w.fused_device()
    out_l, out_e = [], []
    for a, b in zip(acoeff, bcoeff):
        w.parameters["wf2acoeff"], w.parameters["wf2bcoeff"] = a, b
        out_l.append(w.recompute(configs)[1])
        out_e.append(dev.energy(10.0, seed=seed))
    return np.array(out_l), np.array(out_e)


def _check(wf, configs, K, seed=17):
    acoeff, bcoeff = _sets(wf, K, seed)
    wf.recompute(configs)
    dev = wf.fused_device()
    lp, en = dev.correlated(acoeff, bcoeff, 10.0, seed=seed)
    rl, re = _per_set(wf, configs, acoeff, bcoeff, seed)
    assert np.abs(lp - rl).max() < TOL * max(1.0, np.abs(rl).max())
    scale = np.maximum(1.0, np.abs(re).max(axis=2, keepdims=True))
    assert (np.abs(en - re) / scale).max() < TOL, np.abs(en - re).max(axis=(0, 2))
    assert np.ptp(en[:, 0, :].mean(axis=1)) > 1e-6  # (the sets really differ)


def test_correlated_water():
    mol = systems.water()
    wf = helpers.gpu_wf(mol, systems.random_mf(mol))
    _check(wf, OpenConfigs(systems.initial_guess(mol, 256, rng=np.random.default_rng(1)).configs.copy()), 5)


@pytest.mark.parametrize("W", [4096, 65536])
def test_correlated_cluster(W):
    mol = systems.water_cluster()
    wf = helpers.gpu_wf(mol, systems.random_mf(mol))
    _check(wf, OpenConfigs(systems.initial_guess(mol, W, rng=np.random.default_rng(2)).configs.copy()), 3 if W > 4096 else 6)


def test_correlated_diamond_cell():
    sup, wf = helpers.gpu_pbc_wf("k222")
    x = systems.initial_guess(sup, 128, rng=np.random.default_rng(3)).configs.copy()
    _check(wf, _container(sup, x), 4)


def test_correlated_above_32_per_spin():
    mol = systems.water_cluster(3, 3, 2)
    wf = helpers.gpu_wf(mol, systems.random_mf(mol))
    _check(wf, OpenConfigs(systems.initial_guess(mol, 64, rng=np.random.default_rng(4)).configs.copy()), 3)


def test_k1_at_own_coefficients_and_state_unchanged():
    mol = systems.water()
    wf = helpers.gpu_wf(mol, systems.random_mf(mol))
    dev = wf.fused_device()
    configs = OpenConfigs(systems.initial_guess(mol, 512, rng=np.random.default_rng(5)).configs.copy())
    wf.recompute(configs)
    twin = copy.deepcopy(wf)  # (rebuilt from the same walkers: the same state)
    for d in (dev, twin.fused_device()):
        d.vmc_sweeps(0.3, 2, seed=9, energy=False)  # (state after a fused sweep: layouts and stale sums as a driver leaves them)
    sl, ja = wf.wf_factors
    before = (wf.value()[1], dev.configs(), sl._get_state(0), sl._get_state(1))
    a0, b0 = np.asarray(ja.parameters["acoeff"]), np.asarray(ja.parameters["bcoeff"])
    lp, en = dev.correlated(a0[None], b0[None], 10.0, seed=21)
    assert np.abs(lp[0] - before[0]).max() < 1e-12
    assert np.abs(en[0] - dev.energy(10.0, seed=21)).max() < 1e-12
    acoeff, bcoeff = _sets(wf, 4, 6)
    dev.correlated(acoeff, bcoeff, 10.0, seed=22)
    after = (wf.value()[1], dev.configs(), sl._get_state(0), sl._get_state(1))
    assert np.array_equal(before[0], after[0]) and np.array_equal(before[1], after[1])
    for s in (2, 3):
        assert all(np.array_equal(x, y) for x, y in zip(before[s], after[s]))
    p = np.empty(a0.size)
    dev.call("pqa_get_param", b"acoeff", pa._ffi.ptr(p), p.size)
    assert np.array_equal(p.reshape(a0.shape), a0)
    # a VMC trajectory after the call is the one the untouched twin makes
    r1 = dev.vmc_sweeps(0.3, 3, seed=33)
    r2 = twin.fused_device().vmc_sweeps(0.3, 3, seed=33)
    assert np.array_equal(r1[0], r2[0]) and np.array_equal(r1[1], r2[1])
    assert np.array_equal(dev.configs(), twin.fused_device().configs())


def test_g43_correlated_on_device():
    g = helpers.golden("g43_linemin")
    mol = systems.water()
    wf = helpers.gpu_wf(mol, systems.random_mf(mol))
    configs = OpenConfigs(g["b_configs"].copy())
    pgrad = gradient_generator(mol, wf, {k: g["b_opt_" + k] for k in ("wf2acoeff", "wf2bcoeff")})
    assert linemin.correlated_route(wf, pgrad) == "fused"
    sets = [pgrad.transform.deserialize(wf, p) for p in g["b_params"]]
    wf.recompute(configs)
    lp, en = wf.fused_device().correlated(np.stack([s["wf2acoeff"] for s in sets]), np.stack([s["wf2bcoeff"] for s in sets]), 10.0,
                                         rot=g["b_rot"], unif=g["b_unif"])
    assert helpers.relerr(lp, g["b_logpsi"]) < 1e-10
    for i, k in enumerate(("ke", "ee", "ei", "ecp", "grad2", "total")):
        assert helpers.relerr(en[:, i, :], g["b_" + k]) < 1e-10, k


def test_g43_sample_overlap_on_device(monkeypatch):
    g = helpers.golden("g43_linemin")
    mol = systems.water()
    wf = helpers.gpu_wf(mol, systems.random_mf(mol))
    pgrad = gradient_generator(mol, wf, {k: g["b_opt_" + k] for k in ("wf2acoeff", "wf2bcoeff")})
    wfs = [copy.deepcopy(wf), copy.deepcopy(wf)]
    for w, p in zip(wfs, g["c_params"]):
        linemin.set_wf_params(w, p, pgrad)
    normal, rand = iter(g["c_normal"]), iter(g["c_rand"])
    monkeypatch.setattr(np.random, "normal", lambda loc=0.0, scale=1.0, size=None: loc + scale * next(normal))
    monkeypatch.setattr(np.random, "rand", lambda *shape: next(rand))
    cfg = OpenConfigs(g["c_start"].copy())
    _, unweighted, cfg = pa.sample_many.sample_overlap_worker(wfs, cfg, 0.5, 3, None)
    assert np.abs(cfg.configs - g["c_final"]).max() < 1e-9
    assert helpers.relerr(unweighted["overlap"], g["c_overlap"]) < 1e-9
    with pytest.raises(NotImplementedError, match="EnergyAccumulatorMultipleWF"):
        pa.sample_many.sample_overlap_worker(wfs, cfg, 0.5, 1, pa.EnergyAccumulator(mol))


def test_routes():
    mol = systems.water()
    mf = systems.random_mf(mol)
    wf = helpers.gpu_wf(mol, mf)
    to_opt = pwf.default_to_opt(wf)
    assert linemin.correlated_route(wf, gradient_generator(mol, wf, to_opt)) == "fused"
    pg = gradient_generator(mol, wf, to_opt)
    pg.enacc = pa.EnergyAccumulator(mol, use_old_ecp=False)
    assert linemin.correlated_route(wf, pg) == "protocol"
    assert linemin.correlated_route(wf, gradient_generator(mol, wf, pwf.default_to_opt(wf, optimize_orbitals=True))) == "protocol"
    mfd = systems.random_mf(mol, nvirt=6)
    wfd = helpers.gpu_wf(mol, mfd, determinants=systems.random_determinants(mol, mfd, 4))
    assert linemin.correlated_route(wfd, gradient_generator(mol, wfd, pwf.default_to_opt(wfd))) == "protocol"
    wf3 = pa.generate_wf(mol, mf, jastrow3=True)
    assert linemin.correlated_route(wf3, gradient_generator(mol, wf3, pwf.default_to_opt(wf3))) == "protocol"
    c3 = pbc.get_supercell(systems.diamond_primitive(), np.array([[-1.0, 1, 1], [1, -1, 1], [1, 1, -1]]))
    wfc = pa.generate_wf(c3, pbc.random_kmf(c3, complex_coeff=True, twist=(0.25, 0.1, -0.3)))
    assert linemin.correlated_route(wfc, gradient_generator(c3, wfc, pwf.default_to_opt(wfc))) == "protocol"

    # both routes on the same walkers and draws
    configs = OpenConfigs(systems.initial_guess(mol, 256, rng=np.random.default_rng(7)).configs.copy())
    tr = pg.transform
    x0 = tr.serialize_parameters(wf.parameters)
    d = np.random.default_rng(8).standard_normal(len(x0)) * 0.05
    params = [x0 + t * d for t in np.linspace(-0.2, 1.0, 6)]
    pf = gradient_generator(mol, wf, to_opt)
    pf.enacc.seed = 100
    pp = gradient_generator(mol, wf, to_opt)
    pp.enacc.seed = 100
    wf.recompute(configs)
    rf = linemin.correlated_compute_worker(wf, configs, params, pf, [0, 1])
    monkeypatch = pytest.MonkeyPatch()
    monkeypatch.setattr(linemin, "correlated_route", lambda *a: "protocol")
    try:
        rp = linemin.correlated_compute_worker(wf, configs, params, pp, [0, 1])
    finally:
        monkeypatch.undo()
    assert rf["route"] == "fused" and rp["route"] == "protocol"
    for k in ("ke", "ecp", "grad2", "total", "weight"):
        assert helpers.relerr(rf[k], rp[k]) < 1e-9, k
    assert np.array_equal(tr.serialize_parameters(wf.parameters), x0)


def _water_run(tmp_path, max_iterations, hdf):
    mol = systems.water()
    wf = pa.generate_wf(mol, systems.model_mf(mol))
    np.random.seed(1234)
    configs = pa.initial_guess(mol, 2048, rng=np.random.default_rng(1234))
    pgrad = gradient_generator(mol, wf, pwf.default_to_opt(wf))
    return linemin.line_minimization(wf, configs, pgrad, max_iterations=max_iterations, hdf_file=hdf, npts=12, steprange=0.3,
                                     vmcoptions=dict(nblocks=10, nsteps_per_block=5, tstep=0.3),
                                     warmup_options=dict(nblocks=1, nsteps_per_block=30, tstep=0.3))


def test_line_minimization_water_lowers_energy_and_restarts(tmp_path):
    hdf = str(tmp_path / "opt.hdf5")
    wf, df = _water_run(tmp_path, 5, hdf)
    e = np.array([d["energy"] for d in df])
    err = np.array([d["energy_error"] for d in df])
    print("energies", e, "errors", err, "steps", [d["est_min"] for d in df])
    assert e[0] - e[-1] > 5 * np.sqrt(err[0] ** 2 + err[-1] ** 2)
    # restart: a second call with more iterations continues from the file's parameters, walkers and iteration
    from pyqmc_amd.blockfile import BlockFile

    saved = BlockFile(hdf).load_parameters()
    mol = systems.water()
    wf2 = pa.generate_wf(mol, systems.model_mf(mol))
    pgrad = gradient_generator(mol, wf2, pwf.default_to_opt(wf2))
    seen = {}
    orig = linemin.correlated_sampling_minimum

    def spy(*a, **k):
        seen.setdefault("x0", a[7].copy())
        return orig(*a, **k)

    linemin.correlated_sampling_minimum = spy
    try:
        configs = pa.initial_guess(mol, 2048, rng=np.random.default_rng(9))
        _, df2 = linemin.line_minimization(wf2, configs, pgrad, max_iterations=6, hdf_file=hdf, npts=12, steprange=0.3,
                                           vmcoptions=dict(nblocks=4, nsteps_per_block=5, tstep=0.3))
    finally:
        linemin.correlated_sampling_minimum = orig
    assert [d["iteration"] for d in df2] == [5]
    assert np.array_equal(seen["x0"], pgrad.transform.serialize_parameters(saved))
    assert list(BlockFile(hdf).datasets()["iteration"]) == [0, 1, 2, 3, 4, 5]
