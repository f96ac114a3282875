"""Line minimisation for several determinants on the device: pqa_correlated_md against the per-set sequence it replaces (set
det_coeff / acoeff / bcoeff, recompute, energy) at every tail of its tiles (determinant k-steps, set columns, electron and ECP
point rows, per-spin unique-determinant maps), without an ECP, above 16 electrons per spin and in a periodic cell; coefficient
arrays left out; a single determinant against pqa_correlated; K = 1 at the handle's own coefficients and the handle left as it
was; chunk independence and repeatability; route selection and agreement of the routes; line_minimization end to end."""

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

TOL = 1e-10  # (test_gpu_linemin.py's, with its scaling)
KEYS = ("wf1det_coeff", "wf2acoeff", "wf2bcoeff")


def _container(mol, x):
    return PeriodicConfigs(x, mol.lattice_vectors()) if hasattr(mol, "a") else OpenConfigs(x)


def _walkers(mol, W, seed):
    return _container(mol, systems.initial_guess(mol, W, rng=np.random.default_rng(seed)).configs.copy())


def _sets(wf, K, seed, keys=KEYS):
    """{key: (K, ...)}: the handle's coefficients plus 0.05 N(0, 1), the recipe of test_gpu_linemin.py for every array."""
    rng = np.random.default_rng(seed)
    out = {}
    for key in KEYS:  # (the draws of a key do not depend on which keys are asked for)
        c0 = np.asarray(wf.parameters[key])
        v = np.stack([c0 + 0.05 * rng.standard_normal(c0.shape) for _ in range(K)])
        if key in keys:
            out[key] = v
    return out


def _per_set(wf, configs, sets, seed):
    """The sequence pqa_correlated_md stands in for, on a copy of wf."""
    w = copy.deepcopy(wf)
    dev = w.fused_device()
    out_l, out_e = [], []
    for k in range(len(next(iter(sets.values())))):
        for key, v in sets.items():
            w.parameters[key] = v[k]
        out_l.append(w.recompute(configs)[1])
        out_e.append(dev.energy(10.0, seed=seed))
    return np.array(out_l), np.array(out_e)


def _md(dev, sets, **kw):
    return dev.correlated_md(sets.get("wf1det_coeff"), sets.get("wf2acoeff"), sets.get("wf2bcoeff"), 10.0, **kw)


def _compare(lp, en, rl, re):
    dl = np.abs(lp - rl).max() / max(1.0, np.abs(rl).max())
    scale = np.maximum(1.0, np.abs(re).max(axis=2, keepdims=True))
    de = (np.abs(en - re) / scale).max(axis=(0, 2))
    print("scaled differences: logpsi", dl, "ke ee ei ecp grad2 total", de)
    assert dl < TOL
    assert de.max() < TOL, de


def _check(wf, configs, K, seed=17, keys=KEYS):
    sets = _sets(wf, K, seed, keys)
    wf.recompute(configs)
    lp, en = _md(wf.fused_device(), sets, seed=seed)
    _compare(lp, en, *_per_set(wf, configs, sets, seed))
    assert np.ptp(en[:, 0, :].mean(axis=1)) > 1e-6  # (the sets really differ)
    return lp, en


def _water_md(ndet):
    mol = systems.water()
    mf = systems.random_mf(mol, nvirt=6)
    return mol, mf, helpers.gpu_wf(mol, mf, determinants=systems.random_determinants(mol, mf, ndet))


@pytest.mark.parametrize("ndet,W,K", [(4, 70, 5), (13, 96, 40), (50, 64, 3), (50, 32, 70)])
def test_water(ndet, W, K):
    """4: one k-step of determinants, a 5-of-16 column tail, a kinetic row tail and ECP point-row tails; 13: a 12 + 1 k tail, three
    column tiles with a tail of 8, unique-determinant maps that differ per spin; 50: several k-steps, more determinants than a wave;
    50 with K = 70: two groups of set columns (64 + 6) and an LDS plan above 64 KiB (the raised limit)."""
    mol, _, wf = _water_md(ndet)
    dev = wf.fused_device()
    assert dev.ndet == ndet
    if ndet == 13:
        assert dev.ndet_s[0] != dev.ndet_s[1]
    _check(wf, _walkers(mol, W, ndet), K)


def test_unequal_spins():
    mol = systems.Mol(*zip(*systems._WATER), nelec=(5, 3))
    mf = systems.random_mf(mol, nvirt=6)
    wf = helpers.gpu_wf(mol, mf, determinants=systems.random_determinants(mol, mf, 6))
    assert wf.fused_device().nelec == (5, 3)
    _check(wf, _walkers(mol, 64, 2), 4)


def test_no_ecp():
    mol = systems.water_general()
    mf = systems.random_mf(mol, nvirt=6)
    wf = pa.generate_wf(mol, mf, determinants=systems.random_determinants(mol, mf, 4))
    rng = np.random.default_rng(11)  # (all-electron: the electron-ion cusp function comes first and keeps its coefficients)
    a, b = np.array(wf.parameters["wf2acoeff"]), np.array(wf.parameters["wf2bcoeff"])
    a[:, 1:] += 0.05 * rng.standard_normal(a[:, 1:].shape)
    b[1:] += 0.05 * rng.standard_normal(b[1:].shape)
    wf.parameters["wf2acoeff"], wf.parameters["wf2bcoeff"] = a, b
    assert wf.fused_device().necp == 0
    _check(wf, _walkers(mol, 64, 3), 4)


def test_above_16_per_spin():
    mol = systems.water_cluster(5, 1, 1)  # 20 + 20 electrons: three 16-electron tiles with a tail
    mf = systems.random_mf(mol, nvirt=6)
    wf = helpers.gpu_wf(mol, mf, determinants=systems.random_determinants(mol, mf, 6))
    assert wf.fused_device().nelec == (20, 20)
    _check(wf, _walkers(mol, 64, 4), 3)


def test_diamond_cell():
    """The 2 x 2 x 2 diamond supercell at Gamma (32 + 32 electrons) with three determinants (one virtual orbital per k-point)."""
    sup = pbc.get_supercell(systems.diamond_primitive(), helpers.PBC_SLATER_CASES["k222"])
    mf = pbc.random_kmf(sup, nvirt=1)
    base = [5 * k + i for k in range(8) for i in range(4)]  # flat indices into the per-k blocks of 4 + 1 orbitals
    ex1, ex2 = sorted(set(base) - {3} | {4}), sorted(set(base) - {38} | {39})  # (the last column in use: no orbital is cut off)
    dets = [(1.0, [base, base]), (0.3, [ex2, base]), (-0.2, [ex1, ex2])]
    sup, wf = helpers.gpu_pbc_wf("k222", case=(sup, mf), determinants=dets)
    assert wf.fused_device().ndet == 3
    _check(wf, _walkers(sup, 64, 5), 4)


def test_arrays_left_out():
    mol, _, wf = _water_md(4)
    configs = _walkers(mol, 64, 6)
    _check(wf, configs, 4, keys=("wf2acoeff", "wf2bcoeff"))  # det_coeff=None: Jastrow-only sets
    _check(wf, configs, 4, keys=("wf1det_coeff",))  # acoeff = bcoeff = None: determinant-only sets


def test_single_determinant_against_correlated():
    mol = systems.water()
    wf = helpers.gpu_wf(mol, systems.random_mf(mol))
    wf.recompute(_walkers(mol, 128, 7))
    dev = wf.fused_device()
    sets = _sets(wf, 5, 8, keys=("wf2acoeff", "wf2bcoeff"))
    _compare(*_md(dev, sets, seed=9), *dev.correlated(sets["wf2acoeff"], sets["wf2bcoeff"], 10.0, seed=9))


def test_k1_at_own_coefficients_and_state_unchanged():
    mol, _, wf = _water_md(4)
    dev = wf.fused_device()
    configs = _walkers(mol, 256, 5)
    wf.recompute(configs)
    twin = copy.deepcopy(wf)
    for d in (dev, twin.fused_device()):
        d.vmc_sweeps(0.3, 2, seed=9, energy=False)
    sl, ja = wf.wf_factors
    before = (wf.value()[1], dev.configs(), sl._get_state(0), sl._get_state(1))
    own = {k: np.asarray(wf.parameters[k]) for k in KEYS}
    lp, en = _md(dev, {k: v[None] for k, v in own.items()}, seed=21)
    print("K = 1: logpsi", np.abs(lp[0] - before[0]).max(), "en", np.abs(en[0] - dev.energy(10.0, seed=21)).max(axis=1))
    assert np.abs(lp[0] - before[0]).max() < 1e-12
    assert np.abs(en[0] - dev.energy(10.0, seed=21)).max() < 1e-12
    _md(dev, _sets(wf, 4, 6), seed=22)
    after = (wf.value()[1], dev.configs(), sl._get_state(0), sl._get_state(1))
    assert np.array_equal(before[0], after[0]) and np.array_equal(before[1], after[1])
    for s in (2, 3):
        assert all(np.array_equal(x, y) for x, y in zip(before[s], after[s]))
    for name, key in ((b"det_coeff", "wf1det_coeff"), (b"acoeff", "wf2acoeff")):
        p = np.empty(own[key].size)
        dev.call("pqa_get_param", name, pa._ffi.ptr(p), p.size)
        assert np.array_equal(p.reshape(own[key].shape), own[key])
    r1 = dev.vmc_sweeps(0.3, 3, seed=33)
    r2 = twin.fused_device().vmc_sweeps(0.3, 3, seed=33)
    assert np.array_equal(r1[0], r2[0]) and np.array_equal(r1[1], r2[1])
    assert np.array_equal(dev.configs(), twin.fused_device().configs())


def test_chunks_and_repeat_bitwise():
    mol, _, wf = _water_md(4)
    wf.recompute(_walkers(mol, 70, 1))
    dev = wf.fused_device()
    sets = _sets(wf, 5, 3)
    one = _md(dev, sets, seed=4)
    again = _md(dev, sets, seed=4)
    chunked = _md(dev, sets, seed=4, walker_chunk=24)
    for a, b, c in zip(one, again, chunked):
        assert np.array_equal(a, b) and np.array_equal(a, c)


def test_routes():
    mol = systems.water()
    mf = systems.random_mf(mol)
    mfd = systems.random_mf(mol, nvirt=6)
    wfd = helpers.gpu_wf(mol, mfd, determinants=systems.random_determinants(mol, mfd, 4))
    to_opt = pwf.default_to_opt(wfd)
    assert set(k for k, v in to_opt.items() if np.any(v)) == set(KEYS)
    pg = gradient_generator(mol, wfd, to_opt)
    assert linemin.correlated_route(wfd, pg) == "protocol"
    assert linemin.correlated_route(wfd, pg, "fused") == "fused"
    assert linemin.correlated_route(wfd, pg, "protocol") == "protocol"
    wf3 = pa.generate_wf(mol, mf, jastrow3=True)
    c3 = pbc.get_supercell(systems.diamond_primitive(), np.array([[-1.0, 1, 1], [1, -1, 1], [1, 1, -1]]))
    wfc = pa.generate_wf(c3, pbc.random_kmf(c3, complex_coeff=True, twist=(0.25, 0.1, -0.3)))
    pe = gradient_generator(mol, wfd, to_opt)
    pe.enacc = pa.EnergyAccumulator(mol, use_old_ecp=False)
    for w, p in ((wf3, gradient_generator(mol, wf3, pwf.default_to_opt(wf3))), (wfc, gradient_generator(c3, wfc, pwf.default_to_opt(wfc))), (wfd, pe)):
        with pytest.raises(NotImplementedError, match="evaluation_route='protocol'"):
            linemin.correlated_route(w, p, "fused")

    # both routes on the same walkers and draws
    configs = _walkers(mol, 256, 7)
    tr = pg.transform
    x0 = tr.serialize_parameters(wfd.parameters)
    d = np.random.default_rng(8).standard_normal(len(x0)) * 0.05
    params = [x0 + t * d for t in np.linspace(-0.2, 1.0, 6)]
    pf, pp = gradient_generator(mol, wfd, to_opt), gradient_generator(mol, wfd, to_opt)
    pf.enacc.seed = pp.enacc.seed = 100
    wfd.recompute(configs)
    rf = linemin.correlated_compute_worker(wfd, configs, params, pf, [0, 1], evaluation_route="fused")
    rp = linemin.correlated_compute_worker(wfd, configs, params, pp, [0, 1], evaluation_route="protocol")
    assert rf["route"] == "fused" and rf["entry"] == "pqa_correlated_md" and rp["route"] == "protocol"
    for k in ("ke", "ecp", "grad2", "total", "weight"):
        print(k, helpers.relerr(rf[k], rp[k]))
        assert helpers.relerr(rf[k], rp[k]) < 1e-9, k
    assert np.ptp(rf["ke"].mean(axis=1)) > 1e-6
    assert np.array_equal(tr.serialize_parameters(wfd.parameters), x0)


def test_line_minimization_fused(monkeypatch):
    mol = systems.water()
    mf = systems.model_mf(mol)
    wf = pa.generate_wf(mol, mf, determinants=systems.random_determinants(mol, mf, 4))
    np.random.seed(1234)
    configs = pa.initial_guess(mol, 1024, rng=np.random.default_rng(1234))
    pgrad = gradient_generator(mol, wf, pwf.default_to_opt(wf))
    entries = []
    orig = linemin.correlated_compute_worker

    def spy(*a, **k):
        data = orig(*a, **k)
        entries.append((data["route"], data.get("entry")))
        return data

    monkeypatch.setattr(linemin, "correlated_compute_worker", spy)
    wf, df = linemin.line_minimization(wf, configs, pgrad, max_iterations=2, npts=12, steprange=0.3, evaluation_route="fused",
                                       vmcoptions=dict(nblocks=4, nsteps_per_block=5, tstep=0.3),
                                       warmup_options=dict(nblocks=1, nsteps_per_block=20, tstep=0.3))
    assert entries == [("fused", "pqa_correlated_md")] * 2 and len(df) == 2
    assert all(np.all(np.isfinite(np.asarray(v))) for v in wf.parameters.values())
    assert all(np.isfinite(d["energy"]) and np.all(np.isfinite(d["yfit"])) for d in df)
