"""Line minimisation for three-body wave functions on the device: pqa_correlated_j3 against the per-set sequence it replaces (set
det_coeff / acoeff / bcoeff / ccoeff on a deep copy, recompute, energy with the same seed) at the tails of its set columns and
determinant tiles, with unequal spins, above four basis functions per kind, without an ECP, with more ions and electrons, and in a
periodic cell; arrays left out; K = 1 at the handle's own coefficients and the handle left as it was; chunk independence and
repeatability; the scope message; route selection and agreement of the routes; line_minimization end to end.

Bound: the project's own for these routes (tests/test_gpu_correlated_md.py): the difference over max(1, |reference|) per energy row,
and the same for logpsi, below 1e-10."""

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
KEYS = ("wf1det_coeff", "wf2acoeff", "wf2bcoeff", "wf3ccoeff")
ARGS = {"wf1det_coeff": "det_coeff", "wf2acoeff": "acoeff", "wf2bcoeff": "bcoeff", "wf3ccoeff": "ccoeff"}


def _walkers(mol, W, seed):
    x = systems.initial_guess(mol, W, rng=np.random.default_rng(seed)).configs.copy()
    return PeriodicConfigs(x, mol.lattice_vectors()) if hasattr(mol, "a") else OpenConfigs(x)


def _sets(wf, K, seed, keys=KEYS):
    """{key: (K, ...)}: the handle's coefficients plus 0.05 N(0, 1) per set (the draws of a key do not depend on ``keys``)."""
    rng = np.random.default_rng(seed)
    out = {}
    for key in KEYS:
        c0 = np.asarray(wf.parameters[key])
        v = np.stack([c0 + 0.05 * rng.standard_normal(c0.shape) for _ in range(K)])
        if key in keys:
            out[key] = v
    return out


def _per_set(wf, configs, sets, seed):
    """The sequence pqa_correlated_j3 stands in for, on a copy of wf."""
    w = copy.deepcopy(wf)
    dev = w.fused_device()
    out_l, out_e = [], []
    for k in range(len(next(iter(sets.values())))):
        for key, v in sets.items():
            w.parameters[key] = v[k]
        out_l.append(w.recompute(configs)[1])
        out_e.append(dev.energy(10.0, seed=seed))
    return np.array(out_l), np.array(out_e)


def _j3(dev, sets, **kw):
    return dev.correlated_j3(**{ARGS[k]: v for k, v in sets.items()}, threshold=10.0, **kw)


def _compare(lp, en, rl, re):
    dl = np.abs(lp - rl).max() / max(1.0, np.abs(rl).max())
    scale = np.maximum(1.0, np.abs(re).max(axis=2, keepdims=True))
    de = (np.abs(en - re) / scale).max(axis=(0, 2))
    print("scaled differences: logpsi", dl, "ke ee ei ecp grad2 total", de)
    assert dl < TOL, dl
    assert de.max() < TOL, de


def _check(wf, configs, K, seed=17, keys=KEYS):
    sets = _sets(wf, K, seed, keys)
    wf.recompute(configs)
    lp, en = _j3(wf.fused_device(), sets, seed=seed)
    _compare(lp, en, *_per_set(wf, configs, sets, seed))
    assert np.ptp(en[:, 0, :].mean(axis=1)) > 1e-6  # (the sets really differ)
    return lp, en


def _water3(ndet):
    mol = systems.water()
    mf = systems.random_mf(mol, nvirt=6)
    return mol, mf, helpers.gpu_wf3(mol, mf, None if ndet == 1 else systems.random_determinants(mol, mf, ndet))


@pytest.fixture(scope="module")
def water4():
    """Water, four determinants, 64 resident walkers: shared by the checks on one wave function (none of them changes it)."""
    mol, _, wf = _water3(4)
    configs = _walkers(mol, 64, 6)
    wf.recompute(configs)
    return mol, wf, configs


@pytest.mark.parametrize("ndet,W,K", [(1, 70, 5), (1, 32, 70), (4, 64, 5), (13, 64, 5)])
def test_water(ndet, W, K):
    """(1, 70, 5): a lane tail of the set columns; (1, 32, 70): two column groups, 64 + 6, the handle's own column in the second;
    4 and 13 determinants: the determinant k-step tails, per-spin maps that differ, det_coeff varying as well."""
    mol, _, wf = _water3(ndet)
    dev = wf.fused_device()
    assert dev.ndet == ndet and dev.has_j3
    if ndet == 13:
        assert dev.ndet_s[0] != dev.ndet_s[1]
    _check(wf, _walkers(mol, W, ndet), K)


def test_unequal_spins():
    """The uu / ud / dd channel indexing with 5 + 3 electrons."""
    mol = systems.Mol(*zip(*systems._WATER), nelec=(5, 3))
    mf = systems.random_mf(mol, nvirt=6)
    wf = helpers.gpu_wf3(mol, mf, systems.random_determinants(mol, mf, 6))
    assert wf.fused_device().nelec == (5, 3)
    _check(wf, _walkers(mol, 64, 2), 4)


def test_five_functions_per_kind():
    """More than four three-body basis functions per kind (the lengths jas3_eval keeps a second instantiation for).  The default
    basis puts the cusp function in front of the nb Pade functions, so the coefficient array is sized from the handle."""
    mol = systems.water()
    mf = systems.random_mf(mol)
    wf = pa.generate_wf(mol, mf, jastrow3=True, jastrow3_kws=dict(na=5, nb=5))
    dev = wf.fused_device()
    assert dev.na3 == 5 and dev.nb3 > 4
    a, b = helpers.jastrow_params(mol)
    wf.parameters["wf2acoeff"], wf.parameters["wf2bcoeff"] = a, b
    wf.parameters["wf3ccoeff"] = helpers.ccoeff_params(mol, 5, dev.nb3)
    _check(wf, _walkers(mol, 32, 8), 3)


def test_no_ecp():
    """All-electron water: the kinetic part alone."""
    mol = systems.water_general()
    mf = systems.random_mf(mol)
    wf = pa.generate_wf(mol, mf, jastrow3=True)
    rng = np.random.default_rng(11)  # (all-electron: the electron-ion cusp function comes first and keeps its coefficients)
    a, b = np.array(wf.parameters["wf2acoeff"]), np.array(wf.parameters["wf2bcoeff"])
    a[:, 1:] += 0.05 * rng.standard_normal(a[:, 1:].shape)
    b[1:] += 0.05 * rng.standard_normal(b[1:].shape)
    wf.parameters["wf2acoeff"], wf.parameters["wf2bcoeff"] = a, b
    wf.parameters["wf3ccoeff"] = helpers.ccoeff_params(mol)
    assert wf.fused_device().necp == 0
    _check(wf, _walkers(mol, 64, 3), 4)


def test_water_cluster():
    """Two molecules, 8 + 8 electrons and 6 atoms: more table entries than lanes in every component, partners of both spins."""
    mol = systems.water_cluster(2, 1, 1)
    wf = helpers.gpu_wf3(mol, systems.random_mf(mol))
    dev = wf.fused_device()
    assert dev.nelec == (8, 8) and dev.natom == 6
    _check(wf, _walkers(mol, 48, 4), 3)


def test_diamond_cell():
    """A periodic cell at Gamma: minimal images in every three-body distance."""
    c3 = pbc.get_supercell(systems.diamond_primitive(), np.array([[-1.0, 1, 1], [1, -1, 1], [1, 1, -1]]))
    wf = helpers.gpu_wf3(c3, pbc.random_kmf(c3))
    dev = wf.fused_device()
    assert not dev.cplx and not dev.twisted and dev.has_j3
    _check(wf, _walkers(c3, 32, 5), 3)


def test_only_ccoeff_given(water4):
    _, wf, configs = water4
    dev = wf.fused_device()
    sets = _sets(wf, 4, 3, keys=("wf3ccoeff",))
    lp, en = _j3(dev, sets, seed=5)
    own = {k: np.stack([np.asarray(wf.parameters[k])] * 4) for k in KEYS[:3]}
    lp2, en2 = _j3(dev, {**own, **sets}, seed=5)
    assert np.array_equal(lp, lp2) and np.array_equal(en, en2)
    _compare(lp, en, *_per_set(wf, configs, sets, 5))
    assert np.ptp(en[:, 0, :].mean(axis=1)) > 1e-6


def test_k1_at_own_coefficients_and_state_unchanged(water4):
    _, wf, configs = water4
    dev = wf.fused_device()
    lg = wf.recompute(configs)[1]
    before = (dev.configs(), np.array(wf.parameters["wf3ccoeff"]), wf.value()[1], dev.energy(10.0, seed=21))
    lp, en = dev.correlated_j3(seed=21)
    assert lp.shape == (1, dev.W) and en.shape == (1, 6, dev.W)
    _compare(lp, en, lg[None], before[3][None])
    _j3(dev, _sets(wf, 3, 6), seed=22)
    after = (dev.configs(), np.array(wf.parameters["wf3ccoeff"]), wf.value()[1], dev.energy(10.0, seed=21))
    for x, y in zip(before, after):
        assert np.array_equal(x, y)


def test_chunks_and_repeat_bitwise(water4):
    _, wf, _ = water4
    dev = wf.fused_device()
    sets = _sets(wf, 5, 3)
    one = _j3(dev, sets, seed=4)
    again = _j3(dev, sets, seed=4)
    chunked = _j3(dev, sets, seed=4, walker_chunk=7)
    for a, b, c in zip(one, again, chunked):
        assert np.array_equal(a, b) and np.array_equal(a, c)


def test_scope_message():
    mol = systems.water()
    wf = helpers.gpu_wf(mol, systems.random_mf(mol))
    wf.recompute(_walkers(mol, 16, 1))
    with pytest.raises(pa._ffi.PqaError, match="pqa_correlated_j3: needs a Slater x two-body x three-body Jastrow handle"):
        wf.fused_device().correlated_j3(seed=1)
    mol, _, wf3 = _water3(1)
    wf3.recompute(_walkers(mol, 16, 1))
    with pytest.raises(pa._ffi.PqaError, match="pqa_correlated_md: three-body Jastrow factor"):  # (the sibling keeps refusing it)
        wf3.fused_device().correlated_md(seed=1)
    with pytest.raises(ValueError, match="ccoeff"):
        wf3.fused_device().correlated_j3(ccoeff=np.zeros((2, 3, 4, 4, 3, 3)))


def test_routes():
    mol, _, wf3 = _water3(4)
    to_opt = pwf.default_to_opt(wf3)
    assert set(k for k, v in to_opt.items() if np.any(v)) == set(KEYS)
    pg = gradient_generator(mol, wf3, to_opt)
    assert linemin.correlated_route(wf3, pg) == "protocol"
    assert linemin.correlated_route(wf3, pg, three_body_device=True) == "fused"
    assert linemin.correlated_route(wf3, pg, "fused", three_body_device=True) == "fused"
    with pytest.raises(NotImplementedError, match="evaluation_route='protocol'"):
        linemin.correlated_route(wf3, pg, "fused")

    # both routes on the same walkers and draws
    configs = _walkers(mol, 256, 7)
    tr = pg.transform
    x0 = tr.serialize_parameters(wf3.parameters)
    d = np.random.default_rng(8).standard_normal(len(x0)) * 0.05
    params = [x0 + t * d for t in np.linspace(-0.2, 1.0, 6)]
    pf, pp = gradient_generator(mol, wf3, to_opt), gradient_generator(mol, wf3, to_opt)
    pf.enacc.seed = pp.enacc.seed = 100
    wf3.recompute(configs)
    rf = linemin.correlated_compute_worker(wf3, configs, params, pf, [0, 1], evaluation_route=None, three_body_device=True)
    rp = linemin.correlated_compute_worker(wf3, configs, params, pp, [0, 1], evaluation_route="protocol")
    assert rf["route"] == "fused" and rf["entry"] == "pqa_correlated_j3" and rp["route"] == "protocol"
    for k in ("ke", "ecp", "grad2", "total", "weight"):
        print(k, helpers.relerr(rf[k], rp[k]))
        assert helpers.relerr(rf[k], rp[k]) < 1e-9, k
    assert np.ptp(rf["ke"].mean(axis=1)) > 1e-6
    assert np.array_equal(tr.serialize_parameters(wf3.parameters), x0)


def test_line_minimization_fused(monkeypatch):
    mol = systems.water()
    mf = systems.model_mf(mol)
    wf = pa.generate_wf(mol, mf, determinants=systems.random_determinants(mol, mf, 4), jastrow3=True)
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
    wf, df = linemin.line_minimization(wf, configs, pgrad, max_iterations=2, npts=12, steprange=0.3, three_body_device=True,
                                       vmcoptions=dict(nblocks=4, nsteps_per_block=5, tstep=0.3),
                                       warmup_options=dict(nblocks=1, nsteps_per_block=20, tstep=0.3))
    assert entries == [("fused", "pqa_correlated_j3")] * 2 and len(df) == 2
    assert all(np.all(np.isfinite(np.asarray(v))) for v in wf.parameters.values())
    assert all(np.isfinite(d["energy"]) and np.all(np.isfinite(d["yfit"])) for d in df)
