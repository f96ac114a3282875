"""AddWF on the device: device components against the reference (g49 a, b) on both routes, the fused sweeps (pqa_add_sweeps) against
the protocol route from one seed with the state every handle is left in, the energy (pqa_add_energy) against the reference, the
protocol formulas and the single handle, route selection, and vmc end to end with a restart from its file.

Shapes: W = 70 is no multiple of 256 or 64 (the thread-per-walker tail), W = 256 and 512 take several blocks, K = 3 with four
determinants runs the multi-determinant handles, the water cluster has N = 64 with 32 orbitals per spin."""

import copy
import pickle

import numpy as np
import pytest

import pyqmc_amd as pa
from pyqmc_amd import addwf, systems
from pyqmc_amd.configs import OpenConfigs
from pyqmc_amd.vmc import NotOnOneDeviceError
from tests import addwf_ref, helpers

pytestmark = pytest.mark.gpu

TOL = 1e-9
TSTEP = 0.3


def err(a, b):
    a, b = np.asarray(a), np.asarray(b)
    assert a.shape == b.shape, (a.shape, b.shape)
    return float(np.max(np.abs(a - b)) / max(1.0, float(np.max(np.abs(b))))) if b.size else 0.0


@pytest.fixture(scope="module")
def g():
    return helpers.golden(addwf_ref.GOLDEN)


def device_addwf(name, route):
    mol, wfs = addwf_ref.components(name, helpers.gpu_wf)
    return mol, pa.AddWF(list(addwf_ref.CASES[name]["coeffs"]), wfs, route=route)


@pytest.mark.parametrize("name,route", [("a", "fused"), ("a", "protocol"), ("b", "fused"), ("b", "protocol")])
def test_device_components_match_reference(g, name, route):
    _, wf = device_addwf(name, route)
    out = {}
    addwf_ref.protocol_entries(wf, OpenConfigs(g[name + "_configs"].copy()), g, name + "_", out)
    keys = [k for k in g.files if k.startswith(name + "_") and k in out]
    assert len(keys) > 40
    for k in keys:
        if k.endswith("_keys"):
            assert list(out[k]) == list(g[k]), k
        elif g[k].dtype != bool:
            assert err(out[k], g[k]) < TOL, (k, err(out[k], g[k]))
    assert wf.last_route == route


@pytest.mark.parametrize("route", ["fused", "protocol"])
def test_trajectory_matches_reference(g, route):
    _, wf = device_addwf("a", route)
    configs = OpenConfigs(g["a_configs"].copy())
    if route == "fused":
        N, W = configs.configs.shape[1], configs.configs.shape[0]
        tapes = {"gauss": g["a_traj_gauss"].reshape(addwf_ref.NSWEEPS, N, W, 3), "unif": g["a_traj_unif"].reshape(addwf_ref.NSWEEPS, N, W)}
        blk, configs = pa.vmc_worker(wf, configs, addwf_ref.TSTEP, addwf_ref.NSWEEPS, {}, tapes=tapes)
    else:
        with addwf_ref.replay(g["a_traj_gauss"], g["a_traj_unif"]):
            blk, configs = helpers.protocol_vmc_worker(wf, configs, addwf_ref.TSTEP, addwf_ref.NSWEEPS, {})
    assert err(configs.configs, g["a_traj_final"]) < TOL
    assert abs(blk["acceptance"] - float(g["a_traj_acceptance"])) < TOL
    s, l = wf.value()
    assert err(s, g["a_traj_sign"]) < TOL and err(l, g["a_traj_log"]) < TOL
    assert err(wf.ratio_current_config(), g["a_traj_rcc"]) < TOL
    assert wf.last_route == route


def _components(mol, K, ndet, seed):
    """K products over one determinant list (ndet > 1: different det_coeff) or one determinant (different Jastrow b coefficients), each on
    a handle of its own, and positive coefficients."""
    rng = np.random.default_rng(seed)
    if ndet > 1:
        mf = systems.random_mf(mol, nvirt=4)
        dets = systems.random_determinants(mol, mf, ndet)
    else:
        mf, dets = systems.random_mf(mol), None
    base = helpers.gpu_wf(mol, mf, determinants=dets)
    wfs = []
    for k in range(K):
        w = copy.deepcopy(base)
        if ndet > 1:
            c = np.asarray(w.parameters["wf1det_coeff"]).copy()
            w.parameters["wf1det_coeff"] = c + 0.2 * rng.standard_normal(c.shape)
        else:
            b = np.asarray(w.parameters["wf2bcoeff"]).copy()
            b[1:] += 0.05 * rng.standard_normal(b[1:].shape)
            w.parameters["wf2bcoeff"] = b
        wfs.append(w)
    return wfs, [0.6, 0.5, 0.4][:K]


def _walkers(mol, W, seed):
    return systems.initial_guess(mol, W, rng=np.random.default_rng(seed)).configs.copy()


def _tapes(seed, nsteps, N, W):
    """The draws of vmc_worker in its order: per electron np.random.normal then np.random.rand."""
    np.random.seed(seed)
    unit, unif = np.empty((nsteps * N, W, 3)), np.empty((nsteps * N, W))
    for i in range(nsteps * N):
        unit[i] = np.random.normal(size=(W, 3))
        unif[i] = np.random.rand(W)
    return unit, unif


@pytest.mark.parametrize("system,K,W,ndet", [("water", 2, 70, 1), ("water", 3, 256, 4), ("cluster", 2, 512, 1)])
def test_fused_matches_protocol(system, K, W, ndet):
    mol = systems.water() if system == "water" else systems.water_cluster()
    N = sum(mol.nelec)
    comps, coeffs = _components(mol, K, ndet, 61)
    wf_f = pa.AddWF(coeffs, comps, route="fused")
    wf_p = pa.AddWF(coeffs, [copy.deepcopy(c) for c in comps], route="protocol")
    x = _walkers(mol, W, 62)
    unit, unif = _tapes(63, 2, N, W)
    cf, cp = OpenConfigs(x.copy()), OpenConfigs(x.copy())
    wf_f.recompute(cf)
    devs = wf_f.fused_devices()
    acc_f = addwf.add_sweeps(devs, coeffs, TSTEP, np.sqrt(TSTEP) * unit, unif)  # both sweeps in one call
    cf.configs[...] = devs[0].configs()
    acc_p = []
    for n in range(2):
        with addwf_ref.replay(unit[n * N:(n + 1) * N], unif[n * N:(n + 1) * N]):
            blk, cp = helpers.protocol_vmc_worker(wf_p, cp, TSTEP, 1, {})
        acc_p.append(blk["acceptance"])
    assert np.abs(cf.configs - x).max() > 0.1  # (the walkers moved)
    assert np.abs(cf.configs - cp.configs).max() < TOL
    assert np.abs(acc_f - np.array(acc_p)).max() < TOL
    (sf, lf), (sp, lp) = wf_f.value(), wf_p.value()
    assert wf_f.last_route == "fused" and wf_p.last_route == "protocol"
    assert np.array_equal(sf, sp) and err(lf, lp) < TOL
    assert err(wf_f.ratio_current_config(), wf_p.ratio_current_config()) < TOL
    for a, b in zip(wf_f.wf_components, wf_p.wf_components):
        va, vb = a.value(), b.value()
        assert np.array_equal(va[0], vb[0]) and err(va[1], vb[1]) < TOL
        assert np.array_equal(a.fused_device().configs(), cf.configs)
        for s in (0, 1):
            ia, da = a.wf_factors[0]._get_state(s)
            ib, db = b.wf_factors[0]._get_state(s)
            assert helpers.relerr(ia, ib) < 1e-8 and err(da, db) < TOL
    # the next protocol move on the handles (no recompute in between) is the same
    e = mol.nelec[0]
    ep = cf.configs[:, e, :] + 0.1
    ga, va, sa = wf_f.gradient_value(e, cf.make_irreducible(e, ep))
    gb, vb, sb = wf_p.gradient_value(e, cp.make_irreducible(e, ep))
    assert err(ga, gb) < TOL and err(va, vb) < TOL, (err(ga, gb), err(va, vb))
    mask = np.arange(W) % 2 == 0
    cf.move(e, cf.make_irreducible(e, ep), mask)
    cp.move(e, cp.make_irreducible(e, ep), mask)
    wf_f.updateinternals(e, cf.make_irreducible(e, ep), cf, mask=mask, saved_values=sa)
    wf_p.updateinternals(e, cp.make_irreducible(e, ep), cp, mask=mask, saved_values=sb)
    lf = wf_f.value()[1]
    assert err(lf, wf_p.value()[1]) < TOL
    # every handle's state is that of a fresh recompute of the final walkers
    fresh = pa.AddWF(coeffs, [copy.deepcopy(c) for c in comps], route="protocol")
    assert err(lf, fresh.recompute(cf)[1]) < TOL
    for a, b in zip(wf_f.wf_components, fresh.wf_components):
        assert err(a.value()[1], b.value()[1]) < TOL
        for s in (0, 1):
            ia, da = a.wf_factors[0]._get_state(s)
            ib, db = b.wf_factors[0]._get_state(s)
            assert helpers.relerr(ia, ib) < 1e-8 and err(da, db) < TOL


def _ecp_draws(mol, W, seed):
    rng = np.random.default_rng(seed)
    N, necp = sum(mol.nelec), sum(1 for a in mol._atom if a[0] in mol._ecp)
    q = rng.standard_normal((N, necp, 4))
    q /= np.linalg.norm(q, axis=-1, keepdims=True)
    w_, x, y, z = np.moveaxis(q, -1, 0)
    rot = np.stack([np.stack([1 - 2 * (y * y + z * z), 2 * (x * y - z * w_), 2 * (x * z + y * w_)], -1),
                    np.stack([2 * (x * y + z * w_), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w_)], -1),
                    np.stack([2 * (x * z - y * w_), 2 * (y * z + x * w_), 1 - 2 * (x * x + y * y)], -1)], -2)
    return rot, rng.random((N, necp, W))


def test_energy_matches_reference(g):
    mol, wf = device_addwf("a", None)
    configs = OpenConfigs(g["a_traj_final"].copy())
    wf.recompute(configs)
    en = pa.EnergyAccumulator(mol)(configs, wf, rot=g["a_en_rot"], unif=g["a_en_unif"])
    for k in pa.energy.KEYS:
        assert err(en[k], g["a_en_" + k]) < TOL, (k, err(en[k], g["a_en_" + k]))


def test_energy_matches_protocol_formulas():
    mol = systems.water_cluster()
    N, W = sum(mol.nelec), 256
    comps, coeffs = _components(mol, 2, 1, 71)
    wf = pa.AddWF(coeffs, comps)
    configs = OpenConfigs(_walkers(mol, W, 72))
    wf.recompute(configs)
    rot, unif = _ecp_draws(mol, W, 73)
    acc = pa.EnergyAccumulator(mol)
    en = acc(configs, wf, rot=rot, unif=unif)
    ke, grad2 = np.zeros(W), np.zeros(W)
    for e in range(N):
        gr, lap = wf.gradient_laplacian(e, configs.electron(e))
        ke += -0.5 * lap
        grad2 += np.sum(gr**2, axis=0)
    assert err(en["ke"], ke) < TOL and err(en["grad2"], grad2) < TOL
    own = acc(configs, comps[1], rot=rot, unif=unif)
    assert err(en["ee"], own["ee"]) < TOL and err(en["ei"], own["ei"]) < TOL


def test_energy_ecp_against_single_handles():
    mol = systems.water()
    W = 70
    configs = OpenConfigs(_walkers(mol, W, 82))
    configs.configs[:, :3, :] = mol.atom_coords()[0] + 0.35 * np.random.default_rng(3).standard_normal((W, 3, 3))  # both mask outcomes
    rot, unif = _ecp_draws(mol, W, 83)
    acc = pa.EnergyAccumulator(mol)
    # identical components: every key is the single handle's
    one = helpers.gpu_wf(mol, systems.random_mf(mol))
    wf = pa.AddWF([0.3, 0.7], [copy.deepcopy(one), copy.deepcopy(one)])
    wf.recompute(configs)
    one.recompute(configs)
    en, ref = acc(configs, wf, rot=rot, unif=unif), acc(configs, one, rot=rot, unif=unif)
    assert np.abs(ref["ecp"]).max() > 1e-3
    for k in pa.energy.KEYS:
        assert err(en[k], ref[k]) < TOL, (k, err(en[k], ref[k]))
    # distinct components: ecp = sum_k w_k ecp_k of the handles' own energy calls with those draws
    comps, coeffs = _components(mol, 2, 1, 81)
    wf = pa.AddWF(coeffs, comps)
    wf.recompute(configs)
    en = acc(configs, wf, rot=rot, unif=unif)
    w = wf.ratio_current_config()
    own = [acc(configs, c, rot=rot, unif=unif) for c in comps]
    assert err(en["ecp"], sum(w[k] * own[k]["ecp"] for k in range(2))) < TOL
    assert err(en["total"], sum(w[k] * own[k]["total"] for k in range(2))) < TOL
    # what the energy of an AddWF does not do
    with pytest.raises(NotImplementedError):
        pa.EnergyAccumulator(mol, use_old_ecp=False)(configs, wf)
    with pytest.raises(NotImplementedError):
        acc.nonlocal_tmoves(configs, wf, 0, 0.1)


def _out_of_scope(kind):
    if kind == "periodic":
        sup, base = helpers.gpu_pbc_wf("gamma")
        return sup, base, systems.initial_guess(sup, 8, rng=np.random.default_rng(91))
    if kind == "complex":
        sup, mf = helpers.pbc_complex_case()
        return sup, pa.generate_wf(sup, mf), systems.initial_guess(sup, 8, rng=np.random.default_rng(92))
    mol = systems.water()
    return mol, helpers.gpu_wf3(mol, systems.random_mf(mol)), OpenConfigs(_walkers(mol, 8, 93))


@pytest.mark.parametrize("kind", ["periodic", "complex", "three-body"])
def test_routes(kind):
    mol, base, configs = _out_of_scope(kind)
    comps = [base, copy.deepcopy(base)]
    wf = pa.AddWF([0.6, 0.4], comps)
    s, l = wf.recompute(configs)
    assert wf.last_route == "protocol" and np.all(np.isfinite(l))
    assert err(l, base.value()[1]) < TOL  # (two copies of one function)
    with pytest.raises(ValueError, match="out of scope"):
        pa.AddWF([0.6, 0.4], comps, route="fused")
    with pytest.raises(NotOnOneDeviceError):
        pa.vmc_worker(wf, configs, TSTEP, 1, {})
    in_scope = pa.AddWF([0.6, 0.4], _components(systems.water(), 2, 1, 94)[0], route="protocol")
    with pytest.raises(NotOnOneDeviceError):
        pa.vmc_worker(in_scope, OpenConfigs(_walkers(systems.water(), 8, 95)), TSTEP, 1, {})


def test_two_components_on_one_handle_are_refused():
    mol = systems.water()
    one = helpers.gpu_wf(mol, systems.random_mf(mol))
    with pytest.raises(ValueError, match="handle of its own"):
        pa.AddWF([0.5, 0.5], [one, one])
    with pytest.raises(ValueError, match="handle of its own"):
        pa.AddWF([0.5, 0.5], [one, one.wf_factors[0]])


def test_copy_and_pickle():
    mol = systems.water()
    comps, coeffs = _components(mol, 2, 1, 96)
    wf = pa.AddWF(coeffs, comps)
    configs = OpenConfigs(_walkers(mol, 16, 97))
    l0 = wf.recompute(configs)[1]
    for other in (copy.copy(wf), pickle.loads(pickle.dumps(wf))):
        assert other.fused_devices()[0] is not wf.fused_devices()[0]
        assert err(other.value()[1], l0) < TOL  # (resident walkers travel)
        other.parameters["wf2wf2bcoeff"] = np.asarray(wf.parameters["wf1wf2bcoeff"])
        assert np.abs(other.recompute(configs)[1] - l0).max() > 1e-6 and err(wf.value()[1], l0) < TOL


def test_vmc_and_restart(tmp_path):
    mol = systems.water()
    comps, coeffs = _components(mol, 2, 1, 98)
    wf_f = pa.AddWF(coeffs, comps)
    wf_p = pa.AddWF(coeffs, [copy.deepcopy(c) for c in comps], route="protocol")
    x = _walkers(mol, 70, 99)
    out = str(tmp_path / "addwf_vmc")
    np.random.seed(100)
    df_f, cf = pa.vmc(wf_f, OpenConfigs(x.copy()), nblocks=2, nsteps_per_block=2, tstep=TSTEP, accumulators={"energy": pa.EnergyAccumulator(mol)},
                      hdf_file=out)
    assert wf_f.last_route == "fused"
    np.random.seed(100)
    df_p, cp = pa.vmc(wf_p, OpenConfigs(x.copy()), nblocks=2, nsteps_per_block=2, tstep=TSTEP, accumulators={"energy": pa.EnergyAccumulator(mol)},
                      worker=helpers.protocol_vmc_worker)
    assert np.abs(cf.configs - cp.configs).max() < TOL and np.abs(cf.configs - x).max() > 0.1
    for k in ("energytotal", "energyke", "energyecp", "energygrad2", "acceptance"):
        assert err(df_f[k], df_p[k]) < TOL, k
    df_r, cr = pa.vmc(wf_f, OpenConfigs(x.copy()), nblocks=3, nsteps_per_block=2, tstep=TSTEP, accumulators={"energy": pa.EnergyAccumulator(mol)},
                      hdf_file=out)
    assert list(df_r["block"]) == [2] and np.abs(cr.configs - cf.configs).max() > 0.1
