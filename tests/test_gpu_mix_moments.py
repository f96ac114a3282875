"""Mixture estimators from the resident state (pqa_mix_moments, pqa_mix_wtdp) against NumPy einsums of the reference's formulas on the
protocol route's per-walker arrays (wf.pgradient(), the handle's energy rows with the same keys, sample_many.compute_weights): tile
tails and states with different column counts, several 32-column blocks and the mirrored triangle, slices / chunks / determinism,
K = 1 against pqa_sr_moments, a state 1e-100 times smaller than the others, the thin product, the handles left as they were, the
fused worker and both drivers on either accumulator route, and the scope.

Tolerance: both routes use the same per-walker numbers and differ in the order of a walker sum and of the factors of a weight
(~ W 2^-53), checked at the 1e-9 test_gpu_sr_moments.py sets for this product; two device calls give the same bits."""

import copy

import numpy as np
import pytest

import pyqmc_amd as pa
from pyqmc_amd import blockfile, ensemble, ensemble_threaded, sample_many, systems
from pyqmc_amd import wf as pwf
from pyqmc_amd.accumulators import LinearTransform, StochasticReconfigurationMultipleWF, mix_route, sr_columns
from pyqmc_amd.accumulators_multiwf import EnergyAccumulatorMultipleWF
from pyqmc_amd.configs import OpenConfigs, PeriodicConfigs
from pyqmc_amd.energy import KEYS
from tests import helpers
from tests.test_gpu_overlap import _states

pytestmark = pytest.mark.gpu

TOL = 1e-9


def _recompute(wfs, x):
    cfg = OpenConfigs(x.copy())
    for w in wfs:
        w.recompute(cfg)
    return cfg, [w.fused_device() for w in wfs]


def _masks(wf, det=False, a=False, b=False):
    """A to_opt over the three device sources: det_coeff but the first entry, all of acoeff, bcoeff but its cusp row."""
    p = wf.parameters
    m = {"wf1det_coeff": np.zeros(np.shape(p["wf1det_coeff"]), dtype=bool), "wf2acoeff": np.zeros(np.shape(p["wf2acoeff"]), dtype=bool),
         "wf2bcoeff": np.zeros(np.shape(p["wf2bcoeff"]), dtype=bool)}
    if det:
        m["wf1det_coeff"][1:] = True
    if a:
        m["wf2acoeff"][:] = True
    if b:
        m["wf2bcoeff"][1:] = True
    return m


def _reference(wfs, devs, transforms, keys, offset=0.0):
    """The reference's formulas (stochastic_reconfiguration.py:195-227, accumulators_multiwf.py:46-58) on protocol-route arrays ->
    (weights (K, K, W), energies (K, 6, W), {key: value})."""
    weights = np.real(sample_many.compute_weights(wfs))
    en = np.array([d.energy(10.0, seed=k) for d, k in zip(devs, keys)])
    W = weights.shape[-1]
    out = {"overlap": weights.mean(axis=-1)}
    for r, k in enumerate(KEYS):
        out[k] = np.einsum("jc,ijc->ij", en[:, r] - offset, weights) / W
    for i, (t, w) in enumerate(zip(transforms, wfs)):
        if t.nparams == 0:
            continue
        dp = t.serialize_gradients(w.pgradient())
        out[("dp", i)] = np.einsum("cp,jc->pj", dp, weights[i]) / W
        out[("dpipj", i)] = np.einsum("cp,cq,c->pq", dp, dp, weights[i, i]) / W
        out[("dpH", i)] = np.einsum("jc,cp,jc->pj", en[:, 5], dp, weights[i]) / W
    return weights, en, out


def _device(devs, transforms, keys, offset=0.0, **kw):
    """pqa_mix_moments' outputs under the keys of _reference (+ the per-walker outputs with per_walker)."""
    K = len(devs)
    res = sample_many.mix_moments(devs, [sr_columns(t) for t in transforms], offset=offset, seeds=keys, **kw)
    out = {"overlap": res[0]}
    for r, k in enumerate(KEYS):
        out[k] = res[1][r]
    for i, m in enumerate(res[2]):
        if m is not None:
            p = m.shape[1]
            out[("dp", i)], out[("dpipj", i)], out[("dpH", i)] = m[p:p + K].T, m[:p], m[p + K:].T
    return out, res[3:]


def _agree(d, p, tol=TOL):
    assert sorted(map(str, d)) == sorted(map(str, p))
    for k in p:
        err = helpers.relerr(d[k], p[k])
        print(k, err)
        assert np.shape(d[k]) == np.shape(p[k]) and err < tol, (k, err)


def test_tails_and_uneven_states():
    mol = systems.water()
    wfs, x = _states(mol, 3, 200, 4, 61)  # 12 * 16 + 8 walkers
    wfs[2].parameters["wf1det_coeff"] = -np.asarray(wfs[2].parameters["wf1det_coeff"])  # (weights[i, 2] < 0 wherever Psi_i Psi_2 was > 0)
    cfg, devs = _recompute(wfs, x)
    tr = [LinearTransform(wfs[0].parameters, _masks(wfs[0], det=True, b=True)), LinearTransform(wfs[1].parameters, _masks(wfs[1], b=True)),
          LinearTransform(wfs[2].parameters, _masks(wfs[2]))]
    assert [t.nparams for t in tr] == [12, 9, 0] and tr[0].nparams % 16 != 0
    keys, offset = [101, 102, 103], -16.5
    weights, en, ref = _reference(wfs, devs, tr, keys, offset)
    assert any((weights[i, j] < 0).any() for i in range(3) for j in range(3) if i != j)
    dev, (u, enw) = _device(devs, tr, keys, offset, per_walker=True)
    _agree(dev, ref)
    for k in range(3):
        assert np.array_equal(enw[k].T, en[k])  # (the bits pqa_energy gives for that key)
    assert helpers.relerr(np.einsum("ic,jc->ijc", u, u), weights) < TOL
    # the accumulator, both routes with one key sequence
    acc = {}
    for route in ("device", "protocol"):
        sr = StochasticReconfigurationMultipleWF(pa.EnergyAccumulator(mol, seed=40), tr, route=route)
        acc[route] = sr.avg(cfg, wfs, weights)
        assert sr.last_route == route
        assert {k: np.shape(v) for k, v in acc[route].items()} == sr.shapes()
    _agree(acc["device"], acc["protocol"])
    auto = StochasticReconfigurationMultipleWF(pa.EnergyAccumulator(mol), tr)
    assert mix_route(wfs, auto)[0] == "device" and auto.resolve_route(wfs) == "device"


def test_replayed_draws_per_state():
    """rot / unif: K sets, each handle's pass with its own one -> the bits dev.energy gives with that set."""
    mol = systems.water()
    wfs, x = _states(mol, 2, 70, 4, 77)
    _, devs = _recompute(wfs, x)
    N, necp, W = x.shape[1], mol.natm, x.shape[0]
    rng = np.random.default_rng(78)
    rot = np.linalg.qr(rng.standard_normal((2, N, necp, 3, 3)))[0]
    unif = rng.random((2, N, necp, W))
    empty = (np.zeros(0, dtype=np.int32), np.zeros(0, dtype=np.int32))
    _, en, _, _, enw = sample_many.mix_moments(devs, [empty, empty], rot=rot, unif=unif, per_walker=True)
    rows = [d.energy(10.0, rot=rot[k], unif=unif[k]) for k, d in enumerate(devs)]
    for k in range(2):
        assert np.array_equal(enw[k].T, rows[k])
    assert not np.array_equal(devs[0].energy(10.0, rot=rot[1], unif=unif[1])[3], rows[0][3])  # (the sets really differ in the ECP row)
    weights = np.real(sample_many.compute_weights(wfs))
    assert helpers.relerr(en[5], np.einsum("jc,ijc->ij", np.array(rows)[:, 5], weights) / W) < TOL


def test_many_column_blocks_and_mirror():
    mol = systems.water()
    mf = systems.random_mf(mol, nvirt=6)
    base = helpers.gpu_wf(mol, mf, determinants=systems.random_determinants(mol, mf, 40))
    rng = np.random.default_rng(62)
    wfs = []
    for _ in range(2):
        w = copy.deepcopy(base)
        c = np.asarray(w.parameters["wf1det_coeff"]).copy()
        w.parameters["wf1det_coeff"] = c + 0.3 * rng.standard_normal(c.shape)
        wfs.append(w)
    x = systems.initial_guess(mol, 96, rng=np.random.default_rng(63)).configs.copy()
    _, devs = _recompute(wfs, x)
    tr = [LinearTransform(wfs[0].parameters, _masks(wfs[0], det=True, a=True, b=True)), LinearTransform(wfs[1].parameters, _masks(wfs[1], a=True))]
    assert tr[0].nparams == 39 + 24 + 9 and tr[0].nparams > 64 and tr[1].nparams == 24
    keys = [7, 8]
    _, _, ref = _reference(wfs, devs, tr, keys)
    dev, _ = _device(devs, tr, keys)
    _agree(dev, ref)
    for i in (0, 1):
        assert np.array_equal(dev[("dpipj", i)], dev[("dpipj", i)].T)


def test_slices_chunks_determinism():
    mol = systems.water()
    wfs, x = _states(mol, 2, 4096, 4, 64)
    _, devs = _recompute(wfs, x)
    tr = [LinearTransform(w.parameters, _masks(w, det=True, b=True)) for w in wfs]
    keys = [11, 12]
    _, _, ref = _reference(wfs, devs, tr, keys)
    d1, _ = _device(devs, tr, keys)
    _agree(d1, ref)
    d2, _ = _device(devs, tr, keys)
    d3, _ = _device(devs, tr, keys, walker_chunk=1000)
    for k in d1:
        assert np.array_equal(d1[k], d2[k]), k
        assert np.array_equal(d1[k], d3[k]), k
    src, pos = sr_columns(tr[1])
    w1, w2 = sample_many.mix_wtdp(devs, src, pos), sample_many.mix_wtdp(devs, src, pos, walker_chunk=1000)
    assert np.array_equal(w1[1], w2[1]) and np.array_equal(w1[0], d1["overlap"])


def test_one_state_is_sr_moments():
    mol = systems.water()
    wfs, x = _states(mol, 1, 200, 4, 65)
    _, devs = _recompute(wfs, x)
    tr = LinearTransform(wfs[0].parameters, _masks(wfs[0], det=True, b=True))
    src, pos = sr_columns(tr)
    mean, mom = devs[0].sr_moments(src, pos, 1e-100, seed=31)  # (cut-off far below every walker's node distance: f = 1)
    dev, _ = _device(devs, [tr], [31])
    assert np.array_equal(dev["overlap"], np.ones((1, 1)))
    for name, a, b in (("dpipj", dev[("dpipj", 0)], mom[:-2]), ("dp", dev[("dp", 0)][:, 0], mom[-1]), ("dpH", dev[("dpH", 0)][:, 0], mom[-2]),
                       ("total", dev["total"][0, 0], mean[5])):
        err = helpers.relerr(a, b)
        print(name, err)
        assert err < TOL, (name, err)


def test_wide_dynamic_range():
    mol = systems.water()
    wfs, x = _states(mol, 3, 200, 4, 66)
    wfs[1].parameters["wf1det_coeff"] = np.asarray(wfs[1].parameters["wf1det_coeff"]) * 1e-100
    _, devs = _recompute(wfs, x)
    tr = [LinearTransform(w.parameters, _masks(w, det=True, b=True)) for w in wfs]
    keys = [21, 22, 23]
    _, _, ref = _reference(wfs, devs, tr, keys)
    dev, _ = _device(devs, tr, keys)
    assert sorted(map(str, dev)) == sorted(map(str, ref))
    for k, v in ref.items():
        assert np.all(np.isfinite(dev[k])), k
        err = np.abs(dev[k] - v).max() / np.abs(v).max()  # (relative to the block's own largest entry)
        print(k, err, np.abs(v).max())
        assert err < TOL, (k, err)
    assert 0 < ref["overlap"][1, 1] < 1e-150 * ref["overlap"][0, 0]  # (the states really differ in scale)
    assert np.abs(ref[("dp", 1)][:, 1]).max() < 1e-50 * np.abs(ref[("dp", 1)][:, 0]).max()


@pytest.mark.parametrize("K", [2, 3])
def test_wtdp(K):
    mol = systems.water()
    wfs, x = _states(mol, K, 200, 4, 67)
    cfg, devs = _recompute(wfs, x)
    tr = LinearTransform(wfs[-1].parameters, _masks(wfs[-1], det=True, b=True))
    weights = np.real(sample_many.compute_weights(wfs))
    out = {}
    for route in ("device", "protocol"):
        sr = ensemble.StochasticReconfigurationWfbyWf(pa.EnergyAccumulator(mol), tr, mixture_route=route)
        out[route] = sr.avg(cfg, wfs, weights)["wtdp"]
        assert sr.last_route == route
    assert out["device"].shape == (tr.nparams, K, K)
    err = helpers.relerr(out["device"], out["protocol"])
    print(err)
    assert err < TOL
    assert np.array_equal(out["device"], np.swapaxes(out["device"], 1, 2))
    ovl, _ = sample_many.mix_wtdp(devs, *sr_columns(tr))
    assert helpers.relerr(ovl, weights.mean(axis=-1)) < TOL


def test_state_untouched():
    mol = systems.water()
    wfs, x = _states(mol, 2, 256, 4, 68)
    twins = [copy.deepcopy(w) for w in wfs]
    N = x.shape[1]
    rng = np.random.default_rng(69)
    tapes = [(np.sqrt(0.5) * rng.standard_normal((N, 256, 3)), rng.random((N, 256))) for _ in range(2)]
    states = []
    for ws in (wfs, twins):
        _, devs = _recompute(ws, x)
        sample_many.overlap_sweeps(devs, 0.5, *tapes[0])  # (state after a fused sweep, as the worker leaves it)
        states.append(devs)
    devs = states[0]

    def snapshot(ws):
        return [(w.value(), w.fused_device().configs(), w.wf_factors[0]._get_state(0), w.wf_factors[0]._get_state(1)) for w in ws]

    before = snapshot(wfs)
    tr = [LinearTransform(w.parameters, _masks(w, det=True, a=True, b=True)) for w in wfs]
    _device(devs, tr, [1, 2])
    sample_many.mix_wtdp(devs, *sr_columns(tr[1]))
    after = snapshot(wfs)
    for b, a in zip(before, after):
        assert np.array_equal(b[0][0], a[0][0]) and np.array_equal(b[0][1], a[0][1]) and np.array_equal(b[1], a[1])
        for s in (2, 3):
            assert all(np.array_equal(p, q) for p, q in zip(b[s], a[s]))
    r1 = sample_many.overlap_sweeps(devs, 0.5, *tapes[1], weights=True)
    r2 = sample_many.overlap_sweeps(states[1], 0.5, *tapes[1], weights=True)
    assert np.array_equal(r1[0], r2[0]) and np.array_equal(r1[1], r2[1]) and r1[2] == r2[2]
    assert np.array_equal(devs[0].configs(), states[1][0].configs())


def _accumulators(mol, wfs, route):
    tr = [LinearTransform(w.parameters, _masks(w, det=True, b=True)) for w in wfs]
    return {"multi": StochasticReconfigurationMultipleWF(pa.EnergyAccumulator(mol, seed=70), tr, route=route),
            "wtdp": ensemble.StochasticReconfigurationWfbyWf(pa.EnergyAccumulator(mol, seed=70), tr[-1], mixture_route=route),
            "energy": EnergyAccumulatorMultipleWF(pa.EnergyAccumulator(mol, seed=70), offset=-16.5, route=route)}


@pytest.mark.parametrize("name", ["multi", "wtdp", "energy"])
def test_worker_equivalence(name):
    mol = systems.water()
    wfs, x = _states(mol, 2, 256, 4, 71)
    out = {}
    for route in ("device", "protocol"):
        ws = [copy.deepcopy(w) for w in wfs]
        acc = _accumulators(mol, ws, route)[name]
        np.random.seed(72)
        weighted, unweighted, cfg = sample_many.sample_overlap_worker(ws, OpenConfigs(x.copy()), 0.5, 2, acc, route="fused")
        assert acc.last_route == route and sample_many.last_route == "fused"
        out[route] = (weighted, unweighted, cfg.configs.copy())
    assert np.array_equal(out["device"][2], out["protocol"][2])
    assert np.abs(out["device"][2] - x).max() > 0.1  # (the walkers moved)
    assert np.array_equal(out["device"][1]["overlap"], out["protocol"][1]["overlap"])
    _agree(out["device"][0], out["protocol"][0])


def _driver_states(mol):
    mf = systems.random_mf(mol, nvirt=4)
    w0 = helpers.gpu_wf(mol, mf, determinants=systems.random_determinants(mol, mf, 4))
    c = np.array([1.0, 0.3, 0.2, 0.1])
    w0.parameters["wf1det_coeff"] = c
    w1 = copy.deepcopy(w0)
    w1.parameters["wf1det_coeff"] = c + np.array([0.0, 0.08, -0.08, 0.05])
    return [w0, w1]


class RecordingUpdater(ensemble.StochasticReconfigurationWfbyWf):
    """Keeps the covariance matrix S its last step inverted."""

    def _collect_terms(self, avg, error):
        ret = super()._collect_terms(avg, error)
        self.S = np.array(ret["dpidpj"])
        return ret


@pytest.mark.parametrize("driver", ["wfbywf", "threaded"])
def test_driver_end_to_end(driver, tmp_path):
    mol = systems.water()
    x = systems.initial_guess(mol, 256, rng=np.random.default_rng(73)).configs.copy()
    to_opt = {"wf1det_coeff": np.array([False, True, True, True])}
    penalty = np.array([[0.0, 5.0], [5.0, 0.0]])
    eps = 1e-1
    out = {}
    for route in ("device", None):
        wfs = _driver_states(mol)
        updater = [[RecordingUpdater(pa.EnergyAccumulator(mol, seed=74), LinearTransform(w.parameters, to_opt), eps=eps,
                                                             route="protocol", mixture_route=route)] for w in wfs]
        path = str(tmp_path / f"{driver}_{route}.hdf5")
        np.random.seed(75)
        if driver == "wfbywf":
            ensemble.optimize_ensemble(wfs, OpenConfigs(x.copy()), updater, path, tau=0.5, max_iterations=1, overlap_penalty=penalty,
                                       vmc_kwargs=dict(nblocks=2, nsteps=2, tstep=0.5))
        else:
            ensemble_threaded.optimize_ensemble(wfs, OpenConfigs(x.copy()), updater, path, tau=0.5, max_iterations=1, overlap_penalty=penalty,
                                                verbose=False, warmup_kwargs=dict(nblocks=1, nsteps_per_block=2, tstep=0.5),
                                                vmc_kwargs=dict(nblocks=2, nsteps_per_block=2, tstep=0.5),
                                                overlap_kwargs=dict(nblocks=2, nsteps=2, tstep=0.5))
        assert [u[0].last_route for u in updater] == ["device" if route else "protocol"] * 2
        out[route] = (wfs, blockfile.BlockFile(path).datasets(), path, updater)
    dsd, dsp = out["device"][1], out[None][1]
    assert list(dsd["iteration"]) == [0, 0] and list(dsd["wavefunction"]) == [0, 1] and list(dsd["sub_iteration"]) == [0, 0]
    for k in ("energy0", "energy1", "energy_error0", "energy_error1", "overlap0", "overlap1"):
        err = helpers.relerr(dsd[k], dsp[k])
        print(k, err)
        assert err < TOL, (k, err)
    start = _driver_states(mol)
    for a, b, u, w0 in zip(out["device"][0], out[None][0], out[None][3], start):
        bound = TOL * np.linalg.cond(u[0].S + eps * np.eye(len(u[0].S)))  # (the matrix the protocol run inverted for this state)
        pa_, pb = np.asarray(a.parameters["wf1det_coeff"]), np.asarray(b.parameters["wf1det_coeff"])
        err = helpers.relerr(pa_, pb)
        print("parameters", err, bound)
        assert err < bound
        assert np.abs(pb - np.asarray(w0.parameters["wf1det_coeff"])).max() > 1e-4  # (a step was taken)
    if driver == "threaded":
        # restart: the stored parameters and walkers, from iteration 1: with max_iterations=1 nothing is left to run
        wfs, _, path, updater = out["device"]
        stored = blockfile.BlockFile(path).load_parameters()
        assert sorted(k for k in stored if k.endswith("det_coeff")) == ["0/wf1det_coeff", "1/wf1det_coeff"]
        fresh = _driver_states(mol)
        cfg2 = OpenConfigs(np.zeros_like(x))
        ensemble_threaded.optimize_ensemble(fresh, cfg2, updater, path, tau=0.5, max_iterations=1, overlap_penalty=penalty, verbose=False)
        for i, w in enumerate(fresh):
            assert np.array_equal(np.asarray(w.parameters["wf1det_coeff"]), stored[f"{i}/wf1det_coeff"])
        assert np.abs(cfg2.configs).max() > 0 and len(blockfile.BlockFile(path).datasets()["iteration"]) == 2


def test_scope():
    mol = systems.water()
    mf = systems.random_mf(mol)
    wfs, x = _states(mol, 2, 64, 1, 76)
    cfg, devs = _recompute(wfs, x)
    weights = np.real(sample_many.compute_weights(wfs))
    enacc = pa.EnergyAccumulator(mol)

    def refused(ws, tr, why, run=True):
        auto = StochasticReconfigurationMultipleWF(enacc, tr)
        route, reason = mix_route(ws, auto)
        assert route == "protocol" and why in reason, reason
        assert auto.resolve_route(ws) == "protocol"
        forced = StochasticReconfigurationMultipleWF(enacc, tr, route="device")
        with pytest.raises(NotImplementedError, match=why):
            forced.avg(cfg, ws, weights)
        return auto

    # a three-body wave function: route=None falls back and evaluates on the protocol route
    w3 = helpers.gpu_wf3(mol, mf)
    w3.recompute(cfg)
    mixed = [wfs[0], w3]
    tr = [LinearTransform(w.parameters, {"wf2bcoeff": np.ones((4, 3), dtype=bool)}) for w in mixed]
    auto = refused(mixed, tr, "not a real Slater x two-body Jastrow")
    d = auto.avg(cfg, mixed, np.real(sample_many.compute_weights(mixed)))
    assert auto.last_route == "protocol" and d[("dp", 1)].shape == (12, 2)
    # an orbital key
    tro = [LinearTransform(w.parameters, pwf.default_to_opt(w, optimize_orbitals=True)) for w in wfs]
    refused(wfs, tro, "mo_coeff")
    # nine states
    nine = [wfs[0]] + [copy.deepcopy(wfs[0]) for _ in range(8)]
    refused(nine, [LinearTransform(w.parameters, _masks(w, b=True)) for w in nine], "9 wave functions")
    # a periodic handle
    sup, wfp = helpers.gpu_pbc_wf("k222")
    per = [wfp, copy.deepcopy(wfp)]
    trp = [LinearTransform(w.parameters, {"wf2bcoeff": np.ones(np.shape(w.parameters["wf2bcoeff"]), dtype=bool)}) for w in per]
    autop = StochasticReconfigurationMultipleWF(pa.EnergyAccumulator(sup), trp)
    route, reason = mix_route(per, autop)
    assert route == "protocol" and ("periodic" in reason or "not a real" in reason) and autop.resolve_route(per) == "protocol"
    with pytest.raises(NotImplementedError):
        StochasticReconfigurationMultipleWF(pa.EnergyAccumulator(sup), trp, route="device").resolve_route(per)
    # the library refuses what the Python side would not send
    for cols, why in (([([3], [0]), ([], [])], "src must be"), ([([2], [12]), ([], [])], "pos outside"), ([([4], [0]), ([], [])], "src must be")):
        with pytest.raises(pa._ffi.PqaError, match=why):
            sample_many.mix_moments(devs, cols, seeds=[1, 2])
    with pytest.raises(pa._ffi.PqaError, match="pqa_mix_wtdp"):
        sample_many.mix_wtdp(devs, [3], [0])
    with pytest.raises(pa._ffi.PqaError, match="Slater x two-body"):
        sample_many.mix_moments([devs[0], w3.fused_device()], [([], []), ([], [])], seeds=[1, 2])
    pdevs = [w.fused_device() for w in per]
    xp = systems.initial_guess(sup, 8, rng=np.random.default_rng(3)).configs.copy()
    for w in per:
        w.recompute(PeriodicConfigs(xp, sup.lattice_vectors()))
    with pytest.raises(pa._ffi.PqaError, match="pqa_mix_moments"):
        sample_many.mix_moments(pdevs, [([], []), ([], [])], seeds=[1, 2])


@pytest.fixture(scope="module")
def two_states_16():
    """K = 2 states of water at 16 walkers: (devs, entry -> call with one column description (src, pos))."""
    wfs, x = _states(systems.water(), 2, 16, 1, 79)
    _, devs = _recompute(wfs, x)
    return devs, {
        "pqa_sr_moments": lambda s, p: devs[0].sr_moments(s, p, 1e-3),
        "pqa_sr_moments_orb": lambda s, p: devs[0].sr_moments_orb(s, p, 1e-3),
        "pqa_sr_moments_c": lambda s, p: devs[0].sr_moments_c(s, p, [], 1e-3),
        "pqa_mix_moments": lambda s, p: sample_many.mix_moments(devs, [(s, p), ([], [])], seeds=[1, 2]),
        "pqa_mix_wtdp": lambda s, p: sample_many.mix_wtdp(devs, s, p),
    }


@pytest.mark.parametrize("bad", ["src", "pos"])
@pytest.mark.parametrize("entry", ["pqa_sr_moments", "pqa_sr_moments_orb", "pqa_sr_moments_c", "pqa_mix_moments", "pqa_mix_wtdp"])
def test_column_check_names_the_entry(two_states_16, entry, bad):
    """The one column check of the family: a source no entry has, and a position one past the (nb, 3) bcoeff entries, behind a good
    column; the message starts with the entry that was called."""
    devs, call = two_states_16
    nb3 = devs[0].nb * 3
    call[entry]([2, 2], [0, nb3 - 1])  # (the good columns pass)
    src, pos, why = ([2, 7], [0, 0], "src must be") if bad == "src" else ([2, 2], [0, nb3], "pos outside")
    with pytest.raises(pa._ffi.PqaError, match=f"{entry}: {why}"):
        call[entry](src, pos)
