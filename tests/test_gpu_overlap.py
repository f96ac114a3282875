"""Mixture sampling on the device (pqa_overlap_sweeps): the reference's walk replayed (g44 a) on both routes, the fused route against
the protocol route from one seed (walkers, overlaps, weights and the state every handle is left in), the linear invariance of the
mixture, route selection, and optimize_ensemble end to end with a restart from its file."""

import copy

import numpy as np
import pytest

import pyqmc_amd as pa
from pyqmc_amd import ensemble, sample_many, systems
from pyqmc_amd.accumulators import LinearTransform
from pyqmc_amd.accumulators_multiwf import EnergyAccumulatorMultipleWF
from pyqmc_amd.configs import OpenConfigs
from tests import helpers

pytestmark = pytest.mark.gpu

TOL = 1e-9


class WeightRecorder:
    """A multiple-wave-function accumulator that keeps every sweep's (K, K, W) weights."""

    multiple_wf = True

    def __init__(self):
        self.seen = []

    def avg(self, configs, wfs, weights):
        self.seen.append((configs.configs.copy(), np.array(weights)))
        return {"w": np.mean(weights, axis=-1)}


def _states(mol, K, W, ndet, seed, cluster=False):
    """K wave functions over one determinant list (ndet > 1: different det_coeff) or one determinant (different Jastrow b
    coefficients), and W walkers."""
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
            w.parameters["wf1det_coeff"] = c + 0.3 * rng.standard_normal(c.shape)
        else:
            b = np.asarray(w.parameters["wf2bcoeff"]).copy()
            b[1:] += 0.05 * rng.standard_normal(b[1:].shape)
            w.parameters["wf2bcoeff"] = b
        wfs.append(w)
    x = systems.initial_guess(mol, W, rng=np.random.default_rng(seed + 1)).configs.copy()
    return wfs, x


def _run(wfs, x, route, seed, nsteps=2, energy=None):
    np.random.seed(seed)
    cfg = OpenConfigs(x.copy())
    w, u, cfg = sample_many.sample_overlap_worker(wfs, cfg, 0.5, nsteps, energy, route=route)
    assert sample_many.last_route == route
    return w, u, cfg


@pytest.mark.parametrize("system,K,W,ndet", [("water", 2, 256, 1), ("water", 3, 256, 4), ("cluster", 2, 4096, 1), ("cluster", 3, 4096, 3)])
def test_fused_matches_protocol(system, K, W, ndet):
    mol = systems.water() if system == "water" else systems.water_cluster()
    wfs_f, x = _states(mol, K, W, ndet, 31)
    wfs_p = [copy.deepcopy(w) for w in wfs_f]
    rec_f, rec_p = WeightRecorder(), WeightRecorder()
    wf_, uf, cf = _run(wfs_f, x, "fused", 5, energy=rec_f)
    wp_, up, cp = _run(wfs_p, x, "protocol", 5, energy=rec_p)
    assert np.abs(cf.configs - cp.configs).max() < TOL
    assert np.abs(cf.configs - x).max() > 0.1  # (the walkers moved)
    assert helpers.relerr(uf["overlap"], up["overlap"]) < TOL
    assert helpers.relerr(wf_["w"], wp_["w"]) < TOL
    for (xf, wtf), (xp, wtp) in zip(rec_f.seen, rec_p.seen):
        assert np.abs(xf - xp).max() < TOL and helpers.relerr(wtf, wtp) < TOL
    for a, b in zip(wfs_f, wfs_p):
        va, vb = a.value(), b.value()
        assert np.array_equal(va[0], vb[0]) and np.abs(va[1] - vb[1]).max() < TOL * max(1.0, np.abs(vb[1]).max())
        assert np.array_equal(a.fused_device().configs(), cf.configs)
        for s in (0, 1):
            ia, da = a.wf_factors[0]._get_state(s)
            ib, db = b.wf_factors[0]._get_state(s)
            assert helpers.relerr(ia, ib) < 1e-8 and np.abs(da - db).max() < TOL * max(1.0, np.abs(db).max())
    # the next protocol move on the handles (no recompute in between) is the same
    e = mol.nelec[0]
    for a, b in zip(wfs_f, wfs_p):
        ep = cf.configs[:, e, :] + 0.1
        ga, va, sa = a.gradient_value(e, cf.make_irreducible(e, ep))
        gb, vb, sb = b.gradient_value(e, cp.make_irreducible(e, ep))
        assert helpers.relerr(ga, gb) < 1e-8 and helpers.relerr(va, vb) < 1e-8
        mask = np.arange(W) % 2 == 0
        a.updateinternals(e, cf.make_irreducible(e, ep), cf, mask=mask, saved_values=sa)
        b.updateinternals(e, cp.make_irreducible(e, ep), cp, mask=mask, saved_values=sb)
        assert np.abs(a.value()[1] - b.value()[1]).max() < TOL * max(1.0, np.abs(b.value()[1]).max())
    # and the whole-call form (energy=None: all sweeps in one call) walks the same way
    wfs_n = [copy.deepcopy(w) for w in wfs_p]
    _, un, cn = _run(wfs_n, x, "fused", 5)
    assert np.abs(cn.configs - cp.configs).max() < TOL and helpers.relerr(un["overlap"], up["overlap"]) < TOL


def test_linear_invariance():
    """psi'_i = sum_j U_ij psi_j (orthogonal U through det_coeff over one determinant list and one Jastrow): per walker the (K, K)
    weighted energies and overlaps transform as U M U^T, on the host and in the device's weights."""
    mol = systems.water()
    mf = systems.random_mf(mol, nvirt=4)
    dets = systems.random_determinants(mol, mf, 3)
    base = helpers.gpu_wf(mol, mf, determinants=dets)
    K = 3
    rng = np.random.default_rng(40)
    C = rng.standard_normal((K, len(dets)))
    U, _ = np.linalg.qr(rng.standard_normal((K, K)))
    wfs, wfs_u = [], []
    for k in range(K):
        a, b = copy.deepcopy(base), copy.deepcopy(base)
        a.parameters["wf1det_coeff"] = C[k]
        b.parameters["wf1det_coeff"] = U[k] @ C
        wfs.append(a)
        wfs_u.append(b)
    x = systems.initial_guess(mol, 128, rng=np.random.default_rng(41)).configs.copy()
    cfg = OpenConfigs(x.copy())
    for w in wfs + wfs_u:
        w.recompute(cfg)
    enacc = pa.EnergyAccumulator(mol, seed=7)
    per_walker = []
    for ws in (wfs, wfs_u):
        wt = sample_many.compute_weights(ws)
        en = []
        for w in ws:
            enacc._calls = 0  # (the same ECP key for every wave function)
            en.append(enacc(cfg, w)["total"])
        M = np.einsum("jc,ijc->cij", np.array(en), wt)
        per_walker.append((np.transpose(wt, (2, 0, 1)), M))
    # rho = mean_k |psi_k|^2 is the same for both sets, so the per-walker matrices themselves transform
    for a, b in zip(per_walker[0], per_walker[1]):
        assert np.abs(np.einsum("ik,ckl,jl->cij", U, a, U) - b).max() < 1e-10 * max(1.0, np.abs(b).max())
    # the device's weights at the same fixed walkers (every move rejected: uniform draws of 2 against ratios below 1 here would not
    # do, so +inf) transform the same way.  (The walk itself is not invariant: its drift is the mean of the K log-gradients.)
    N = sum(mol.nelec)
    outs = []
    for ws in (wfs, wfs_u):
        for w in ws:
            w.recompute(cfg)
        ovl, wts, acc = sample_many.overlap_sweeps([w.fused_device() for w in ws], 0.5, np.zeros((N, 128, 3)), np.full((N, 128), np.inf),
                                                   weights=True)
        assert acc == 0.0 and np.array_equal(ws[0].fused_device().configs(), x)
        assert np.abs(wts - sample_many.compute_weights(ws)).max() < 1e-10 * np.abs(wts).max()
        outs.append((ovl[0], wts))
    assert np.abs(np.einsum("ik,kl,jl->ij", U, outs[0][0], U) - outs[1][0]).max() < 1e-10
    assert np.abs(np.einsum("ik,klc,jl->ijc", U, outs[0][1], U) - outs[1][1]).max() < 1e-10 * np.abs(outs[1][1]).max()


def test_scope():
    mol = systems.water()
    mf = systems.random_mf(mol)
    wfs, x = _states(mol, 2, 64, 1, 50)
    cfg = OpenConfigs(x.copy())
    assert sample_many.fused_handles(wfs, cfg) is not None
    # a three-body Jastrow factor
    w3 = pa.generate_wf(mol, mf, jastrow3=True)
    mixed = [wfs[0], w3]
    assert sample_many.fused_handles(mixed, cfg) is None
    sample_many.sample_overlap_worker(mixed, OpenConfigs(x.copy()), 0.5, 1, None)
    assert sample_many.last_route == "protocol"
    with pytest.raises(ValueError, match="fused"):
        sample_many.sample_overlap_worker(mixed, OpenConfigs(x.copy()), 0.5, 1, None, route="fused")
    # the same handle twice
    assert sample_many.fused_handles([wfs[0], wfs[0]], cfg) is None
    # mismatched walker counts are refused by the C entry itself
    wfs[0].recompute(cfg)
    wfs[1].recompute(OpenConfigs(x[:32].copy()))
    devs = [w.fused_device() for w in wfs]
    with pytest.raises(pa._ffi.PqaError, match="same walkers"):
        sample_many.overlap_sweeps(devs, 0.5, np.zeros((mol.nelec[0] + mol.nelec[1], 64, 3)), np.zeros((10, 64)))
    # a periodic handle
    sup, wfp = helpers.gpu_pbc_wf("k222")
    xp = systems.initial_guess(sup, 8, rng=np.random.default_rng(3)).configs.copy()
    from pyqmc_amd.configs import PeriodicConfigs

    assert sample_many.fused_handles([wfp, copy.deepcopy(wfp)], PeriodicConfigs(xp, sup.lattice_vectors())) is None


def test_g44a_replay_both_routes(monkeypatch):
    g = helpers.golden("g44_ensemble")
    mol = systems.water()
    mf = systems.random_mf(mol, nvirt=4)
    dets = systems.random_determinants(mol, mf, int(g["a_ndet"]))
    for route in ("fused", "protocol"):
        wfs = []
        for c in g["a_det_coeff"]:
            w = helpers.gpu_wf(mol, mf, determinants=dets)
            w.parameters["wf1det_coeff"] = c
            wfs.append(w)
        normal, rand = iter(g["a_normal"]), iter(g["a_rand"])
        rot, runif = iter(g["a_rot"]), iter(g["a_unif"])
        monkeypatch.setattr(np.random, "normal", lambda loc=0.0, scale=1.0, size=None: loc + scale * next(normal))
        monkeypatch.setattr(np.random, "rand", lambda *shape: next(rand))

        class Replay(pa.EnergyAccumulator):
            def __call__(self, configs, wf, rot=None, unif=None):
                return super().__call__(configs, wf, rot=next(rot_it), unif=next(unif_it))

        rot_it, unif_it = rot, runif
        acc = EnergyAccumulatorMultipleWF(Replay(mol, threshold=10.0), offset=-16.5)
        cfg = OpenConfigs(g["a_start"].copy())
        weighted, unweighted, cfg = sample_many.sample_overlap_worker(wfs, cfg, 0.5, int(g["a_nsteps"]), acc, route=route)
        assert sample_many.last_route == route
        assert np.abs(cfg.configs - g["a_final"]).max() < 1e-9, route
        assert helpers.relerr(unweighted["overlap"], g["a_overlap"]) < 1e-9, route
        assert float(weighted["offset"]) == float(g["a_w_offset"])
        for k in ("total", "ke", "ee", "ei", "ecp", "grad2"):
            assert helpers.relerr(weighted[k], g["a_w_" + k]) < 1e-9, (route, k)


def test_optimize_ensemble_end_to_end(tmp_path):
    """Two water states, state 1 a small det_coeff perturbation of state 0 (normalised overlap about 0.99).  With a strong
    overlap penalty the SR steps on state 1 push |S_01| down; 4 iterations at 400 walkers.  The statistical error of S_01 at this
    sample size is about 0.01 (checked against the block spread below), so a drop to below 0.8 is far outside the noise."""
    mol = systems.water()
    mf = systems.random_mf(mol, nvirt=4)
    dets = systems.random_determinants(mol, mf, 4)
    w0 = helpers.gpu_wf(mol, mf, determinants=dets)
    c = np.asarray(w0.parameters["wf1det_coeff"]).copy()
    c = np.array([1.0, 0.3, 0.2, 0.1])
    w0.parameters["wf1det_coeff"] = c
    w1 = copy.deepcopy(w0)
    w1.parameters["wf1det_coeff"] = c + np.array([0.0, 0.08, -0.08, 0.05])
    wfs = [w0, w1]
    np.random.seed(3)
    configs = OpenConfigs(systems.initial_guess(mol, 400, rng=np.random.default_rng(3)).configs.copy())
    to_opt = {"wf1det_coeff": np.array([False, True, True, True])}
    updater = [[ensemble.StochasticReconfigurationWfbyWf(pa.EnergyAccumulator(mol), LinearTransform(w.parameters, to_opt), eps=1e-1)]
               for w in wfs]
    path = str(tmp_path / "ens.hdf5")
    kws = dict(nblocks=4, nsteps=5, tstep=0.5)
    _, u0, _ = sample_many.sample_overlap(wfs, copy.deepcopy(configs), None, **kws)
    avg0, err0 = sample_many.normalize({}, u0)
    s0 = abs(avg0["overlap"][0, 1]) / np.sqrt(avg0["overlap"][0, 0] * avg0["overlap"][1, 1])
    assert s0 > 0.95
    penalty = np.array([[0.0, 5.0], [5.0, 0.0]])
    ensemble.optimize_ensemble(wfs, configs, updater, path, tau=0.5, max_iterations=4, overlap_penalty=penalty, vmc_kwargs=kws)
    from pyqmc_amd.blockfile import BlockFile

    ds = BlockFile(path).datasets()
    assert list(ds["iteration"]) == [0, 0, 1, 1, 2, 2, 3, 3] and list(ds["wavefunction"]) == [0, 1] * 4
    assert np.all(np.isfinite(ds["energy0"])) and np.all(np.isfinite(ds["energy1"]))
    ov = ds["overlap1"][-1]
    s1 = abs(ov[1, 0])
    assert s1 < 0.8, (s0, s1)
    # a restart with everything done runs nothing and restores the stored parameters
    stored = BlockFile(path).load_parameters()
    fresh = [copy.deepcopy(w0), copy.deepcopy(w0)]
    cfg2 = OpenConfigs(np.zeros_like(configs.configs))
    ensemble.optimize_ensemble(fresh, cfg2, updater, path, tau=0.5, max_iterations=4, overlap_penalty=penalty, vmc_kwargs=kws)
    assert len(BlockFile(path).datasets()["iteration"]) == 8
    for i, w in enumerate(fresh):
        assert np.array_equal(np.asarray(w.parameters["wf1det_coeff"]), stored[f"{i}/wf1det_coeff"])
    assert np.array_equal(cfg2.configs, configs.configs)
