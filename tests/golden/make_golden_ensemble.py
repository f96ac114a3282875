"""Golden vectors of the reference's ensemble optimisation (pyqmc/method/ensemble_optimization_wfbywf.py, sample_many.py,
observables/accumulators_multiwf.py) -> g44_ensemble.npz.

    python tests/golden/make_golden_ensemble.py

Uses make_golden's stubs (numba as an identity decorator, pyscf / h5py mocked), its wave-function builder and its draw recorder.
  a  sample_overlap_worker for three water wave functions (Slater x two-body Jastrow over one list of random determinants, different
     det_coeff), 6 walkers, 2 sweeps, EnergyAccumulatorMultipleWF(EnergyAccumulator(mol), offset -16.5): the normal / uniform / ECP draws, the final
     walkers, the overlap and every weighted energy key;
  b  StochasticReconfigurationWfbyWf.avg, block_average, _collect_terms and delta_p (overlap_penalty not uniform) on fixed inputs;
  c  renormalize on fixed norms (wf1det_coeff and det_coeff);
  d  one optimize_ensemble iteration over 2 states with sample_overlap and vmc replaced by stubs that return fixed data (stored here),
     the updated parameters and the records it saves.
"""

import os
import sys
import types

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import make_golden as mg  # noqa: E402  (installs the stubs, puts the reference on the path)

import numpy as np  # noqa: E402
import pyqmc.api as pyq  # noqa: E402
import pyqmc.method.ensemble_optimization_wfbywf as ens  # noqa: E402
import pyqmc.method.sample_many as sm  # noqa: E402
from pyqmc.observables.accumulators import LinearTransform  # noqa: E402
from pyqmc.observables.accumulators_multiwf import EnergyAccumulatorMultipleWF  # noqa: E402

from pyqmc_amd import systems  # noqa: E402

KEYS = ("total", "ke", "ee", "ei", "ecp", "grad2")


def part_a(out):
    mol = systems.water()
    mf = systems.random_mf(mol, nvirt=4)
    ndet = 4
    dets = systems.random_determinants(mol, mf, ndet)
    coeffs = np.array([[1.0, 0.2, -0.1, 0.05], [0.3, 1.0, 0.2, -0.2], [-0.2, 0.4, 1.0, 0.3]])
    wfs = []
    for c in coeffs:
        wf = mg.make_wf(mol, mf, determinants=dets)
        wf.parameters["wf1det_coeff"] = c.copy()
        wfs.append(wf)
    W, nsteps = 6, 2
    cfg = mg.walkers(mol, W, 450)
    out["a_ndet"] = ndet
    out["a_nsteps"] = nsteps
    out["a_det_coeff"] = coeffs
    out["a_start"] = cfg.configs.copy()
    # (a NumPy scalar offset: the reference's rolling_average needs .shape, which its default int 0 lacks)
    acc = EnergyAccumulatorMultipleWF(pyq.EnergyAccumulator(mol), offset=np.float64(-16.5))
    with mg.Tapes(451) as t:
        weighted, unweighted, cfg = sm.sample_overlap_worker(wfs, cfg, 0.5, nsteps, acc)
    N, necp, K = sum(mol.nelec), 3, len(wfs)
    out["a_normal"] = np.asarray(t.log["normal"])  # (nsteps N, W, 3), unit normals (scale applied by the caller)
    out["a_rand"] = np.asarray(t.log["rand"]).reshape(nsteps * N, W)
    out["a_rot"] = np.asarray(t.log["rot"]).reshape(nsteps * K, N, necp, 3, 3)  # one energy evaluation per (sweep, wave function)
    out["a_unif"] = np.asarray(t.log["random"]).reshape(nsteps * K, N, necp, W)
    out["a_final"] = cfg.configs.copy()
    out["a_overlap"] = np.asarray(unweighted["overlap"])
    out["a_w_offset"] = np.asarray(weighted["offset"])
    for k in KEYS:
        out["a_w_" + k] = np.asarray(weighted[k])
    print("a overlap", out["a_overlap"].ravel(), file=sys.stderr)


class FakeEnacc:
    def keys(self):
        return {"total"}

    def shapes(self):
        return {"total": ()}


def fake_wf(params, pgrad=None):
    return types.SimpleNamespace(parameters=params, pgradient=lambda: pgrad)


def part_b(out):
    rng = np.random.default_rng(452)
    nconf, K = 7, 3
    params = {"wf1det_coeff": np.array([1.0, 0.3, -0.2]), "wf2bcoeff": rng.standard_normal((3, 3))}
    to_opt = {"wf1det_coeff": np.array([False, True, True]), "wf2bcoeff": np.ones((3, 3), dtype=bool)}
    to_opt["wf2bcoeff"][0] = False
    tr = LinearTransform(params, to_opt)
    P = int(tr.nparams)
    pgrad = {"wf1det_coeff": rng.standard_normal((nconf, 3)), "wf2bcoeff": rng.standard_normal((nconf, 3, 3))}
    weights = rng.standard_normal((K, K, nconf))
    sr = ens.StochasticReconfigurationWfbyWf(FakeEnacc(), tr, eps=0.05)
    wfs = [fake_wf(params), fake_wf(params), fake_wf(params, pgrad)]
    out["b_pg_det"], out["b_pg_b"], out["b_weights"] = pgrad["wf1det_coeff"], pgrad["wf2bcoeff"], weights
    out["b_params_b"] = params["wf2bcoeff"]
    out["b_avg_wtdp"] = sr.avg(None, wfs, weights)["wtdp"]
    nb = 5
    ov = rng.standard_normal((nb, K, K)) * 0.1 + np.eye(K) * np.array([1.0, 0.8, 1.3])
    data = {"wtdp": rng.standard_normal((nb, P, K, K))}
    s1 = {"total": -17.0 + 0.1 * rng.standard_normal(nb), "dppsi": rng.standard_normal((nb, P)),
          "dpH": rng.standard_normal((nb, P)), "dpidpj": None}
    A = rng.standard_normal((nb, P, P))
    s1["dpidpj"] = np.einsum("bij,bkj->bik", A, A) + 3 * np.eye(P)
    out["b_ov"], out["b_wtdp"] = ov, data["wtdp"]
    for k, v in s1.items():
        out["b_s1_" + k] = v
    avg, err = sr.block_average(s1, data, ov)
    for k, v in avg.items():
        out["b_ba_avg_" + k] = np.asarray(v)
    for k, v in err.items():
        out["b_ba_err_" + k] = np.asarray(v)
    terms = sr._collect_terms(avg, err)
    for k, v in terms.items():
        out["b_ct_" + k] = np.asarray(v)
    penalty = np.array([[0.0, 0.7, 1.5], [0.7, 0.0, 2.5], [1.5, 2.5, 0.0]])
    out["b_penalty"] = penalty
    dp, report = sr.delta_p([0.1, 0.4], avg, penalty)
    out["b_dp"] = np.asarray(dp)
    out["b_report"] = np.array([report["pgrad"], report["SRdot"]])


def part_c(out):
    norms = np.array([1.3, 0.7, 2.1])
    out["c_norms"] = norms
    for key in ("wf1det_coeff", "det_coeff"):
        wfs = [fake_wf({key: np.array([1.0, 0.5 * i, -0.25])}) for i in range(3)]
        ens.renormalize(wfs, norms, pivot=1, N=1.5)
        out["c_" + key] = np.array([w.parameters[key] for w in wfs])


def part_d(out):
    rng = np.random.default_rng(453)
    nb, nconf = 3, 5
    base = {"wf1det_coeff": np.array([1.0, 0.3, -0.2]), "wf2bcoeff": np.array([0.1, 0.2])}
    to_opt = {"wf1det_coeff": np.array([False, True, True]), "wf2bcoeff": np.array([True, True])}
    wfs = [fake_wf({k: v.copy() for k, v in base.items()}), fake_wf({k: v + 0.05 for k, v in base.items()})]
    P = 4
    updater = [[ens.StochasticReconfigurationWfbyWf(FakeEnacc(), LinearTransform(w.parameters, to_opt), eps=0.02)] for w in wfs]
    # the stubs' returns, in call order: for state i: mixture (all states), vmc on state i, mixture (states 0 .. i) with wtdp
    for i in range(2):
        ov = np.eye(2) * np.array([1.0, 0.6 + 0.2 * i]) + 0.05 * rng.standard_normal((nb, 2, 2))
        out[f"d_ov_all{i}"] = ov
        k = i + 1
        out[f"d_ov_sub{i}"] = np.eye(k) + 0.05 * rng.standard_normal((nb, k, k))
        out[f"d_wtdp{i}"] = 0.1 * rng.standard_normal((nb, P, k, k))
        A = rng.standard_normal((nb, P, P))
        out[f"d_s1_total{i}"] = -17.0 + 0.1 * rng.standard_normal(nb)
        out[f"d_s1_dppsi{i}"] = rng.standard_normal((nb, P))
        out[f"d_s1_dpH{i}"] = rng.standard_normal((nb, P))
        out[f"d_s1_dpidpj{i}"] = np.einsum("bij,bkj->bik", A, A) + 2 * np.eye(P)
    out["d_configs"] = rng.standard_normal((nconf, 2, 3))
    calls = {"so": 0, "vmc": 0}
    configs = types.SimpleNamespace(configs=out["d_configs"].copy())

    def sample_overlap(wfs_, configs_, energy, **kw):
        i = calls["so"] // 2
        first = calls["so"] % 2 == 0
        calls["so"] += 1
        if first:
            return {}, {"overlap": out[f"d_ov_all{i}"]}, configs_
        return {"wtdp": out[f"d_wtdp{i}"]}, {"overlap": out[f"d_ov_sub{i}"]}, configs_

    def vmc(wf, configs_, accumulators=None, **kw):
        if accumulators is None:
            return None, configs_
        i = calls["vmc"]
        calls["vmc"] += 1
        return {k: out[f"d_s1_{k}{i}"] for k in ("total", "dppsi", "dpH", "dpidpj")}, configs_

    saved = []
    ens.pyqmc.method.sample_many.sample_overlap = sample_overlap
    ens.pyqmc.method.mc.vmc = vmc
    ens.hdf_save = lambda hdf_file, data, attr, wfs_, configs_: saved.append(
        (dict(data), [{k: np.array(v) for k, v in w.parameters.items()} for w in wfs_]))
    penalty = np.array([[0.0, 1.7], [1.7, 0.0]])
    out["d_penalty"] = penalty
    ens.optimize_ensemble(wfs, configs, updater, None, tau=0.3, max_iterations=1, overlap_penalty=penalty)
    assert len(saved) == 2
    for n, (data, params) in enumerate(saved):
        for k, v in data.items():
            out[f"d_rec{n}_{k}"] = np.asarray(v)
        for i, p in enumerate(params):
            for k, v in p.items():
                out[f"d_rec{n}_wf{i}_{k}"] = v


def main():
    out = {}
    part_a(out)
    part_b(out)
    part_c(out)
    part_d(out)
    mg.save("g44_ensemble", **out)


if __name__ == "__main__":
    main()
