"""Golden vectors of the reference's simultaneous ensemble estimator and its threaded driver (pyqmc/observables/
stochastic_reconfiguration.py:179-369, pyqmc/method/ensemble_optimization_threaded.py) -> g52_ensemble_multi.npz.

    python tests/golden/make_golden_ensemble_multi.py

Uses make_golden's stubs (numba as an identity decorator, pyscf / h5py mocked).
  a  StochasticReconfigurationMultipleWF.avg for K = 3 states on fixed pgradient dictionaries and random (K, K, nconf) weights: state 0
     optimises part of det_coeff and bcoeff, state 1 part of bcoeff, state 2 nothing (nparams == 0); the energy object returns fixed
     per-state rows.  Tuple keys ("dp", i) are stored as "dp_i";
  b  its block_average, _collect_terms and delta_p (overlap_penalty not uniform) on fixed blocks;
  c  round_to_fixed_sum cases, the error branch included;
  d  one iteration of the threaded optimize_ensemble over 2 states with vmc and sample_overlap replaced by stubs that return fixed data
     (stored here) chosen by their arguments (which wf, how many wfs, energy is None): the reference calls them from threads.  The
     updated parameters and the records it saves.
"""

import os
import sys
import types

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import make_golden as mg  # noqa: E402  (installs the stubs, puts the reference on the path)

import numpy as np  # noqa: E402
import pyqmc.method.ensemble_optimization_threaded as thr  # noqa: E402
from pyqmc.method.ensemble_optimization_wfbywf import StochasticReconfigurationWfbyWf  # noqa: E402
from pyqmc.observables.accumulators import LinearTransform  # noqa: E402
from pyqmc.observables.stochastic_reconfiguration import StochasticReconfigurationMultipleWF  # noqa: E402

K = 3


class FakeEnacc:
    def __init__(self, table=None):
        self.table = table

    def __call__(self, configs, wf):
        return {k: v[wf.index] for k, v in self.table.items()}

    def keys(self):
        return {"total"}

    def shapes(self):
        return {"total": ()}


def fake_wf(params, pgrad=None, index=0):
    return types.SimpleNamespace(parameters=params, pgradient=lambda: pgrad, index=index)


def to_opts():
    """Per state: what it optimises (state 2: nothing)."""
    det = [np.array([False, True, True]), np.zeros(3, dtype=bool), np.zeros(3, dtype=bool)]
    b = [np.ones((3, 3), dtype=bool), np.zeros((3, 3), dtype=bool), np.zeros((3, 3), dtype=bool)]
    b[0][0] = False
    b[1][1:, :2] = True
    return [{"wf1det_coeff": det[i], "wf2bcoeff": b[i]} for i in range(K)]


def key_name(k):
    return k if isinstance(k, str) else f"{k[0]}_{k[1]}"


def part_ab(out):
    rng = np.random.default_rng(520)
    nconf = 7
    params = [{"wf1det_coeff": np.array([1.0, 0.3, -0.2]) + 0.1 * i, "wf2bcoeff": rng.standard_normal((3, 3))} for i in range(K)]
    transforms = [LinearTransform(p, o) for p, o in zip(params, to_opts())]
    assert [int(t.nparams) for t in transforms] == [8, 4, 0]
    pgrads = [{"wf1det_coeff": rng.standard_normal((nconf, 3)), "wf2bcoeff": rng.standard_normal((nconf, 3, 3))} for _ in range(K)]
    table = {"total": -17.0 + rng.standard_normal((K, nconf)), "ke": rng.standard_normal((K, nconf))}
    weights = rng.standard_normal((K, K, nconf))
    for i in range(K):
        out[f"a_params_b{i}"] = params[i]["wf2bcoeff"]
        out[f"a_pg_det{i}"], out[f"a_pg_b{i}"] = pgrads[i]["wf1det_coeff"], pgrads[i]["wf2bcoeff"]
    out["a_total"], out["a_ke"], out["a_weights"] = table["total"], table["ke"], weights
    sr = StochasticReconfigurationMultipleWF(FakeEnacc(table), transforms, eps=0.05)
    wfs = [fake_wf(params[i], pgrads[i], i) for i in range(K)]
    avg = sr.avg(None, wfs, weights)
    for k, v in avg.items():
        out["a_avg_" + key_name(k)] = np.asarray(v)
    # b: blocks of what avg returns
    nb = 5
    P = [int(t.nparams) for t in transforms]
    ov = rng.standard_normal((nb, K, K)) * 0.1 + np.eye(K) * np.array([1.0, 0.8, 1.3])
    data = {"total": -17.0 + 0.1 * rng.standard_normal((nb, K, K))}
    for i in range(K):
        if P[i] == 0:
            continue
        A = rng.standard_normal((nb, P[i], P[i]))
        data[("dp", i)] = rng.standard_normal((nb, P[i], K))
        data[("dpH", i)] = rng.standard_normal((nb, P[i], K))
        data[("dpipj", i)] = np.einsum("bij,bkj->bik", A, A) + 3 * np.eye(P[i])
    out["b_ov"] = ov
    for k, v in data.items():
        out["b_data_" + key_name(k)] = v
    avg, err = sr.block_average(data, ov)
    for k, v in avg.items():
        out["b_ba_avg_" + key_name(k)] = np.asarray(v)
    for k, v in err.items():
        out["b_ba_err_" + key_name(k)] = np.asarray(v)
    terms = sr._collect_terms(avg, err)
    for k, v in terms.items():
        out["b_ct_" + key_name(k)] = np.asarray(v)
    penalty = np.array([[0.0, 0.7, 1.5], [0.7, 0.0, 2.5], [1.5, 2.5, 0.0]])
    out["b_penalty"] = penalty
    dp, report = sr.delta_p([0.1, 0.4], avg, penalty)
    for i in range(K):
        out[f"b_dp{i}"] = np.asarray(dp[i])
    out["b_report"] = np.array([report["pgrad"], report["SRdot"]])


def part_c(out):
    cases = [(np.array([1.0, 1.0, 0.5, 1.0]), 8), (np.array([1.0, 1.0, 1.0]), 10), (np.array([0.2, 3.1, 0.01, 1.7]), 16),
             (np.array([1.0, 0.5]), 1), (np.array([2.5]), 4)]
    out["c_n"] = len(cases)
    for n, (x, t) in enumerate(cases):
        out[f"c_x{n}"], out[f"c_t{n}"] = x, t
        out[f"c_y{n}"] = thr.round_to_fixed_sum(x, t)
    # the error branch: a total that is not finite leaves a difference no rounding can close
    bad = np.array([1.0, -1.0])
    out["c_bad_x"], out["c_bad_t"] = bad, 3
    try:
        thr.round_to_fixed_sum(bad, 3)
        raise AssertionError("round_to_fixed_sum took a zero-sum input")
    except ValueError:
        pass


def part_d(out):
    rng = np.random.default_rng(523)
    nb, nconf, P = 3, 5, 4
    base = {"wf1det_coeff": np.array([1.0, 0.3, -0.2]), "wf2bcoeff": np.array([0.1, 0.2])}
    to_opt = {"wf1det_coeff": np.array([False, True, True]), "wf2bcoeff": np.array([True, True])}
    wfs = [fake_wf({k: v.copy() for k, v in base.items()}, index=0), fake_wf({k: v + 0.05 for k, v in base.items()}, index=1)]
    updater = [[StochasticReconfigurationWfbyWf(FakeEnacc(), LinearTransform(w.parameters, to_opt), eps=0.02)] for w in wfs]
    out["d_ov_norm"] = np.eye(2) * np.array([1.0, 0.7]) + 0.05 * rng.standard_normal((nb, 2, 2))
    for i in range(2):
        k = i + 1
        out[f"d_ov_sub{i}"] = np.eye(k) + 0.05 * rng.standard_normal((nb, k, k))
        out[f"d_wtdp{i}"] = 0.1 * rng.standard_normal((nb, P, k, k))
        A = rng.standard_normal((nb, P, P))
        out[f"d_s1_total{i}"] = -17.0 + 0.1 * rng.standard_normal(nb)
        out[f"d_s1_dppsi{i}"] = rng.standard_normal((nb, P))
        out[f"d_s1_dpH{i}"] = rng.standard_normal((nb, P))
        out[f"d_s1_dpidpj{i}"] = np.einsum("bij,bkj->bik", A, A) + 2 * np.eye(P)
    out["d_configs"] = rng.standard_normal((nconf, 2, 3))
    configs = types.SimpleNamespace(configs=out["d_configs"].copy())

    def sample_overlap(wfs_, configs_, energy, **kw):
        if energy is None:  # the normalisation sampling of all states
            assert len(wfs_) == 2
            return {}, {"overlap": out["d_ov_norm"]}, configs_
        i = len(wfs_) - 1
        return {"wtdp": out[f"d_wtdp{i}"]}, {"overlap": out[f"d_ov_sub{i}"]}, configs_

    def vmc(wf, configs_, accumulators=None, **kw):
        if accumulators is None:  # the warm-up
            return None, configs_
        i = wf.index
        return {k: out[f"d_s1_{k}{i}"] for k in ("total", "dppsi", "dpH", "dpidpj")}, configs_

    saved = []
    thr.pyqmc.method.sample_many.sample_overlap = sample_overlap
    thr.pyqmc.method.mc.vmc = vmc
    thr.hdf_save = lambda hdf_file, data, attr, wfs_, configs_: saved.append(
        (dict(data), [{k: np.array(v) for k, v in w.parameters.items()} for w in wfs_]))
    penalty = np.array([[0.0, 1.7], [1.7, 0.0]])
    out["d_penalty"] = penalty
    thr.optimize_ensemble(wfs, configs, updater, None, None, tau=0.3, max_iterations=1, overlap_penalty=penalty, npartitions=4, verbose=False)
    assert len(saved) == 2
    for n, (data, params) in enumerate(saved):
        for k, v in data.items():
            out[f"d_rec{n}_{k}"] = np.asarray(v)
        for i, p in enumerate(params):
            for k, v in p.items():
                out[f"d_rec{n}_wf{i}_{k}"] = v


def main():
    out = {}
    part_ab(out)
    part_c(out)
    part_d(out)
    mg.save("g52_ensemble_multi", **out)


if __name__ == "__main__":
    main()
