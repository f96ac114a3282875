"""Golden vectors of the reference's line minimisation (pyqmc/method/linemin.py, sample_many.py) -> g43_linemin.npz.

    python tests/golden/make_golden_linemin.py

Uses make_golden's stubs (numba as an identity decorator, pyscf / h5py mocked), its wave-function builder and its draw recorder.
  a  find_minimum, stable_fit (both tolerances' branches) and the np.linspace step grid on fixed curves;
  b  correlated_compute_worker on water with ECP: 6 fixed walkers, make_wf's wave function, 5 parameter sets along a fixed
     direction of the Jastrow coefficients (the to_opt of generate_jastrow), threshold 10.  The reference resets numpy's random
     state before every set; the recorder follows that reset, so every set takes the same recorded draws (rot, unif of set 0);
  c  sample_overlap_worker for two parameter sets, 3 sweeps of 4 walkers, with its recorded normal / uniform draws.
"""

import copy
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import make_golden as mg  # noqa: E402  (installs the stubs, puts the reference on the path)

import numpy as np  # noqa: E402
import pyqmc.api as pyq  # noqa: E402
import pyqmc.method.linemin as lm  # noqa: E402
import pyqmc.method.sample_many as sm  # noqa: E402
from pyqmc.observables.accumulators import LinearTransform  # noqa: E402
from pyqmc.observables.stochastic_reconfiguration import StochasticReconfiguration  # noqa: E402

from pyqmc_amd import systems  # noqa: E402


def curves():
    """(x, y) pairs: a clean parabola, a noisy one, a line going down, a line going up, a concave curve."""
    rng = np.random.default_rng(440)
    x = np.linspace(-0.2 / 38, 0.2, 40)
    return [x, x, x, x, x], [(x - 0.08) ** 2, (x - 0.05) ** 2 + 1e-4 * rng.standard_normal(40), -2.0 * x + 1.0, 3.0 * x - 0.5,
                             -((x - 0.1) ** 2) + 1e-6 * rng.standard_normal(40)]


def to_opt_jastrow(wf):
    a = np.ones(wf.parameters["wf2acoeff"].shape, dtype=bool)
    b = np.ones(wf.parameters["wf2bcoeff"].shape, dtype=bool)
    b[0] = False
    return {"wf2acoeff": a, "wf2bcoeff": b}


class ResetTapes(mg.Tapes):
    """mg.Tapes whose generator restarts when np.random.set_state is called (the reference's per-set reset)."""

    def __init__(self, seed):
        super().__init__(seed)
        self._seed = seed

    def set_state(self, st):
        self.rng = np.random.default_rng(self._seed)

    def __enter__(self):
        self._ss = np.random.set_state
        np.random.set_state = self.set_state
        return super().__enter__()

    def __exit__(self, *a):
        np.random.set_state = self._ss
        return super().__exit__(*a)


def main():
    out = {}
    xs, ys = curves()
    for i, (x, y) in enumerate(zip(xs, ys)):
        out[f"a{i}_x"], out[f"a{i}_y"] = x, y
        out[f"a{i}_find"] = np.asarray(lm.find_minimum(x, y))
        out[f"a{i}_stable"] = np.asarray(lm.stable_fit(x, y))
        out[f"a{i}_stable_tol"] = np.asarray(lm.stable_fit(x, y, tolerance=1e-6))
    out["a_linspace"] = np.linspace(-0.2 / (40 - 2), 0.2, 40)

    mol = systems.water()
    mf = systems.random_mf(mol)
    wf = mg.make_wf(mol, mf)
    W = 6
    configs = mg.walkers(mol, W, 441)
    to_opt = to_opt_jastrow(wf)
    tr = LinearTransform(wf.parameters, to_opt)
    enacc = pyq.EnergyAccumulator(mol, threshold=10.0)
    sr = StochasticReconfiguration(enacc, tr)
    x0 = tr.serialize_parameters(wf.parameters)
    d = np.random.default_rng(442).standard_normal(len(x0))
    d /= np.linalg.norm(d)
    params = [x0 + t * d for t in np.linspace(-0.1, 0.3, 5)]
    out["b_configs"] = configs.configs.copy()
    out["b_params"] = np.asarray(params)
    out["b_x0"] = x0
    for k, m in to_opt.items():
        out["b_opt_" + k] = m
    with ResetTapes(443) as t:
        res = lm.correlated_compute_worker(wf, configs, params, sr, [0, 1])
    N, necp = sum(mol.nelec), 2 + 1  # (water: O and both H carry an ECP)
    n_rot = N * necp
    out["b_rot"] = np.asarray(t.log["rot"][:n_rot]).reshape(N, necp, 3, 3)
    out["b_unif"] = np.asarray(t.log["random"][:n_rot]).reshape(N, necp, W)
    assert len(t.log["rot"]) == len(params) * n_rot
    for k, v in res.items():
        out["b_" + k] = np.asarray(v)
    # the log values the worker forms its weights from: a recompute at each set
    logpsi = []
    for p in params:
        lm.set_wf_params(wf, p, sr)
        logpsi.append(wf.recompute(configs)[1])
    out["b_logpsi"] = np.asarray(logpsi)

    # c: the mixture walk
    wf0 = copy.deepcopy(wf)
    wfs = [copy.deepcopy(wf0), copy.deepcopy(wf0)]
    lm.set_wf_params(wfs[0], params[0], sr)
    lm.set_wf_params(wfs[1], params[4], sr)
    Wc = 4
    cfg = mg.walkers(mol, Wc, 444)
    out["c_start"] = cfg.configs.copy()
    out["c_params"] = np.asarray([params[0], params[4]])
    with mg.Tapes(445) as t:
        _, unweighted, cfg = sm.sample_overlap_worker(wfs, cfg, 0.5, 3, None)
    out["c_normal"] = np.asarray(t.log["normal"])  # (3 * N, Wc, 3): scale sqrt(tstep) applied by the caller
    out["c_rand"] = np.asarray(t.log["rand"]).reshape(3 * N, Wc)
    out["c_final"] = cfg.configs.copy()
    out["c_overlap"] = np.asarray(unweighted["overlap"])
    print("b total", res["total"].mean(axis=1), "c overlap", unweighted["overlap"].ravel(), file=sys.stderr)
    mg.save("g43_linemin", **out)


if __name__ == "__main__":
    main()
