"""Golden vectors of the reference's variance optimisation (pyqmc/method/optvariance.py) -> g45_optvariance.npz.

    python tests/golden/make_golden_optvariance.py

Uses make_golden's stubs (numba as an identity decorator, pyscf / h5py mocked), its wave-function builder and its draw recorder.
Water with ECP, make_wf's wave function, 12 fixed walkers:
  Enref      the reference's EnergyAccumulator (threshold 10, recorded ECP draws) once: total and ke;
  cost_*     the reference's own variance_cost_function (captured from optvariance through scipy.optimize.minimize) over the
             flattened wf2acoeff, wf2bcoeff at x0 and at 5 perturbed vectors;
  nm_*       one complete optvariance(..., params=["wf2bcoeff"], method="Nelder-Mead", options={"maxiter": 40}): res.fun and the
             final wf2bcoeff.
Both runs see Enref through an energy callable that returns the recorded values, so the costs involve no draws.  The reference's
cost adds the whole return value of observables.energy.kinetic, the pair (ke, grad2), to the fixed part, and so takes the variance
over 2W numbers; both runs here patch kinetic to its first element, the kinetic energy the cost is documented to use.
"""

import os
import sys
from unittest import mock

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import make_golden as mg  # noqa: E402  (installs the stubs, puts the reference on the path)

import numpy as np  # noqa: E402
import pyqmc.api as pyq  # noqa: E402
import pyqmc.method.optvariance as ov  # noqa: E402
import scipy.optimize  # noqa: E402

from pyqmc_amd import systems  # noqa: E402

NM_MAXITER = 40


def main():
    out = {}
    mol = systems.water()
    mf = systems.random_mf(mol)
    wf = mg.make_wf(mol, mf)
    configs = mg.walkers(mol, 12, 450)
    wf.recompute(configs)
    kinetic = mg.refenergy.kinetic
    patch_ke = mock.patch.object(mg.refenergy, "kinetic", lambda coords, wf: kinetic(coords, wf)[0])
    with mg.Tapes(451):
        en = pyq.EnergyAccumulator(mol, threshold=10.0)(configs, wf)
    patch_ke.start()  # (after the energy evaluation, which unpacks the pair)
    Enref = {"total": np.asarray(en["total"]).copy(), "ke": np.asarray(en["ke"]).copy()}
    out["configs"] = configs.configs.copy()
    out["enref_total"], out["enref_ke"] = Enref["total"], Enref["ke"]

    def energy(coords, wf):
        return Enref

    # the reference's variance_cost_function, captured from its minimize call and evaluated at fixed vectors.  Its np.array of the
    # parameter shapes fails on NumPy >= 1.24 for keys of different rank (acoeff 3-d, bcoeff 2-d), so it is captured once per key;
    # the acoeff function sets that key, and the bcoeff function then sets its own and evaluates with both
    params = ["wf2acoeff", "wf2bcoeff"]
    x0 = np.concatenate([wf.parameters[k].flatten() for k in params])
    rng = np.random.default_rng(452)
    xs = np.stack([x0] + [x0 + 0.05 * rng.standard_normal(x0.shape) for _ in range(5)])
    funs = {}
    for k in params:
        def fake_minimize(fun, x0, callback=None, k=k, **kw):
            funs[k] = fun
            return scipy.optimize.OptimizeResult(x=x0, fun=0.0)

        with mock.patch.object(scipy.optimize, "minimize", fake_minimize):
            ov.optvariance(energy, wf, configs, params=[k])
    Pa = wf.parameters["wf2acoeff"].size
    cost = []
    for x in xs:
        funs["wf2acoeff"](x[:Pa])
        cost.append(funs["wf2bcoeff"](x[Pa:]))
    out["cost_x"], out["cost"] = xs, np.array(cost)

    # one complete Nelder-Mead run over the two-body coefficients, from make_wf's parameters
    wf = mg.make_wf(mol, mf)
    wf.recompute(configs)
    out["nm_x0"] = wf.parameters["wf2bcoeff"].copy()
    fun, wf = ov.optvariance(energy, wf, configs, params=["wf2bcoeff"], method="Nelder-Mead", options={"maxiter": NM_MAXITER})
    out["nm_maxiter"] = np.asarray(NM_MAXITER)
    out["nm_fun"] = np.asarray(fun)
    out["nm_bcoeff"] = np.asarray(wf.parameters["wf2bcoeff"]).copy()
    patch_ke.stop()
    print("costs", out["cost"], "Nelder-Mead", fun, file=sys.stderr)
    mg.save("g45_optvariance", **out)


if __name__ == "__main__":
    main()
