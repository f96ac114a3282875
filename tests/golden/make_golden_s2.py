"""Golden vectors of the reference's S2Accumulator (pyqmc/observables/s2_accumulator.py) -> g40_s2.npz.

    python tests/golden/make_golden_s2.py

Uses make_golden's stubs (numba as an identity decorator, pyscf / h5py mocked) and its wave-function builder.  Three water
cases, 32 walkers each, per-walker S^2 of the real reference together with every input: configurations, MO coefficients
(2, nao, nmo), determinant list, Jastrow coefficients.
  a  restricted closed-shell water (the same orbitals for both spins), Slater x JastrowSpin
  b  water with nelec (5, 3), separate up / down orbitals, Slater x JastrowSpin
  c  10-determinant water, Slater x JastrowSpin
"""

import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import make_golden as mg  # noqa: E402  (installs the stubs, puts the reference on the path)

import numpy as np  # noqa: E402
from pyqmc.observables.s2_accumulator import S2Accumulator  # noqa: E402

from pyqmc_amd import systems  # noqa: E402

W = 32


def cases():
    """(name, mol, mf, determinants) of the three cases."""
    mol = systems.water()
    mf = systems.random_mf(mol)
    restricted = systems.MeanField(np.stack([mf.mo_coeff[0], mf.mo_coeff[0]]), mf.mo_occ)
    sym, xyz = zip(*systems._WATER)
    mol53 = systems.Mol(sym, xyz, nelec=(5, 3))
    mfc = systems.random_mf(mol, nvirt=6)
    return [("a", mol, restricted, None), ("b", mol53, systems.random_mf(mol53), None),
            ("c", mol, mfc, systems.random_determinants(mol, mfc, 10))]


def main():
    out = {}
    for k, (name, mol, mf, dets) in enumerate(cases()):
        wf = mg.make_wf(mol, mf, determinants=dets)
        configs = mg.walkers(mol, W, 400 + k)
        x0 = configs.configs.copy()
        wf.recompute(configs)
        s2 = S2Accumulator(mol.nelec)(configs, wf)["S2"]
        jas = wf.wf_factors[1]
        out[f"{name}_configs"] = x0
        out[f"{name}_nelec"] = np.asarray(mol.nelec)
        out[f"{name}_mo"] = np.asarray(mf.mo_coeff)
        out[f"{name}_det_json"] = np.asarray(json.dumps(dets))
        out[f"{name}_acoeff"] = np.asarray(jas.parameters["acoeff"])
        out[f"{name}_bcoeff"] = np.asarray(jas.parameters["bcoeff"])
        out[f"{name}_s2"] = np.asarray(s2, dtype=float)
        print(name, mol.nelec, "S2 mean", float(np.mean(s2)), file=sys.stderr)
    mg.save("g40_s2", **out)


if __name__ == "__main__":
    main()
