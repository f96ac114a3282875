"""Golden vectors of the reference's symmetry accumulators (pyqmc/observables/accumulators.py:237-341) -> g41_symmetry.npz.

    python tests/golden/make_golden_symmetry.py

Uses make_golden's stubs (numba as an identity decorator, pyscf / h5py mocked), its molecular wave-function builder and its
periodic one (ref_pbc_objects through ref_pbc_wf).  32 walkers per case; per operator the reference's ratios together with every
input: configurations, operators (and origins), MO coefficients (2, nao, nmo), determinant list, Jastrow coefficients.
  a  water, Slater x JastrowSpin, SymmetryAccumulator: the C2v operations (x -> -x, y -> -y, C2 about z) and a generic rotation
  b  10-determinant water, the same operators
  p  diamond primitive cell at Gamma, SymmetryAccumulatorPBC: inversion through a bond centre, a C2 rotation and a generic rotation,
     each about a nonzero origin; the transformed points leave the cell, so enforce_pbc matters
"""

import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import make_golden as mg  # noqa: E402  (installs the stubs, puts the reference on the path)

import numpy as np  # noqa: E402
from pyqmc.observables.accumulators import SymmetryAccumulator, SymmetryAccumulatorPBC  # noqa: E402

from pyqmc_amd import systems  # noqa: E402

W = 32


def rotation(axis, angle):
    """Row-vector rotation matrix (x' = x @ R) about `axis` by `angle`."""
    k = np.asarray(axis, dtype=float)
    k /= np.linalg.norm(k)
    K = np.array([[0, -k[2], k[1]], [k[2], 0, -k[0]], [-k[1], k[0], 0]])
    return (np.eye(3) + np.sin(angle) * K + (1 - np.cos(angle)) * K @ K).T


def molecule_ops():
    return {"sigma_yz": np.diag([-1.0, 1.0, 1.0]), "sigma_xz": np.diag([1.0, -1.0, 1.0]), "c2z": np.diag([-1.0, -1.0, 1.0]),
            "generic": rotation([0.3, -0.5, 0.8], 0.7)}


def crystal_ops(cell):
    a = cell.atom_coords()
    centre = 0.5 * (a[0] + a[1])  # bond centre of diamond: an inversion centre
    ops = {"inversion": -np.eye(3), "c2_110": rotation([1.0, 1.0, 0.0], np.pi), "generic": rotation([0.2, 0.9, -0.4], 1.1)}
    origins = {"inversion": centre, "c2_110": a[1].copy(), "generic": np.array([0.7, -0.3, 1.9])}
    return ops, origins


def main():
    out = {}
    mol = systems.water()
    mf = systems.random_mf(mol)
    mfc = systems.random_mf(mol, nvirt=6)
    for k, (name, m, dets) in enumerate([("a", mf, None), ("b", mfc, systems.random_determinants(mol, mfc, 10))]):
        wf = mg.make_wf(mol, m, determinants=dets)
        configs = mg.walkers(mol, W, 410 + k)
        x0 = configs.configs.copy()
        wf.recompute(configs)
        ops = molecule_ops()
        res = SymmetryAccumulator(ops)(configs, wf)
        jas = wf.wf_factors[1]
        out[f"{name}_configs"] = x0
        out[f"{name}_mo"] = np.asarray(m.mo_coeff)
        out[f"{name}_det_json"] = np.asarray(json.dumps(dets))
        out[f"{name}_acoeff"] = np.asarray(jas.parameters["acoeff"])
        out[f"{name}_bcoeff"] = np.asarray(jas.parameters["bcoeff"])
        out[f"{name}_names"] = np.asarray(list(ops))
        out[f"{name}_ops"] = np.stack([ops[n] for n in ops])
        out[f"{name}_ratio"] = np.stack([np.asarray(res[n], dtype=float) for n in ops])
        print(name, {n: float(np.mean(res[n])) for n in ops}, file=sys.stderr)

    from pyqmc.configurations.coord import PeriodicConfigs

    sup, wf = mg.ref_pbc_wf("gamma")
    lat = sup.lattice_vectors()
    configs = PeriodicConfigs(systems.initial_guess(sup, W, rng=np.random.default_rng(420)).configs.copy(), lat)
    x0, wrap0 = configs.configs.copy(), configs.wrap.copy()
    wf.recompute(configs)
    ops, origins = crystal_ops(sup)
    res = SymmetryAccumulatorPBC(ops, origins)(configs, wf)
    for n in ops:  # the transformed points leave the cell: enforce_pbc folds some of them back
        y = np.einsum("ijk,kl->ijl", x0 - origins[n], ops[n]) + origins[n]
        frac = y @ np.linalg.inv(lat)
        print("p", n, "points outside the cell", int(np.sum(np.any((frac < 0) | (frac >= 1), axis=-1))), file=sys.stderr)
    jas = wf.wf_factors[1]
    out["p_configs"], out["p_wrap"] = x0, wrap0
    out["p_acoeff"] = np.asarray(jas.parameters["acoeff"])
    out["p_bcoeff"] = np.asarray(jas.parameters["bcoeff"])
    out["p_names"] = np.asarray(list(ops))
    out["p_ops"] = np.stack([ops[n] for n in ops])
    out["p_origins"] = np.stack([origins[n] for n in ops])
    out["p_ratio"] = np.stack([np.asarray(res[n], dtype=float) for n in ops])
    print("p", {n: float(np.mean(res[n])) for n in ops}, file=sys.stderr)
    mg.save("g41_symmetry", **out)


if __name__ == "__main__":
    main()
