"""Golden vectors of the reference's GPSJastrow (pyqmc/wf/gps2.py) -> g47_gps.npz.

    python tests/golden/make_golden_gps.py

Uses make_golden's stubs (numba as an identity decorator, pyscf / h5py mocked) and the real pyqmc.wf.gps2.GPSJastrow.  Inputs and
outputs only.  The cases (tests/gps_ref.py: CASES, case_mol):
  a  water (4, 4), 24 walkers, 6 support pairs, f = 0.5
  b  water cluster (32, 32), 70 walkers, 33 support pairs, f = 1.0 (e_cs of the first 4 walkers only)
  c  three He atoms in a triclinic cell, PeriodicConfigs, 8 walkers, 5 support pairs inside the cell, f = 0.8
Support points are electron positions picked from the walkers plus N(0, 0.3) noise, alpha ~ N(0, 0.3): the reference's default
f = 100 leaves e_cs empty and every ratio exactly 1.  Per case: value and e_cs of the start; for one electron of each spin, in turn,
gradient_value, gradient_laplacian, testvalue (2-D, under a mask, with 5 auxiliary points without and under the mask), then a masked
updateinternals and value(); e_cs and the three pgradient arrays of the state after both updates.
"""

import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import make_golden as mg  # noqa: E402  (installs the stubs, puts the reference on the path)

import numpy as np  # noqa: E402
from pyqmc.configurations.coord import OpenConfigs, PeriodicConfigs  # noqa: E402
from pyqmc.wf.gps2 import GPSJastrow  # noqa: E402

from pyqmc_amd import systems  # noqa: E402

sys.path.insert(0, os.path.join(mg.ROOT, "tests"))
import gps_ref  # noqa: E402

NAUX = 5


def dump(name, out, seed):
    W, nsup, f, electrons = gps_ref.CASES[name]
    mol = gps_ref.case_mol(name)
    rng = np.random.default_rng(seed)
    start = systems.initial_guess(mol, W, rng=np.random.default_rng(seed + 1)).configs
    periodic = hasattr(mol, "a")
    configs = PeriodicConfigs(start.copy(), mol.lattice_vectors()) if periodic else OpenConfigs(start.copy())
    N = configs.configs.shape[1]
    X = configs.configs[rng.integers(W, size=(nsup, 2)), rng.integers(N, size=(nsup, 2))] + 0.3 * rng.standard_normal((nsup, 2, 3))
    if periodic:  # supports inside the cell
        lat = mol.lattice_vectors()
        X = (X @ np.linalg.inv(lat) % 1.0) @ lat
        out[f"{name}_lattice"] = np.asarray(lat)
    wf = GPSJastrow(mol, X, f=f)
    wf.parameters["alpha"] = 0.3 * rng.standard_normal(nsup)
    p = name + "_"
    out[p + "configs"], out[p + "Xsupport"], out[p + "alpha"], out[p + "f"] = configs.configs.copy(), X, wf.parameters["alpha"].copy(), np.array([f])
    out[p + "electrons"] = np.asarray(electrons)
    _, val = wf.recompute(configs)
    keep = slice(0, 4) if name == "b" else slice(None)
    out[p + "value"], out[p + "e_cs"] = val, wf.e_cs[keep].copy()
    # the inputs must exercise the factor: a quarter of the Gaussians above 1e-3 and a log value off zero.  Case b is eight molecules
    # 6 bohr apart and exp(-r^2) > 1e-3 needs r < 2.63 bohr, so a support point reaches the electrons of its own molecule only:
    # a quarter of one eighth there
    frac, need = float(np.mean(wf.e_cs > 1e-3)), 0.25 / (8 if name == "b" else 1)
    assert frac >= need and np.max(np.abs(val)) > 0.1, (name, frac, np.max(np.abs(val)))
    spans = {"ratio": [], "grad": [], "lap": []}
    for e in electrons:
        q = p + f"e{e}_"
        newpos = configs.configs[:, e, :] + 0.6 * rng.standard_normal((W, 3))
        aux = configs.configs[:, e, None, :] + 0.8 * rng.standard_normal((W, NAUX, 3))
        mask = rng.random(W) > 0.35
        mask[0], mask[1] = True, False
        accept = rng.random(W) > 0.4
        accept[-1], accept[0] = True, False
        ep = configs.make_irreducible(e, newpos)
        ea = configs.make_irreducible(e, aux)
        out[q + "newpos"], out[q + "aux"], out[q + "mask"], out[q + "accept"] = ep.configs.copy(), ea.configs.copy(), mask, accept
        g, v, _ = wf.gradient_value(e, ep)
        out[q + "gv_grad"], out[q + "gv_val"] = g, v
        out[q + "grad"] = wf.gradient(e, ep)
        g, lap = wf.gradient_laplacian(e, ep)
        out[q + "gl_grad"], out[q + "gl_lap"] = g, lap
        out[q + "testvalue"] = wf.testvalue(e, ep)[0]
        out[q + "testvalue_mask"] = wf.testvalue(e, ep, mask)[0]
        out[q + "testvalue_aux"] = wf.testvalue(e, ea)[0]
        out[q + "testvalue_aux_mask"] = wf.testvalue(e, ea, mask)[0]
        spans["ratio"] += [v.min(), v.max()]
        spans["grad"].append(np.abs(g).max())
        spans["lap"].append(np.abs(lap).max())
        wf.updateinternals(e, ep, configs, mask=accept)  # (moves `configs` as well: gps2.py:74)
        out[q + "post_value"] = wf.value()[1]
    # the state after both updates: the columns of the two moved electrons for every walker (the final walkers follow from
    # newpos and accept)
    out[p + "final_e_cs_moved"] = wf.e_cs[:, :, list(electrons), :].copy()
    fresh = GPSJastrow(mol, X, f=f)
    fresh.parameters["alpha"] = wf.parameters["alpha"]
    assert np.array_equal(fresh.recompute(configs)[1], wf.value()[1])  # update-then-value() is a fresh recompute, exactly
    assert max(abs(min(spans["ratio"]) - 1), abs(max(spans["ratio"]) - 1)) > 0.05, (name, spans["ratio"])
    for k, v in wf.pgradient().items():
        out[p + "pgrad_" + k] = v
    print(name, f"e_cs > 1e-3: {frac:.2f}; log {val.min():.2f}..{val.max():.2f}; ratio {min(spans['ratio']):.2f}..{max(spans['ratio']):.2f}; "
          f"|grad| <= {max(spans['grad']):.2f}; |lap| <= {max(spans['lap']):.2f}", file=sys.stderr)


def main():
    out = {}
    for k, name in enumerate(gps_ref.CASES):
        dump(name, out, 4700 + 10 * k)
    mg.save(gps_ref.GOLDEN, **out)


if __name__ == "__main__":
    main()
