"""Golden vectors of the reference's GeminalJastrow (pyqmc/wf/geminaljastrow.py) -> g48_geminal.npz.

    python tests/golden/make_golden_geminal.py

Uses make_golden's stubs (numba as an identity decorator, pyscf / h5py mocked) and the real pyqmc.wf.geminaljastrow.GeminalJastrow
with the reference's own orbital evaluators handed in through ``orbitals=``: MoleculeOrbitalEvaluator(evaluate_orbitals_with="numba")
for the molecules, the PBCOrbitalEvaluatorKpoints make_golden.ref_pbc_objects builds (Gamma point, S = 1) for the cell.  The
constructor only asks ``mol.eval_gto`` for the number of AOs, so it gets a stand-in that forwards to that evaluator.  Inputs and
outputs only.  The cases (tests/geminal_ref.py: CASES, case_mol):
  a  water (4, 4), nao = 23, 24 walkers
  b  water cluster (32, 32), nao = 184, 70 walkers (ao_val and pgradient of the first 2 walkers, final ao_val of every 8th)
  c  diamond primitive cell (4, 4), nao = 26, PeriodicConfigs, 8 walkers
gcoeff = sigma N(0, 1) with sigma per case (SIGMA; stored): the reference's zeros make every ratio exactly 1.  The generator asserts
max |log Psi| > 0.1 and every stored ratio inside (1e-2, 1e2) before it saves.  Per case: value and ao_val of the start; for one
electron of each spin, in turn, gradient_value, gradient, gradient_laplacian, testvalue (plain, under a mask, with 5 auxiliary points
without and under the mask), testvalue_many of three electrons (plain and under the mask), a masked updateinternals and value();
the moved electrons' ao_val and pgradient after both updates.
"""

import os
import sys
import types

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import make_golden as mg  # noqa: E402  (installs the stubs, puts the reference on the path)

import numpy as np  # noqa: E402
from pyqmc.configurations.coord import OpenConfigs, PeriodicConfigs  # noqa: E402
from pyqmc.wf.geminaljastrow import GeminalJastrow  # noqa: E402
from pyqmc.wf.orbitals import MoleculeOrbitalEvaluator  # noqa: E402

from pyqmc_amd import pbc as mypbc, systems  # noqa: E402

sys.path.insert(0, os.path.join(mg.ROOT, "tests"))
import geminal_ref  # noqa: E402

NAUX = 5
SIGMA = {"a": 0.05, "b": 0.005, "c": 0.05}


def evaluator(mol):
    if hasattr(mol, "a"):
        sup = mypbc.get_supercell(mol, np.eye(3))
        nao = geminal_ref.AOs(mol).nao
        mo = [[np.eye(nao)[:, : sup.nelec[s]]] for s in (0, 1)]
        Ls = mypbc.lattice_points_within(mol.lattice_vectors(), 30.0)
        return mg.ref_pbc_objects(sup, np.zeros((1, 3)), mo, Ls)[1]
    return MoleculeOrbitalEvaluator(mol, [0, 0], evaluate_orbitals_with="numba")


def dump(name, out, seed):
    W, electrons, many, keep = geminal_ref.CASES[name]
    mol = geminal_ref.case_mol(name)
    orb = evaluator(mol)
    periodic = hasattr(mol, "a")
    standin = types.SimpleNamespace(eval_gto=orb.eval_gto)  # (the constructor reads .shape[-1] of one evaluation: the number of AOs)
    rng = np.random.default_rng(seed)
    start = systems.initial_guess(mol, W, rng=np.random.default_rng(seed + 1)).configs
    configs = PeriodicConfigs(start.copy(), mol.lattice_vectors()) if periodic else OpenConfigs(start.copy())
    wf = GeminalJastrow(standin, orbitals=orb)
    npar = len(wf.parameters["gcoeff"])
    wf.parameters["gcoeff"] = SIGMA[name] * rng.standard_normal(npar)
    p = name + "_"
    if periodic:
        out[p + "lattice"] = np.asarray(mol.lattice_vectors())
    out[p + "configs"], out[p + "gcoeff"], out[p + "sigma"] = configs.configs.copy(), wf.parameters["gcoeff"].copy(), np.array([SIGMA[name]])
    out[p + "electrons"], out[p + "many"] = np.asarray(electrons), np.asarray(many)
    _, val = wf.recompute(configs)
    nao = wf.ao_val.shape[-1]
    assert npar == nao * (nao + 1) // 2
    ksl = slice(None) if keep is None else slice(0, keep)
    fsl = slice(None) if keep is None else slice(None, None, 8)
    out[p + "value"], out[p + "ao_val"] = val, wf.ao_val[ksl].copy()
    ratios = []
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
        out[q + "testvalue_many"] = wf.testvalue_many(list(many), ep)
        out[q + "testvalue_many_mask"] = wf.testvalue_many(list(many), ep, mask)
        assert out[q + "testvalue_aux"].shape == (W, NAUX) and out[q + "testvalue_many_mask"].shape == (int(mask.sum()), len(many))
        ratios += [out[q + k] for k in ("gv_val", "testvalue", "testvalue_mask", "testvalue_aux", "testvalue_aux_mask", "testvalue_many",
                                        "testvalue_many_mask")]
        wf.updateinternals(e, ep, configs, mask=accept)
        configs.move(e, ep, accept)
        out[q + "post_value"] = wf.value()[1]
    out[p + "final_ao_moved"] = wf.ao_val[fsl][:, list(electrons), :].copy()
    out[p + "pgrad_gcoeff"] = wf.pgradient()["gcoeff"][ksl]
    allr = np.concatenate([np.ravel(r) for r in ratios])
    assert np.max(np.abs(val)) > 0.1, (name, np.max(np.abs(val)))
    assert allr.min() > 1e-2 and allr.max() < 1e2, (name, allr.min(), allr.max())
    print(name, f"nao {nao}; log {val.min():.2f}..{val.max():.2f}; ratio {allr.min():.3f}..{allr.max():.3f}", file=sys.stderr)


def main():
    out = {}
    for k, name in enumerate(geminal_ref.CASES):
        dump(name, out, 4800 + 10 * k)
    mg.save(geminal_ref.GOLDEN, **out)


if __name__ == "__main__":
    main()
