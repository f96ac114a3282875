"""Fixture correlated_parent: every output of pqa_correlated, pqa_correlated_md, pqa_correlated_j3 and pqa_variance on small cases that
reach every line of their host driver and kernels (tests/test_gpu_correlated_parent.py replays the same calls and compares bit for
bit).  Record it on the GPU from a tree of the commit BEFORE the three correlated entries got their one host driver, with that
tree's library and Python; only public classes and methods are used, so the file runs unchanged in both:

    python tools/make_correlated_golden.py --tree <parent tree> --out tests/golden/correlated_parent.npz"""
import functools
import os
import sys

import numpy as np

W, W70 = 7, 3  # walkers: no multiple of anything, more than one block; three where a case has 70 sets
ARGS = {"wf1det_coeff": "det_coeff", "wf2acoeff": "acoeff", "wf2bcoeff": "bcoeff", "wf3ccoeff": "ccoeff"}


def _perturbed(wf, seed=11):
    """All-electron Jastrow factors: the cusp function comes first and keeps its coefficients, the others are drawn."""
    rng = np.random.default_rng(seed)
    a, b = np.array(wf.parameters["wf2acoeff"]), np.array(wf.parameters["wf2bcoeff"])
    a[:, 1:] += 0.05 * rng.standard_normal(a[:, 1:].shape)
    b[1:] += 0.05 * rng.standard_normal(b[1:].shape)
    wf.parameters["wf2acoeff"], wf.parameters["wf2bcoeff"] = a, b
    return wf


@functools.lru_cache(maxsize=None)
def system(name, ndet=1, three_body=False):
    """(system, wave function) of a case: water (ECP, 4 + 4 electrons), water53 (5 + 3), general (all-electron water, no ECP) and
    diamond (the 8-atom cell at Gamma, 16 + 16 electrons; ndet > 1: three determinants with one virtual orbital per k-point)."""
    import pyqmc_amd as pa
    from pyqmc_amd import pbc, systems
    from tests import helpers

    build = helpers.gpu_wf3 if three_body else helpers.gpu_wf
    if name == "diamond":
        cell = pbc.get_supercell(systems.diamond_primitive(), np.array([[-1.0, 1, 1], [1, -1, 1], [1, 1, -1]]))
        if ndet == 1:
            return cell, build(cell, pbc.random_kmf(cell))
        base = [5 * k + i for k in range(4) for i in range(4)]  # flat indices into the per-k blocks of 4 + 1 orbitals
        ex1, ex2 = sorted(set(base) - {3} | {4}), sorted(set(base) - {18} | {19})
        dets = [(1.0, [base, base]), (0.3, [ex2, base]), (-0.2, [ex1, ex2])]
        return cell, build(cell, pbc.random_kmf(cell, nvirt=1), dets)
    if name == "general":
        mol = systems.water_general()
        mf = systems.random_mf(mol, nvirt=6)
        wf = _perturbed(pa.generate_wf(mol, mf, determinants=None if ndet == 1 else systems.random_determinants(mol, mf, ndet), jastrow3=three_body))
        if three_body:
            wf.parameters["wf3ccoeff"] = helpers.ccoeff_params(mol)
        return mol, wf
    mol = systems.water()
    if name == "water53":
        mol = systems.Mol([mol.atom_symbol(i) for i in range(mol.natm)], mol.atom_coords(), nelec=(5, 3))
    mf = systems.random_mf(mol, nvirt=6)
    return mol, build(mol, mf, None if ndet == 1 else systems.random_determinants(mol, mf, ndet))


def walkers(mol, nw, seed):
    from pyqmc_amd import systems
    from pyqmc_amd.configs import OpenConfigs, PeriodicConfigs

    x = systems.initial_guess(mol, nw, rng=np.random.default_rng(seed)).configs.copy()
    return PeriodicConfigs(x, mol.lattice_vectors()) if hasattr(mol, "a") else OpenConfigs(x)


def sets(wf, K, seed, keys):
    """{argument: (K, ...)}: the handle's coefficients plus 0.05 N(0, 1) per set, for the parameters ``keys``."""
    rng = np.random.default_rng(seed)
    out = {}
    for key in keys:
        c0 = np.asarray(wf.parameters[key])
        out[ARGS[key]] = np.stack([c0 + 0.05 * rng.standard_normal(c0.shape) for _ in range(K)])
    return out


J2, MD, J3 = tuple(ARGS)[1:3], tuple(ARGS)[:3], tuple(ARGS)
# name -> (entry, system arguments, walkers, K, the parameters given, further keywords); seeds fixed by the position in the table
CASES = {
    "correlated__water_k5": ("correlated", ("water",), W, 5, J2, {}),
    "correlated__water_k70": ("correlated", ("water",), W70, 70, J2, {}),  # two groups of set columns
    "correlated__general_k3": ("correlated", ("general",), W, 3, J2, {}),  # no ECP
    "correlated__water53_k4": ("correlated", ("water53",), W, 4, J2, {}),
    "correlated__diamond_k3": ("correlated", ("diamond",), W, 3, J2, {}),  # the periodic instantiation
    "variance__water_k5": ("variance", ("water",), W, 5, J2, dict(grad=False, ke=True)),
    "variance__water_k3_dvar": ("variance", ("water",), W, 3, J2, dict(grad=True, ke=True)),
    "md__water4_k5": ("correlated_md", ("water", 4), W, 5, MD, {}),
    "md__water13_k17": ("correlated_md", ("water", 13), W, 17, MD, {}),  # per-spin maps differ; two 16-column tiles, a k-step tail
    "md__water4_k70": ("correlated_md", ("water", 4), W70, 70, MD, {}),
    "md__water4_det_only": ("correlated_md", ("water", 4), W, 5, MD[:1], {}),
    "md__water4_jastrow_only": ("correlated_md", ("water", 4), W, 5, MD[1:], {}),
    "md__water4_k5_chunk3": ("correlated_md", ("water", 4), W, 5, MD, dict(walker_chunk=3)),  # chunks of 3, 3, 1
    "md__diamond_k3": ("correlated_md", ("diamond", 3), W, 3, MD, {}),
    "j3__water1_k5": ("correlated_j3", ("water", 1, True), W, 5, J3, {}),
    "j3__water4_k64": ("correlated_j3", ("water", 4, True), W, 64, J3, {}),  # the handle's own column alone forms the second group
    "j3__water1_k70": ("correlated_j3", ("water", 1, True), W70, 70, J3, {}),
    "j3__water4_ccoeff_only": ("correlated_j3", ("water", 4, True), W, 5, J3[3:], {}),
    "j3__water53_6det_k4": ("correlated_j3", ("water53", 6, True), W, 4, J3, {}),
    "j3__general_k3": ("correlated_j3", ("general", 1, True), W, 3, J3, {}),
    "j3__diamond_k3": ("correlated_j3", ("diamond", 1, True), W, 3, J3, {}),
    "j3__water4_k5_chunk3": ("correlated_j3", ("water", 4, True), W, 5, J3, dict(walker_chunk=3)),
}


def replay(name):
    """The call of one case -> {"<name>__<output>": array}."""
    entry, sysargs, nw, K, keys, kw = CASES[name]
    seed = 100 + list(CASES).index(name)
    mol, wf = system(*sysargs)
    wf.recompute(walkers(mol, nw, seed))
    dev = wf.fused_device()
    given = sets(wf, K, seed + 1, keys)
    if entry == "variance":
        eoff = -17.0 + np.random.default_rng(seed + 2).standard_normal(nw)
        var, dvar, ke = dev.variance(given["acoeff"], given["bcoeff"], eoff, **kw)
        out = {"var": var, "ke": ke, **({"dvar": dvar} if kw["grad"] else {})}
    else:
        logpsi, en = getattr(dev, entry)(**given, threshold=10.0, rot=None, unif=None, seed=seed + 3, **kw)
        out = {"logpsi": logpsi, "en": en}
    return {f"{name}__{k}": np.array(v) for k, v in out.items()}


def record():
    arrays = {}
    for name in CASES:
        arrays.update(replay(name))
    return arrays


if __name__ == "__main__":
    def option(name, default):
        return sys.argv[sys.argv.index(name) + 1] if name in sys.argv else default

    root = os.path.abspath(option("--tree", os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))  # the tree whose package is used
    sys.path.insert(0, root)
    path = option("--out", os.path.join(root, "tests", "golden", "correlated_parent.npz"))
    arrays = record()
    bad = [k for k, v in arrays.items() if not np.all(np.isfinite(v))]
    assert not bad, f"not finite: {bad}"
    np.savez_compressed(path, **arrays)
    print(f"wrote {path}: {len(arrays)} arrays, {os.path.getsize(path)} bytes")
