"""Fixture protocol_parent: every output of the per-electron protocol of each factor (tests/test_gpu_protocol_stage.py replays the
same calls and compares bit for bit).  Record it on the GPU from a tree of the commit BEFORE the protocol entries got their shared
staging path, with that tree's library and Python; only public classes and methods are used, so the file runs unchanged in both:

    python tools/make_protocol_golden.py --tree <parent tree> --out tests/golden/protocol_parent.npz"""
import os
import sys

import numpy as np

W, NAUX, E, ES, E_SAVED = 7, 3, 3, [0, 5], 6  # walkers, auxiliary points per walker, the electrons moved
MIXED = np.array([1, 0, 1, 1, 0, 0, 1], dtype=bool)
MIXED2 = np.array([0, 1, 1, 0, 1, 0, 0], dtype=bool)


def factors():
    """(name, factor, system) of every case: the five factors and their product on water (8 electrons), the complex periodic Slater."""
    import pyqmc_amd as pa
    from tests import helpers

    rng = np.random.default_rng(49)
    mol = pa.systems.water()
    mf = pa.systems.random_mf(mol)
    yield "slater", pa.Slater(mol, mf), mol
    a, b = pa.default_jastrow_basis(mol, False)
    j2 = pa.JastrowSpin(mol, a, b)
    j2.parameters["acoeff"], j2.parameters["bcoeff"] = helpers.jastrow_params(mol, na=len(a), nb=len(b))
    yield "jastrow", j2, mol
    j3 = pa.ThreeBodyJastrow(mol, a, b)
    j3.parameters["ccoeff"] = helpers.ccoeff_params(mol, na=len(a), nb=len(b))
    yield "j3", j3, mol
    gps = pa.GPSJastrow(mol, 1.5 * rng.standard_normal((3, 2, 3)), f=0.4)
    gps.parameters["alpha"] = np.array([0.3, -0.2, 0.15])
    yield "gps", gps, mol
    gem = pa.GeminalJastrow(mol)
    gem.parameters["gcoeff"] = 0.02 * rng.standard_normal(gem.parameters["gcoeff"].shape)
    yield "geminal", gem, mol
    yield "product", helpers.gpu_wf(mol, mf), mol
    sup, kmf = helpers.pbc_complex_case()
    yield "slater_complex", pa.Slater(sup, kmf), sup


def replay(name, wf, mol):
    """The protocol calls of one factor -> {"<name>__<call>": array}."""
    import pyqmc_amd as pa

    rng = np.random.default_rng(len(name))
    configs = pa.initial_guess(mol, W, rng=rng)
    out = {}

    def put(key, *arrays):
        for i, v in enumerate(arrays):
            out[f"{name}__{key}" + (f"_{i}" if len(arrays) > 1 else "")] = np.array(v)

    def proposal(e, shape):
        x = configs.configs[:, e].reshape((W,) + (1,) * (len(shape) - 2) + (3,))
        return configs.make_irreducible(e, x + 0.3 * rng.standard_normal(shape))

    put("recompute", *wf.recompute(configs))
    put("value", *wf.value())
    ep, ea = proposal(E, (W, 3)), proposal(E, (W, NAUX, 3))
    for tag, pos in (("one", ep), ("aux", ea)):
        for mtag, mask in (("all", None), ("mixed", MIXED), ("none", np.zeros(W, dtype=bool))):
            put(f"testvalue_{tag}_{mtag}", wf.testvalue(E, pos, mask=mask)[0])
    if hasattr(wf, "testvalue_many"):
        put("testvalue_many_all", wf.testvalue_many(ES, ep))
        put("testvalue_many_mixed", wf.testvalue_many(ES, ep, mask=MIXED))
    put("gradient", wf.gradient(E, ep))
    put("gradient_value", *wf.gradient_value(E, ep)[:2])
    put("gradient_laplacian", *wf.gradient_laplacian(E, ep))
    configs.move(E, ep, MIXED)
    wf.updateinternals(E, ep, configs, mask=MIXED)
    put("updated_value", *wf.value())
    for k, v in wf.pgradient().items():
        put("pgradient_" + k, v)
    # the saved-values route: gradient_value, then updateinternals with what it returned
    ep = proposal(E_SAVED, (W, 3))
    g, v, saved = wf.gradient_value(E_SAVED, ep)
    put("saved_gradient_value", g, v)
    configs.move(E_SAVED, ep, MIXED2)
    wf.updateinternals(E_SAVED, ep, configs, mask=MIXED2, saved_values=saved)
    put("saved_updated_value", *wf.value())
    return out


def record():
    arrays = {}
    for name, wf, mol in factors():
        arrays.update(replay(name, wf, mol))
    return arrays


if __name__ == "__main__":
    def option(name, default):
        return sys.argv[sys.argv.index(name) + 1] if name in sys.argv else default

    root = os.path.abspath(option("--tree", os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))  # the tree whose package is used
    sys.path.insert(0, root)
    path = option("--out", os.path.join(root, "tests", "golden", "protocol_parent.npz"))
    arrays = record()
    np.savez_compressed(path, **arrays)
    print(f"wrote {path}: {len(arrays)} arrays, {os.path.getsize(path)} bytes")
