"""Fixture multi_parent: every output of the six multi-handle entries (pqa_overlap_sweeps; pqa_add_weights, pqa_add_sweeps,
pqa_add_energy; pqa_mix_moments, pqa_mix_wtdp) on small cases that reach every line of their host code and kernels, and after the two
sweep entries every handle's walkers and value (tests/test_gpu_multi_parent.py replays the same calls and compares bit for bit).
Record it on the GPU from a tree of the commit BEFORE the family got its one call prologue and one sweep driver, with that tree's
library and Python; only public functions are used, so the file runs unchanged in both:

    python tools/make_multi_golden.py --tree <parent tree> --out tests/golden/multi_parent.npz"""
import copy
import os
import sys

import numpy as np

TSTEP = 0.4
_cache = {}


def states(name, K):
    """(system, K wave functions on handles of their own) of a case: water1 / water4 (ECP, 4 + 4 electrons, 1 / 4 determinants), water53
    (5 + 3 electrons) and general (all-electron water, no ECP).  The states differ in det_coeff (4 determinants) or in the Jastrow b
    coefficients below the cusp row (1 determinant).  Built once per system, state after state from one generator."""
    import pyqmc_amd as pa
    from pyqmc_amd import systems
    from tests import helpers

    if name not in _cache:
        if name == "general":
            mol = systems.water_general()
            base = pa.generate_wf(mol, systems.random_mf(mol, nvirt=6))
        else:
            mol = systems.water()
            if name == "water53":
                mol = systems.Mol([mol.atom_symbol(i) for i in range(mol.natm)], mol.atom_coords(), nelec=(5, 3))
            mf = systems.random_mf(mol, nvirt=6)
            base = helpers.gpu_wf(mol, mf, systems.random_determinants(mol, mf, 4) if name == "water4" else None)
        _cache[name] = (mol, base, np.random.default_rng(7), [])
    mol, base, rng, wfs = _cache[name]
    while len(wfs) < K:
        w = copy.deepcopy(base)
        key = "wf1det_coeff" if name == "water4" else "wf2bcoeff"
        c = np.asarray(w.parameters[key]).copy()
        if name == "water4":
            c += 0.3 * rng.standard_normal(c.shape)
        else:
            c[1:] += 0.05 * rng.standard_normal(c[1:].shape)
        w.parameters[key] = c
        wfs.append(w)
    return mol, wfs[:K]


def columns(name, k):
    """(src, pos) of state k: det_coeff but its first entry (4 determinants), the Jastrow b coefficients below the cusp row, and for
    even k all of the a coefficients (so the states' column counts differ)."""
    src, pos = ([0] * 3, [1, 2, 3]) if name == "water4" else ([], [])
    src, pos = src + [2] * 9, pos + list(range(3, 12))
    if k % 2 == 0:
        src, pos = src + [1] * 24, pos + list(range(24))
    return src, pos


COEFFS = [0.6, -0.5, 0.4, 0.3, -0.2, 0.25, 0.35, -0.45]  # mixed sign
# name -> (entry, system, walkers, K, keywords).  Walkers: 7 (less than one 256-thread block) and 300 (two blocks with a tail; four
# slices of 80 walkers in the estimators' products, so walker_chunk=80 gives four chunks).  Seeds are fixed by the position in the table.
CASES = {
    "ovl__water1_w7_k1": ("overlap_sweeps", "water1", 7, 1, dict(nsteps=1, weights=True)),
    "ovl__water4_w7_k2_n3": ("overlap_sweeps", "water4", 7, 2, dict(nsteps=3, weights=True)),
    "ovl__water4_w300_k3_n3": ("overlap_sweeps", "water4", 300, 3, dict(nsteps=3, weights=True)),
    "ovl__water1_w300_k2_noweights": ("overlap_sweeps", "water1", 300, 2, dict(nsteps=1, weights=False)),
    "ovl__water1_w7_k8": ("overlap_sweeps", "water1", 7, 8, dict(nsteps=1, weights=True)),
    "ovl__water4_w7_k2_n0": ("overlap_sweeps", "water4", 7, 2, dict(nsteps=0, weights=False)),
    "ovl__water53_w7_k3": ("overlap_sweeps", "water53", 7, 3, dict(nsteps=1, weights=True)),
    "ovl__general_w7_k2": ("overlap_sweeps", "general", 7, 2, dict(nsteps=1, weights=True)),  # no ECP
    "ovl__water4_w7_k2_never": ("overlap_sweeps", "water4", 7, 2, dict(nsteps=1, weights=True, never=True)),
    "ovl__water1_w7_k2_vanished": ("overlap_sweeps", "water1", 7, 2, dict(nsteps=1, weights=True, vanished=True)),
    "addsw__water1_w7_k1": ("add_sweeps", "water1", 7, 1, dict(nsteps=1)),
    "addsw__water4_w7_k2_n3": ("add_sweeps", "water4", 7, 2, dict(nsteps=3)),
    "addsw__water4_w300_k3_n3": ("add_sweeps", "water4", 300, 3, dict(nsteps=3)),
    "addsw__water4_w7_k2_n0": ("add_sweeps", "water4", 7, 2, dict(nsteps=0)),
    "addsw__water53_w7_k3": ("add_sweeps", "water53", 7, 3, dict(nsteps=1)),
    "addsw__water4_w7_k2_never": ("add_sweeps", "water4", 7, 2, dict(nsteps=1, never=True)),
    "addsw__water1_w7_k2_vanished": ("add_sweeps", "water1", 7, 2, dict(nsteps=1, vanished=True)),
    "addw__water4_w7_k1": ("add_weights", "water4", 7, 1, {}),
    "addw__water4_w300_k2": ("add_weights", "water4", 300, 2, {}),
    "addw__water4_w7_k3": ("add_weights", "water4", 7, 3, {}),
    "addw__water1_w7_k8": ("add_weights", "water1", 7, 8, {}),
    "addw__water4_w7_k2_nosign": ("add_weights", "water4", 7, 2, dict(sign=False)),
    "addw__water4_w7_k2_nolog": ("add_weights", "water4", 7, 2, dict(logabs=False)),
    "addw__water4_w7_k2_now": ("add_weights", "water4", 7, 2, dict(w=False)),
    "adden__water4_w7_k1_seed": ("add_energy", "water4", 7, 1, dict(seed=5)),
    "adden__water4_w300_k2_tapes": ("add_energy", "water4", 300, 2, dict(tapes=True)),
    "adden__water1_w7_k3_seed": ("add_energy", "water1", 7, 3, dict(seed=6)),
    "adden__water4_w7_k3_tapes": ("add_energy", "water4", 7, 3, dict(tapes=True)),
    "mixm__water4_w7_k1": ("mix_moments", "water4", 7, 1, dict(per_walker=True)),
    "mixm__water4_w300_k2_chunk80": ("mix_moments", "water4", 300, 2, dict(per_walker=True, walker_chunk=80)),
    "mixm__water4_w7_k3_p0_tapes": ("mix_moments", "water4", 7, 3, dict(per_walker=False, tapes=True, empty=(1,))),
    "mixm__water1_w300_k3_p0": ("mix_moments", "water1", 300, 3, dict(per_walker=False, empty=(0,))),
    "mixm__water4_w300_k2_tapes_chunk80": ("mix_moments", "water4", 300, 2, dict(per_walker=True, tapes=True, walker_chunk=80)),
    "mixw__water4_w7_k1": ("mix_wtdp", "water4", 7, 1, {}),
    "mixw__water1_w7_k2": ("mix_wtdp", "water1", 7, 2, {}),
    "mixw__water4_w300_k3_chunk80": ("mix_wtdp", "water4", 300, 3, dict(walker_chunk=80)),
}
NAN_CASES = tuple(n for n in CASES if CASES[n][4].get("vanished"))  # compared with NaNs counting as equal; need not be finite


def replay(name):
    """The call of one case -> {"<name>__<output>": array}."""
    from pyqmc_amd import addwf, sample_many, systems
    from pyqmc_amd.configs import OpenConfigs

    entry, sysname, W, K, kw = CASES[name]
    seed = 200 + 3 * list(CASES).index(name)
    mol, wfs = states(sysname, K)
    x = systems.initial_guess(mol, W, rng=np.random.default_rng(seed)).configs.copy()
    if kw.get("vanished"):
        x[0, 1] = x[0, 0]  # two up electrons of walker 0 at one point: its spin-up determinants vanish
    with np.errstate(all="ignore"):
        for w in wfs:
            w.recompute(OpenConfigs(x.copy()))
    devs = [w.fused_device() for w in wfs]
    N, necp = x.shape[1], sum(1 for a in mol._atom if a[0] in mol._ecp)
    rng = np.random.default_rng(seed + 1)
    coeffs = COEFFS[:K]
    if entry in ("overlap_sweeps", "add_sweeps"):
        n = kw["nsteps"]
        gauss = np.sqrt(TSTEP) * rng.standard_normal((n * N, W, 3))
        unif = np.full((n * N, W), np.inf) if kw.get("never") else rng.random((n * N, W))
        if entry == "overlap_sweeps":
            ovl, wts, acc = sample_many.overlap_sweeps(devs, TSTEP, gauss, unif, weights=kw["weights"])
            out = {"overlap": ovl, "acc": acc, **({"weights": wts} if kw["weights"] else {})}
        else:
            out = {"acc": addwf.add_sweeps(devs, coeffs, TSTEP, gauss, unif)}
        for k, d in enumerate(devs):
            out[f"configs{k}"] = d.configs()
            out[f"sign{k}"], out[f"log{k}"] = wfs[k].value()
        return {f"{name}__{k}": np.array(v) for k, v in out.items()}
    if entry == "add_weights":
        res = addwf.add_weights(devs, coeffs, **kw)
        out = {k: v for k, v in zip(("sign", "logabs", "w"), res) if v is not None}
    elif entry == "add_energy":
        rot = np.linalg.qr(rng.standard_normal((N, necp, 3, 3)))[0] if kw.get("tapes") else None
        unif = rng.random((N, necp, W)) if kw.get("tapes") else None
        out = {"en": addwf.add_energy(devs, coeffs, 10.0, rot=rot, unif=unif, seed=kw.get("seed", 0))}
    elif entry == "mix_moments":
        none = (np.zeros(0, dtype=np.int32), np.zeros(0, dtype=np.int32))
        cols = [none if k in kw.get("empty", ()) else columns(sysname, k) for k in range(K)]
        draws = dict(seeds=[seed + 10 + k for k in range(K)])
        if kw.get("tapes"):
            draws = dict(rot=np.linalg.qr(rng.standard_normal((K, N, necp, 3, 3)))[0], unif=rng.random((K, N, necp, W)))
        res = sample_many.mix_moments(devs, cols, offset=-16.5, walker_chunk=kw.get("walker_chunk", 0), per_walker=kw["per_walker"], **draws)
        out = {"overlap": res[0], "en": res[1], **{f"moments{k}": m for k, m in enumerate(res[2]) if m is not None}}
        if kw["per_walker"]:
            out["u"], out["en_walker"] = res[3], res[4]
    else:
        out = dict(zip(("overlap", "wtdp"), sample_many.mix_wtdp(devs, *columns(sysname, K - 1), walker_chunk=kw.get("walker_chunk", 0))))
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
    path = option("--out", os.path.join(root, "tests", "golden", "multi_parent.npz"))
    arrays = record()
    bad = [k for k, v in arrays.items() if not k.startswith(NAN_CASES) and not np.all(np.isfinite(v))]
    assert not bad, f"not finite: {bad}"
    np.savez_compressed(path, **arrays)
    print(f"wrote {path}: {len(arrays)} arrays, {os.path.getsize(path)} bytes")
