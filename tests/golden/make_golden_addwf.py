"""Golden vectors of the reference's AddWF (pyqmc/wf/addwf.py) -> g49_addwf.npz.

    python tests/golden/make_golden_addwf.py

Uses make_golden's stubs (numba as an identity decorator, pyscf / h5py mocked), its wave-function builder and its draw recorder, and
the real pyqmc.wf.addwf.AddWF over the reference's Slater x JastrowSpin products.  Inputs and outputs only.  The cases
(tests/addwf_ref.py: CASES, components):
  a  water, K = 2, one determinant per component, different Jastrow coefficients, 70 walkers
  b  water, K = 3, four determinants with different det_coeff, 24 walkers
  c  water, K = 2, one complex entry in coeffs, 8 walkers
Per case (addwf_ref.protocol_entries, the same function the tests run): value; for one electron of each spin, in turn, gradient_value,
gradient, gradient_laplacian, testvalue (plain, under a mask, with 5 auxiliary points without and under the mask), testvalue_many
(plain: the reference's Slater.testvalue_many allocates for all walkers and fails on a real mask, see make_golden), ratio, ratio_current_config (plain and under the mask), a masked updateinternals (always with
saved_values: the reference's default reads a missing attribute) and value(); pgradient and the parameter keys at the end.
Case a also: a 2-sweep vmc_worker trajectory with its recorded draws (unit normals, uniforms, the accept masks, the final walkers and
value, the acceptance), and the reference EnergyAccumulator's six keys on the final walkers with the ECP draws recorded as in g10.
The walkers are 5 vmc_worker sweeps of the sum away from the initial guess; every displaced, auxiliary and testvalue_many point is, per
walker, the first candidate for which the reference's ratios lie inside (0.03, 30).  Before saving, the generator asserts for every walker of every stored state |Psi| / max_k |c_k Psi_k| > 0.05 and every stored ratio
inside (1e-2, 1e2) in magnitude.
"""

import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import make_golden as mg  # noqa: E402  (installs the stubs, puts the reference on the path)

import numpy as np  # noqa: E402
import pyqmc.api as pyq  # noqa: E402
from pyqmc.configurations.coord import OpenConfigs  # noqa: E402
from pyqmc.method.mc import vmc_worker  # noqa: E402
from pyqmc.wf.addwf import AddWF  # noqa: E402

sys.path.insert(0, os.path.join(mg.ROOT, "tests"))
import addwf_ref  # noqa: E402

WARM = 5
LO, HI = 0.03, 30.0  # the window the inputs are chosen for (the assertion below is the wider (1e-2, 1e2))
RATIO_KEYS = ("gv_val", "testvalue", "testvalue_mask", "testvalue_aux", "testvalue_aux_mask", "testvalue_many",
              "ratio", "rcc", "rcc_mask")


def pick(W, draw, ratios, tries=60):
    """Per walker the first of the candidate points draw() whose ratios(points) (W, ...) all lie inside (LO, HI) in magnitude."""
    chosen, ok = draw(), np.zeros(W, dtype=bool)
    for _ in range(tries):
        cand = draw()
        r = np.abs(ratios(cand)).reshape(W, -1)
        good = np.all((r > LO) & (r < HI), axis=1)
        take = good & ~ok
        chosen[take], ok = cand[take], ok | good
        if ok.all():
            return chosen
    raise AssertionError("no candidate point inside the ratio window for some walker")


def check_weights(tag, rcc):
    big = np.max(np.abs(rcc))  # max_k |c_k Psi_k| / |Psi| over the walkers
    assert 1.0 / big > 0.05, (tag, 1.0 / big)
    return 1.0 / big


def dump(name, out, seed):
    c = addwf_ref.CASES[name]
    W = c["W"]
    mol, wfs = addwf_ref.components(name, mg.make_wf)
    wf = AddWF(list(c["coeffs"]), wfs)
    rng = np.random.default_rng(seed)
    configs = mg.walkers(mol, W, seed + 1)
    np.random.seed(seed)
    configs = vmc_worker(wf, configs, addwf_ref.TSTEP, WARM, {})[1]  # walkers of |Psi|^2: few of them next to a node
    p = name + "_"
    out[p + "configs"], out[p + "coeffs"] = configs.configs.copy(), np.asarray(c["coeffs"])
    # inputs: per walker the first candidate point whose stored ratios lie inside (LO, HI); the state advances as in protocol_entries
    start = configs.configs.copy()
    wf.recompute(configs)
    many = np.asarray(c["many"])
    for e in c["electrons"]:
        q = p + f"e{e}_"
        here = configs.configs[:, e, :].copy()
        out[q + "newpos"] = pick(W, lambda: here + 0.15 * rng.standard_normal((W, 3)),
                                 lambda x: wf.testvalue(e, configs.make_irreducible(e, x))[0])
        out[q + "aux"] = pick(W, lambda: here[:, None, :] + 0.2 * rng.standard_normal((W, addwf_ref.NAUX, 3)),
                              lambda x: wf.testvalue(e, configs.make_irreducible(e, x))[0])
        # testvalue_many moves other electrons to its point: another walker's electron e, a typical point of the density
        out[q + "manypos"] = pick(W, lambda: here[rng.permutation(W)] + 0.15 * rng.standard_normal((W, 3)),
                                  lambda x: wf.testvalue_many(many, configs.make_irreducible(e, x)))
        mask = rng.random(W) > 0.35
        mask[0], mask[1] = True, False
        accept = rng.random(W) > 0.4
        accept[-1], accept[0] = True, False
        out[q + "mask"], out[q + "accept"] = mask, accept
        ep = configs.make_irreducible(e, out[q + "newpos"])
        _, _, saved = wf.gradient_value(e, ep)
        configs.move(e, ep, accept)
        wf.updateinternals(e, ep, configs, mask=accept, saved_values=saved)
    configs = OpenConfigs(start)
    addwf_ref.protocol_entries(wf, configs, out, p, out)
    cancel = min(check_weights(name, out[p + f"e{e}_rcc"]) for e in c["electrons"])
    cancel = min(cancel, check_weights(name, out[p + "final_rcc"]))
    allr = np.concatenate([np.abs(np.ravel(out[p + f"e{e}_{k}"])) for e in c["electrons"] for k in RATIO_KEYS])
    assert allr.min() > 1e-2 and allr.max() < 1e2, (name, allr.min(), allr.max())
    print(name, f"|Psi| / max|c_k Psi_k| >= {cancel:.3f}; ratios {allr.min():.3f}..{allr.max():.3f}", file=sys.stderr)
    return mol, wf


def trajectory(mol, wf, out):
    """Case a: vmc_worker over the AddWF, then the reference's energy on the walkers it left."""
    W = addwf_ref.CASES["a"]["W"]
    N = sum(mol.nelec)
    configs = OpenConfigs(out["a_configs"].copy())
    accepts = []
    orig = wf.updateinternals

    def spy(e, epos, cfg, mask=None, saved_values=None):
        accepts.append(np.asarray(mask).copy())
        return orig(e, epos, cfg, mask=mask, saved_values=saved_values)

    wf.updateinternals = spy
    with mg.Tapes(4950) as t:
        blk, configs = vmc_worker(wf, configs, addwf_ref.TSTEP, addwf_ref.NSWEEPS, {})
    wf.updateinternals = orig
    out["a_traj_gauss"] = np.asarray(t.log["normal"]).reshape(addwf_ref.NSWEEPS * N, W, 3)  # unit normals
    out["a_traj_unif"] = np.asarray(t.log["rand"]).reshape(addwf_ref.NSWEEPS * N, W)
    out["a_traj_accepts"] = np.asarray(accepts).reshape(addwf_ref.NSWEEPS, N, W)
    out["a_traj_final"] = configs.configs.copy()
    out["a_traj_acceptance"] = np.asarray(blk["acceptance"])
    out["a_traj_sign"], out["a_traj_log"] = wf.value()
    rcc = wf.ratio_current_config()
    out["a_traj_rcc"] = rcc
    print("a trajectory: acceptance", blk["acceptance"], "cancellation", check_weights("a traj", rcc), file=sys.stderr)
    necp = sum(1 for a in mol._atom if a[0] in mol._ecp)
    with mg.Tapes(4951) as t:
        en = pyq.EnergyAccumulator(mol)(configs, wf)
    out["a_en_rot"] = np.asarray(t.log["rot"]).reshape(N, necp, 3, 3)
    out["a_en_unif"] = np.asarray(t.log["random"]).reshape(N, necp, W)
    for k, v in en.items():
        out["a_en_" + k] = np.asarray(v)
    print("a energy: total", np.mean(out["a_en_total"]), "ecp", np.mean(out["a_en_ecp"]), file=sys.stderr)


def main():
    out = {}
    for k, name in enumerate(addwf_ref.CASES):
        for attempt in range(6):  # the first seed whose walkers and displacements pass the assertions
            seed, trial = 4900 + 1000 * k + 2 * attempt, {}
            try:
                mol, wf = dump(name, trial, seed)
                if name == "a":
                    trajectory(mol, wf, trial)
            except AssertionError as err:
                print(name, seed, err, file=sys.stderr)
                continue
            trial[name + "_seed"] = np.array([seed])
            out.update(trial)
            break
        else:
            raise RuntimeError(f"case {name}: no seed passes the assertions")
    mg.save(addwf_ref.GOLDEN, **out)


if __name__ == "__main__":
    main()
