"""DMC mixed estimators: wall clock of one dmc_propagate block on the "resident" and the "host" accumulator route, one JSON line per
configuration.

    python tools/dmc_mixed_bench.py [--configs rdm:4096,rdm:16384,all:4096,all:16384] [--reps 5] [--steps 5] [--norb 32] [--out FILE]

A configuration is SET:WALKERS on (H2O)8 (64 electrons) with SET rdm = {energy, rdm1_up, rdm1_down} or all = rdm + {s2, sq}; the
one-body matrices take ``--norb`` orbitals and ``--nsweeps`` auxiliary sweeps.  Per configuration, in one process: both routes
from equal numpy seeds first — the energy keys and the walkers must agree bit for bit and every other key within 1e-9 (relative to
the key's largest entry) before anything is timed — then one warm-up block per route and ``--reps`` timed blocks per route,
alternating resident, host, resident, ...  Every timed block starts from the same walkers, weights and seed.  Reported: median,
minimum and maximum wall time per route (perf_counter around the call, which returns after its last device-to-host copy), the
ratio of the medians, and the worst disagreement.  The library must be built (python __graft_entry__.py)."""

import argparse
import copy
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def relerr(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return float(np.max(np.abs(a - b)) / max(np.max(np.abs(b)), 1e-300))


def run(cfg, reps, steps, norb, nsweeps):
    import pyqmc_amd as pa
    from pyqmc_amd import systems
    from tests import helpers

    which, W = cfg.split(":")
    W = int(W)
    mol = systems.water_cluster()
    mf = systems.random_mf(mol, nvirt=max(0, norb - mol.nelec[0]))
    wf = helpers.gpu_wf(mol, mf)
    C = np.asarray(mf.mo_coeff)[0]
    basis = C[:, :norb] if C.shape[1] >= norb else 0.4 * np.random.default_rng(2).standard_normal((C.shape[0], norb))
    start = pa.initial_guess(mol, W, rng=np.random.default_rng(1))
    # a short equilibration, so that the block is timed on walkers distributed as |Psi|^2
    _, start = pa.vmc_worker(wf, start, 0.3, 5, {}, seed=3)
    w0 = np.exp(0.1 * np.random.default_rng(4).standard_normal(W))

    def accumulators():
        d = {"energy": pa.EnergyAccumulator(mol)}
        for name, spin in (("rdm1_up", 0), ("rdm1_down", 1)):
            d[name] = pa.OBDMAccumulator(mol, basis, nsweeps=nsweeps, warmup=20, spin=spin)
        if which == "all":
            d["s2"] = pa.S2Accumulator(mol.nelec)
            d["sq"] = pa.SqAccumulator(mol, qlist=np.random.default_rng(2).uniform(-2.0, 2.0, (64, 3)))
        return d

    accs = {r: accumulators() for r in ("resident", "host")}
    wf.recompute(start)
    en = float(np.mean(np.real(pa.EnergyAccumulator(mol)(start, wf)["total"])))

    def block(route, seed):
        np.random.seed(seed)
        t0 = time.perf_counter()
        blk, cfg_, wts = pa.dmc_propagate(wf, copy.deepcopy(start), w0.copy(), 0.02, 10.0, en, en, nsteps=steps, accumulators=accs[route],
                                          accumulator_route=route)
        return time.perf_counter() - t0, blk, cfg_, wts

    out = {"config": cfg, "system": "H2O8", "walkers": W, "set": which, "norb": norb, "nsweeps": nsweeps, "steps": steps, "reps": reps,
           "route_none": pa.dmc_accumulator_route(wf, accs["resident"])[0]}
    # agreement from equal seeds, before anything is timed (these two blocks are also each route's first warm-up: the auxiliary walks
    # start here)
    (_, br, cr, wr), (_, bh, ch, wh) = block("resident", 100), block("host", 100)
    worst = 0.0
    for k in br:
        if k.startswith("energy") or k in ("weight", "acceptance", "tmove_acceptance"):
            assert np.array_equal(br[k], bh[k]), k
        else:
            worst = max(worst, relerr(br[k], bh[k]))
    assert np.array_equal(cr.configs, ch.configs) and np.array_equal(wr, wh)
    assert worst < 1e-9, worst
    out["worst_relerr"] = worst
    for r in ("resident", "host"):
        block(r, 101)
    t = {"resident": [], "host": []}
    for i in range(reps):
        for r in ("resident", "host"):
            t[r].append(block(r, 200 + i)[0])
    for r in t:
        out[r + "_s"] = {"median": float(np.median(t[r])), "min": float(np.min(t[r])), "max": float(np.max(t[r]))}
    out["host_over_resident"] = out["host_s"]["median"] / out["resident_s"]["median"]
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--configs", default="rdm:4096,rdm:16384,all:4096,all:16384")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--norb", type=int, default=32)
    ap.add_argument("--nsweeps", type=int, default=2)
    ap.add_argument("--out", default=None, help="also append the JSON lines to this file")
    a = ap.parse_args()
    for cfg in a.configs.split(","):
        line = json.dumps(run(cfg, max(a.reps, 5), a.steps, a.norb, a.nsweeps))
        print(line, flush=True)
        if a.out:
            with open(a.out, "a") as f:
                f.write(line + "\n")


if __name__ == "__main__":
    main()
