"""DMC with the batched ECP integrator (EnergyAccumulator(use_old_ecp=False)): wall clock of one dmc_propagate block three ways, one
JSON line per configuration.

    python tools/dmc_batched_bench.py [--configs c5:4096,h2o8:4096] [--reps 5] [--protocol-reps 2] [--steps 5] [--out FILE]

A configuration is SYSTEM:WALKERS with SYSTEM c5 (BASELINE config C5: diamond 2x2x2 supercell, 64 electrons, Ewald) or h2o8 ((H2O)8, 64
electrons, open boundaries); tstep 0.02.  The three ways, all from the same equilibrated walkers and unit weights:

  fused_batched    pyqmc_amd.dmc_propagate with use_old_ecp=False: the whole step loop in one pqa_dmc_steps call, T-move candidates from
                   k_ecpb_fill + k_tmb_count / k_tmb_compact;
  protocol_batched the same accumulator under the reference's control flow over the protocol objects (tests/dmc_batched_ref.py form (b):
                   nonlocal_tmoves, updateinternals, gradient_value per electron, one host round trip each) — what a user of that
                   accumulator had to run before the fused route took it;
  fused_semilocal  pyqmc_amd.dmc_propagate with use_old_ecp=True, as context: another estimator of the same integral, not a competitor.

One warm-up block per way, then ``--reps`` timed blocks of the two fused ways, alternating, and ``--protocol-reps`` of the protocol way
(perf_counter around the call, which returns after its last device-to-host copy).  Also reported: the live T-move candidates of one step
on the start walkers — slots of the batched table whose weight is not exactly 0 (what k_tmb_compact keeps) out of W N nsel, and the
semi-local table's candidates with a non-zero weight — counted through the protocol entry ``nonlocal_tmoves``.  The library must be built
(python __graft_entry__.py)."""

import argparse
import copy
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def system(name):
    import pyqmc_amd as pa
    from pyqmc_amd import pbc, systems

    if name == "c5":
        sup = pbc.get_supercell(systems.diamond_primitive(), 2.0 * np.eye(3))
        return sup, pa.generate_wf(sup, pbc.random_kmf(sup)), {}
    if name == "h2o8":
        from tests import helpers

        mol = systems.water_cluster()
        return mol, helpers.gpu_wf(mol, systems.random_mf(mol)), {}
    raise ValueError(f"system {name!r}: c5 or h2o8")


def live_candidates(acc, cfg, wf, tstep):
    """Candidates with a non-zero weight in the T-move tables of all electrons at the walkers ``cfg`` (the state is left as it was)."""
    n = 0
    for e in range(cfg.configs.shape[1]):
        n += int(np.count_nonzero(acc.nonlocal_tmoves(cfg, wf, e, tstep)["weight"]))
    return n


def run(cfg_name, reps, protocol_reps, steps):
    import pyqmc_amd as pa
    from tests import dmc_batched_ref as ref

    name, W = cfg_name.split(":")
    W = int(W)
    mol, wf, kws = system(name)
    dev = wf.fused_device()
    start = pa.initial_guess(mol, W, rng=np.random.default_rng(1))
    wf.recompute(start)
    dev.vmc_sweeps(0.3, 5, seed=3, energy=False)  # a short equilibration: the blocks are timed on walkers distributed as |Psi|^2
    start.configs[...] = dev.configs()
    if hasattr(start, "wrap"):
        start.wrap += dev.wrap_delta()
    accs = {"batched": pa.EnergyAccumulator(mol, use_old_ecp=False, **kws), "semilocal": pa.EnergyAccumulator(mol, **kws)}
    wf.recompute(start)
    e0 = np.real(accs["semilocal"](start, wf)["total"])
    tstep, args = 0.02, (0.02, 10 * float(e0.std()), float(e0.mean()), float(e0.mean()))
    N = start.configs.shape[1]
    out = {"config": cfg_name, "system": name, "walkers": W, "electrons": N, "steps": steps, "tstep": tstep, "reps": reps,
           "protocol_reps": protocol_reps, "complex": bool(wf.dtype == complex)}
    nsel = accs["batched"].ecp.nselect_deterministic + accs["batched"].ecp.nselect_random
    nsel = min(nsel, int(np.sum(accs["batched"].ecp.naip)))
    out["nsel"] = nsel
    out["dense_slots_per_step"] = W * N * nsel
    out["live_batched_per_step"] = live_candidates(accs["batched"], start, wf, tstep)
    out["live_semilocal_per_step"] = live_candidates(accs["semilocal"], start, wf, tstep)

    def block(way, seed):
        np.random.seed(seed)
        c, w = copy.deepcopy(start), np.ones(W)
        t0 = time.perf_counter()
        if way == "protocol_batched":
            blk, _, _ = ref.protocol_propagate(wf, c, w, *args, steps, accs["batched"])
        else:
            blk, _, _ = pa.dmc_propagate(wf, c, w, *args, nsteps=steps, accumulators={"energy": accs[way.split("_")[1]]})
        return time.perf_counter() - t0, blk

    ways = ("fused_batched", "fused_semilocal", "protocol_batched")
    t = {w_: [] for w_ in ways}
    for w_ in ways:
        _, blk = block(w_, 100)
        out[w_ + "_energy"] = float(np.real(blk["energytotal"]))
        out[w_ + "_tmove_acceptance"] = float(blk["tmove_acceptance"])
    for i in range(reps):
        for w_ in ways[:2]:
            t[w_].append(block(w_, 200 + i)[0])
    for i in range(protocol_reps):
        t[ways[2]].append(block(ways[2], 200 + i)[0])
    for w_ in ways:
        out[w_ + "_s"] = {"median": float(np.median(t[w_])), "min": float(np.min(t[w_])), "max": float(np.max(t[w_]))}
    out["protocol_over_fused_batched"] = out["protocol_batched_s"]["median"] / out["fused_batched_s"]["median"]
    out["fused_batched_over_semilocal"] = out["fused_batched_s"]["median"] / out["fused_semilocal_s"]["median"]
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--configs", default="c5:4096,h2o8:4096")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--protocol-reps", type=int, default=2)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--out", default=None, help="also append the JSON lines to this file")
    a = ap.parse_args()
    for cfg in a.configs.split(","):
        line = json.dumps(run(cfg, max(a.reps, 1), max(a.protocol_reps, 1), a.steps))
        print(line, flush=True)
        if a.out:
            with open(a.out, "a") as f:
                f.write(line + "\n")


if __name__ == "__main__":
    main()
