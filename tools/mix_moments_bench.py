"""Mixture estimators: sample_overlap with each multi-state accumulator on its device route (pqa_mix_moments / pqa_mix_wtdp,
avg_resident in the fused worker) against its protocol route (walkers fetched, energy.avg on the host every sweep), and one
optimize_ensemble sub-iteration with and without mixture_route="device".

    python tools/mix_moments_bench.py [--walkers 4096 16384] [--K 2 3] [--reps 5] [--no-ensemble] [--out FILE] [--step-timeout S]

(H2O)8, 3 determinants per state, 1 block x 3 sweeps, tstep 0.5, the mixture walk on the fused route either way.  Every grid point and
the sub-iteration run as a child process of their own under `timeout`; the first one that fails ends the run.  In a child the two
accumulator routes are timed alternately from the same walkers and seed, warm (one untimed call of each first), wall clock with a
device synchronisation at the end of every timed region; the sampling without an accumulator is timed the same way, so that the share
of a sampling the accumulator takes, 1 - t(no accumulator) / t, can be given for both routes.  Before a grid point counts, the routes'
walkers (equal bits) and weighted blocks (1e-9) are checked against each other.  One JSON line per measurement: the median over the
repeats and their least and greatest value.
"""

import argparse
import copy
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

ACCUMULATORS = ("multi", "wtdp", "energy")


def states(mol, K):
    from pyqmc_amd import systems
    from tests import helpers

    mf = systems.random_mf(mol, nvirt=4)
    dets = systems.random_determinants(mol, mf, 3)
    base = helpers.gpu_wf(mol, mf, determinants=dets)
    rng = np.random.default_rng(60)
    wfs = []
    for _ in range(K):
        w = copy.deepcopy(base)
        w.parameters["wf1det_coeff"] = np.asarray(w.parameters["wf1det_coeff"]) + 0.3 * rng.standard_normal(3)
        wfs.append(w)
    return wfs


def accumulator(name, mol, wfs, route):
    from pyqmc_amd import ensemble
    from pyqmc_amd import wf as pwf
    from pyqmc_amd.accumulators import LinearTransform, StochasticReconfigurationMultipleWF
    from pyqmc_amd.accumulators_multiwf import EnergyAccumulatorMultipleWF
    from pyqmc_amd.energy import EnergyAccumulator

    tr = [LinearTransform(w.parameters, pwf.default_to_opt(w)) for w in wfs]
    if name == "multi":
        return StochasticReconfigurationMultipleWF(EnergyAccumulator(mol, seed=7), tr, route=route), tr[0].nparams
    if name == "wtdp":
        return ensemble.StochasticReconfigurationWfbyWf(EnergyAccumulator(mol, seed=7), tr[-1], mixture_route=route), tr[-1].nparams
    return EnergyAccumulatorMultipleWF(EnergyAccumulator(mol, seed=7), offset=-130.0, route=route), 0


def timed(wfs, x, acc, seed):
    from pyqmc_amd import sample_many
    from pyqmc_amd.configs import OpenConfigs

    np.random.seed(seed)
    if acc is not None:
        acc.enacc._calls = 0  # (the same energy keys on every call)
    cfg = OpenConfigs(x.copy())
    t0 = time.perf_counter()
    w, u, cfg = sample_many.sample_overlap(wfs, cfg, acc, nsteps=3, nblocks=1, route="fused")
    wfs[0].fused_device().sync()
    return time.perf_counter() - t0, w, cfg.configs


def spread(ts):
    return {"median_s": float(np.median(ts)), "min_s": float(np.min(ts)), "max_s": float(np.max(ts))}


def step_grid(out, W, K, reps):
    from pyqmc_amd import systems
    from tests import helpers

    mol = systems.water_cluster()
    sets = {r: states(mol, K) for r in ("device", "protocol", "none")}
    x = systems.initial_guess(mol, W, rng=np.random.default_rng(61)).configs.copy()
    timed(sets["none"], x, None, 1)
    for name in ACCUMULATORS:
        accs, nparams = {}, 0
        for r in ("device", "protocol"):
            accs[r], nparams = accumulator(name, mol, sets[r], r)
            timed(sets[r], x, accs[r], 1)
        ts = {"device": [], "protocol": [], "none": []}
        for rep in range(reps):
            res = {}
            for r in ("device", "protocol"):
                dt, res[r], cfg = timed(sets[r], x, accs[r], 10 + rep)
                assert accs[r].last_route == r
                ts[r].append(dt)
                res[r] = (res[r], cfg)
            ts["none"].append(timed(sets["none"], x, None, 10 + rep)[0])
            assert np.array_equal(res["device"][1], res["protocol"][1]), "the routes' walkers differ"
            for k, v in res["protocol"][0].items():
                assert helpers.relerr(res["device"][0][k], v) < 1e-9, ("the routes' blocks differ", k)
        med = {r: float(np.median(t)) for r, t in ts.items()}
        rec = {"what": "sample_overlap", "accumulator": name, "system": "(H2O)8", "walkers": W, "K": K, "nparams": int(nparams), "blocks": 1,
               "sweeps": 3, "reps": reps, "device": spread(ts["device"]), "protocol": spread(ts["protocol"]), "no_accumulator": spread(ts["none"]),
               "device_over_protocol": med["device"] / med["protocol"], "accumulator_share_protocol": 1.0 - med["none"] / med["protocol"],
               "accumulator_share_device": 1.0 - med["none"] / med["device"], "outputs_match": True}
        out.write(json.dumps(rec) + "\n")
        out.flush()
        print(json.dumps(rec), flush=True)


def step_ensemble(out, W, reps):
    """One sub-iteration of state 1 (K = 2) of optimize_ensemble, the routes alternated; its mixture samplings timed by wrapping the
    module's hook."""
    from pyqmc_amd import ensemble, systems
    from pyqmc_amd.accumulators import LinearTransform
    from pyqmc_amd.configs import OpenConfigs
    from pyqmc_amd.energy import EnergyAccumulator

    mol = systems.water_cluster()
    x0 = systems.initial_guess(mol, W, rng=np.random.default_rng(62)).configs.copy()
    to_opt = {"wf1det_coeff": np.array([False, True, True])}
    kws = dict(nblocks=1, nsteps=3, tstep=0.5)
    so = ensemble._sample_overlap
    runs = {}
    for route in ("device", None):
        wfs = states(mol, 2)
        upd = [[ensemble.StochasticReconfigurationWfbyWf(EnergyAccumulator(mol), LinearTransform(w.parameters, to_opt), mixture_route=route)]
               for w in wfs]
        runs[route] = (wfs, upd, OpenConfigs(x0.copy()))
    ts = {"device": [], "protocol": []}
    mix = {"device": [], "protocol": []}
    try:
        for rep in range(reps + 1):  # (the first pass warms both: one full iteration each)
            for route in ("device", None):
                wfs, upd, x = runs[route]
                spent = [0.0]

                def so_t(*a, **k):
                    t = time.perf_counter()
                    r = so(*a, **k)
                    wfs[0].fused_device().sync()
                    spent[0] += time.perf_counter() - t
                    return r

                ensemble._sample_overlap = so_t
                np.random.seed(5 + rep)
                if rep == 0:
                    ensemble.optimize_ensemble(wfs, x, upd, None, tau=0.1, max_iterations=1, vmc_kwargs=kws)
                    continue
                warm = [0.0]
                vm = ensemble._vmc

                def vm_t(wf, configs, accumulators=None, **k):
                    t = time.perf_counter()
                    r = vm(wf, configs, accumulators=accumulators, **k)
                    if not accumulators:
                        warm[0] += time.perf_counter() - t
                    return r

                ensemble._vmc = vm_t
                try:
                    t0 = time.perf_counter()
                    ensemble.optimize_ensemble(wfs, x, [[], upd[1]], None, tau=0.1, max_iterations=1, vmc_kwargs=kws)
                    wfs[0].fused_device().sync()
                    total = time.perf_counter() - t0 - warm[0]
                finally:
                    ensemble._vmc = vm
                name = route or "protocol"
                assert upd[1][0].last_route == name
                ts[name].append(total)
                mix[name].append(spent[0])
    finally:
        ensemble._sample_overlap = so
    rec = {"what": "optimize_ensemble sub-iteration (state 1 of 2)", "system": "(H2O)8", "walkers": W, "blocks": 1, "sweeps": 3, "reps": reps,
           "device": spread(ts["device"]), "protocol": spread(ts["protocol"]), "mixture_sampling_device": spread(mix["device"]),
           "mixture_sampling_protocol": spread(mix["protocol"]),
           "device_over_protocol": float(np.median(ts["device"]) / np.median(ts["protocol"]))}
    out.write(json.dumps(rec) + "\n")
    out.flush()
    print(json.dumps(rec), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--walkers", type=int, nargs="+", default=[4096, 16384])
    ap.add_argument("--K", type=int, nargs="+", default=[2, 3])
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--no-ensemble", action="store_true")
    ap.add_argument("--out", default="profiles/mix_moments_bench.jsonl")
    ap.add_argument("--step-timeout", type=int, default=240, help="seconds a child step may take")
    ap.add_argument("--step", nargs="+", help="(child) grid W K | ensemble W")
    a = ap.parse_args()
    if a.step:  # a child: one step, appended to the file
        with open(a.out, "a") as out:
            if a.step[0] == "grid":
                step_grid(out, int(a.step[1]), int(a.step[2]), a.reps)
            else:
                step_ensemble(out, int(a.step[1]), a.reps)
        return 0
    os.makedirs(os.path.dirname(a.out) or ".", exist_ok=True)
    open(a.out, "w").close()
    steps = [["grid", str(W), str(K)] for W in a.walkers for K in a.K] + ([] if a.no_ensemble else [["ensemble", "16384"]])
    for s in steps:
        cmd = ["timeout", "-k", "10", str(a.step_timeout), sys.executable, os.path.abspath(__file__), "--out", a.out, "--reps", str(a.reps), "--step"] + s
        rc = subprocess.run(cmd, cwd=ROOT).returncode
        if rc != 0:
            print(f"step {' '.join(s)} ended with status {rc}: stopping", file=sys.stderr, flush=True)
            return rc
    return 0


if __name__ == "__main__":
    sys.exit(main())
