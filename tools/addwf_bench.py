"""Superposition wave functions: vmc_worker over an AddWF on the fused route (pqa_add_sweeps) against the protocol route, and the
energy call (pqa_add_energy) on its own.

    python tools/addwf_bench.py [--walkers 4096 16384] [--K 2 3] [--reps 2] [--out FILE]

(H2O)8 with 3 determinants per component, 1 block x 3 sweeps, tstep 0.3, no accumulator in the timed sweeps.  The two routes are timed
alternately in one process from the same walkers and seed, warm (one untimed call of each first), wall clock with a device
synchronisation at the end of every timed region.  Before a size counts, the routes' walkers and values are checked against each other
(1e-9).  The energy call is EnergyAccumulator(mol)(configs, wf) on the final walkers, warm, beside the K single-handle energy calls it
contains.  One JSON line per measurement.
"""

import argparse
import copy
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import pyqmc_amd as pa  # noqa: E402
from pyqmc_amd import systems  # noqa: E402
from pyqmc_amd.configs import OpenConfigs  # noqa: E402
from tests import helpers  # noqa: E402

TSTEP, SWEEPS = 0.3, 3


def components(mol, K):
    mf = systems.random_mf(mol, nvirt=4)
    dets = systems.random_determinants(mol, mf, 3)
    base = helpers.gpu_wf(mol, mf, determinants=dets)
    rng = np.random.default_rng(60)
    wfs = []
    for _ in range(K):
        w = copy.deepcopy(base)
        w.parameters["wf1det_coeff"] = np.asarray(w.parameters["wf1det_coeff"]) + 0.2 * rng.standard_normal(3)
        wfs.append(w)
    return wfs, [0.6, 0.5, 0.4][:K]


def timed(wf, x, route, seed):
    np.random.seed(seed)
    cfg = OpenConfigs(x.copy())
    dev = wf.wf_components[0].fused_device()
    dev.sync()
    t0 = time.perf_counter()
    if route == "fused":
        _, cfg = pa.vmc_worker(wf, cfg, TSTEP, SWEEPS, {})
    else:
        _, cfg = helpers.protocol_vmc_worker(wf, cfg, TSTEP, SWEEPS, {})
    dev.sync()
    dt = time.perf_counter() - t0
    assert wf.last_route == route
    return dt, cfg.configs, wf.value()[1]


def bench(out, W, K, reps):
    mol = systems.water_cluster()
    comps, coeffs = components(mol, K)
    wf_f = pa.AddWF(coeffs, comps, route="fused")
    wf_p = pa.AddWF(coeffs, [copy.deepcopy(c) for c in comps], route="protocol")
    x = systems.initial_guess(mol, W, rng=np.random.default_rng(61)).configs.copy()
    timed(wf_f, x, "fused", 1)
    timed(wf_p, x, "protocol", 1)
    tf, tp = [], []
    for r in range(reps):
        dt, cf, lf = timed(wf_f, x, "fused", 10 + r)
        tf.append(dt)
        dt, cp, lp = timed(wf_p, x, "protocol", 10 + r)
        tp.append(dt)
        assert np.abs(cf - cp).max() < 1e-9 and np.abs(lf - lp).max() < 1e-9 * max(1.0, np.abs(lp).max()), "routes disagree"
    rec = {"what": "vmc_worker(AddWF)", "system": "(H2O)8", "determinants": 3, "walkers": W, "K": K, "blocks": 1, "sweeps": SWEEPS,
           "fused_s": float(np.median(tf)), "protocol_s": float(np.median(tp)), "ratio": float(np.median(tp) / np.median(tf)),
           "outputs_match": True}
    out.write(json.dumps(rec) + "\n")
    print(json.dumps(rec), flush=True)
    # the energy call on the final walkers
    cfg = OpenConfigs(cf.copy())
    acc = pa.EnergyAccumulator(mol, seed=3)
    dev = comps[0].fused_device()
    acc(cfg, wf_f)
    te, ts = [], []
    for r in range(reps):
        dev.sync()
        t0 = time.perf_counter()
        acc(cfg, wf_f)
        dev.sync()
        te.append(time.perf_counter() - t0)
        t0 = time.perf_counter()
        for c in comps:
            acc(cfg, c)
        dev.sync()
        ts.append(time.perf_counter() - t0)
    rec = {"what": "EnergyAccumulator(AddWF)", "system": "(H2O)8", "determinants": 3, "walkers": W, "K": K,
           "add_energy_s": float(np.median(te)), "K_single_energy_calls_s": float(np.median(ts))}
    out.write(json.dumps(rec) + "\n")
    out.flush()
    print(json.dumps(rec), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--walkers", type=int, nargs="+", default=[4096, 16384])
    ap.add_argument("--K", type=int, nargs="+", default=[2, 3])
    ap.add_argument("--reps", type=int, default=2)
    ap.add_argument("--out", default="profiles/addwf_bench.jsonl")
    a = ap.parse_args()
    os.makedirs(os.path.dirname(a.out) or ".", exist_ok=True)
    with open(a.out, "w") as out:
        for W in a.walkers:
            for K in a.K:
                bench(out, W, K, a.reps)


if __name__ == "__main__":
    main()
