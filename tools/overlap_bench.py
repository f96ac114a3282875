"""Mixture sampling: sample_overlap(energy=None) on the fused route (pqa_overlap_sweeps) against the protocol route, and one
optimize_ensemble sub-iteration split into its parts.

    python tools/overlap_bench.py [--walkers 4096 16384] [--K 2 3] [--reps 2] [--fused-only] [--no-ensemble] [--out FILE]

(H2O)8, 1 block x 3 sweeps, tstep 0.5.  The two routes are timed alternately in one process from the same walkers and seed, warm
(one untimed call of each first), wall clock with a device synchronisation at the end of every timed region; the host draw time of
the fused route (the tapes drawn with np.random in the reference's order) is reported on its own.  Before a size counts, the routes'
walkers and overlaps are checked against each other (1e-9).  One JSON line per measurement.
"""

import argparse
import copy
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from pyqmc_amd import ensemble, sample_many, systems  # noqa: E402
from pyqmc_amd.accumulators import LinearTransform  # noqa: E402
from pyqmc_amd.configs import OpenConfigs  # noqa: E402
from pyqmc_amd.energy import EnergyAccumulator  # noqa: E402
from tests import helpers  # noqa: E402


def states(mol, K):
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


def timed(wfs, x, route, seed, draws=None):
    np.random.seed(seed)
    cfg = OpenConfigs(x.copy())
    nr, rr = np.random.normal, np.random.rand
    spent = [0.0]

    def normal(*a, **k):
        t = time.perf_counter()
        r = nr(*a, **k)
        spent[0] += time.perf_counter() - t
        return r

    def rand(*a):
        t = time.perf_counter()
        r = rr(*a)
        spent[0] += time.perf_counter() - t
        return r

    np.random.normal, np.random.rand = normal, rand
    try:
        t0 = time.perf_counter()
        _, u, cfg = sample_many.sample_overlap(wfs, cfg, None, nsteps=3, nblocks=1, route=route)
        wfs[0].fused_device().sync()
        dt = time.perf_counter() - t0
    finally:
        np.random.normal, np.random.rand = nr, rr
    assert sample_many.last_route == route
    return dt, spent[0], u["overlap"], cfg.configs


def bench_routes(out, W, K, reps, fused_only):
    mol = systems.water_cluster()
    wfs_f = states(mol, K)
    wfs_p = [copy.deepcopy(w) for w in wfs_f]
    x = systems.initial_guess(mol, W, rng=np.random.default_rng(61)).configs.copy()
    timed(wfs_f, x, "fused", 1)
    if not fused_only:
        timed(wfs_p, x, "protocol", 1)
    tf, tp, df = [], [], []
    for r in range(reps):
        dt, dr, ovf, cf = timed(wfs_f, x, "fused", 10 + r)
        tf.append(dt)
        df.append(dr)
        if not fused_only:
            dt, _, ovp, cp = timed(wfs_p, x, "protocol", 10 + r)
            tp.append(dt)
            assert np.abs(cf - cp).max() < 1e-9 and helpers.relerr(ovf, ovp) < 1e-9, "routes disagree"
    rec = {"what": "sample_overlap", "system": "(H2O)8", "walkers": W, "K": K, "blocks": 1, "sweeps": 3,
           "fused_s": float(np.median(tf)), "fused_draw_s": float(np.median(df))}
    if tp:
        rec.update({"protocol_s": float(np.median(tp)), "ratio": float(np.median(tp) / np.median(tf)), "outputs_match": True})
    out.write(json.dumps(rec) + "\n")
    out.flush()
    print(json.dumps(rec), flush=True)


def bench_ensemble(out, W):
    """One sub-iteration of state 1 (K = 2), its parts timed by wrapping the module's sampling and VMC hooks."""
    mol = systems.water_cluster()
    wfs = states(mol, 2)
    x = OpenConfigs(systems.initial_guess(mol, W, rng=np.random.default_rng(62)).configs.copy())
    to_opt = {"wf1det_coeff": np.array([False, True, True])}
    upd = [[ensemble.StochasticReconfigurationWfbyWf(EnergyAccumulator(mol), LinearTransform(w.parameters, to_opt))] for w in wfs]
    kws = dict(nblocks=1, nsteps=3, tstep=0.5)
    parts = {"mixture": 0.0, "sr_vmc": 0.0, "warmup_vmc": 0.0}
    so, vm = ensemble._sample_overlap, ensemble._vmc

    def so_t(*a, **k):
        t = time.perf_counter()
        r = so(*a, **k)
        wfs[0].fused_device().sync()
        parts["mixture"] += time.perf_counter() - t
        return r

    def vm_t(wf, configs, accumulators=None, **k):
        t = time.perf_counter()
        r = vm(wf, configs, accumulators=accumulators, **k)
        parts["sr_vmc" if accumulators else "warmup_vmc"] += time.perf_counter() - t
        return r

    ensemble._sample_overlap, ensemble._vmc = so_t, vm_t
    try:
        np.random.seed(5)
        # warm: one full iteration, then time the next one's second sub-iteration (state 1)
        ensemble.optimize_ensemble(wfs, x, upd, None, tau=0.1, max_iterations=1, vmc_kwargs=kws)
        for k in parts:
            parts[k] = 0.0
        upd1 = [[], upd[1]]
        t0 = time.perf_counter()
        ensemble.optimize_ensemble(wfs, x, upd1, None, tau=0.1, max_iterations=1, vmc_kwargs=kws)
        total = time.perf_counter() - t0
    finally:
        ensemble._sample_overlap, ensemble._vmc = so, vm
    total -= parts.pop("warmup_vmc")
    rec = {"what": "optimize_ensemble sub-iteration (state 1 of 2)", "system": "(H2O)8", "walkers": W, "blocks": 1, "sweeps": 3,
           "total_s": total, "mixture_sampling_s": parts["mixture"], "sr_vmc_s": parts["sr_vmc"],
           "rest_s": total - parts["mixture"] - parts["sr_vmc"]}
    out.write(json.dumps(rec) + "\n")
    print(json.dumps(rec), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--walkers", type=int, nargs="+", default=[4096, 16384])
    ap.add_argument("--K", type=int, nargs="+", default=[2, 3])
    ap.add_argument("--reps", type=int, default=2)
    ap.add_argument("--fused-only", action="store_true")
    ap.add_argument("--no-ensemble", action="store_true")
    ap.add_argument("--out", default="profiles/overlap_bench.jsonl")
    a = ap.parse_args()
    os.makedirs(os.path.dirname(a.out) or ".", exist_ok=True)
    with open(a.out, "w") as out:
        for W in a.walkers:
            for K in a.K:
                bench_routes(out, W, K, a.reps, a.fused_only)
        if not a.no_ensemble:
            bench_ensemble(out, 16384)


if __name__ == "__main__":
    main()
