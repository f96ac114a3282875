"""Structure factor (pqa_sq) timing: one JSON line per configuration.

    python tools/sq_bench.py [--configs C5:2:4096,...] [--reps 10] [--no-host]

A configuration is SYSTEM:NQ:WALKERS with SYSTEM C5 (diamond 2x2x2 supercell, 64 electrons; NQ = half-width of the q grid:
recurrence path), PRIM (the primitive cell, 8 electrons) or H2O8 ((H2O)8, 64 electrons, NQ = 0: a 364-vector Cartesian qlist,
direct path).  Per configuration: ms of one mean-mode call and of one per-walker call (HIP events on the handle's stream, warm,
median), the mean-mode call right after a fused sweep (the coordinates read in place from the sweep's planes), the host route at a
walker count it holds (host wall time), and the work from the shapes: (q, electron) terms, fp64 flops, LDS bytes and the
per-walker bytes written, with the bound they imply.  A per-walker call is skipped where its output passes 1 GB (nq = 8 at 65 536
walkers).  The kernel split comes from a rocprofv3 --kernel-trace --stats run of this tool.
"""

import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

F64_VECTOR_FLOPS = 78.6e12  # MI355X fp64 vector peak (FMA = 2)
LDS_BYTES_PER_S = 150e12  # MI355X aggregate ds_read_b128 rate, every CU streaming
HBM_BYTES_PER_S = 8.0e12
DEFAULT = ("C5:2:4096,C5:2:32768,C5:2:65536,C5:4:4096,C5:4:32768,C5:4:65536,C5:8:4096,C5:8:32768,C5:8:65536,"
           "H2O8:0:4096,H2O8:0:65536,PRIM:4:4096,PRIM:4:65536")


def build(system):
    from pyqmc_amd import systems
    from tests import helpers

    if system == "C5":
        return helpers.gpu_pbc_wf("k222")
    if system == "PRIM":
        return helpers.gpu_pbc_wf("gamma")
    if system == "H2O8":
        mol = systems.water_cluster()
        return mol, helpers.gpu_wf(mol, systems.random_mf(mol))
    raise KeyError(system)


def model(N, Q, W, rec):
    """(terms, flops, LDS bytes, output bytes) from the shapes.  Recurrence: two complex products and two additions per term (14
    flops), three 16-byte table reads; direct: a sincos (counted as 40 flops) and two additions, one 24-byte coordinate read."""
    terms = W * N * Q
    return terms, terms * (14 if rec else 42), terms * (48 if rec else 24), W * Q * 2 * 8


def timed(dev, fn, reps, before=None):
    out = []
    for r in range(reps + 2):
        if before is not None:
            before(r)
        dev.sync()
        dev.timer_start()
        fn()
        ms = dev.timer_stop()
        if r >= 2:
            out.append(ms)
    return float(np.median(out))


def run(cfg, reps, host):
    import pyqmc_amd as pa
    from pyqmc_amd.configs import PeriodicConfigs
    from pyqmc_amd.sq import device_sq

    system, nq, W = cfg.split(":")
    nq, W = int(nq), int(W)
    mol, wf = build(system)
    if nq > 0:
        acc = pa.SqAccumulator(mol, nq=nq)
    else:
        acc = pa.SqAccumulator(mol, qlist=np.random.default_rng(2).uniform(-2.0, 2.0, (364, 3)))
    configs = pa.initial_guess(mol, W, rng=np.random.default_rng(1))
    if hasattr(mol, "a"):
        configs = PeriodicConfigs(configs.configs, mol.lattice_vectors())
    wf.recompute(configs)
    dev = wf.fused_device()
    N, Q = sum(mol.nelec), len(acc.qlist)
    rec = acc.qn is not None
    args = (dev, acc.qlist, acc.qn, acc.recip)
    out = {"config": cfg, "system": system, "nq": nq, "walkers": W, "nelec": N, "Q": Q, "path": "recurrence" if rec else "direct"}
    out["chunks"] = -(-W // max(1, (256 << 20) // (16 * Q)))
    out["mean_ms"] = timed(dev, lambda: device_sq(*args, mean=True), reps)
    if W * Q * 16 <= 1 << 30:
        out["per_walker_ms"] = timed(dev, lambda: device_sq(*args), max(2, reps // 2))
    out["after_sweep_mean_ms"] = timed(dev, lambda: device_sq(*args, mean=True), max(2, reps // 2),
                                       before=lambda r: dev.vmc_sweeps(0.3, 1, seed=50 + r, energy=False))
    terms, flops, lds, ob = model(N, Q, W, rec)
    out.update(terms=terms, model_flops=flops, model_lds_bytes=lds, per_walker_bytes=ob)
    t = out["mean_ms"] * 1e-3
    bound = max(flops / F64_VECTOR_FLOPS, lds / LDS_BYTES_PER_S, 2 * ob / HBM_BYTES_PER_S)
    out["bound_ms"] = bound * 1e3
    out["frac_of_bound"] = bound / t
    out["frac_peak_f64"], out["frac_peak_lds"] = flops / t / F64_VECTOR_FLOPS, lds / t / LDS_BYTES_PER_S
    if host:
        Wh = min(W, 1024)
        x = np.asarray(configs.configs)[:Wh]
        t0 = time.perf_counter()
        acc._host(x, True)
        out["host_walkers"], out["host_ms"] = Wh, (time.perf_counter() - t0) * 1e3
        out["host_ms_per_walker_over_fused"] = (out["host_ms"] / Wh) / (out["mean_ms"] / W)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--configs", default=DEFAULT)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--no-host", action="store_true")
    ap.add_argument("--out", default=None, help="also append the JSON lines to this file")
    a = ap.parse_args()
    import __graft_entry__

    __graft_entry__.build()
    for cfg in a.configs.split(","):
        line = json.dumps(run(cfg, a.reps, not a.no_host))
        print(line, flush=True)
        if a.out:
            with open(a.out, "a") as f:
                f.write(line + "\n")


if __name__ == "__main__":
    main()
