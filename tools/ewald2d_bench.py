"""Slab Ewald sum (pqa_ewald2d) timing: one JSON line per configuration.

    python tools/ewald2d_bench.py [--configs 4x2:65536,...] [--reps 10] [--no-host] [--out profiles/ewald2d_bench.jsonl]

A configuration is SxT:WALKERS: the carbon slab cell (two atoms, eight electrons per oblique 5 x 4.5 cell, 30 bohr tall) repeated
S x T times in the plane (4x2: 16 atoms, 64 electrons).  Per configuration: ms of one per-walker call and of one mean-mode call
(HIP events on the handle's stream, warm, median of --reps calls), at positions after two VMC sweeps; the algorithmic work from the
shapes ((pair, k) terms and fp64 flops, see `model`) with the share of the fp64 vector rate it implies; and the host route
(NumPy / scipy, `Ewald._host`) on --host-walkers of the same walkers spread over --host-procs processes, scaled linearly to the
walker count.  The host processes are started (spawn) and finished before the device is opened.  The library must be built.
"""

import argparse
import json
import multiprocessing as mp
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

F64_VECTOR_FLOPS = 78.6e12  # MI355X fp64 vector peak (FMA = 2)
DEFAULT = "2x2:4096,4x2:4096,4x2:65536"
LATTICE = np.array([[5.0, 0.0, 0.0], [1.5, 4.5, 0.0], [0.0, 0.0, 30.0]])


def slab(s, t):
    from pyqmc_amd import pbc, systems

    prim = systems.Cell(["C", "C"], [(0.6, 0.5, 14.3), (3.2, 2.6, 15.7)], LATTICE, dimension=2)
    return pbc.get_supercell(prim, np.diag([float(s), float(t), 1.0]))


def walkers(cell, W, seed=1, sigma=1.5):
    rng = np.random.default_rng(seed)
    N = sum(cell.nelec)
    x = np.concatenate([rng.uniform(0, 1, (W, N, 2)), np.full((W, N, 1), 0.5)], axis=-1) @ cell.lattice_vectors()
    x[..., 2] += sigma * rng.standard_normal((W, N))
    return x


def model(N, natom, nk, nlat, W):
    """((pair, k) terms, flops) from the shapes.  Per (pair, k) term: two complex products and the real part of a third (14 flops),
    two erfcx polynomials of degree 9 with their interval arithmetic (2 x 24), the bracket, weight and accumulation (8): 70 flops;
    the exp(-k |z|) of the terms with alpha |z| > k / 2 alpha is not counted.  Per (pair, in-plane image): 60 flops (distance, rsqrt
    with two Newton steps, erfcx polynomial, exp); per pair 150 (minimal image, charge term)."""
    pairs = N * (N - 1) // 2 + N * natom
    terms = W * pairs * nk
    return terms, terms * 70 + W * pairs * (60 * nlat + 150)


def host_chunk(args):
    s, t, x = args
    from pyqmc_amd import ewald2d

    ee, ei = ewald2d.Ewald(slab(s, t))._host(x)
    return float(ee.sum() + ei.sum())


def host_time(s, t, x, procs):
    """Wall time of the host route on the walkers x over `procs` processes (started before the clock, one warm-up task each)."""
    parts = np.array_split(x, procs)
    with mp.get_context("spawn").Pool(procs) as pool:
        pool.map(host_chunk, [(s, t, p[:1]) for p in parts])
        t0 = time.perf_counter()
        pool.map(host_chunk, [(s, t, p) for p in parts])
        return (time.perf_counter() - t0) * 1e3


def timed(dev, fn, reps):
    out = []
    for r in range(reps + 2):
        dev.sync()
        dev.timer_start()
        fn()
        ms = dev.timer_stop()
        if r >= 2:
            out.append(ms)
    return float(np.median(out))


def run(cfg, reps, host_ms, host_walkers, host_procs):
    import pyqmc_amd as pa
    from pyqmc_amd import ewald2d, pbc
    from pyqmc_amd.configs import PeriodicConfigs
    from pyqmc_amd.ewald2d import device_ewald2d
    from pyqmc_amd.vmc import _fetch

    st, W = cfg.split(":")
    s, t = (int(v) for v in st.split("x"))
    W = int(W)
    cell = slab(s, t)
    wf = pa.generate_wf(cell, pbc.random_kmf(cell))
    configs = PeriodicConfigs(walkers(cell, W), cell.lattice_vectors())
    wf.recompute(configs)
    dev = wf.fused_device()
    dev.vmc_sweeps(0.3, 2, seed=7, energy=False)
    ew = ewald2d.Ewald(cell)
    N, natom, nk, nlat = sum(cell.nelec), cell.natm, len(ew.gnorm), len(ew.lattice_displacements)
    out = {"config": cfg, "walkers": W, "nelec": N, "natom": natom, "nk": nk, "nlat": nlat}
    out["per_walker_ms"] = timed(dev, lambda: device_ewald2d(dev, ew.tab), reps)
    out["mean_ms"] = timed(dev, lambda: device_ewald2d(dev, ew.tab, mean=True), reps)
    terms, flops = model(N, natom, nk, nlat, W)
    out.update(terms=terms, model_flops=flops, model_mflop_per_walker=flops / W / 1e6)
    out["frac_peak_f64"] = flops / (out["mean_ms"] * 1e-3) / F64_VECTOR_FLOPS
    if host_ms is not None:
        Wh = min(W, host_walkers)
        _fetch(dev, configs)
        hee, hei = ew._host(np.asarray(configs.configs)[:16])
        ee, ei = device_ewald2d(dev, ew.tab)
        out["relerr_vs_host"] = float(max(np.max(np.abs(ee[:16] - hee) / np.abs(hee)), np.max(np.abs(ei[:16] - hei) / np.abs(hei))))
        out.update(host_walkers=Wh, host_procs=host_procs, host_ms=host_ms[cfg], host_ms_scaled=host_ms[cfg] * W / Wh)
        out["host_over_fused"] = out["host_ms_scaled"] / out["per_walker_ms"]
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--configs", default=DEFAULT)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--no-host", action="store_true")
    ap.add_argument("--host-walkers", type=int, default=512)
    ap.add_argument("--host-procs", type=int, default=16)
    ap.add_argument("--out", default=None, help="also append the JSON lines to this file")
    a = ap.parse_args()
    cfgs = a.configs.split(",")
    host_ms = None
    if not a.no_host:  # every host process ends before the device is opened
        host_ms = {}
        for cfg in cfgs:
            st, W = cfg.split(":")
            s, t = (int(v) for v in st.split("x"))
            x = walkers(slab(s, t), min(int(W), a.host_walkers))
            host_ms[cfg] = host_time(s, t, x, a.host_procs)
    for cfg in cfgs:
        line = json.dumps(run(cfg, a.reps, host_ms, a.host_walkers, a.host_procs))
        print(line, flush=True)
        if a.out:
            with open(a.out, "a") as f:
                f.write(line + "\n")


if __name__ == "__main__":
    main()
