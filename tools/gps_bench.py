"""Protocol-call timing of the GPSJastrow device unit next to a bare JastrowSpin of the same system: one JSON line per walker count,
appended to profiles/gps_bench.jsonl with --record.

    python tools/gps_bench.py [--walkers 4096,65536] [--nsup 32] [--reps 7] [--record]

System: ``systems.water_cluster()`` (32/32 electrons).  Per factor: wall-clock milliseconds of one ``gradient_value`` +
``updateinternals`` pair (one electron move as ``pyqmc.method.mc`` makes it, host arrays in and out, ending with a stream
synchronisation) and of one ``pgradient``.  Two warm-up calls, then ``reps`` timed ones: median, minimum, maximum and
spread = (max - min) / median.  The GPS factor uses f = 1.0, support points at electron positions plus N(0, 0.3) noise and
alpha ~ N(0, 0.3).  ``model_*``: bytes the unit's kernels move per call, from the shapes, and the time they take at the HBM peak.
The library is used as built (no build on import)."""

import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

HBM_BYTES_PER_S = 8.0e12  # MI355X HBM3E peak


def stats(ms):
    med = float(np.median(ms))
    return {"ms": med, "min_ms": float(min(ms)), "max_ms": float(max(ms)), "spread": float((max(ms) - min(ms)) / med), "reps": len(ms)}


def time_factor(wf, configs, reps, rng):
    W, N, _ = configs.configs.shape
    wf.recompute(configs)
    pair, pg = [], []
    for r in range(reps + 2):
        e = r % N
        ep = configs.make_irreducible(e, configs.configs[:, e] + 0.3 * rng.standard_normal((W, 3)))
        mask = rng.random(W) > 0.5
        t0 = time.perf_counter()
        _, _, saved = wf.gradient_value(e, ep)
        wf.updateinternals(e, ep, configs, mask=mask, saved_values=saved)
        t1 = time.perf_counter()
        configs.move(e, ep, mask)
        t2 = time.perf_counter()
        wf.pgradient()
        t3 = time.perf_counter()
        if r >= 2:
            pair.append((t1 - t0) * 1e3)
            pg.append((t3 - t2) * 1e3)
    return {"gradient_value+updateinternals": stats(pair), "pgradient": stats(pg)}


def gps_model(W, N, nsup):
    """Bytes of the unit's kernels per call (8-byte words): the eval reads the electron's column, S and the support table per walker and
    writes four outputs; the update reads e of the touched walkers (half of them here) and writes a column and S; pgradient reads e,
    the walkers and S and writes 7 nsup + 1 derivatives per walker."""
    K = 2 * nsup
    pair = 8 * (W * (2 * K + 3 + 4) + 0.5 * W * (N * K + 2 * K + 6))
    pgrad = 8 * W * (N * K + 3 * N + K + 7 * nsup + 1)
    return {"model_bytes_pair": pair, "model_floor_ms_pair": pair / HBM_BYTES_PER_S * 1e3,
            "model_bytes_pgradient": pgrad, "model_floor_ms_pgradient": pgrad / HBM_BYTES_PER_S * 1e3}


def run(W, nsup, reps):
    import pyqmc_amd as pa
    from pyqmc_amd import systems
    from pyqmc_amd.wf import generate_jastrow

    mol = systems.water_cluster()
    rng = np.random.default_rng(7)
    configs = pa.initial_guess(mol, W, rng=np.random.default_rng(1))
    N = configs.configs.shape[1]
    X = configs.configs[rng.integers(W, size=(nsup, 2)), rng.integers(N, size=(nsup, 2))] + 0.3 * rng.standard_normal((nsup, 2, 3))
    gps = pa.GPSJastrow(mol, X, f=1.0)
    gps.parameters["alpha"] = 0.3 * rng.standard_normal(nsup)
    rec = {"system": "water_cluster", "walkers": W, "nelec": list(mol.nelec), "nsup": nsup}
    rec["gps"] = time_factor(gps, configs.copy(), reps, rng)
    rec.update(gps_model(W, N, nsup))
    del gps
    ja, _ = generate_jastrow(mol)
    rec["jastrowspin"] = time_factor(ja, configs.copy(), reps, rng)
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--walkers", default="4096,65536")
    ap.add_argument("--nsup", type=int, default=32)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--record", action="store_true", help="append the lines to profiles/gps_bench.jsonl")
    a = ap.parse_args()
    for W in a.walkers.split(","):
        line = json.dumps(run(int(W), a.nsup, a.reps))
        print(line, flush=True)
        if a.record:
            with open(os.path.join(ROOT, "profiles", "gps_bench.jsonl"), "a") as f:
                f.write(line + "\n")


if __name__ == "__main__":
    main()
