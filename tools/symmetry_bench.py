"""Symmetry-operator ratios (pqa_symmetry) timing: one JSON line per configuration.

    python tools/symmetry_bench.py [--configs M,M4,C2,K222,MD50] [--reps 10] [--no-protocol]

Per configuration: walkers; ms for one evaluation of one operator (a generic rotation; about a general origin in the periodic
cell) by pqa_symmetry from HIP events on the handle's stream, warm, on resident walker-major state ("fused_ms") and right after a
fused sweep, which leaves the state in the sweep's lane-per-walker layout so that the call includes the layout sync
("after_sweep_ms"); the walker chunks and their scratch; bytes and flops from the shapes and the fraction of peak they imply; and
the protocol route (the reference's copy, transform, recompute, recompute back) on the same handle and walkers, host wall time,
for the speed-up.  The kernel split comes from a rocprofv3 --kernel-trace --stats run of this tool (--reps 5 --no-protocol).
"""

import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

HBM_BYTES_PER_S = 8.0e12  # MI355X HBM3E peak
F64_MATRIX_FLOPS = 78.6e12  # MI355X fp64 MFMA peak
SCRATCH_CAP = 256 << 20  # pqa_symmetry.hip: kSymScratchBytes


def rotation(axis, angle):
    k = np.asarray(axis, dtype=float)
    k /= np.linalg.norm(k)
    K = np.array([[0, -k[2], k[1]], [k[2], 0, -k[0]], [-k[1], k[0], 0]])
    return (np.eye(3) + np.sin(angle) * K + (1 - np.cos(angle)) * K @ K).T


OP = rotation([0.3, -0.5, 0.8], 0.7)


def build(name):
    from pyqmc_amd import systems
    from tests import helpers

    if name in ("M", "M4"):
        mol = systems.water_cluster()
        return mol, helpers.gpu_wf(mol, systems.random_mf(mol)), 65536 if name == "M" else 4096
    if name == "C2":
        mol = systems.water()
        return mol, helpers.gpu_wf(mol, systems.random_mf(mol)), 4096
    if name == "K222":
        sup, wf = helpers.gpu_pbc_wf("k222")
        return sup, wf, 4096
    if name == "MD50":
        mol = systems.water()
        mf = systems.random_mf(mol, nvirt=6)
        return mol, helpers.gpu_wf(mol, mf, systems.random_determinants(mol, mf, 50)), 2048
    raise KeyError(name)


def shapes_model(dev, W):
    """(bytes, flops, scratch bytes per walker) of one evaluation from the shapes: transformed coordinates and orbital scratch written
    and read back, coordinates and inverses read; MFMA work of the B products (padded to the 16x16x4 tiles), the LU and the Jastrow
    pairs of both configurations.  The orbital pass itself is counted in neither (it is the orbital kernel's own roofline)."""
    nu, nd = dev.nelec
    N = nu + nd
    nmo, nds = dev.nmo, dev.ndet_s
    pad = lambda n: -(-n // 16) * 16  # noqa: E731
    scratch = (3 * N + nu * nmo[0] + nd * nmo[1] + 2 * (nds[0] + nds[1])) * 8
    by = W * (2 * scratch + (nds[0] * nu * nu + nds[1] * nd * nd) * 8 + 2 * N * 3 * 8 + 8)
    mfma = sum(2 * nds[s] * pad(n) * pad(n) * (-(-n // 4) * 4) for s, n in enumerate((nu, nd)))
    lu = sum(nds[s] * 2 * n ** 3 // 3 for s, n in enumerate((nu, nd)))
    jas = 2 * (N * (N - 1) // 2 + N * dev.natom) * 2 * 12 * max(getattr(dev, "nb", 4), 1)
    return by, W * (mfma + lu + jas), scratch


def fused_ms(dev, reps, after_sweep, origins):
    from pyqmc_amd.symmetry import device_symmetry

    out = []
    for r in range(reps + 2):
        if after_sweep:
            dev.vmc_sweeps(0.3, 1, seed=100 + r, energy=False)
        dev.sync()
        dev.timer_start()
        device_symmetry(dev, OP[None], origins)
        ms = dev.timer_stop()
        if r >= 2:
            out.append(ms)
    return float(np.median(out))


def run(name, reps, protocol):
    import pyqmc_amd as pa

    mol, wf, W = build(name)
    dev = wf.fused_device()
    configs = pa.initial_guess(mol, W, rng=np.random.default_rng(1))
    periodic = hasattr(mol, "a")
    if periodic:
        from pyqmc_amd.configs import PeriodicConfigs

        configs = PeriodicConfigs(configs.configs, mol.lattice_vectors())
    origin = np.array([0.7, -0.3, 1.9])
    wf.recompute(configs)
    rec = {"config": name, "walkers": W, "nelec": list(dev.nelec), "ndet": dev.ndet, "periodic": periodic}
    rec["fused_ms"] = fused_ms(dev, reps, False, origin[None] if periodic else None)
    by, fl, per = shapes_model(dev, W)
    chunk = max(1, min(W, SCRATCH_CAP // per))
    rec["walkers_per_chunk"], rec["scratch_MiB"] = chunk, chunk * per / 2**20
    rec["model_bytes"], rec["model_flops"] = by, fl
    t = rec["fused_ms"] * 1e-3
    fb, ff = by / t / HBM_BYTES_PER_S, fl / t / F64_MATRIX_FLOPS
    rec["frac_peak_hbm"], rec["frac_peak_f64_mfma"] = fb, ff
    if protocol:
        acc = pa.SymmetryAccumulatorPBC({"g": OP}, {"g": origin}) if periodic else pa.SymmetryAccumulator({"g": OP})
        times = []
        for _ in range(2):
            dev.sync()
            t0 = time.perf_counter()
            acc._protocol(configs, wf)
            dev.sync()
            times.append((time.perf_counter() - t0) * 1e3)
        rec["protocol_ms"] = min(times)
        rec["speedup"] = rec["protocol_ms"] / rec["fused_ms"]
    rec["after_sweep_ms"] = fused_ms(dev, reps, True, origin[None] if periodic else None)
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--configs", default="M,M4,C2,K222,MD50")
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--no-protocol", action="store_true")
    ap.add_argument("--out", default=None, help="also append the JSON lines to this file")
    a = ap.parse_args()
    import __graft_entry__

    __graft_entry__.build()
    for name in a.configs.split(","):
        line = json.dumps(run(name, a.reps, not a.no_protocol))
        print(line, flush=True)
        if a.out:
            with open(a.out, "a") as f:
                f.write(line + "\n")


if __name__ == "__main__":
    main()
