"""Total-spin estimator (pqa_s2) timing: one JSON line per configuration.

    python tools/s2_bench.py [--configs M,C2,K222,MD50] [--reps 10] [--protocol-walkers 4096]

Per configuration: walkers; ms per pqa_s2 from HIP events on the handle's stream, warm, on resident walker-major state
("warm_ms") and right after a fused sweep, which leaves the state in the sweep's lane-per-walker layout so that the call
includes the layout sync ("after_sweep_ms"); the orbital scratch of the walker chunks; bytes and flops from the shapes and
the fraction of peak they imply; and the protocol route (S2Accumulator over testvalue / updateinternals) at a small walker
count with the fused time at that count, for the speed-up.  The k_s2 kernel time comes from a rocprofv3 --kernel-trace --stats
run of this tool (--reps 5 --no-protocol).
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
SCRATCH_CAP = 256 << 20  # pqa_s2.hip: kS2ScratchBytes


def build(name):
    from pyqmc_amd import systems
    from tests import helpers

    if name == "M":
        mol = systems.water_cluster()
        return mol, helpers.gpu_wf(mol, systems.random_mf(mol)), 65536
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
    """(bytes, flops) of one pqa_s2 evaluation from the shapes: orbital scratch written and read back, inverses and coordinates
    read; MFMA work of the two rho products per full determinant (padded to the 16x16x4 tiles the kernel issues) and the Jastrow
    pairs.  The orbital pass itself is counted in neither (it is the orbital kernel's own roofline)."""
    nu, nd = dev.nelec
    N = nu + nd
    nmo = dev.nmo
    ndet, nds = dev.ndet, dev.ndet_s
    pad = lambda n: -(-n // 16) * 16  # noqa: E731
    scratch = (nd * nmo[0] + nu * nmo[1]) * 8
    by = W * (2 * scratch + (nds[0] * nu * nu + nds[1] * nd * nd) * 8 + N * 3 * 8 + 8)
    mfma = 2 * ndet * pad(nu) * pad(nd) * (-(-nu // 4) * 4 + -(-nd // 4) * 4)
    jas = (N * N + nu * nd) * 2 * 12 * max(getattr(dev, "nb", 4), 1)
    return by, W * (mfma + jas), scratch


def device_ms(dev, reps, after_sweep):
    from pyqmc_amd.s2 import device_s2

    out = []
    for r in range(reps + 2):
        if after_sweep:
            dev.vmc_sweeps(0.3, 1, seed=100 + r, energy=False)
        dev.sync()
        dev.timer_start()
        device_s2(dev)
        ms = dev.timer_stop()
        if r >= 2:
            out.append(ms)
    return float(np.median(out))


def run(name, reps, protocol_walkers, protocol):
    import pyqmc_amd as pa

    mol, wf, W = build(name)
    dev = wf.fused_device()
    configs = pa.initial_guess(mol, W, rng=np.random.default_rng(1))
    if hasattr(mol, "a"):
        from pyqmc_amd.configs import PeriodicConfigs

        configs = PeriodicConfigs(configs.configs, mol.lattice_vectors())
    wf.recompute(configs)
    rec = {"config": name, "walkers": W, "nelec": list(dev.nelec), "ndet": dev.ndet}
    rec["warm_ms"] = device_ms(dev, reps, False)
    rec["after_sweep_ms"] = device_ms(dev, reps, True)
    by, fl, per = shapes_model(dev, W)
    chunk = max(1, min(W, SCRATCH_CAP // per))
    rec["orbital_scratch_MiB"] = chunk * per / 2**20
    rec["walkers_per_chunk"] = chunk
    rec["model_bytes"], rec["model_flops"] = by, fl
    t = rec["warm_ms"] * 1e-3
    fb, ff = by / t / HBM_BYTES_PER_S, fl / t / F64_MATRIX_FLOPS
    rec["frac_peak_hbm"], rec["frac_peak_f64_mfma"] = fb, ff
    rec["bound"] = "memory (HBM)" if fb >= ff else "fp64 matrix"
    if protocol:
        Wp = min(protocol_walkers, W)
        x = configs.configs[:Wp].copy()
        small = type(configs)(x, mol.lattice_vectors()) if hasattr(mol, "a") else pa.OpenConfigs(x)
        wf.recompute(small)
        rec["protocol_walkers"] = Wp
        rec["fused_ms_at_protocol_walkers"] = device_ms(dev, reps, False)
        acc = pa.S2Accumulator(mol.nelec)
        t0 = time.perf_counter()
        acc._protocol(small, wf)
        dev.sync()
        rec["protocol_ms"] = (time.perf_counter() - t0) * 1e3
        rec["speedup"] = rec["protocol_ms"] / rec["fused_ms_at_protocol_walkers"]
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--configs", default="M,C2,K222,MD50")
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--protocol-walkers", type=int, default=4096)
    ap.add_argument("--no-protocol", action="store_true")
    a = ap.parse_args()
    import __graft_entry__

    __graft_entry__.build()
    for name in a.configs.split(","):
        print(json.dumps(run(name, a.reps, a.protocol_walkers, not a.no_protocol)), flush=True)


if __name__ == "__main__":
    main()
