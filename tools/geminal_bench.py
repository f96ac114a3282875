"""Protocol-call timing of the GeminalJastrow device unit next to the route the package offered before it: ``DeviceWF.eval_ao`` on
the device followed by the reference's einsums (geminaljastrow.py:139-152, :196-204) in NumPy on the host.  One JSON line per walker
count, appended to profiles/geminal_bench.jsonl with --record.

    python tools/geminal_bench.py [--walkers 4096,65536] [--reps 7] [--pgrad-walkers 256] [--record]

System: ``systems.water_cluster()`` (32/32 electrons, 184 AOs), gcoeff ~ 0.005 N(0, 1).  Per route: wall-clock milliseconds of one
``gradient_value`` + ``updateinternals`` pair (one electron move as ``pyqmc.method.mc`` makes it, host arrays in and out, ending with
a stream synchronisation) and of one ``pgradient`` on the first ``--pgrad-walkers`` walkers (the full derivative array is 8.9 GB at
65 536 walkers).  Two warm-up calls, then ``reps`` timed ones: median, minimum, maximum and spread = (max - min) / median.
``model_*``: flop of the GEMM and bytes the unit's kernels move per call, from the shapes, and the time they take at the fp64 matrix
and HBM peaks.  The library is used as built (no build on import)."""

import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

HBM_BYTES_PER_S = 8.0e12  # MI355X HBM3E peak
MFMA_F64_FLOPS = 78.6e12  # MI355X fp64 matrix peak


def stats(ms):
    med = float(np.median(ms))
    return {"ms": med, "min_ms": float(min(ms)), "max_ms": float(max(ms)), "spread": float((max(ms) - min(ms)) / med), "reps": len(ms)}


class HostEinsum:
    """The parent route: AOs from the device's AO-only entry point, everything else the reference's einsums on the host."""

    def __init__(self, dev, gcoeff):
        self.dev, nao = dev, dev.nao
        G = np.zeros((nao, nao))
        G[np.triu_indices(nao)] = gcoeff
        self.G = G + G.T

    def recompute(self, configs):
        W, N, _ = configs.configs.shape
        self.ao_val = self.dev.eval_ao(configs.configs, 1)[0].reshape(W, N, -1)

    def _compute_value(self, ao_e, e):
        v = np.einsum("mn,...cm,cjn->...c", self.G, ao_e, self.ao_val[:, :e], optimize="greedy")
        return v + np.einsum("mn,...cn,cim->...c", self.G, ao_e, self.ao_val[:, e + 1 :], optimize="greedy")

    def gradient_value(self, e, epos):
        ao = self.dev.eval_ao(epos.configs, 4)
        deriv = self._compute_value(ao, e)
        return deriv[1:], np.exp(deriv[0] - self._compute_value(self.ao_val[:, e], e)), ao[0]

    def updateinternals(self, e, epos, configs, mask=None, saved_values=None):
        self.ao_val[mask, e] = saved_values[mask]

    def pgradient(self):
        a = self.ao_val
        tri = np.tril(np.ones((a.shape[1], a.shape[1])), -1)
        d = np.einsum("cim,cjn,ij->cmn", a, a, tri, optimize="greedy")
        d = d + d.transpose(0, 2, 1)
        iu = np.triu_indices(d.shape[-1])
        return {"gcoeff": d[:, iu[0], iu[1]]}


def time_route(wf, small, configs, small_configs, reps, rng):
    W, N, _ = configs.configs.shape
    wf.recompute(configs)
    small.recompute(small_configs)
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
        small.pgradient()
        t3 = time.perf_counter()
        if r >= 2:
            pair.append((t1 - t0) * 1e3)
            pg.append((t3 - t2) * 1e3)
    return {"gradient_value+updateinternals": stats(pair), "pgradient": stats(pg)}


def model(W, Wp, N, nao):
    """Per pair: the GEMM H = (T - a_e) G, 2 W nao^2 flop; bytes: four AO planes written and read, the kept value plane copied, B and h
    rows, and the update's pass over A and T of the touched walkers (half of them here).  pgradient: 2 flop per pair, electron and
    walker; bytes: A read once, the derivatives written."""
    npair = nao * (nao + 1) // 2
    pair_bytes = 8 * (W * nao * (4 + 4 + 2 + 2 + 2) + 0.5 * W * nao * (N + 2))
    pg_bytes = 8 * Wp * (N * nao + npair)
    return {"model_flop_gemm": 2.0 * W * nao * nao, "model_floor_ms_gemm": 2.0 * W * nao * nao / MFMA_F64_FLOPS * 1e3,
            "model_bytes_pair": pair_bytes, "model_floor_ms_pair": pair_bytes / HBM_BYTES_PER_S * 1e3,
            "model_flop_pgradient": 2.0 * Wp * N * npair, "model_bytes_pgradient": pg_bytes,
            "model_floor_ms_pgradient": pg_bytes / HBM_BYTES_PER_S * 1e3}


def run(W, Wp, reps, baseline):
    import pyqmc_amd as pa
    from pyqmc_amd import systems

    mol = systems.water_cluster()
    rng = np.random.default_rng(7)
    configs = pa.initial_guess(mol, W, rng=np.random.default_rng(1))
    N = configs.configs.shape[1]
    Wp = min(Wp, W)
    small_configs = type(configs)(configs.configs[:Wp].copy())
    wf, small = pa.GeminalJastrow(mol), pa.GeminalJastrow(mol)
    gcoeff = 0.005 * rng.standard_normal(wf.parameters["gcoeff"].shape)
    wf.parameters["gcoeff"] = small.parameters["gcoeff"] = gcoeff
    rec = {"system": "water_cluster", "walkers": W, "pgradient_walkers": Wp, "nelec": list(mol.nelec), "nao": wf.nao}
    rec["geminal"] = time_route(wf, small, configs.copy(), small_configs, reps, rng)
    rec.update(model(W, Wp, N, wf.nao))
    if baseline:
        dev = wf._gem  # (any handle with the basis tables evaluates AOs)
        rec["eval_ao+numpy"] = time_route(HostEinsum(dev, gcoeff), HostEinsum(dev, gcoeff), configs.copy(), small_configs, reps, rng)
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--walkers", default="4096,65536")
    ap.add_argument("--pgrad-walkers", type=int, default=256)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--no-baseline", action="store_true", help="skip the eval_ao + NumPy route")
    ap.add_argument("--record", action="store_true", help="append the lines to profiles/geminal_bench.jsonl")
    a = ap.parse_args()
    for W in a.walkers.split(","):
        line = json.dumps(run(int(W), a.pgrad_walkers, a.reps, not a.no_baseline))
        print(line, flush=True)
        if a.record:
            with open(os.path.join(ROOT, "profiles", "geminal_bench.jsonl"), "a") as f:
                f.write(line + "\n")


if __name__ == "__main__":
    main()
