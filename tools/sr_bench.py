"""Gradient-VMC timings on one MI355X -> profiles/sr_bench.jsonl (one JSON line per case, appended).

    python tools/sr_bench.py [--walkers 16384 65536] [--sweeps 10] [--reps 2] [--cluster 2 2 2] [--orbitals [--orbital-rows N]]
                             [--complex] [--out profiles/sr_bench.jsonl]

One vmc_worker block of `sweeps` sweeps for a water cluster ((H2O)8 by default; --cluster nx ny nz) with the gradient accumulator of
line minimisation (gradient_generator, default_to_opt), on the device route (pqa_sr_moments on the resident state) and on the protocol
route (walkers and derivative arrays through the host, pqa_gram), alternately in one process.  --orbitals optimises the orbital
coefficients too (default_to_opt(..., optimize_orbitals=True); the device route is pqa_sr_moments_orb and is asked for by name);
--orbital-rows N keeps only the orbital rows of the first N AOs (the full (H2O)8 selection, P = 11 776, is beyond the 256 MiB the
moments of a device call may take).  Each route gets a warm-up block first; the block averages of the two routes from the same walkers,
sweep keys and energy keys are checked equal (1e-9) before anything is timed.  Wall clock of the whole block (both routes end with the
walkers on the host), the best of `reps`; every repeat is recorded.

--complex: the same for the 8-atom twisted diamond cell of tools/config_bench.py c3 (16 + 16 electrons, complex orbitals; default
walkers 8192 16384) with default_to_opt; the device route is pqa_sr_moments_c, asked for with complex_device=True (rows carry
"complex": true).
"""

import argparse
import copy
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402

import pyqmc_amd as pa  # noqa: E402
from pyqmc_amd import systems  # noqa: E402
from pyqmc_amd import wf as pwf  # noqa: E402
from pyqmc_amd.accumulators import gradient_generator  # noqa: E402

ROUTES = ("device", "protocol")


def twisted_cell():
    """The c3 configuration of tools/config_bench.py: the conventional diamond cell with a k-point twist."""
    from pyqmc_amd import pbc

    sup = pbc.get_supercell(systems.diamond_primitive(), np.array([[-1.0, 1, 1], [1, -1, 1], [1, 1, -1]]))
    return sup, pa.generate_wf(sup, pbc.random_kmf(sup, complex_coeff=True, twist=(0.25, 0.1, -0.3)))


def case(W, sweeps, reps, cluster=(2, 2, 2), orbitals=False, orbital_rows=0, cplx=False):
    mol, wf = twisted_cell() if cplx else (systems.water_cluster(*cluster), None)
    if wf is None:
        wf = pa.generate_wf(mol, systems.random_mf(mol))
    rng = np.random.default_rng(11)  # (a non-trivial Jastrow: small random coefficients, the electron-electron cusp row kept)
    ja = wf.wf_factors[1].parameters
    wf.parameters["wf2acoeff"] = 0.05 * rng.standard_normal(np.shape(ja["acoeff"]))
    wf.parameters["wf2bcoeff"] = np.concatenate([np.asarray(ja["bcoeff"])[:1], 0.05 * rng.standard_normal((np.shape(ja["bcoeff"])[0] - 1, 3))])
    start = pa.initial_guess(mol, W, rng=np.random.default_rng(2))
    to_opt = pwf.default_to_opt(wf, optimize_orbitals=orbitals)
    if orbitals and orbital_rows:
        for k in ("wf1mo_coeff_alpha", "wf1mo_coeff_beta"):
            to_opt[k][orbital_rows:] = False
    sr = {r: gradient_generator(mol, wf, to_opt, route=r, complex_device=cplx) for r in ROUTES}

    def block(route, nsteps, seed):
        sr[route].enacc.seed, sr[route].enacc._calls = 1000 * seed, 0
        t0 = time.perf_counter()
        blk, _ = pa.vmc_worker(wf, copy.deepcopy(start), 0.3, nsteps, {"pgrad": sr[route]}, seed=seed)
        dt = time.perf_counter() - t0
        assert sr[route].last_route == route
        return blk, dt

    warm = {r: block(r, 2, 1)[0] for r in ROUTES}  # (warm-up, and the check that the routes agree)
    worst = 0.0
    for k, v in warm["protocol"].items():
        if "time" not in k:
            worst = max(worst, float(np.max(np.abs(warm["device"][k] - v)) / max(np.max(np.abs(v)), 1e-300)))
    assert worst < 1e-9, worst
    assert not cplx or (wf.fused_device().twisted and np.iscomplexobj(warm["device"]["pgraddpH"]))
    best = {r: (np.inf, None) for r in ROUTES}
    every = {r: [] for r in ROUTES}
    for rep in range(reps):
        for r in ROUTES:
            blk, dt = block(r, sweeps, 2 + rep)
            every[r].append(dt)
            if dt < best[r][0]:
                best[r] = (dt, blk)
    row = {"what": "gradient VMC block (vmc_worker, gradient_generator)",
           "system": "C3 twisted diamond cell" if cplx else "(H2O)%d" % (cluster[0] * cluster[1] * cluster[2]), "complex": bool(cplx),
           "orbitals": bool(orbitals), "orbital_rows": int(orbital_rows) if orbitals else None, "walkers": W, "sweeps": sweeps,
           "nparams": int(sr["device"].transform.nparams), "routes_max_relerr": worst}
    for r in ROUTES:
        dt, blk = best[r]
        row.update({f"seconds_{r}": dt, f"seconds_all_{r}": every[r], f"move_ms_per_sweep_{r}": 1e3 * float(blk["move time"]),
                    f"accumulator_ms_per_sweep_{r}": 1e3 * float(blk["accumulator time"])})
    row["speedup"] = row["seconds_protocol"] / row["seconds_device"]
    print(json.dumps(row), flush=True)
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--walkers", type=int, nargs="+", default=None, help="default: 16384 65536; with --complex: 8192 16384")
    ap.add_argument("--sweeps", type=int, default=10)
    ap.add_argument("--reps", type=int, default=2)
    ap.add_argument("--cluster", type=int, nargs=3, default=[2, 2, 2], metavar=("NX", "NY", "NZ"))
    ap.add_argument("--orbitals", action="store_true", help="optimise the orbital coefficients too")
    ap.add_argument("--orbital-rows", type=int, default=0, help="with --orbitals: only the orbital rows of the first N AOs (0: all)")
    ap.add_argument("--complex", dest="cplx", action="store_true", help="the twisted diamond cell (complex handle, pqa_sr_moments_c)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "sr_bench.jsonl"))
    a = ap.parse_args()
    if a.cplx and a.orbitals:
        ap.error("--complex takes no --orbitals: orbital coefficients of a complex handle stay on the protocol route")
    walkers = a.walkers or ([8192, 16384] if a.cplx else [16384, 65536])
    rows = [case(W, a.sweeps, a.reps, tuple(a.cluster), a.orbitals, a.orbital_rows, a.cplx) for W in walkers]
    if a.out:
        with open(a.out, "a") as f:
            for r in rows:
                f.write(json.dumps(r) + "\n")


if __name__ == "__main__":
    main()
