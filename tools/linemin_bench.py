"""Line minimisation timings on one MI355X -> profiles/linemin_bench.jsonl (one JSON line per measurement).

    python tools/linemin_bench.py [--walkers 16384 65536] [--npts 40] [--fused-only] [--out profiles/linemin_bench.jsonl]

1. correlated_compute_worker at npts parameter sets for the (H2O)8 cluster, fused route (pqa_correlated) against the protocol
   route (set, recompute, energy per set), on the same walkers; the first call of each route is an untimed warm-up.
2. One line_minimization iteration at the smaller walker count (mixture sampling 1 x 3 and the reference's 10 x 10 sweeps), split into warm-up VMC, gradient VMC, mixture sampling and
   correlated evaluation (wall clock of the driver's own calls, synchronised by their host read-backs).
--fused-only: part 1's fused route only (for a rocprofv3 --kernel-trace --stats run).

    python tools/linemin_bench.py --ndet 50 --system water --walkers 16384

--ndet N: instead of the above, correlated_compute_worker for a multi-determinant handle (N determinants from
systems.random_determinants over random_mf(nvirt=6) orbitals; --system water | cluster), det_coeff, acoeff and bcoeff varying:
evaluation_route="fused" (pqa_correlated_md) against "protocol" on the same handle in one process, alternately, each after a
warm-up, --repeats timed calls of each; the rows are appended to --out.

    python tools/linemin_bench.py --three-body [--ndet 50] [--walkers 2048 16384]

--three-body: the same comparison for a Slater x two-body x three-body Jastrow wave function (config C4 with --ndet 50; --ndet 0 or 1:
single-determinant water), ccoeff varying as well: three_body_device=True (pqa_correlated_j3) against evaluation_route="protocol",
the per-set loop it replaces; default walker counts 2048 and 16384; the rows are appended to --out.
"""

import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402

import pyqmc_amd as pa  # noqa: E402
from pyqmc_amd import linemin, systems  # noqa: E402
from pyqmc_amd import wf as pwf  # noqa: E402
from pyqmc_amd.accumulators import gradient_generator  # noqa: E402
from pyqmc_amd.configs import OpenConfigs  # noqa: E402


def _params(wf, pgrad, npts, seed=3):
    x0 = pgrad.transform.serialize_parameters(wf.parameters)
    d = np.random.default_rng(seed).standard_normal(len(x0)) * 0.02
    return [x0 + t * d for t in np.linspace(-0.2 / (npts - 2), 0.2, npts)]


def correlated(W, npts, fused_only):
    mol = systems.water_cluster()
    wf = pa.generate_wf(mol, systems.random_mf(mol))
    rng = np.random.default_rng(11)  # (a non-trivial Jastrow: small random coefficients, the electron-electron cusp row kept)
    ja = wf.wf_factors[1].parameters
    wf.parameters["wf2acoeff"] = 0.05 * rng.standard_normal(np.shape(ja["acoeff"]))
    wf.parameters["wf2bcoeff"] = np.concatenate([np.asarray(ja["bcoeff"])[:1], 0.05 * rng.standard_normal((np.shape(ja["bcoeff"])[0] - 1, 3))])
    configs = OpenConfigs(systems.initial_guess(mol, W, rng=np.random.default_rng(1)).configs.copy())
    pgrad = gradient_generator(mol, wf, pwf.default_to_opt(wf))
    params = _params(wf, pgrad, npts)
    wf.recompute(configs)
    rows = []
    routes = ["fused"] if fused_only else ["fused", "protocol"]
    for route in routes:
        force = None if route == "fused" else (lambda *a: "protocol")
        orig = linemin.correlated_route
        if force:
            linemin.correlated_route = force
        try:
            linemin.correlated_compute_worker(wf, configs, params[:3], pgrad, [0, 1])  # (warm-up)
            t0 = time.perf_counter()
            res = linemin.correlated_compute_worker(wf, configs, params, pgrad, [0, 1])
            dt = time.perf_counter() - t0
        finally:
            linemin.correlated_route = orig
        assert res["route"] == route
        rows.append({"what": "correlated_compute_worker", "system": "(H2O)8", "walkers": W, "npts": npts, "route": route,
                     "seconds": dt, "ms_per_set": 1e3 * dt / npts, "mean_total_first_last": [float(res["total"][0].mean()),
                                                                                           float(res["total"][-1].mean())]})
        print(json.dumps(rows[-1]), flush=True)
    return rows


def correlated_md(W, npts, ndet, system, fused_only, repeats, three_body=False):
    mol = systems.water() if system == "water" else systems.water_cluster()
    mf = systems.random_mf(mol, nvirt=6)
    wf = pa.generate_wf(mol, mf, determinants=systems.random_determinants(mol, mf, ndet) if ndet > 0 else None, jastrow3=three_body)
    rng = np.random.default_rng(11)
    ja = wf.wf_factors[1].parameters
    wf.parameters["wf2acoeff"] = 0.05 * rng.standard_normal(np.shape(ja["acoeff"]))
    wf.parameters["wf2bcoeff"] = np.concatenate([np.asarray(ja["bcoeff"])[:1], 0.05 * rng.standard_normal((np.shape(ja["bcoeff"])[0] - 1, 3))])
    if three_body:
        wf.parameters["wf3ccoeff"] = 0.1 * rng.standard_normal(np.shape(wf.wf_factors[2].parameters["ccoeff"]))
    configs = OpenConfigs(systems.initial_guess(mol, W, rng=np.random.default_rng(1)).configs.copy())
    pgrad = gradient_generator(mol, wf, pwf.default_to_opt(wf))
    params = _params(wf, pgrad, npts)
    wf.recompute(configs)
    routes = ["fused"] if fused_only else ["fused", "protocol"]
    for route in routes:  # (warm-up)
        linemin.correlated_compute_worker(wf, configs, params[:3], pgrad, [0, 1], evaluation_route=route, three_body_device=three_body)
    rows = []
    for rep in range(repeats):
        for route in routes:
            t0 = time.perf_counter()
            res = linemin.correlated_compute_worker(wf, configs, params, pgrad, [0, 1], evaluation_route=route, three_body_device=three_body)
            dt = time.perf_counter() - t0
            assert res["route"] == route
            rows.append({"what": "correlated_compute_worker", "system": "H2O" if system == "water" else "(H2O)8", "ndet": max(ndet, 1),
                         "three_body": bool(three_body),
                         "ndet_unique": list(wf.fused_device().ndet_s), "walkers": W, "npts": npts, "route": route, "entry": res.get("entry"),
                         "repeat": rep, "seconds": dt, "ms_per_set": 1e3 * dt / npts,
                         "mean_total_first_last": [float(res["total"][0].mean()), float(res["total"][-1].mean())]})
            print(json.dumps(rows[-1]), flush=True)
    return rows


def one_iteration(W, npts, correlatedoptions):
    """Wall clock of the parts of one line_minimization iteration (the driver's own functions, wrapped)."""
    mol = systems.water_cluster()
    wf = pa.generate_wf(mol, systems.random_mf(mol))
    configs = pa.initial_guess(mol, W, rng=np.random.default_rng(2))
    pgrad = gradient_generator(mol, wf, pwf.default_to_opt(wf))
    times = {"warmup_vmc": 0.0, "gradient_vmc": 0.0, "mixture_sampling": 0.0, "correlated_evaluation": 0.0}
    o_vmc, o_sample, o_worker = linemin._vmc, linemin.sm.sample_overlap, linemin.correlated_compute_worker

    def vmc(wf_, coords, accumulators, options):
        t0 = time.perf_counter()
        r = o_vmc(wf_, coords, accumulators, options)
        times["gradient_vmc" if accumulators else "warmup_vmc"] += time.perf_counter() - t0
        return r

    def sample(*a, **k):
        t0 = time.perf_counter()
        r = o_sample(*a, **k)
        times["mixture_sampling"] += time.perf_counter() - t0
        return r

    def worker(*a, **k):
        t0 = time.perf_counter()
        r = o_worker(*a, **k)
        times["correlated_evaluation"] += time.perf_counter() - t0
        times["route"] = r["route"]
        return r

    linemin._vmc, linemin.sm.sample_overlap, linemin.correlated_compute_worker = vmc, sample, worker
    try:
        t0 = time.perf_counter()
        linemin.line_minimization(wf, configs, pgrad, max_iterations=1, npts=npts, vmcoptions=dict(nblocks=10, nsteps_per_block=1, tstep=0.3),
                                  warmup_options=dict(nblocks=1, nsteps_per_block=10, tstep=0.3), correlatedoptions=dict(correlatedoptions))
        total = time.perf_counter() - t0
    finally:
        linemin._vmc, linemin.sm.sample_overlap, linemin.correlated_compute_worker = o_vmc, o_sample, o_worker
    row = {"what": "line_minimization, one iteration", "system": "(H2O)8", "walkers": W, "npts": npts,
           "options": "warm-up 10 sweeps; gradient VMC 10 blocks x 1 sweep; mixture %d block(s) x %d sweeps"
           % (correlatedoptions["nblocks"], correlatedoptions["nsteps"]), "seconds_total": total,
           **{"seconds_" + k: v for k, v in times.items() if k != "route"}, "route": times.get("route")}
    print(json.dumps(row), flush=True)
    return [row]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--walkers", type=int, nargs="+", default=None)
    ap.add_argument("--npts", type=int, default=40)
    ap.add_argument("--fused-only", action="store_true")
    ap.add_argument("--ndet", type=int, default=0)
    ap.add_argument("--system", choices=["water", "cluster"], default="water")
    ap.add_argument("--repeats", type=int, default=2)
    ap.add_argument("--three-body", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "linemin_bench.jsonl"))
    a = ap.parse_args()
    if a.walkers is None:
        a.walkers = [2048, 16384] if a.three_body else [16384, 65536]
    rows = []
    if a.ndet > 0 or a.three_body:
        for W in a.walkers:
            rows += correlated_md(W, a.npts, a.ndet, a.system, a.fused_only, a.repeats, a.three_body)
        if a.out:
            with open(a.out, "a") as f:
                for r in rows:
                    f.write(json.dumps(r) + "\n")
        return
    for W in a.walkers:
        rows += correlated(W, a.npts, a.fused_only)
    if not a.fused_only:
        # this package's default mixture sampling, and the reference's effective one (it drops correlatedoptions: 10 x 10 sweeps)
        for co in (dict(nsteps=3, nblocks=1), dict(nsteps=10, nblocks=10)):
            rows += one_iteration(min(a.walkers), a.npts, co)
    if a.out:
        with open(a.out, "w") as f:
            for r in rows:
                f.write(json.dumps(r) + "\n")


if __name__ == "__main__":
    main()
