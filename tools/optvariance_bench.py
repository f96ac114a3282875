"""Variance optimisation timings on one MI355X -> profiles/optvariance_bench.jsonl (one JSON line per measurement).

    python tools/optvariance_bench.py [--walkers 65536] [--maxiter 5] [--fused-only] [--out profiles/optvariance_bench.jsonl]

(H2O)8 with generate_wf's default Jastrow (24 x 5 x 2 + 4 x 3 = 252 two-body coefficients) and small random coefficients:
1. one cost evaluation: fused (pqa_variance, K = 1), fused with the gradient, and protocol (set, recompute, energy pass), each after
   an untimed warm-up call;
2. a full optvariance(..., method="BFGS", options={"maxiter": N}) over wf2acoeff and wf2bcoeff, without jac (scipy's
   forward-difference gradient: P + 1 costs per gradient) and with jac=True: wall time, nfev, the variance reached.
--fused-only: part 1's fused calls only (for a rocprofv3 --kernel-trace --stats run).
"""

import argparse
import contextlib
import importlib
import io
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import scipy.optimize  # noqa: E402

import pyqmc_amd as pa  # noqa: E402
from pyqmc_amd import systems  # noqa: E402
from pyqmc_amd.configs import OpenConfigs  # noqa: E402

ov = importlib.import_module("pyqmc_amd.optvariance")
PARAMS = ["wf2acoeff", "wf2bcoeff"]


def _setup(W):
    mol = systems.water_cluster()
    wf = pa.generate_wf(mol, systems.random_mf(mol))
    rng = np.random.default_rng(11)
    ja = wf.wf_factors[1].parameters
    wf.parameters["wf2acoeff"] = 0.05 * rng.standard_normal(np.shape(ja["acoeff"]))
    wf.parameters["wf2bcoeff"] = np.concatenate([np.asarray(ja["bcoeff"])[:1], 0.05 * rng.standard_normal((np.shape(ja["bcoeff"])[0] - 1, 3))])
    configs = OpenConfigs(systems.initial_guess(mol, W, rng=np.random.default_rng(1)).configs.copy())
    wf.recompute(configs)
    enacc = pa.EnergyAccumulator(mol, seed=5)
    en = enacc(configs, wf)
    return mol, wf, configs, enacc, en["total"] - en["ke"]


def _timed(f, x, reps=5):
    f(x)  # (warm-up)
    t0 = time.perf_counter()
    for _ in range(reps):
        r = f(x)
    return (time.perf_counter() - t0) / reps, r


def one_cost(W, fused_only):
    mol, wf, configs, enacc, eoff = _setup(W)
    x0, shapes = ov.flatten(wf, PARAMS)
    cost, cost_jac = ov._fused_cost(wf, PARAMS, shapes, eoff)
    rows = []
    for what, f in [("fused cost", cost), ("fused cost + gradient", cost_jac)] + ([] if fused_only else [
            ("protocol cost", ov._protocol_cost(enacc, wf, configs, PARAMS, shapes, eoff))]):
        dt, r = _timed(f, x0, reps=5 if "fused" in what else 2)
        v = r[0] if isinstance(r, tuple) else r
        rows.append({"what": what, "system": "(H2O)8", "walkers": W, "P": int(x0.size), "ms": 1e3 * dt, "variance": float(v)})
        print(json.dumps(rows[-1]), flush=True)
    return rows


def bfgs(W, maxiter):
    rows = []
    for jac in (False, True):
        mol, wf, configs, enacc, _ = _setup(W)
        seen = {}
        orig = scipy.optimize.minimize

        def spy(*a, **k):
            res = orig(*a, **k)
            seen["nfev"], seen["nit"] = int(res.nfev), int(res.nit)
            return res

        scipy.optimize.minimize = spy
        try:
            t0 = time.perf_counter()
            with contextlib.redirect_stdout(io.StringIO()):  # (the reference's callback prints every iterate)
                fun, _ = pa.optvariance(enacc, wf, configs, params=PARAMS, method="BFGS", options={"maxiter": maxiter},
                                        **({"jac": True} if jac else {}))
            dt = time.perf_counter() - t0
        finally:
            scipy.optimize.minimize = orig
        rows.append({"what": "optvariance BFGS", "jac": jac, "system": "(H2O)8", "walkers": W, "maxiter": maxiter, "seconds": dt,
                     "nfev": seen["nfev"], "nit": seen["nit"], "variance": float(fun), "route": ov.optvariance_route(wf, PARAMS)})
        print(json.dumps(rows[-1]), flush=True)
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--walkers", type=int, nargs="+", default=[65536])
    ap.add_argument("--maxiter", type=int, default=5)
    ap.add_argument("--fused-only", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "optvariance_bench.jsonl"))
    a = ap.parse_args()
    rows = []
    for W in a.walkers:
        rows += one_cost(W, a.fused_only)
        if not a.fused_only:
            rows += bfgs(W, a.maxiter)
    if a.out and not a.fused_only:
        os.makedirs(os.path.dirname(a.out), exist_ok=True)
        with open(a.out, "w") as f:
            for r in rows:
                f.write(json.dumps(r) + "\n")


if __name__ == "__main__":
    main()
