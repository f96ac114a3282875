"""One-body density matrix timing, fused route against protocol route: one JSON line per configuration, appended to
profiles/obdm_bench.jsonl with --record.

    python tools/obdm_bench.py [--configs C2,M4096,M,MD50,K222,C3,CX311,C4,M4096J3] [--reps 7] [--routes fused,protocol] [--protocol-budget-s 90]
                               [--driver 16384,65536] [--driver-complex 8192,16384] [--record]

Per configuration and route: wall-clock milliseconds per ``OBDMAccumulator.avg`` and per ``OBDMAccumulator.__call__`` (nsweeps = 5,
spin = 0, 32 orbitals) — the auxiliary walk, the orbitals at the electrons, the five sweeps and the fetch of the result, which ends
with a stream synchronisation.  Before the timing the two routes' results from equal seeds are compared at the bounds of
tests/test_gpu_obdm_fused.py.  Two warm-up calls (the first also warms the walk up), then ``reps`` timed calls: median, minimum,
maximum and spread = (max - min) / median; the routes alternate call by call.  ``fused_device`` is the fused route with
``rng="device"``.  The protocol route at more than 4 096 walkers runs only when 16 x its 4 096-walker time fits --protocol-budget-s;
otherwise the record says that it was left out for time.  ``--driver``: one 10-sweep ``vmc_worker`` block with {energy, rdm1_up,
rdm1_down} of (H2O)8 on the resident and on the host driver path at those walker counts.  The library is used as built (no build on
import); another checkout of the package (the parent commit's accumulator) is timed with OBDM_BENCH_TREE and --routes parent.
C3 (the twisted 8-atom diamond cell of tools/config_bench.py, 16 + 16 electrons) and CX311 (the complex 3 x 1 x 1 cell) are complex
handles with the evaluator's orbitals from the k-point mean field: their fused route is ``complex_device=True`` (``pqa_obdm_sweeps_c``),
and ``--driver-complex`` runs the {energy, rdm1_up} block on C3.
C4 (BASELINE's 50 determinants x two-body x three-body water molecule, 2 048 walkers) and M4096J3 ((H2O)8 with ``jastrow3=True``, 4 096
walkers) are three-body handles: their fused route is ``three_body_device=True`` (``pqa_obdm_sweeps_j3``).
The kernel split comes from a ``rocprofv3 --kernel-trace --stats`` run of this tool with --routes fused --reps 3.
"""

import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.environ.get("OBDM_BENCH_TREE", ROOT))

HBM_BYTES_PER_S = 8.0e12  # MI355X HBM3E peak
F64_VECTOR_FLOPS = 78.6e12  # MI355X fp64 vector peak
F64_MATRIX_FLOPS = 78.6e12  # MI355X fp64 matrix peak
NORB, NSWEEPS = 32, 5


def build(name):
    """(mol, wf, walkers, OBDMAccumulator keyword arguments)"""
    from pyqmc_amd import systems
    from tests import helpers

    def open_orbitals(mol):
        C = np.asarray(systems.random_mf(mol, seed=5, nvirt=NORB).mo_coeff)[0]
        if C.shape[1] < NORB:  # (a basis smaller than 32 functions: any 32 combinations of it)
            C = 0.4 * np.random.default_rng(5).standard_normal((C.shape[0], NORB))
        return dict(orb_coeff=C[:, :NORB])

    if name in ("M", "M4096", "M16384"):
        mol = systems.water_cluster()
        W = {"M": 65536, "M4096": 4096, "M16384": 16384}[name]
        return mol, helpers.gpu_wf(mol, systems.random_mf(mol)), W, open_orbitals(mol)
    if name == "C2":
        mol = systems.water()
        return mol, helpers.gpu_wf(mol, systems.random_mf(mol)), 4096, open_orbitals(mol)
    if name == "MD50":
        mol = systems.water()
        mf = systems.random_mf(mol, nvirt=6)
        return mol, helpers.gpu_wf(mol, mf, systems.random_determinants(mol, mf, 50)), 2048, open_orbitals(mol)
    if name == "C4":
        mol = systems.water()
        mf = systems.random_mf(mol, nvirt=6)
        return mol, helpers.gpu_wf3(mol, mf, systems.random_determinants(mol, mf, 50)), 2048, dict(open_orbitals(mol), three_body_device=True)
    if name == "M4096J3":
        mol = systems.water_cluster()
        return mol, helpers.gpu_wf3(mol, systems.random_mf(mol)), 4096, dict(open_orbitals(mol), three_body_device=True)
    if name == "K222":  # diamond, 2 x 2 x 2 primitive cells: 8 k-points, four orbitals of each
        sup, wf = helpers.gpu_pbc_wf("k222")
        _, kmf = helpers.pbc_slater_case("k222")
        kpts = np.asarray(kmf.kpts)
        per_k = NORB // len(kpts)
        return sup, wf, 4096, dict(orb_coeff=[np.asarray(kmf.mo_coeff[0][k])[:, :per_k] for k in range(len(kpts))], kpts=kpts)
    if name in ("C3", "CX311"):  # complex handles: eight orbitals of every k-point of the mean field (32 / 24 orbitals)
        from pyqmc_amd import pbc

        if name == "C3":
            sup = pbc.get_supercell(systems.diamond_primitive(), np.array([[-1.0, 1, 1], [1, -1, 1], [1, 1, -1]]))
            kmf = pbc.random_kmf(sup, complex_coeff=True, twist=(0.25, 0.1, -0.3), nvirt=4)
        else:
            sup = pbc.get_supercell(systems.diamond_primitive(), np.diag([3.0, 1.0, 1.0]))
            kmf = pbc.random_kmf(sup, complex_coeff=True, nvirt=4)
        sup, wf = helpers.gpu_pbc_wf(name, case=(sup, kmf))
        kpts = np.asarray(kmf.kpts)
        orb = [np.asarray(kmf.mo_coeff[0][k])[:, :8] for k in range(len(kpts))]
        return sup, wf, 4096, dict(orb_coeff=orb, kpts=kpts, complex_device=True)
    raise KeyError(name)


def shapes_model(dev, W, ne, norb):
    """(bytes, flops) per sweep of k_obdm_rt and of the mean product, from the shapes.  k_obdm_rt reads the spin's inverses, the
    coordinates, the orbital row at r', the ne x norb orbitals at the electrons and the kept row, and writes three panel rows; it
    spends 2 flops per inverse entry, ~60 per Jastrow basis function and pair (2 N pairs per listed electron) and 2 ne norb on t.
    The mean product reads the panels once per tile column and spends 2 W norb^2 flops on the matrix cores."""
    nu, nd = dev.nelec
    N, nb = nu + nd, 4
    rt_bytes = W * 8 * (dev.ndet_s[0] * nu * nu + 3 * N + max(dev.nmo) + ne * norb + norb + 3 * norb)
    rt_flops = W * (2 * dev.ndet_s[0] * nu * nu + 60 * nb * 2 * N * ne + 2 * ne * norb + 2 * dev.ndet * ne)
    tiles = (norb + 15) // 16
    mean_bytes = W * 8 * norb * (2 * tiles + 1)
    mean_flops = 2 * W * norb * norb
    return {"rt_bytes": rt_bytes, "rt_flops": rt_flops, "mean_bytes": mean_bytes, "mean_flops": mean_flops,
            "rt_floor_ms": max(rt_bytes / HBM_BYTES_PER_S, rt_flops / F64_VECTOR_FLOPS) * 1e3,
            "mean_floor_ms": max(mean_bytes / HBM_BYTES_PER_S, mean_flops / F64_MATRIX_FLOPS) * 1e3}


def _stats(ms, reps):
    med = float(np.median(ms))
    return {"ms": med, "min_ms": float(min(ms)), "max_ms": float(max(ms)), "spread": float((max(ms) - min(ms)) / med), "reps": reps}


def accumulator(pa, mol, kw, route):
    extra = {"route": "protocol"} if route == "protocol" else {} if route == "parent" else {"route": "fused"}
    if route == "fused_device":
        extra["rng"] = "device"
    if route in ("protocol", "parent"):  # (the parent's accumulator does not know the keyword; the protocol route does not need it)
        kw = {k: v for k, v in kw.items() if k not in ("complex_device", "three_body_device")}
    return pa.OBDMAccumulator(mol, spin=0, nsweeps=NSWEEPS, warmup=20, **kw, **extra)


def check_equal(pa, mol, wf, configs, kw):
    """Worst deviations of the fused route from the protocol route at equal seeds; raises beyond the tests' bounds."""
    out = {}
    for route in ("fused", "protocol"):
        acc = accumulator(pa, mol, kw, route)
        np.random.seed(7)
        out[route] = (acc(configs, wf), acc.avg(configs, wf))
    err = lambda a, b: float(np.max(np.abs(a - b) / (1 + np.abs(b))))  # noqa: E731
    worst = {"call_value": err(out["fused"][0]["value"], out["protocol"][0]["value"]),
             "call_norm": err(out["fused"][0]["norm"], out["protocol"][0]["norm"]),
             "avg_value": err(out["fused"][1]["value"], out["protocol"][1]["value"]),
             "avg_norm": err(out["fused"][1]["norm"], out["protocol"][1]["norm"])}
    if max(worst.values()) >= 1e-10:
        raise RuntimeError(f"the routes disagree: {worst}")
    return worst


def time_routes(pa, mol, wf, configs, kw, routes, reps, method):
    """The routes alternate call by call in one process; ``method``: "avg" or "call"."""
    accs = {r: accumulator(pa, mol, kw, r) for r in routes}
    ms = {r: [] for r in routes}
    np.random.seed(11)
    for rep in range(reps + 2):
        for r, acc in accs.items():
            t0 = time.perf_counter()
            (acc.avg if method == "avg" else acc)(configs, wf)
            if rep >= 2:
                ms[r].append((time.perf_counter() - t0) * 1e3)
    return {r: dict(_stats(ms[r], reps), route_taken=getattr(accs[r], "last_route", "protocol")) for r in routes}


def run(name, reps, routes, budget_s, small_protocol_ms):
    import pyqmc_amd as pa

    mol, wf, W, kw = build(name)
    dev = wf.fused_device()
    configs = pa.initial_guess(mol, W, rng=np.random.default_rng(1))
    if hasattr(mol, "a"):
        from pyqmc_amd.configs import PeriodicConfigs

        configs = PeriodicConfigs(configs.configs, mol.lattice_vectors())
    wf.recompute(configs)
    cplx = bool(kw.get("complex_device"))
    norb = sum(np.asarray(c).shape[1] for c in kw["orb_coeff"]) if "kpts" in kw else NORB
    rec = {"config": name, "walkers": W, "nelec": list(dev.nelec), "ndet": dev.ndet, "nsweeps": NSWEEPS, "norb": norb, "spin": 0,
           "complex": cplx, "twisted": bool(dev.twisted), "three_body": bool(dev.has_j3)}
    slow = [r for r in routes if r in ("protocol", "parent")]
    if W > 4096 and small_protocol_ms is not None and small_protocol_ms * (W / 4096) * 2 * (min(reps, 2) + 3) * 1e-3 > budget_s:
        for r in slow:
            rec[r] = {"skipped": "time", "projected_ms_per_call": small_protocol_ms * W / 4096}
        routes = [r for r in routes if r not in slow]
        rec["checked"] = "left out with the protocol route"
    elif "fused" in routes and "protocol" in routes:
        rec["checked"] = check_equal(pa, mol, wf, configs, kw)
    if W > 4096 and slow and slow[0] in routes:
        reps = min(reps, 2)
    for method in ("avg", "call"):
        for r, v in time_routes(pa, mol, wf, configs, kw, routes, reps, method).items():
            rec.setdefault(r, {})[method] = v
    if any(r.startswith("fused") for r in routes) and not cplx and not dev.has_j3:  # (the model is that of the real two-body kernels)
        rec["model_per_sweep"] = shapes_model(dev, W, dev.nelec[0], NORB)
    if "fused" in rec and "avg" in rec.get("protocol", {}):
        rec["speedup_avg"] = rec["protocol"]["avg"]["ms"] / rec["fused"]["avg"]["ms"]
        rec["speedup_call"] = rec["protocol"]["call"]["ms"] / rec["fused"]["call"]["ms"]
        for m in ("avg", "call"):  # whether the two routes' [min, max] intervals are disjoint
            f, p = rec["fused"][m], rec["protocol"][m]
            rec["beyond_spread_" + m] = bool(f["max_ms"] < p["min_ms"] or p["max_ms"] < f["min_ms"])
    return rec


def run_driver(W, reps, cplx=False):
    """One 10-sweep vmc_worker block of (H2O)8 with {energy, rdm1_up, rdm1_down}: resident path (fused accumulators) against host
    path (protocol accumulators), alternating; the first block of each (which holds the walk's warm-up) is timed on its own.
    ``cplx``: the block of the twisted cell C3 with {energy, rdm1_up}, the resident path through ``complex_device=True``."""
    import pyqmc_amd as pa

    mol, wf, _, kw = build("C3" if cplx else "M4096")
    start = pa.initial_guess(mol, W, rng=np.random.default_rng(1))
    rec = {"config": "driver_C3" if cplx else "driver", "walkers": W, "nsteps": 10, "nsweeps": NSWEEPS,
           "norb": sum(np.asarray(c).shape[1] for c in kw["orb_coeff"]) if cplx else NORB}
    accs = {}
    for path, route in (("resident", "fused"), ("resident_device_rng", "fused_device"), ("host", "protocol")):
        accs[path] = {"energy": pa.EnergyAccumulator(mol), "rdm1_up": accumulator(pa, mol, kw, route)}
        if not cplx:
            accs[path]["rdm1_down"] = pa.OBDMAccumulator(mol, spin=1, nsweeps=NSWEEPS, warmup=20, **kw,
                                                         **({"route": "protocol"} if route == "protocol" else
                                                            {"route": "fused", "rng": "device"} if route == "fused_device" else {"route": "fused"}))
    ms = {p: [] for p in accs}
    np.random.seed(3)
    for rep in range(reps + 1):
        for path, a in accs.items():
            cfg = type(start)(start.configs.copy(), mol.lattice_vectors()) if cplx else pa.OpenConfigs(start.configs.copy())
            t0 = time.perf_counter()
            pa.vmc_worker(wf, cfg, 0.3, 10, a, seed=5)
            ms[path].append((time.perf_counter() - t0) * 1e3)
    for path in accs:
        rec[path] = dict(_stats(ms[path][1:], reps), first_block_ms=ms[path][0])
    rec["speedup"] = rec["host"]["ms"] / rec["resident"]["ms"]
    rec["beyond_spread"] = bool(rec["resident"]["max_ms"] < rec["host"]["min_ms"] or rec["host"]["max_ms"] < rec["resident"]["min_ms"])
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--configs", default="C2,M4096,M,MD50,K222")
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--routes", default="fused,fused_device,protocol",
                    help="fused, fused_device, protocol, parent (a tree without the route keyword: OBDM_BENCH_TREE)")
    ap.add_argument("--protocol-budget-s", type=float, default=90.0)
    ap.add_argument("--driver", default="", help="walker counts of the vmc_worker block, e.g. 16384,65536")
    ap.add_argument("--driver-complex", default="", help="walker counts of the twisted cell's vmc_worker block, e.g. 8192,16384")
    ap.add_argument("--record", action="store_true", help="append the lines to profiles/obdm_bench.jsonl")
    a = ap.parse_args()

    def emit(rec):
        line = json.dumps(rec)
        print(line, flush=True)
        if a.record:
            with open(os.path.join(ROOT, "profiles", "obdm_bench.jsonl"), "a") as f:
                f.write(line + "\n")

    small = None
    for name in [c for c in a.configs.split(",") if c]:
        rec = run(name, a.reps, a.routes.split(","), a.protocol_budget_s, small)
        if name == "M4096":
            small = ((rec.get("protocol") or rec.get("parent") or {}).get("avg") or {}).get("ms")
        emit(rec)
    for W in [int(w) for w in a.driver.split(",") if w]:
        emit(run_driver(W, min(a.reps, 3)))
    for W in [int(w) for w in a.driver_complex.split(",") if w]:
        emit(run_driver(W, min(a.reps, 3), cplx=True))


if __name__ == "__main__":
    main()
