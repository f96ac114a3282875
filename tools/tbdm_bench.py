"""Two-body density matrix timing, fused route against protocol route: one JSON line per configuration, appended to
profiles/tbdm_bench.jsonl with --record.

    python tools/tbdm_bench.py [--configs C2,M4096,M,MD50,K222,C3,CX311,C4,M4096J3] [--reps 7] [--routes fused,protocol] [--protocol-budget-s 90] [--record]

Per configuration and route: wall-clock milliseconds per ``TBDMAccumulator.__call__`` (nsweeps = 4, 8 orbitals per spin, sector
(up, down)) — the auxiliary walks, the orbitals at the electrons, the four sweeps and the fetch of the result, which ends with a
stream synchronisation.  Two warm-up calls (the first also warms the walks up), then ``reps`` timed calls: median, minimum, maximum
and spread = (max - min) / median.  The protocol route at more than 4 096 walkers runs only when 16 x its 4 096-walker time fits
--protocol-budget-s; otherwise the record says that it was left out for time.  The library is used as built (no build on import).
C3 (the twisted 8-atom diamond cell of tools/config_bench.py, 16 + 16 electrons) and CX311 (the complex 3 x 1 x 1 cell, 12 + 12), built
as tools/obdm_bench.py builds them, are complex handles with the evaluator's orbitals from the k-point mean field (two of every k-point):
their fused route is ``complex_device=True`` (``pqa_tbdm_sweep_c``).  For them ``__call__`` and ``avg`` are timed with the two routes
alternating call by call in one process, after their results from equal seeds were found equal at the bound of
tests/test_gpu_tbdm_complex.py; the rows carry ``"complex": true`` and say whether the routes' [min, max] intervals are disjoint.
C4 (BASELINE's 50 determinants x two-body x three-body water molecule, 2 048 walkers) and M4096J3 ((H2O)8 with ``jastrow3=True``, 4 096
walkers) are three-body handles: their fused route is ``three_body_device=True`` (``pqa_tbdm_sweep_j3``); they are timed like the
complex configurations and their rows carry ``"three_body": true``.
The kernel split comes from a ``rocprofv3 --kernel-trace --stats`` run of this tool with --routes fused --reps 3.
"""

import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.environ.get("TBDM_BENCH_TREE", ROOT))  # (another checkout of the package: the parent commit's protocol route)

HBM_BYTES_PER_S = 8.0e12  # MI355X HBM3E peak
F64_VECTOR_FLOPS = 78.6e12  # MI355X fp64 vector peak
NORB, NSWEEPS = 8, 4


def build(name):
    """(mol, wf, walkers, TBDMAccumulator keyword arguments)"""
    from pyqmc_amd import systems
    from tests import helpers

    def open_orbitals(mol):
        C = np.asarray(systems.random_mf(mol, seed=5, nvirt=NORB).mo_coeff)
        return dict(orb_coeff=[C[0][:, :NORB], C[1][:, :NORB]])

    if name in ("M", "M4096"):
        mol = systems.water_cluster()
        return mol, helpers.gpu_wf(mol, systems.random_mf(mol)), 65536 if name == "M" else 4096, open_orbitals(mol)
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
    if name == "K222":  # diamond, 2 x 2 x 2 primitive cells: 8 k-points, one orbital of each
        sup, wf = helpers.gpu_pbc_wf("k222")
        _, kmf = helpers.pbc_slater_case("k222")
        kpts = np.asarray(kmf.kpts)
        per_k = NORB // len(kpts)
        return sup, wf, 4096, dict(orb_coeff=[np.asarray(kmf.mo_coeff[0][k])[:, :per_k] for k in range(len(kpts))], kpts=kpts)
    if name in ("C3", "CX311"):  # complex handles: two orbitals of every k-point of the mean field (8 / 6 orbitals)
        from pyqmc_amd import pbc

        if name == "C3":
            sup = pbc.get_supercell(systems.diamond_primitive(), np.array([[-1.0, 1, 1], [1, -1, 1], [1, 1, -1]]))
            kmf = pbc.random_kmf(sup, complex_coeff=True, twist=(0.25, 0.1, -0.3), nvirt=4)
        else:
            sup = pbc.get_supercell(systems.diamond_primitive(), np.diag([3.0, 1.0, 1.0]))
            kmf = pbc.random_kmf(sup, complex_coeff=True, nvirt=4)
        sup, wf = helpers.gpu_pbc_wf(name, case=(sup, kmf))
        kpts = np.asarray(kmf.kpts)
        per_k = max(1, NORB // len(kpts))
        return sup, wf, 4096, dict(orb_coeff=[np.asarray(kmf.mo_coeff[0][k])[:, :per_k] for k in range(len(kpts))], kpts=kpts, complex_device=True)
    raise KeyError(name)


def shapes_model(dev, W):
    """(bytes, flops) of the fused route's own kernels for one sweep, from the shapes: inverses, coordinates and the two orbital rows
    read, the ratios written by k_tbdm_pairs and read back by k_tbdm_acc; the inverse products, the Jastrow pairs (~60 flops per basis
    function and pair) and the combination.  The orbital pass is the orbital kernel's own roofline and is counted in neither."""
    nu, nd = dev.nelec
    N = nu + nd
    nds, nb = dev.ndet_s, 4
    by = W * 8 * (nds[0] * nu * nu + nds[1] * nd * nd + 3 * N + 2 * max(dev.nmo) + 2 * nu * nd)
    fl = W * (2 * (nds[0] * nu * nu + nds[1] * nd * nd) + 60 * nb * (2 * N * N + nu * nd) + 4 * dev.ndet * nu * nd)
    return by, fl


def time_route(pa, mol, wf, configs, kw, route, reps):
    extra = {} if route is None else {"route": route}  # (route None: a tree without the keyword, the parent commit)
    acc = pa.TBDMAccumulator(mol, spin=(0, 1), nsweeps=NSWEEPS, warmup=20, **kw, **extra)
    np.random.seed(11)
    ms = []
    for r in range(reps + 2):
        t0 = time.perf_counter()
        acc(configs, wf)
        if r >= 2:
            ms.append((time.perf_counter() - t0) * 1e3)
    med = float(np.median(ms))
    return {"ms": med, "min_ms": float(min(ms)), "max_ms": float(max(ms)), "spread": float((max(ms) - min(ms)) / med), "reps": reps,
            "route_taken": getattr(acc, "last_route", "protocol")}


def accumulator_c(pa, mol, kw, route):
    """The accumulator of the configurations behind an opt-in flag: the fused route is complex_device=True / three_body_device=True, the
    protocol route does not need the keyword."""
    if route == "protocol":
        kw = dict({k: v for k, v in kw.items() if k not in ("complex_device", "three_body_device")}, route="protocol")
    else:
        kw = dict(kw, route="fused")
    return pa.TBDMAccumulator(mol, spin=(0, 1), nsweeps=NSWEEPS, warmup=20, **kw)


def check_equal(pa, mol, wf, configs, kw):
    """Worst deviations of the fused route from the protocol route at equal seeds; raises beyond the tests' bound.  Three-body
    configurations record the figures and go on (``beyond_bound``): (H2O)8 at 4 096 walkers exceeds the bound in ``__call__``'s
    per-walker values, and the protocol route is the only yardstick these handles have (DESIGN 45 says what is known about it)."""
    out = {}
    for route in ("fused", "protocol"):  # (the protocol route last: its moves there and back leave round-off in the state)
        acc = accumulator_c(pa, mol, kw, route)
        np.random.seed(7)
        out[route] = (acc(configs, wf), acc.avg(configs, wf))
    err = lambda a, b: float(np.max(np.abs(a - b) / (1 + np.abs(b))))  # noqa: E731
    worst = {f"{m}_{k}": err(out["fused"][i][k], out["protocol"][i][k]) for i, m in enumerate(("call", "avg")) for k in ("value", "norm_a", "norm_b")}
    if max(worst.values()) >= 1e-10:
        if not kw.get("three_body_device"):
            raise RuntimeError(f"the routes disagree: {worst}")
        worst["beyond_bound"] = True
    return worst


def run_complex(pa, name, mol, wf, configs, W, kw, reps, routes):
    """C3 / CX311 / C4 / M4096J3: the routes alternate call by call in one process, ``__call__`` and ``avg``, after the seeded results
    were found equal."""
    dev = wf.fused_device()
    rec = {"config": name, "walkers": W, "nelec": list(dev.nelec), "ndet": dev.ndet, "nsweeps": NSWEEPS,
           "norb": sum(np.asarray(c).shape[1] for c in kw["orb_coeff"]) if "kpts" in kw else NORB, "sector": [0, 1],
           "complex": bool(kw.get("complex_device")), "twisted": bool(dev.twisted), "three_body": bool(dev.has_j3)}
    if "fused" in routes and "protocol" in routes:
        rec["checked"] = check_equal(pa, mol, wf, configs, kw)
    for method in ("call", "avg"):
        accs = {r: accumulator_c(pa, mol, kw, r) for r in routes}
        ms = {r: [] for r in routes}
        np.random.seed(11)
        for r_ in range(reps + 2):
            for r, acc in accs.items():
                t0 = time.perf_counter()
                (acc.avg if method == "avg" else acc)(configs, wf)
                if r_ >= 2:
                    ms[r].append((time.perf_counter() - t0) * 1e3)
        for r in routes:
            med = float(np.median(ms[r]))
            rec.setdefault(r, {})[method] = {"ms": med, "min_ms": float(min(ms[r])), "max_ms": float(max(ms[r])),
                                             "spread": float((max(ms[r]) - min(ms[r])) / med), "reps": reps, "route_taken": accs[r].last_route}
    if "fused" in rec and "protocol" in rec:
        for m in ("call", "avg"):  # the ratio of medians, and whether the two routes' [min, max] intervals are disjoint
            f, p = rec["fused"][m], rec["protocol"][m]
            rec["speedup_" + m] = p["ms"] / f["ms"]
            rec["beyond_spread_" + m] = bool(f["max_ms"] < p["min_ms"] or p["max_ms"] < f["min_ms"])
    return rec


def run(name, reps, routes, budget_s, small_protocol_ms):
    import pyqmc_amd as pa

    mol, wf, W, kw = build(name)
    dev = wf.fused_device()
    configs = pa.initial_guess(mol, W, rng=np.random.default_rng(1))
    if hasattr(mol, "a"):
        from pyqmc_amd.configs import PeriodicConfigs

        configs = PeriodicConfigs(configs.configs, mol.lattice_vectors())
    wf.recompute(configs)
    if kw.get("complex_device") or kw.get("three_body_device"):
        return run_complex(pa, name, mol, wf, configs, W, kw, reps, [r for r in routes if r in ("fused", "protocol")])
    rec = {"config": name, "walkers": W, "nelec": list(dev.nelec), "ndet": dev.ndet, "nsweeps": NSWEEPS, "norb": NORB, "sector": [0, 1]}
    if "fused" in routes:
        rec["fused"] = time_route(pa, mol, wf, configs, kw, "fused", reps)
        by, fl = shapes_model(dev, W)
        rec["model_bytes_per_sweep"], rec["model_flops_per_sweep"] = by, fl
        rec["model_floor_ms_per_call"] = NSWEEPS * max(by / HBM_BYTES_PER_S, fl / F64_VECTOR_FLOPS) * 1e3
    for route in [r for r in routes if r != "fused"]:
        key = "protocol" if route == "protocol" else "parent"
        if W > 4096 and small_protocol_ms is not None and small_protocol_ms * (W / 4096) * (min(reps, 2) + 2) * 1e-3 > budget_s:
            rec[key] = {"skipped": "time", "projected_ms_per_call": small_protocol_ms * W / 4096}
            continue
        rec[key] = time_route(pa, mol, wf, configs, kw, "protocol" if route == "protocol" else None, reps if W <= 4096 else min(reps, 2))
    if "fused" in rec and "ms" in rec.get("protocol", {}):
        rec["speedup"] = rec["protocol"]["ms"] / rec["fused"]["ms"]
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--configs", default="C2,M4096,M,MD50,K222")
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--routes", default="fused,protocol", help="fused, protocol, parent (a tree without the route keyword: TBDM_BENCH_TREE)")
    ap.add_argument("--protocol-budget-s", type=float, default=90.0)
    ap.add_argument("--record", action="store_true", help="append the lines to profiles/tbdm_bench.jsonl")
    a = ap.parse_args()
    small = None
    for name in a.configs.split(","):
        rec = run(name, a.reps, a.routes.split(","), a.protocol_budget_s, small)
        if name == "M4096":
            small = (rec.get("protocol") or rec.get("parent") or {}).get("ms")
        line = json.dumps(rec)
        print(line, flush=True)
        if a.record:
            with open(os.path.join(ROOT, "profiles", "tbdm_bench.jsonl"), "a") as f:
                f.write(line + "\n")


if __name__ == "__main__":
    main()
