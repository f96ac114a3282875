"""The oracle side of the conditioning tests' fixture cases -> g50_conditioning.npz (the cluster case, about 20 s) and
g51_conditioning_pbc.npz (the six periodic cases and the two periodic DMC chains: about 40 minutes of CPU, 6 minutes on eight processes; the
molecular cases run live in the tests).

    python tests/golden/make_golden_conditioning.py [g50|g51]

Oracle only (tests/conditioning.py: oracle_run, permuted_run, combine_runs).  g50: (H2O)8 with occupied orbitals 0 and 1 of each spin
parallel up to 1e-5, 13 walkers, 12 sweeps without a recompute, every proposal of sweep 3 accepted.  g51, keys "<case>/<key>": diamond
at Gamma, twisted, 3x1x1 with complex coefficients, 2x2x2, and the conventional cell real and twisted (conditioning.PBC_CASES), columns 0
and 1 of k-point 0 parallel up to 1e-5.
Stored per case: the decisions, the final (folded) coordinates and for g51 the wrap counters, the oracle's own chain
errors (inverse, log, max |q0 - 1|, for complex cases the phase of Psi and its error) and cond(D), its updated-against-fresh kinetic rows,
the smallest unforced |ratio - u|, the smallest
forced ratio, and what a second oracle run with the occupied columns permuted differs by (final coordinates, ratios of the chain errors,
decisions equal or not).  The tapes are regenerated from their seeds (conditioning.tapes) and not stored.  Under "dmc/" and "dmc_cubic/": the
oracle side of the periodic DMC chains (conditioning.oracle_pbc_dmc: gamma-1e-5, 30 steps, and cubic-1e-5, 12 steps, on seeded host tapes,
each run twice, and once cut short for the wrap counters the CPU test reproduces).  The eighteen runs of g51 are independent and are spread
over up to eight processes.
"""

import concurrent.futures
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

import numpy as np  # noqa: E402

import conditioning  # noqa: E402


def _run(task):
    name, permuted = task
    if name.startswith("dmc:"):  # permuted: False, True, or "first" for the run cut short
        case = name[4:]
        if permuted == "first":
            return conditioning.oracle_pbc_dmc(case, nsteps=conditioning.pbc_dmc_first(case))
        return conditioning.oracle_pbc_dmc(case, permuted)
    r = conditioning.permuted_run(name) if permuted else conditioning.oracle_run(name)
    return {k: v for k, v in r.items() if k not in ("owf", "cfg")}


def _report(path, keep):
    print(path, os.path.getsize(path), "bytes")
    for k, v in keep.items():
        if np.ndim(v) == 0:
            print(f"  {k} = {v}")


def g50():
    o = conditioning.compute_case("cluster-1e-5")
    keep = {k: o[k] for k in conditioning.FIXTURE_KEYS}
    keep["decisions_equal_permuted"] = o["decisions_equal_permuted"]
    path = os.path.join(HERE, conditioning.FIXTURE + ".npz")
    np.savez_compressed(path, **keep)
    _report(path, keep)


def g51():
    tasks = [(n, p) for n in conditioning.PBC_CASES for p in (False, True)] + [("dmc:" + n, p) for n in conditioning.PBC_DMC for p in (False, True, "first")]
    tasks.sort(key=lambda t: t[0] not in ("k222-1e-5", "dmc:cubic-1e-5"))  # the longest runs first
    with concurrent.futures.ProcessPoolExecutor(max_workers=min(8, os.cpu_count() or 1)) as pool:
        runs = dict(zip(tasks, pool.map(_run, tasks)))
    keep = {}
    for name in conditioning.PBC_CASES:
        o = conditioning.combine_runs(name, runs[(name, False)], runs[(name, True)])
        keys = conditioning.PBC_KEYS + (conditioning.COMPLEX_KEYS if conditioning.case(name).complex else ()) + ("decisions_equal_permuted",)
        keep.update({f"{name}/{k}": o[k] for k in keys})
    for name, (prefix, _, _) in conditioning.PBC_DMC.items():
        o = conditioning.combine_dmc(*(runs[("dmc:" + name, p)] for p in (False, True, "first")))
        keep.update({f"{prefix}/{k}": o[k] for k in conditioning.PBC_DMC_KEYS})
    path = os.path.join(HERE, conditioning.PBC_FIXTURE + ".npz")
    np.savez_compressed(path, **keep)
    _report(path, keep)


if __name__ == "__main__":
    which = sys.argv[1:] or ["g50", "g51"]
    if "g50" in which:
        g50()
    if "g51" in which:
        g51()
