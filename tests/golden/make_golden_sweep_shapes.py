"""The oracle side of the periodic sweep-shape cases -> g52_sweep_shapes.npz (about 40 s of CPU, four independent runs on up to four processes;
the open and multi-determinant cases run live in the tests).

    python tests/golden/make_golden_sweep_shapes.py

Oracle only (tests/sweep_shapes.py: oracle_run, combine).  Keys "<case>/<key>": the conventional diamond cell whose carbon table has an f
shell (16 + 16 electrons), real at Gamma-compatible k-points (cubic-f, 160 AOs) and complex with the twist of config C3 (c3-f, the table
s, s, p, f: 96 AOs); 4 walkers,
2 sweeps, every proposal of sweep 1 accepted.  Stored per case: decisions, margins (ratio - u of every move), final folded coordinates
and wrap counters of the run and of a second run with the occupied columns permuted, the oracle's own chain errors (inverse, log, max
|q0 - 1|, for c3-f the phase of Psi and its error), cond(D), its updated-against-fresh kinetic rows, the smallest unforced |ratio - u| and
the acceptance of the unforced sweep.  The tapes are regenerated from their seeds (conditioning.tapes) and not stored.
"""

import concurrent.futures
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

import numpy as np  # noqa: E402

import sweep_shapes  # noqa: E402


def _run(task):
    return sweep_shapes.oracle_run(*task)


def main():
    tasks = [(n, p) for n in sweep_shapes.PBC_CASES for p in (False, True)]
    with concurrent.futures.ProcessPoolExecutor(max_workers=min(4, os.cpu_count() or 1)) as pool:
        runs = dict(zip(tasks, pool.map(_run, tasks)))
    keep = {}
    for name in sweep_shapes.PBC_CASES:
        o = sweep_shapes.combine(name, runs[(name, False)], runs[(name, True)])
        keys = sweep_shapes.PBC_KEYS + (sweep_shapes.COMPLEX_KEYS if sweep_shapes.case(name).complex else ())
        keep.update({f"{name}/{k}": o[k] for k in keys})
    path = os.path.join(HERE, sweep_shapes.FIXTURE + ".npz")
    np.savez_compressed(path, **keep)
    print(path, os.path.getsize(path), "bytes")
    for k, v in keep.items():
        if np.ndim(v) == 0:
            print(f"  {k} = {v}")


if __name__ == "__main__":
    main()
