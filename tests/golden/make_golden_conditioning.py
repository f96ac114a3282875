"""The oracle side of the conditioning tests' cluster case -> g50_conditioning.npz (about 20 s; the water cases run live in the tests).

    python tests/golden/make_golden_conditioning.py

Oracle only (tests/conditioning.py: compute_case): (H2O)8 with occupied orbitals 0 and 1 of each spin parallel up to 1e-5, 13 walkers,
12 sweeps without a recompute, every proposal of sweep 3 accepted.  Stored: the decisions, the final coordinates, the oracle's own chain
errors (inverse, log, max |q0 - 1|) and cond(D), its updated-against-fresh kinetic rows, the smallest unforced |ratio - u|, the smallest
forced ratio, and what a second oracle run with the occupied columns permuted differs by (final coordinates, ratios of the chain errors,
decisions equal or not).  The tapes are regenerated from their seeds (conditioning.tapes) and not stored.
"""

import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

import numpy as np  # noqa: E402

import conditioning  # noqa: E402

if __name__ == "__main__":
    o = conditioning.compute_case("cluster-1e-5")
    keep = {k: o[k] for k in conditioning.FIXTURE_KEYS}
    keep["decisions_equal_permuted"] = o["decisions_equal_permuted"]
    path = os.path.join(HERE, conditioning.FIXTURE + ".npz")
    np.savez_compressed(path, **keep)
    print(path, os.path.getsize(path), "bytes")
    for k, v in keep.items():
        if np.ndim(v) == 0:
            print(f"  {k} = {v}")
