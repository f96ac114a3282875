"""The oracle's ECP rows of the periodic sweep-shape cases -> g53_ecp_shapes.npz (about a minute of CPU, one process per case; the open,
multi-determinant and conditioning cases run live in the tests).

    python tests/golden/make_golden_ecp_shapes.py

Oracle only (tests/ecp_shapes.py: compute_pbc_case).  Keys "<case>/...": per case the yardstick of its ECP row with its three parts
(updated against fresh, permuted columns, cond(D)) and, per mask ("det": every point, "thr10": threshold 10), at the final coordinates and
wrap counters that g52_sweep_shapes.npz stores for the oracle's chain: the fresh oracle's ECP row (complex for c3-f), its local part, the
absolute sum A of its terms and the point counts.  The ECP tapes are regenerated from their seed (ecp_shapes.ecp_tapes) and not stored;
g52 is read, not regenerated.
"""

import concurrent.futures
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

import numpy as np  # noqa: E402

import ecp_shapes  # noqa: E402


def main():
    keep = {}
    with concurrent.futures.ProcessPoolExecutor(max_workers=min(2, os.cpu_count() or 1)) as pool:
        for out in pool.map(ecp_shapes.compute_pbc_case, ecp_shapes.PBC_CASES):
            keep.update(out)
    path = os.path.join(HERE, ecp_shapes.FIXTURE + ".npz")
    np.savez_compressed(path, **keep)
    print(path, os.path.getsize(path), "bytes")
    for k, v in keep.items():
        if np.ndim(v) == 0:
            print(f"  {k} = {v}")


if __name__ == "__main__":
    main()
