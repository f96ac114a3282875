"""The Laplacian component of k_sweep_r8's contraction (two v_mfma_f64_4x4x4_4b_f64 per k-step beside the two 16x16x4 of the value and
gradient components) against the launch-per-move sweep, which forms its orbital rows in k_orb."""
import numpy as np
import pytest

from tests import helpers
from pyqmc_amd import systems

pytestmark = pytest.mark.gpu

# Largest max |a - b| / max(1, |a|) over the cases below with the sixteen-row Laplacian MFMA this kernel had before, measured with that
# build on an MI355X (the two sweeps add the orbital rows' K terms in different orders): ke 2.759e-15 (cluster-8), grad2 1.953e-14
# (cluster-13).  The bounds are twice that.
PARENT_KE, PARENT_GRAD2 = 2.759e-15, 1.953e-14
CASES = {
    "cluster-8": (systems.water_cluster, 8),    # the headline system, one full block of 8 walkers (two orbital tiles, K split two ways)
    "cluster-13": (systems.water_cluster, 13),  # a partly filled second block: shadow walkers store nothing
    "water-13": (systems.water, 13),            # 4 orbitals per spin: one tile, K split four ways; 23 AOs, not a multiple of 4 (a zero row pads
                                                # the tile, and waves 2, 3 clamp their last k-step); the cluster's 184 AOs leave no padding row
}


def _run(make, W, res, monkeypatch):
    import pyqmc_amd as pa

    monkeypatch.setenv("PQA_RES", res)  # read when the handle is created
    monkeypatch.setenv("PQA_R8", "1")
    mol = make()
    wf = helpers.gpu_wf(mol, systems.random_mf(mol))
    dev = wf.fused_device()
    wf.recompute(pa.initial_guess(mol, W, rng=np.random.default_rng(11)))
    acc, _, rec = dev.vmc_sweeps(0.3, 2, seed=21, energy=True, record=True)
    return {"rec": rec, "acc": np.asarray(acc), "x": dev.configs(), "en": np.real(dev.energy())}


@pytest.mark.parametrize("case", list(CASES))
def test_r8_laplacian_rows_against_the_launch_per_move_sweep(case, monkeypatch):
    """Two VMC sweeps through k_sweep_r8 (PQA_RES=1, PQA_R8=1) and through the launch-per-move sweep (PQA_RES=0) on the same seeds: every
    decision equal, the coordinates equal to rounding (the bound of test_resident_sweep_against_the_launch_per_move_sweep: the drift takes
    the gradient rows, whose K terms the two sweeps add in different orders — 2.3e-14 bohr before and after this kernel's change), the
    per-walker kinetic energy (from the Laplacian rows the sweep leaves in the row cache) and grad2
    within twice what the kernel showed against the same target before the Laplacian moved to the 4x4x4 MFMAs."""
    make, W = CASES[case]
    a = _run(make, W, "0", monkeypatch)
    b = _run(make, W, "1", monkeypatch)
    rel = lambda k: float(np.max(np.abs(a["en"][k] - b["en"][k]) / np.maximum(1.0, np.abs(a["en"][k]))))
    dke, dg2, dx = rel(0), rel(4), float(np.max(np.abs(a["x"] - b["x"])))
    print(f"[r8_laplacian] {case}: ke {dke:.3e} grad2 {dg2:.3e} max|dx| {dx:.3e} max|ke| {np.max(np.abs(a['en'][0])):.3e}")
    assert np.array_equal(a["rec"], b["rec"]) and np.array_equal(a["acc"], b["acc"])
    assert float(np.max(np.abs(a["x"] - b["x"]) / np.maximum(1.0, np.abs(a["x"])))) < 1e-10
    assert dke <= 2 * PARENT_KE
    assert dg2 <= 2 * PARENT_GRAD2
