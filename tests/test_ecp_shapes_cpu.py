"""The inputs of the ECP-shape tests (tests/ecp_shapes.py) test something — on the oracle alone, at the configurations
test_gpu_ecp_shapes.py uses: the cases' start coordinates on step 0 of the ECP tapes and the oracle chain's final coordinates (the device's
to ~1e-9) on the last step.  No GPU.

Measured with the oracle (ECP tape seed 21), smallest over both configurations.  Non-local part per walker at the deterministic mask:
h-atom 3.1e-6, c2-high-l-md 1.3e-5, h-atom-df 2.4e-5, water-f-53 3.7e-4, every other case above 1e-3 (h33s-1917 2.0); smallest
|prob - uniform| at threshold 10 over all cases 5.2e-6 (h36-1917); smallest |row| / A 8.8e-4 (water-f-53).  Yardsticks 1.1e-14 (water-53)
.. 4.9e-13 (water-f-md), 2.2e-16 for the one-orbital cases, 6.7e-10 and 6.7e-8 for water-1e-5 and water-1e-7; the cond(D) * 2.2e-16 floor
is the largest of the three parts everywhere but on w4f-1715 (updated against fresh 1.55e-13).  Under the project's own table the
hydrogen cases' ECP row is bit for bit its local part: their point lists are built and their ratios computed, then multiplied by the
coefficient 0 of the table's l = 0 term.
"""

import numpy as np
import pytest

import ecp_shapes as es
import sweep_shapes as ss
from pyqmc_amd import systems


def _configurations(name):
    """(coordinates, tape step) of the two evaluations of a live case."""
    c = es.case(name)
    return (c.tapes()[0].configs, 0), (es.compute_yardstick(name)["x"], c.ns - 1)


def test_table_differs_in_the_hydrogen_term_alone():
    assert set(es.ECP) == set(systems._ECP)
    for sym in es.ECP:
        assert (es.ECP[sym] == systems._ECP[sym]) == (sym != "H")
    assert es.ECP["H"][1][0] == systems._ECP["H"][1][0] and es.ECP["H"][1][1] == [0, [[], [], [[1.0, 0.5]]]]
    for name in es.PBC_CASES:  # carbon only: the periodic cases run the project's table
        assert es.case(name).mol._ecp == ss.case(name).mol._ecp
    for name in es.LIVE_CASES + es.COND_CASES:
        c = es.case(name)
        assert c.mol._ecp == {k: es.ECP[k] for k in c.mol._ecp} and c.mol.nao() == (ss.table(name)[2] if name in ss.ALL_CASES else 23)
        rot, unif = es.ecp_tapes(name)
        N, k = sum(c.mol.nelec), c.mol.natm
        assert rot.shape == (c.ns, N, k, 3, 3) and unif.shape == (c.ns, N, k, c.W)
        assert np.allclose(rot @ np.swapaxes(rot, -1, -2), np.eye(3), atol=1e-14) and np.allclose(np.linalg.det(rot), 1.0)


@pytest.mark.parametrize("name", es.LIVE_CASES)
def test_inputs_exercise_the_nonlocal_part(name):
    """Deterministic mask: every walker's non-local part is at least 1e-6.  Threshold 10: every walker has points, except in the
    one-electron cases (and c2-high-l-md: ecp_shapes.SPARSE), where at least one walker has points and at least one has none; no
    |prob - uniform| is below 1e-9.  h33s* and
    h36*: pairs beyond the table's range and pairs within it."""
    for x, step in _configurations(name):
        det, thr = es.oracle_at(name, x, -1.0, step), es.oracle_at(name, x, 10.0, step)
        print(f"[ecp_shapes] {name} step {step}: min non-local {np.abs(det['nonlocal']).min():.3g}, points {det['points'].min()} | "
              f"{thr['points'].min()} .. {thr['points'].max()}, min tie {thr['min_tie']:.3g}, pairs out / in {det['pairs_out']} / {det['pairs_in']}, "
              f"min |row| / A {np.min(np.abs(det['row']) / det['A']):.3g}")
        assert np.abs(det["nonlocal"]).min() >= 1e-6
        assert np.all(det["points"] == det["points"][0]) and det["points"][0] > 0  # every point of every pair
        if name in es.ONE_ELECTRON + es.SPARSE:
            assert (thr["points"] > 0).any() and (thr["points"] == 0).any()
        else:
            assert (thr["points"] > 0).all()
        assert thr["min_tie"] >= 1e-9
        if name in es.RANGE_CASES:
            assert det["pairs_out"] > 0 and det["pairs_in"] > 0
        if name in es.ONE_ELECTRON:
            assert det["pairs_out"] == 0 and np.array_equal(det["points"], det["points_seen"])
        assert np.all(det["points_seen"] <= det["points"]) and np.array_equal(thr["points"], thr["points_seen"])


@pytest.mark.parametrize("name", es.LIVE_CASES + es.COND_CASES)
def test_yardstick_is_the_oracles_own_error(name):
    """(a) updated against fresh, (b) permuted columns, (c) cond(D) * 2.2e-16: each is far below the size of a term, and the
    conditioning cases are the ill-conditioned ones."""
    y = es.compute_yardstick(name)
    print(f"[ecp_shapes] {name}: updated {y['updated']:.3g}, permuted {y['permuted']:.3g}, cond {y['cond']:.3g}, yardstick {y['yardstick']:.3g}")
    assert y["yardstick"] == max(y["updated"], y["permuted"], y["cond"] * es.EPS) == es.yardstick(name)
    assert y["yardstick"] < 1e-6
    if name in es.COND_CASES:
        assert y["cond"] > 1e6
    if name in es.ONE_ELECTRON:
        assert y["permuted"] == 0 and y["cond"] == 1  # one orbital: nothing to permute, the floor is one rounding


@pytest.mark.parametrize("name", es.HYDROGEN_CASES)
def test_project_table_leaves_hydrogen_cases_blind(name):
    """With the project's own hydrogen table the oracle's ECP row is exactly its local part, at the deterministic mask, where every
    ratio is computed (three walkers: the statement does not depend on their number)."""
    c = es.case(name)
    assert name.startswith("h") and set(c.mol._names) == {"H"}
    rot, unif = es.ecp_tapes(name)
    cfg = c.configs(c.tapes()[0].configs[:3])
    o = es.oracle_ecp(c, cfg, -1.0, rot[0], unif[0][..., :3], mol=es.with_table(c.mol, systems._ECP))
    assert o["points"].min() > 0 and np.array_equal(o["row"], o["local"]) and np.any(o["local"] != 0)
    t = es.oracle_ecp(c, cfg, -1.0, rot[0], unif[0][..., :3])
    assert np.array_equal(t["local"], o["local"]) and np.abs(t["row"] - t["local"]).min() >= 1e-6


def test_periodic_fixture_belongs_to_these_inputs():
    """cubic-f regenerated live (the oracle's ECP rows at the coordinates g52 stores; ~10 s with the chain of the yardstick left out)
    equals the fixture: point counts exactly, rows, local part and A to what two evaluation orders differ by."""
    g = ss.oracle_case("cubic-f")
    for thr in es.THRESHOLDS:
        o, f = es.oracle_at("cubic-f", g["x"], thr, 0, g["wrap"]), es.pbc_oracle("cubic-f", thr)
        assert np.array_equal(o["points"], f["points"]) and np.array_equal(o["points_seen"], f["points_seen"])
        assert es.measure(f["row"], o) < 1e-12 and np.max(np.abs(o["A"] / f["A"] - 1)) < 1e-12 and np.max(np.abs(o["local"] - f["local"])) < 1e-12
        assert (o["points"] > 0).all() and (thr < 0 or o["min_tie"] >= 1e-9)
    assert 0 < es.yardstick("cubic-f") < 1e-10 and 0 < es.yardstick("c3-f") < 1e-10
    assert np.iscomplexobj(es.pbc_oracle("c3-f", 10.0)["row"]) and not np.iscomplexobj(es.pbc_oracle("cubic-f", 10.0)["row"])
