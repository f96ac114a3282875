"""The inputs of the sweep-shape tests (tests/sweep_shapes.py) are what their table says, and the oracle's chains on them decide nothing
near a tie — so test_gpu_sweep_shapes.py may ask for every decision of every walker.  No GPU.

Smallest unforced |ratio - u| measured with the oracle (tape seed 3, start seed 11): water-f 7.7e-3, water-53 1.3e-3, water-f-53 6.4e-3,
h-atom 3.8e-2, h-atom-df 9.2e-2, h36 7.3e-4, h36-1917 8.1e-5, h33s 1.1e-3, h33s-1917 9.8e-4, w4-1715 8.1e-4, w4f-1715 9.1e-4, water-f-md 3.8e-3,
c2-high-l-md 3.0e-3, cubic-f 7.7e-3, c3-f 2.2e-3 (the periodic two on 4 walkers and 2 sweeps).
"""

import numpy as np
import pytest

import sweep_shapes as ss


@pytest.mark.parametrize("name", list(ss.ALL_CASES))
def test_case_has_the_shape_it_was_built_for(name):
    """Electron counts, atoms, AOs and the highest shell of the basis: the compile-time instantiation, the tile counts per spin and the
    number of ion passes follow from these."""
    c = ss.case(name)
    nelec, natm, nao, lmax, seed = ss.table(name)
    assert tuple(c.mol.nelec) == nelec and c.mol.natm == natm and c.mol.nao() == nao and ss.highest_l(c.mol) == lmax
    assert c.seed == seed == 3  # (a case whose margin falls below 1e-6 gets another tape seed, recorded in its table entry)
    start, gauss, unif, _ = c.tapes()
    N = sum(nelec)
    assert start.configs.shape == (c.W, N, 3) and gauss.shape == (c.ns, N, c.W, 3) and not unif[1].any() and unif[0].all()
    if name in ss.MD_CASES:
        assert len(c.dets) == 6 and np.asarray(c.mf.mo_coeff).shape[2] == 10
    if name in ss.PBC_CASES:
        assert c.periodic and c.complex == (name == "c3-f") and (c.W, c.ns) == (4, 2)
    else:
        assert (c.W, c.ns) == (13, 3)


def test_shapes_reach_the_lines_they_name():
    """What the kernels' host code derives from the shapes (pqa_res8.hip: 16 orbitals per tile, eight atoms per work item, a second ion
    pass above 32 atoms)."""
    tiles = lambda n: (n + 15) // 16
    nt = {n: tuple(tiles(k) for k in ss.case(n).mol.nelec) for n in ss.OPEN_CASES}
    assert nt["w4-1715"] == nt["w4f-1715"] == (2, 1) and nt["h36"] == nt["h36-1917"] == nt["h33s"] == nt["h33s-1917"] == (2, 2)
    assert nt["h-atom"] == nt["h-atom-df"] == (1, 0)
    for n in ("h36", "h36-1917", "h33s", "h33s-1917"):
        natm = ss.case(n).mol.natm
        assert natm > 32 and natm // 8 == 4 and natm % 8 != 0  # four full items and a partial one per shell type
    names = ss.case("w4-1715").mol._names
    assert names.count("O") == 4 and names.count("H") == 8  # half-filled O items
    for n in ss.DEFAULT_ROUTE_CASES:
        assert 16 <= max(ss.case(ss.REPLACEMENT.get((n, "default"), n)).mol.nelec) < 32
    for (n, _), r in ss.REPLACEMENT.items():  # a replacement keeps what its case was built for
        assert (ss.case(n).mol.natm > 32) == (ss.case(r).mol.natm > 32) and nt[n] == nt[r]


@pytest.mark.parametrize("name", list(ss.OPEN_CASES) + list(ss.MD_CASES))
def test_live_oracle_chain_is_far_from_ties(name):
    """No unforced decision of the oracle's chain is within 1e-6 of a tie, the unforced sweeps accept and reject, and the second oracle
    run (occupied columns permuted) takes the same decisions."""
    o = ss.oracle_case(name)
    print(f"[sweep_shapes] {name}: min margin {o['min_margin']:.3g}, acceptance {o['acceptance']:.3f}, cond {o['cond']:.3g}, "
          f"inv {o['inv']:.3g}, log {o['log']:.3g}, q0m1 {o['q0m1']:.3g}, spread_x {o['spread_x']:.3g}")
    assert o["min_margin"] > 1e-6
    assert 0.1 < o["acceptance"] < 1.0
    assert o["decisions"][1].all() and o["decisions_equal_permuted"]
    assert o["spread_x"] < 1e-9 and o["inv"] < 1e-9 and o["q0m1"] < 1e-9
    # the coordinate yardstick is the two runs' difference itself; only a case with one orbital (the same run twice) falls back to a floor
    assert (o["spread_x"] == 0) == (name in ("h-atom", "h-atom-df")) and (ss.yardstick(o, "x") == o["spread_x"]) == (o["spread_x"] > 0)


@pytest.mark.parametrize("name", list(ss.PBC_CASES))
def test_periodic_fixture_is_far_from_ties(name):
    o = ss.oracle_case(name)
    assert o["min_margin"] > 1e-6 and o["min_margin"] == np.abs(o["margins"][0]).min()
    assert 0.1 < o["acceptance"] < 1.0
    assert o["decisions"][1].all() and o["decisions_equal_permuted"] and np.array_equal(o["wrap"], o["wrap_permuted"])
    assert o["spread_x"] == np.max(np.abs(o["x"] - o["x_permuted"])) < 1e-9


def test_periodic_fixture_belongs_to_these_inputs():
    """cubic-f regenerated (one oracle chain, ~10 s) equals the fixture: decisions and wraps exactly, margins and coordinates to what two
    evaluation orders differ by."""
    o, r = ss.oracle_case("cubic-f"), ss.oracle_run("cubic-f")
    assert np.array_equal(r["decisions"], o["decisions"]) and np.array_equal(r["wrap"], o["wrap"])
    assert np.max(np.abs(r["margins"] - o["margins"])) < 1e-9 and np.max(np.abs(r["x"] - o["x"])) < 1e-9
    assert abs(r["cond"] / o["cond"] - 1) < 1e-6
