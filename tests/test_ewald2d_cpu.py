"""Slab Ewald sum on the host (pyqmc_amd.ewald2d): tables and the host route against the reference's values (g46), the Madelung
constants, the scaled weight where the reference's product overflows, invariances, chunking, and SlabEnergyAccumulator.

Largest relative error of the host route over all golden cases, measured: 5.5e-16 in ee and 1.8e-15 in ei (asserted: 1e-12, the
tolerance of the 3D sums)."""

import numpy as np
import pytest

import helpers
from pyqmc_amd import ewald2d, pbc, systems
from pyqmc_amd.configs import PeriodicConfigs, enforce_pbc

CASES = ["a1", "a2", "b", "c", "d", "e"]


def golden_cell(g, name):
    cell = systems.Cell([str(s) for s in g[f"{name}_symbols"]], g[f"{name}_atoms"], g[f"{name}_lattice"], nelec=tuple(g[f"{name}_nelec"]),
                        charges=g[f"{name}_charges"], dimension=2)
    return pbc.get_supercell(cell, np.eye(3))


def _relerr(a, b):
    return float(np.max(np.abs(np.asarray(a) - np.asarray(b)) / np.abs(np.asarray(b))))


@pytest.mark.parametrize("name", CASES)
def test_tables_match_reference(name):
    g = helpers.golden("g46_ewald2d")
    cell = golden_cell(g, name)
    assert cell.dimension == 2
    ew = ewald2d.Ewald(cell, nlatvec=int(g[f"{name}_nlatvec"]))
    assert abs(ew.alpha - float(g[f"{name}_alpha"])) < 1e-14
    assert ew.gpoints.shape == g[f"{name}_gpoints"].shape  # the index box keeps the reference's survivors, in its order
    assert np.max(np.abs(ew.gpoints - g[f"{name}_gpoints"])) < 1e-14
    assert np.max(np.abs(ew.gweight - g[f"{name}_gweight"])) < 1e-13
    assert abs(ew.ewald_ion_ion - float(g[f"{name}_ii"])) < 1e-11 * abs(float(g[f"{name}_ii"]))
    t = ew.tab
    np.testing.assert_allclose(t["gidx"] @ t["recip"], ew.gpoints, rtol=0, atol=1e-14)
    assert len(ew.lattice_displacements) == (2 * int(g[f"{name}_nlatvec"]) + 1) ** 2


@pytest.mark.parametrize("name", CASES)
def test_host_route_matches_reference(name):
    g = helpers.golden("g46_ewald2d")
    cell = golden_cell(g, name)
    ew = ewald2d.Ewald(cell, nlatvec=int(g[f"{name}_nlatvec"]))
    ee, ei, ii = ew.energy(PeriodicConfigs(g[f"{name}_configs"], cell.lattice_vectors()))
    assert ew.last_route == "host"
    print(name, "relerr ee", _relerr(ee, g[f"{name}_ee"]), "ei", _relerr(ei, g[f"{name}_ei"]))
    assert ee.shape == ei.shape == (len(g[f"{name}_configs"]),)
    assert _relerr(ee, g[f"{name}_ee"]) < 1e-12
    assert _relerr(ei, g[f"{name}_ei"]) < 1e-12


@pytest.mark.parametrize("name, answer", [("a1", -1.6155), ("a2", -5.1122)])
def test_madelung_constants(name, answer):
    g = helpers.golden("g46_ewald2d")
    cell = golden_cell(g, name)
    ee, ei, ii = ewald2d.Ewald(cell).energy(PeriodicConfigs(g[f"{name}_configs"], cell.lattice_vectors()))
    assert abs(float(ee[0] + ei[0]) + ii - answer) < 1e-4


def tall_case():
    """Two electrons 850 bohr apart in height in a cell 2000 bohr tall; alpha_scaling = 1 keeps k vectors of norm > 1, so
    k |z| > 850 > 709."""
    cell = systems.Cell(["He"], [(1.0, 2.0, 100.0)], np.array([[6.0, 0, 0], [1.0, 5.0, 0], [0, 0, 2000.0]]), nelec=(1, 1), dimension=2)
    x = np.array([[[0.5, 0.7, 100.0], [2.5, 3.1, 950.0]], [[0.5, 0.7, 100.0], [2.5, 3.1, 101.5]]])
    return pbc.get_supercell(cell, np.eye(3)), x


def test_overflow_of_the_reference_weight_is_avoided():
    cell, x = tall_case()
    ew = ewald2d.Ewald(cell, alpha_scaling=1.0)
    k, alpha, area = ew.gnorm, ew.alpha, ew.cell_area
    z = 850.0
    assert len(k) >= 3 and k.min() * z > 709.8
    with np.errstate(over="ignore", invalid="ignore"):
        from scipy.special import erfc

        naive = np.pi / (area * k) * (np.exp(k * z) * erfc(k / (2 * alpha) + alpha * z) + np.exp(-k * z) * erfc(k / (2 * alpha) - alpha * z))
    assert np.all(np.isnan(naive))  # inf * 0
    w = ewald2d.recip_weight(np.array([z, -z]), k, alpha, area)
    assert np.all(np.isfinite(w)) and np.array_equal(w[0], w[1])
    # large |z|: W -> (2 pi / (A k)) exp(-k |z|); where the naive product is still finite all three agree
    for zz in (300.0, 600.0, 705.0 / k.max()):
        lim = 2 * np.pi / (area * k) * np.exp(-k * zz)
        np.testing.assert_allclose(ewald2d.recip_weight(np.array([zz]), k, alpha, area)[0], lim, rtol=1e-14, atol=0)
    zz = 700.0 / k.max()
    assert alpha * zz - k.max() / (2 * alpha) > 6  # (erfc(a - s) = 2 to rounding)
    with np.errstate(over="ignore"):
        naive = np.pi / (area * k) * (np.exp(k * zz) * erfc(k / (2 * alpha) + alpha * zz) + np.exp(-k * zz) * erfc(k / (2 * alpha) - alpha * zz))
    np.testing.assert_allclose(ewald2d.recip_weight(np.array([zz]), k, alpha, area)[0], naive, rtol=1e-13, atol=0)
    # the energies: finite, and the far pair's reciprocal part is its limit (zero to rounding at k |z| > 850)
    ee, ei, ii = ew.energy(PeriodicConfigs(x, cell.lattice_vectors()))
    assert np.all(np.isfinite(ee)) and np.all(np.isfinite(ei)) and np.isfinite(ii)
    d = x[0, 0] - x[0, 1]
    lim = 2 * np.pi / (area * k) * np.exp(-k * abs(d[2]))
    expect = (ewald2d.real_cij(d, ew.lattice_displacements, alpha) + 2 * np.sum(np.cos(ew.gpoints @ d) * lim)
              + 2 * ewald2d.charge_weight(d[2], alpha, area) + ew.ewald_self(2))
    assert abs(ee[0] - expect) <= 4e-16 * abs(expect)


def test_overflow_with_extra_k_vectors():
    """The same overflow inside a cell 30 bohr tall: k vectors far beyond the weight cut-off, passed in explicitly, and a pair 14 bohr
    apart in height with alpha |z| > k / 2 alpha (the branch erfcx(t) = 2 exp(t^2) - erfcx(-t))."""
    from scipy.special import erfc

    lat = np.array([[5.0, 0.0, 0.0], [1.5, 4.5, 0.0], [0.0, 0.0, 30.0]])
    cell = pbc.get_supercell(systems.Cell(["He"], [(1.0, 2.0, 15.0)], lat, nelec=(1, 1), dimension=2), np.eye(3))
    sel = ewald2d.Ewald(cell, alpha_scaling=8.0)
    extra = np.array([[45, 0], [44, -3], [0, 50]], dtype=np.int32)
    ew = ewald2d.Ewald(cell, alpha_scaling=8.0, gidx=np.concatenate([sel.tab["gidx"], extra]))
    k, alpha, area, z = ew.gnorm[-3:], ew.alpha, ew.cell_area, 14.0
    assert k.min() * z > 709.8 and np.all(alpha * z > k / (2 * alpha))
    with np.errstate(over="ignore", invalid="ignore"):
        naive = np.pi / (area * k) * (np.exp(k * z) * erfc(k / (2 * alpha) + alpha * z) + np.exp(-k * z) * erfc(k / (2 * alpha) - alpha * z))
    assert np.all(np.isnan(naive))
    w = ewald2d.recip_weight(np.array([z]), k, alpha, area)[0]
    np.testing.assert_allclose(w, 2 * np.pi / (area * k) * np.exp(-k * z), rtol=1e-12, atol=0)
    x = np.array([[[0.5, 0.7, 1.0], [2.5, 3.1, 15.0]], [[0.5, 0.7, 14.0], [2.5, 3.1, 15.5]]])
    configs = PeriodicConfigs(x, lat)
    ee, ei, ii = ew.energy(configs)
    assert np.all(np.isfinite(ee)) and np.all(np.isfinite(ei)) and np.isfinite(ii)
    # the extra vectors add their limit for the far pair (zero to rounding) and W(k, 0) exp(...) terms elsewhere
    ee0, ei0, _ = sel.energy(configs)
    assert abs(ee[0] - ee0[0] - 2 * np.sum(ew.gweight[-3:])) <= 1e-15 * abs(ee[0])


def test_translation_invariance():
    g = helpers.golden("g46_ewald2d")
    rng = np.random.default_rng(5)
    for name in ("b", "c"):
        cell = golden_cell(g, name)
        lat = cell.lattice_vectors()
        x = g[f"{name}_configs"]
        ee, ei, ii = ewald2d.Ewald(cell).energy(PeriodicConfigs(x, lat))
        for shift in (2 * lat[0] - lat[1], np.array([0.0, 0.0, 1.3]), rng.uniform(-3, 3, 3)):
            atoms = enforce_pbc(lat, cell.atom_coords() + shift)[0]  # (the reference's minimal image searches the 27 cells around in-cell points)
            moved = systems.Cell(cell._names, atoms, lat, nelec=cell.nelec, charges=cell.atom_charges(), dimension=2)
            ee2, ei2, ii2 = ewald2d.Ewald(moved).energy(PeriodicConfigs(x + shift, lat))
            np.testing.assert_allclose(ee2 + ei2 + ii2, ee + ei + ii, rtol=1e-12, atol=0)


def test_chunked_host_evaluation_gives_the_same_bits():
    g = helpers.golden("g46_ewald2d")
    cell = golden_cell(g, "c")
    configs = PeriodicConfigs(g["c_configs"], cell.lattice_vectors())
    ew = ewald2d.Ewald(cell)
    whole = ew.energy(configs)
    ew.host_chunk_bytes = 3 * 8 * 6 * (45 + 50) * len(ew.gnorm)  # three walkers per chunk
    parts = ew.energy(configs)
    assert np.array_equal(whole[0], parts[0]) and np.array_equal(whole[1], parts[1])
    m = ew.energy(configs, mean=True)
    assert m[0] == whole[0].mean() and m[1] == whole[1].mean()


class _StandIn:
    """What SlabEnergyAccumulator reads of the accumulator it wraps."""

    def __init__(self, W):
        rng = np.random.default_rng(3)
        self.res = {k: rng.standard_normal(W) for k in ("ke", "ee", "ei", "ecp", "grad2", "total")}

    def __call__(self, configs, wf):
        return {k: v.copy() for k, v in self.res.items()}

    def has_nonlocal_moves(self):
        return True

    def nonlocal_tmoves(self, configs, wf, e, tau, **kw):
        return {"e": e, "tau": tau}


def test_slab_energy_accumulator():
    import pyqmc_amd as pa

    g = helpers.golden("g46_ewald2d")
    cell = golden_cell(g, "c")
    configs = PeriodicConfigs(g["c_configs"], cell.lattice_vectors())
    inner = _StandIn(len(g["c_configs"]))
    acc = pa.SlabEnergyAccumulator(cell, energy=inner, nlatvec=1)
    assert not isinstance(acc, pa.EnergyAccumulator)
    out = acc(configs, None)
    assert acc.last_route == "host"
    assert set(out) == acc.keys() == pa.EnergyAccumulator(cell).keys() and acc.shapes() == pa.EnergyAccumulator(cell).shapes()
    for k in ("ke", "ecp", "grad2"):
        assert np.array_equal(out[k], inner.res[k])
    assert _relerr(out["ee"], g["c_ee"]) < 1e-12 and _relerr(out["ei"], g["c_ei"]) < 1e-12
    assert np.array_equal(out["total"], out["ke"] + out["ecp"] + out["ee"] + out["ei"] + acc.ewald.ewald_ion_ion)
    avg = acc.avg(configs, None)
    for k in out:
        assert np.shape(avg[k]) == ()
        np.testing.assert_allclose(avg[k], out[k].mean(), rtol=1e-13, atol=0)
    assert acc.has_nonlocal_moves() and acc.nonlocal_tmoves(configs, None, 2, 0.1) == {"e": 2, "tau": 0.1}
