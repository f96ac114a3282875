"""Slab Ewald sum on the device (pqa_ewald2d / Ewald's fused route / SlabEnergyAccumulator): the reference's values (g46), a
production size against the host route, the overflow case, every periodic handle kind of the fixtures (single determinant,
three-body, complex, twisted), open handles refused, no side effects on the handle, the chunked path, and the VMC driver.

Every system is a slab cell (dimension = 2, Lz of 30 bohr or more) built through generate_wf."""

import numpy as np
import pytest

import pyqmc_amd as pa
from pyqmc_amd import ewald2d, pbc, systems
from pyqmc_amd.configs import PeriodicConfigs
from pyqmc_amd.ewald2d import device_ewald2d
from tests import helpers

pytestmark = pytest.mark.gpu

OBLIQUE = np.array([[5.0, 0.0, 0.0], [1.5, 4.5, 0.0], [0.0, 0.0, 30.0]])


def relerr(a, b):
    return float(np.max(np.abs(np.asarray(a) - np.asarray(b)) / np.abs(np.asarray(b))))


def golden_cell(g, name):
    cell = systems.Cell([str(s) for s in g[f"{name}_symbols"]], g[f"{name}_atoms"], g[f"{name}_lattice"], nelec=tuple(g[f"{name}_nelec"]),
                        charges=g[f"{name}_charges"], dimension=2)
    return pbc.get_supercell(cell, np.eye(3))


def carbon_slab(S=(2, 2, 1), Lz=30.0):
    """Two carbon atoms per oblique 5 x 4.5 cell, 8 electrons; S = (2, 2, 1): 8 atoms, 16 + 16 electrons."""
    lat = OBLIQUE.copy()
    lat[2, 2] = Lz
    prim = systems.Cell(["C", "C"], [(0.6, 0.5, Lz / 2 - 0.7), (3.2, 2.6, Lz / 2 + 0.7)], lat, dimension=2)
    return pbc.get_supercell(prim, np.diag(np.asarray(S, dtype=float)))


def slab_walkers(cell, W, seed, sigma=1.5):
    rng = np.random.default_rng(seed)
    N = sum(cell.nelec)
    lat = cell.lattice_vectors()
    x = np.concatenate([rng.uniform(0, 1, (W, N, 2)), np.full((W, N, 1), 0.5)], axis=-1) @ lat
    x[..., 2] += sigma * rng.standard_normal((W, N))
    return PeriodicConfigs(x, lat)


@pytest.mark.parametrize("name", ["b", "c", "d"])
def test_golden(name):
    g = helpers.golden("g46_ewald2d")
    cell = golden_cell(g, name)
    assert cell.dimension == 2
    wf = pa.generate_wf(cell, pbc.random_kmf(cell))
    configs = PeriodicConfigs(g[f"{name}_configs"].copy(), cell.lattice_vectors())
    wf.recompute(configs)
    ew = ewald2d.Ewald(cell, nlatvec=int(g[f"{name}_nlatvec"]))
    ee, ei, ii = ew.energy(configs, wf)
    assert ew.last_route == "fused"
    print(name, "relerr ee", relerr(ee, g[f"{name}_ee"]), "ei", relerr(ei, g[f"{name}_ei"]))
    assert relerr(ee, g[f"{name}_ee"]) < 1e-12 and relerr(ei, g[f"{name}_ei"]) < 1e-12
    mee, mei, _ = ew.energy(configs, wf, mean=True)
    assert abs(mee - g[f"{name}_ee"].mean()) < 1e-12 * abs(g[f"{name}_ee"].mean())
    assert abs(mei - g[f"{name}_ei"].mean()) < 1e-12 * abs(g[f"{name}_ei"].mean())


def test_one_electron_one_atom():
    g = helpers.golden("g46_ewald2d")
    cell = golden_cell(g, "e")
    wf = pa.generate_wf(cell, pbc.random_kmf(cell))
    configs = PeriodicConfigs(g["e_configs"].copy(), cell.lattice_vectors())
    wf.recompute(configs)
    ew = ewald2d.Ewald(cell)
    ee, ei, ii = ew.energy(configs, wf)
    assert ew.last_route == "fused"
    assert relerr(ee, g["e_ee"]) < 1e-12 and relerr(ei, g["e_ei"]) < 1e-12


def test_production_size_against_host_route():
    cell = carbon_slab()
    assert sum(cell.nelec) == 32
    wf = pa.generate_wf(cell, pbc.random_kmf(cell))
    W = 4096
    configs = slab_walkers(cell, W, 3)
    wf.recompute(configs)
    dev = wf.fused_device()
    dev.vmc_sweeps(0.3, 3, seed=11, energy=False)
    ew = ewald2d.Ewald(cell)
    ee, ei = device_ewald2d(dev, ew.tab)  # (the coordinates are read from the sweep's planes)
    m1, m2 = device_ewald2d(dev, ew.tab, mean=True), device_ewald2d(dev, ew.tab, mean=True)
    from pyqmc_amd.vmc import _fetch

    _fetch(dev, configs)
    ee2, ei2, _ = ew.energy(configs, wf)
    assert ew.last_route == "fused" and relerr(ee2, ee) < 1e-12 and relerr(ei2, ei) < 1e-12  # (the walker-major layout after the fetch)
    hee, hei = ew._host(np.asarray(configs.configs))
    print("relerr ee", relerr(ee, hee), "ei", relerr(ei, hei))
    assert relerr(ee, hee) < 1e-12 and relerr(ei, hei) < 1e-12
    assert m1 == m2
    assert abs(m1[0] - ee.mean()) <= 1e-13 * abs(ee.mean()) and abs(m1[1] - ei.mean()) <= 1e-13 * abs(ei.mean())


def test_overflow_case():
    """k |z| > 709 with alpha |z| > k / 2 alpha, where the reference's weight is inf * 0 (tests/test_ewald2d_cpu.py,
    test_overflow_with_extra_k_vectors): k vectors far beyond the weight cut-off passed in, pairs 14 bohr apart in height."""
    cell = carbon_slab((1, 1, 1))
    wf = pa.generate_wf(cell, pbc.random_kmf(cell))
    configs = slab_walkers(cell, 8, 9)
    x = configs.configs.copy()
    x[:, 0, 2] = 1.0
    x[:, 1, 2] = 15.0
    configs = PeriodicConfigs(x, cell.lattice_vectors())
    wf.recompute(configs)
    sel = ewald2d.Ewald(cell, alpha_scaling=8.0)
    extra = np.array([[45, 0], [44, -3], [0, 50]], dtype=np.int32)
    ew = ewald2d.Ewald(cell, alpha_scaling=8.0, gidx=np.concatenate([sel.tab["gidx"], extra]))
    k = ew.gnorm[-3:]
    assert k.min() * 14.0 > 709.8 and np.all(ew.alpha * 14.0 > k / (2 * ew.alpha))
    ee, ei, ii = ew.energy(configs, wf)
    assert ew.last_route == "fused"
    assert np.all(np.isfinite(ee)) and np.all(np.isfinite(ei))
    hee, hei = ew._host(np.asarray(configs.configs))
    print("relerr ee", relerr(ee, hee), "ei", relerr(ei, hei))
    assert relerr(ee, hee) < 1e-12 and relerr(ei, hei) < 1e-12


def _kind(kind):
    if kind == "single":
        cell = carbon_slab((1, 1, 1))
        return cell, pa.generate_wf(cell, pbc.random_kmf(cell))
    if kind == "three_body":
        cell = carbon_slab((1, 1, 1))
        wf = pa.generate_wf(cell, pbc.random_kmf(cell), jastrow3=True)
        wf.parameters["wf3ccoeff"] = 0.02 * np.random.default_rng(2).standard_normal(wf.parameters["wf3ccoeff"].shape)
        return cell, wf
    if kind == "complex":
        cell = carbon_slab((3, 1, 1))  # k = 1/3, 2/3 b1: complex supercell orbitals
        return cell, pa.generate_wf(cell, pbc.random_kmf(cell, complex_coeff=True))
    if kind == "twisted":
        cell = carbon_slab((2, 1, 1))
        return cell, pa.generate_wf(cell, pbc.random_kmf(cell, complex_coeff=True, twist=(0.25, 0.1, 0.0)))
    raise KeyError(kind)


@pytest.mark.parametrize("kind", ["single", "three_body", "complex", "twisted"])
def test_every_periodic_handle_kind(kind):
    from pyqmc_amd.vmc import _fetch

    cell, wf = _kind(kind)
    configs = slab_walkers(cell, 128, 8)
    wf.recompute(configs)
    dev = wf.fused_device()
    assert dev is not None and dev.pbc
    dev.vmc_sweeps(0.3, 2, seed=4, energy=False)  # (twisted: the handle's coordinates now leave the cell)
    _fetch(dev, configs)
    ew = ewald2d.Ewald(cell)
    ee, ei, _ = ew.energy(configs, wf)
    assert ew.last_route == "fused"
    hee, hei = ew._host(np.asarray(configs.configs))
    assert relerr(ee, hee) < 1e-12 and relerr(ei, hei) < 1e-12


def test_open_boundary_handle_is_refused():
    from pyqmc_amd import _ffi

    mol = systems.water()
    wf = helpers.gpu_wf(mol, systems.random_mf(mol))
    wf.recompute(systems.initial_guess(mol, 16, rng=np.random.default_rng(1)))
    ew = ewald2d.Ewald(carbon_slab((1, 1, 1)))
    with pytest.raises(_ffi.PqaError, match="open-boundary"):
        device_ewald2d(wf.fused_device(), ew.tab)
    # ... and Ewald.energy never takes an open handle to the device
    cell = carbon_slab((1, 1, 1))
    assert ew._fused(slab_walkers(cell, 16, 2), wf) is None


def test_handle_state_unchanged():
    """Two handles built and seeded alike, one of which evaluates the slab sum between sweeps, end with the same bits."""
    runs = []
    for call in (False, True):
        cell = carbon_slab()
        wf = pa.generate_wf(cell, pbc.random_kmf(cell))
        configs = slab_walkers(cell, 512, 6)
        wf.recompute(configs)
        dev = wf.fused_device()
        ew = ewald2d.Ewald(cell)
        out = []
        for step in range(3):
            if call:
                device_ewald2d(dev, ew.tab)
                device_ewald2d(dev, ew.tab, mean=True)
            a, en, _ = dev.vmc_sweeps(0.3, 2, seed=20 + step, energy=True)
            out += [np.asarray(a), en.copy()]
        out += [dev.configs(), dev.wrap_delta(), *dev.value()]
        runs.append(out)
    for u, v in zip(*runs):
        assert np.array_equal(u, v)


def test_chunked_path_gives_the_same_bits():
    cell = carbon_slab()
    wf = pa.generate_wf(cell, pbc.random_kmf(cell))
    configs = slab_walkers(cell, 1000, 7)
    wf.recompute(configs)
    dev = wf.fused_device()
    ew = ewald2d.Ewald(cell)
    whole, mean = device_ewald2d(dev, ew.tab), device_ewald2d(dev, ew.tab, mean=True)
    for chunk in (96, 333):
        parts = device_ewald2d(dev, ew.tab, walker_chunk=chunk)
        assert np.array_equal(whole[0], parts[0]) and np.array_equal(whole[1], parts[1])
        assert device_ewald2d(dev, ew.tab, mean=True, walker_chunk=chunk) == mean


def test_slab_energy_accumulator_in_vmc():
    cell = carbon_slab((1, 1, 1))
    runs = {}
    for tag in ("slab", "plain"):
        wf = pa.generate_wf(cell, pbc.random_kmf(cell))
        acc = pa.SlabEnergyAccumulator(cell, seed=3) if tag == "slab" else pa.EnergyAccumulator(cell, seed=3)
        np.random.seed(6)
        df, cfg = pa.vmc(wf, slab_walkers(cell, 256, 12), nblocks=3, nsteps_per_block=2, tstep=0.3,
                         accumulators={"energy": acc, "other": _Nothing()}, seed=5)
        runs[tag] = (df, cfg.configs.copy(), acc)
    slab, plain = runs["slab"][0], runs["plain"][0]
    acc = runs["slab"][2]
    assert acc.last_route == "fused"
    assert np.array_equal(runs["slab"][1], runs["plain"][1])
    for k in ("energyke", "energyecp", "energygrad2"):
        assert np.array_equal(slab[k], plain[k])
    np.testing.assert_allclose(slab["energytotal"] - slab["energyke"] - slab["energyecp"],
                               slab["energyee"] + slab["energyei"] + acc.ewald.ewald_ion_ion, rtol=1e-12, atol=0)
    assert np.max(np.abs(slab["energyee"] - plain["energyee"])) > 1e-6  # (the 3D sum includes the copies of the slab)
    # the last block's walkers are the handle's: the accumulator's slab sums are the host route's
    configs = PeriodicConfigs(runs["slab"][1], cell.lattice_vectors())
    hee, hei = acc.ewald._host(np.asarray(configs.configs))
    wf = pa.generate_wf(cell, pbc.random_kmf(cell))
    wf.recompute(configs)
    out = acc(configs, wf)
    assert relerr(out["ee"], hee) < 1e-12 and relerr(out["ei"], hei) < 1e-12


class _Nothing:
    """A host-called accumulator: both runs of test_slab_energy_accumulator_in_vmc take the driver's host-accumulator route."""

    def avg(self, configs, wf):
        return {}

    def __call__(self, configs, wf):
        return {}

    def keys(self):
        return {}.keys()

    def shapes(self):
        return {}
