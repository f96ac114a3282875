"""Structure factor on the device (pqa_sq / SqAccumulator's fused route): the reference's values (g42), the recurrence path
against the direct path, the coordinates read in place after a fused sweep, no side effects on the handle, every handle kind, a
walker count that takes several chunks, and the drivers."""

import numpy as np
import pytest

from pyqmc_amd import pbc, systems
from pyqmc_amd.configs import OpenConfigs, PeriodicConfigs
from tests import helpers

pytestmark = pytest.mark.gpu

TOL = dict(rtol=1e-11, atol=1e-11)


def _c5():
    sup = pbc.get_supercell(systems.diamond_primitive(), 2.0 * np.eye(3))
    return sup, helpers.gpu_pbc_wf("k222")[1]


def _c3():
    import pyqmc_amd as pa

    sup = pbc.get_supercell(systems.diamond_primitive(), np.array([[-1.0, 1, 1], [1, -1, 1], [1, 1, -1]]))
    return sup, pa.generate_wf(sup, pbc.random_kmf(sup, complex_coeff=True, twist=(0.25, 0.1, -0.3)))


def _primitive_53():
    import pyqmc_amd as pa

    p = systems.diamond_primitive()
    sup = pbc.get_supercell(systems.Cell(p._names, p.atom_coords(), p.lattice_vectors(), nelec=(5, 3)), np.eye(3))
    return sup, pa.generate_wf(sup, pbc.random_kmf(sup))


def _container(mol, x):
    return PeriodicConfigs(x, mol.lattice_vectors()) if hasattr(mol, "a") else OpenConfigs(x)


def _walkers(mol, W, seed):
    x = systems.initial_guess(mol, W, rng=np.random.default_rng(seed)).configs.copy()
    return _container(mol, x)


def _host(acc, x):
    return acc._host(np.asarray(x, dtype=float), False)


def _golden_system(name):
    if name == "a":
        return helpers.gpu_pbc_wf("gamma")
    if name == "b":
        return _c5()
    if name == "c":
        return _primitive_53()
    mol = systems.water()
    return mol, helpers.gpu_wf(mol, systems.random_mf(mol))


@pytest.mark.parametrize("name", ["a", "b", "c", "d"])
def test_sq_golden(name):
    import pyqmc_amd as pa

    g = helpers.golden("g42_sq")
    mol, wf = _golden_system(name)
    assert tuple(mol.nelec) == tuple(g[f"{name}_nelec"])
    configs = _container(mol, g[f"{name}_configs"].copy())
    wf.recompute(configs)
    acc = pa.SqAccumulator(mol, nq=int(g[f"{name}_nq"])) if f"{name}_nq" in g.files else pa.SqAccumulator(mol, qlist=g[f"{name}_qlist"])
    assert (acc.qn is not None) == (name in "ab")  # a, b: recurrence path; c, d: direct path
    np.testing.assert_array_equal(acc.qlist, g[f"{name}_qlist"])
    res = acc(configs, wf)
    assert acc.last_route == "fused"
    for k in ("Sq", "spinSq"):
        np.testing.assert_allclose(res[k], g[f"{name}_{k}"], **TOL)
    avg = acc.avg(configs, wf)
    assert acc.last_route == "fused"
    for k in ("Sq", "spinSq"):
        np.testing.assert_allclose(avg[k], g[f"{name}_{k}"].mean(axis=0), **TOL)


def test_recurrence_equals_direct():
    import pyqmc_amd as pa

    sup, wf = _c5()
    configs = _walkers(sup, 512, 3)
    wf.recompute(configs)
    rec = pa.SqAccumulator(sup, nq=4)
    direct = pa.SqAccumulator(sup, qlist=rec.qlist)
    a, b = rec(configs, wf), direct(configs, wf)
    assert rec.last_route == direct.last_route == "fused"
    for k in ("Sq", "spinSq"):
        np.testing.assert_allclose(a[k], b[k], **TOL)


@pytest.mark.parametrize("system", ["water_cluster", "C5"])
def test_after_a_fused_sweep_before_any_fetch(system):
    """A fused sweep leaves the live coordinates in its lane-per-walker planes: pqa_sq reads them there."""
    import pyqmc_amd as pa
    from pyqmc_amd.sq import device_sq
    from pyqmc_amd.vmc import _fetch

    if system == "C5":
        mol, wf = _c5()
        acc = pa.SqAccumulator(mol, nq=4)
    else:
        mol = systems.water_cluster()
        wf = helpers.gpu_wf(mol, systems.random_mf(mol))
        acc = pa.SqAccumulator(mol, qlist=np.random.default_rng(4).uniform(-1.5, 1.5, (40, 3)))
    configs = _walkers(mol, 4096, 5)
    wf.recompute(configs)
    dev = wf.fused_device()
    dev.vmc_sweeps(0.3, 1, seed=9, energy=False)
    sq, sp = device_sq(dev, acc.qlist, acc.qn, acc.recip)
    msq, msp = device_sq(dev, acc.qlist, acc.qn, acc.recip, mean=True)
    _fetch(dev, configs)
    hsq, hsp = _host(acc, configs.configs)
    np.testing.assert_allclose(sq, hsq, **TOL)
    np.testing.assert_allclose(sp, hsp, **TOL)
    np.testing.assert_allclose(msq, hsq.mean(axis=0), **TOL)
    np.testing.assert_allclose(msp, hsp.mean(axis=0), **TOL)


def test_handle_state_unchanged():
    """Two handles built and seeded alike, one of which evaluates S(q) between sweeps, end with the same bits."""
    import pyqmc_amd as pa
    from pyqmc_amd.sq import device_sq

    runs = []
    for call in (False, True):
        sup, wf = _c5()
        configs = _walkers(sup, 1024, 6)
        wf.recompute(configs)
        dev = wf.fused_device()
        acc = pa.SqAccumulator(sup, nq=4)
        off = pa.SqAccumulator(sup, qlist=np.random.default_rng(7).uniform(-1.0, 1.0, (30, 3)))
        out = []
        for step in range(3):
            if call:
                device_sq(dev, acc.qlist, acc.qn, acc.recip)
                device_sq(dev, acc.qlist, acc.qn, acc.recip, mean=True)
                device_sq(dev, off.qlist)
            a, en, _ = dev.vmc_sweeps(0.3, 2, seed=20 + step, energy=True)
            out += [np.asarray(a), en.copy()]
        out += [dev.configs(), dev.wrap_delta(), *dev.value()]
        runs.append(out)
    for u, v in zip(*runs):
        assert np.array_equal(u, v)


def _kind(kind):
    import pyqmc_amd as pa

    if kind == "twisted_C3":
        sup, wf = _c3()
        return sup, wf, 256
    if kind == "multidet50_j3":
        mol = systems.water()
        mf = systems.random_mf(mol, nvirt=8)
        return mol, helpers.gpu_wf3(mol, mf, systems.random_determinants(mol, mf, 50)), 256
    if kind == "72_per_spin":
        mol, mf, _, _ = helpers.case("g35_big")
        assert min(mol.nelec) > 64
        return mol, helpers.gpu_wf(mol, mf), 64
    raise KeyError(kind)


@pytest.mark.parametrize("kind", ["twisted_C3", "multidet50_j3", "72_per_spin"])
def test_every_handle_kind(kind):
    import pyqmc_amd as pa
    from pyqmc_amd.vmc import _fetch

    mol, wf, W = _kind(kind)
    configs = _walkers(mol, W, 8)
    wf.recompute(configs)
    dev = wf.fused_device()
    assert dev is not None
    dev.vmc_sweeps(0.3, 1, seed=4, energy=False)  # (twisted: the handle's coordinates now leave the cell)
    _fetch(dev, configs)
    accs = [pa.SqAccumulator(mol, qlist=np.random.default_rng(9).uniform(-1.2, 1.2, (25, 3)))]
    if hasattr(mol, "a"):
        accs.append(pa.SqAccumulator(mol, nq=2))
    for acc in accs:
        res = acc(configs, wf)
        assert acc.last_route == "fused"
        hsq, hsp = _host(acc, configs.configs)
        np.testing.assert_allclose(res["Sq"], hsq, **TOL)
        np.testing.assert_allclose(res["spinSq"], hsp, **TOL)


def test_c5_65536_walkers_several_chunks():
    import pyqmc_amd as pa

    sup, wf = _c5()
    W = 65536
    configs = _walkers(sup, W, 10)
    wf.recompute(configs)
    acc = pa.SqAccumulator(sup, nq=4)
    Q = len(acc.qlist)
    assert (256 << 20) // (16 * Q) < W  # more than one walker chunk of pqa_sq's scratch
    res = acc(configs, wf)
    assert acc.last_route == "fused" and res["Sq"].shape == (W, Q)
    chunk = (256 << 20) // (16 * Q)
    idx = np.unique(np.concatenate([np.arange(8), chunk + np.arange(-4, 4), W - 1 - np.arange(8),
                                    np.random.default_rng(11).integers(0, W, 40)]))
    hsq, hsp = _host(acc, configs.configs[idx])
    np.testing.assert_allclose(res["Sq"][idx], hsq, **TOL)
    np.testing.assert_allclose(res["spinSq"][idx], hsp, **TOL)
    m1, m2 = acc.avg(configs, wf), acc.avg(configs, wf)
    for k in ("Sq", "spinSq"):
        np.testing.assert_allclose(m1[k], res[k].mean(axis=0), rtol=1e-12, atol=0)
        assert np.array_equal(m1[k], m2[k])


class _Nothing:
    def avg(self, configs, wf):
        return {}

    def __call__(self, configs, wf):
        return {}

    def keys(self):
        return {}.keys()

    def shapes(self):
        return {}


def _host_only(acc):
    acc._fused = lambda configs, wf: None
    return acc


def test_vmc_and_dmc_drivers_c5():
    import pyqmc_amd as pa

    sup, _ = _c5()
    runs = {}
    for tag in ("fused", "host", "none"):
        _, wf = _c5()
        other = {"fused": lambda: pa.SqAccumulator(sup), "host": lambda: _host_only(pa.SqAccumulator(sup)), "none": _Nothing}[tag]()
        np.random.seed(6)
        df, cfg = pa.vmc(wf, _walkers(sup, 128, 12), nblocks=2, nsteps_per_block=2, tstep=0.3,
                         accumulators={"energy": pa.EnergyAccumulator(sup), "sq": other}, seed=5)
        np.random.seed(7)
        ddf, dcfg, dw = pa.rundmc(wf, cfg, tstep=0.02, nblocks=2, nsteps_per_block=2, vmc_warmup=1,
                                  accumulators={"energy": pa.EnergyAccumulator(sup), "sq": other})
        if tag != "none":
            assert other.last_route == tag
        runs[tag] = (df, cfg.configs.copy(), ddf, dcfg.configs.copy(), dw.copy())
    for tag in ("fused", "host"):
        df, c, ddf, dc, dw = runs[tag]
        n_df, n_c, n_ddf, n_dc, n_dw = runs["none"]
        assert np.array_equal(df["energytotal"], n_df["energytotal"]) and np.array_equal(c, n_c)
        assert np.array_equal(ddf["energytotal"], n_ddf["energytotal"]) and np.array_equal(dc, n_dc) and np.array_equal(dw, n_dw)
        for k in ("sqSq", "sqspinSq"):
            assert np.shape(df[k]) == (2, 364) and np.shape(ddf[k]) == (2, 364)
    for k in ("sqSq", "sqspinSq"):
        np.testing.assert_allclose(runs["fused"][0][k], runs["host"][0][k], **TOL)
        np.testing.assert_allclose(runs["fused"][2][k], runs["host"][2][k], **TOL)
