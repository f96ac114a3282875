"""Total-spin estimator on the device (pqa_s2 / S2Accumulator's fused route): the reference's values (g40), the swap ratios
against recomputes of swapped configurations, exact spin eigenfunctions, agreement with the protocol route, no side effects on
the handle, route selection and the drivers."""

import ast

import numpy as np
import pytest

from pyqmc_amd import systems
from tests import helpers

pytestmark = pytest.mark.gpu


def _water(nelec=(4, 4)):
    sym, xyz = zip(*systems._WATER)
    return systems.Mol(sym, xyz, nelec=nelec)


def _restricted(mf, s=0):
    return systems.MeanField(np.stack([mf.mo_coeff[s], mf.mo_coeff[s]]), mf.mo_occ)


def _symmetric_jastrow(wf, seed=11):
    """Equal two-body channels and equal one-body spins: Psi is then a spin eigenfunction when the determinants are."""
    mol = wf.wf_factors[0]._dev.mol
    a, b = helpers.jastrow_params(mol, seed)
    b = np.repeat(b[:, 1:2], 3, axis=1)
    wf.parameters["wf2acoeff"] = np.repeat(a[..., :1], 2, axis=-1)
    wf.parameters["wf2bcoeff"] = b
    return wf


def _swapped(wf, x, pairs=None):
    """Psi(R^{i<->j})/Psi(R) (W, N_up, N_dn) from device recomputes of the swapped walkers (pairs: subset of (i, j))."""
    nu, nd = wf.wf_factors[0]._dev.nelec
    from pyqmc_amd.configs import OpenConfigs

    s0, l0 = wf.recompute(OpenConfigs(x.copy()))
    out = np.full((x.shape[0], nu, nd), np.nan)
    for i, j in pairs or [(i, j) for i in range(nu) for j in range(nd)]:
        y = x.copy()
        y[:, i], y[:, nu + j] = x[:, nu + j], x[:, i]
        s, l = wf.recompute(OpenConfigs(y))
        out[:, i, j] = s / s0 * np.exp(l - l0)
    wf.recompute(OpenConfigs(x.copy()))
    return out


def _configs(mol, W, seed):
    import pyqmc_amd as pa

    return pa.initial_guess(mol, W, rng=np.random.default_rng(seed))


@pytest.mark.parametrize("name", ["a", "b", "c"])
def test_s2_golden(name):
    import pyqmc_amd as pa
    from pyqmc_amd.s2 import device_s2

    g = helpers.golden("g40_s2")
    mol = _water(tuple(int(n) for n in g[f"{name}_nelec"]))
    dets = ast.literal_eval(str(g[f"{name}_det_json"]).replace("null", "None"))
    occ = np.zeros((2, g[f"{name}_mo"].shape[-1]))
    occ[0, : mol.nelec[0]], occ[1, : mol.nelec[1]] = 1, 1
    wf = pa.generate_wf(mol, systems.MeanField(g[f"{name}_mo"], occ), determinants=dets)
    wf.parameters["wf2acoeff"], wf.parameters["wf2bcoeff"] = g[f"{name}_acoeff"], g[f"{name}_bcoeff"]
    configs = pa.OpenConfigs(g[f"{name}_configs"].copy())
    wf.recompute(configs)
    acc = pa.S2Accumulator(mol.nelec)
    s2 = acc(configs, wf)["S2"]
    assert acc.last_route == "fused"
    _, rat = device_s2(wf.fused_device(), with_ratios=True)
    ref = g[f"{name}_s2"]
    assert np.all(np.abs(s2 - ref) <= 1e-9 * (1 + np.abs(rat).sum(axis=(1, 2)))), np.max(np.abs(s2 - ref))


def test_ratios_water_against_recompute():
    from pyqmc_amd.s2 import device_s2

    mol = systems.water()
    wf = helpers.gpu_wf(mol, systems.random_mf(mol))
    x = _configs(mol, 256, 1).configs
    direct = _swapped(wf, x)
    s2, rat = device_s2(wf.fused_device(), with_ratios=True)
    assert np.max(np.abs(rat - direct) / (1 + np.abs(direct))) < 1e-10
    assert np.allclose(s2, 4 - rat.sum(axis=(1, 2)), rtol=0, atol=1e-12 * (1 + np.abs(rat).sum()))


def test_ratios_diamond_primitive_against_recompute():
    from pyqmc_amd.s2 import device_s2

    sup, wf = helpers.gpu_pbc_wf("gamma")
    x = np.random.default_rng(2).random((64, sum(sup.nelec), 3)) @ sup.lattice_vectors()
    direct = _swapped(wf, x)
    _, rat = device_s2(wf.fused_device(), with_ratios=True)
    assert np.max(np.abs(rat - direct) / (1 + np.abs(direct))) < 1e-10


def test_ratios_above_32_electrons_per_spin():
    """The g35 cluster (more than 32 electrons per spin): several 16x16 tiles in both directions."""
    from pyqmc_amd.s2 import device_s2

    mol, mf, _, _ = helpers.case("g35_big")
    wf = helpers.gpu_wf(mol, mf)
    x = _configs(mol, 4, 5).configs
    nu, nd = mol.nelec
    pairs = [(0, 0), (nu - 1, nd - 1), (17, 40), (nu // 2, 3), (40, nd // 2)]
    direct = _swapped(wf, x, pairs)
    _, rat = device_s2(wf.fused_device(), with_ratios=True)
    for i, j in pairs:
        assert np.max(np.abs(rat[:, i, j] - direct[:, i, j]) / (1 + np.abs(direct[:, i, j]))) < 1e-9, (i, j)


def _per_walker_exact(wf, expect):
    from pyqmc_amd.s2 import device_s2

    s2, rat = device_s2(wf.fused_device(), with_ratios=True)
    tol = 1e-10 * (1 + np.abs(rat).sum(axis=(1, 2)))
    return np.all(np.abs(s2 - expect) <= tol), float(np.max(np.abs(s2 - expect)))


@pytest.mark.parametrize("jastrow", ["none", "symmetric"])
def test_exact_closed_shell_cluster_65536(jastrow):
    import pyqmc_amd as pa

    mol = systems.water_cluster()
    mf = _restricted(systems.random_mf(mol))
    wf = helpers.gpu_wf(mol, mf)
    if jastrow == "none":
        wf.parameters["wf2acoeff"] = np.zeros_like(wf.parameters["wf2acoeff"])
        wf.parameters["wf2bcoeff"] = np.zeros_like(wf.parameters["wf2bcoeff"])
    else:
        _symmetric_jastrow(wf)
    wf.recompute(_configs(mol, 65536, 6))
    ok, err = _per_walker_exact(wf, 0.0)
    assert ok, err


@pytest.mark.parametrize("jastrow", ["none", "symmetric"])
def test_exact_restricted_triplet(jastrow):
    mol = _water((5, 3))
    wf = helpers.gpu_wf(mol, _restricted(systems.random_mf(mol)))
    if jastrow == "none":
        wf.parameters["wf2acoeff"] = np.zeros_like(wf.parameters["wf2acoeff"])
        wf.parameters["wf2bcoeff"] = np.zeros_like(wf.parameters["wf2bcoeff"])
    else:
        _symmetric_jastrow(wf)
    wf.recompute(_configs(mol, 512, 7))
    ok, err = _per_walker_exact(wf, 2.0)
    assert ok, err


@pytest.mark.parametrize("jastrow", ["none", "symmetric"])
def test_exact_two_determinant_open_shell(jastrow):
    """core + (a_up b_dn +- b_up a_dn): one sign is the Sz = 0 triplet (S^2 = 2), the other the open-shell singlet (0)."""
    mol = _water((4, 4))
    mf = _restricted(systems.random_mf(mol, nvirt=2))
    found = []
    for sign in (1.0, -1.0):
        dets = [(1.0, [[0, 1, 2, 3], [0, 1, 2, 4]]), (sign, [[0, 1, 2, 4], [0, 1, 2, 3]])]
        wf = helpers.gpu_wf(mol, mf, dets)
        if jastrow == "none":
            wf.parameters["wf2acoeff"] = np.zeros_like(wf.parameters["wf2acoeff"])
            wf.parameters["wf2bcoeff"] = np.zeros_like(wf.parameters["wf2bcoeff"])
        else:
            _symmetric_jastrow(wf)
        wf.recompute(_configs(mol, 512, 8))
        for S in (0.0, 2.0):
            if _per_walker_exact(wf, S)[0]:
                found.append(S)
    assert sorted(found) == [0.0, 2.0], found


@pytest.mark.parametrize("case", ["asymmetric_jastrow", "multidet"])
def test_fused_matches_protocol(case):
    import pyqmc_amd as pa
    from pyqmc_amd.s2 import device_s2

    mol = _water((5, 3)) if case == "asymmetric_jastrow" else systems.water()
    if case == "asymmetric_jastrow":
        wf = helpers.gpu_wf(mol, _restricted(systems.random_mf(mol)))
    else:
        mf = systems.random_mf(mol, nvirt=6)
        wf = helpers.gpu_wf(mol, mf, systems.random_determinants(mol, mf, 50))
    configs = _configs(mol, 128, 9)
    wf.recompute(configs)
    s2f, rat = device_s2(wf.fused_device(), with_ratios=True)
    acc = pa.S2Accumulator(mol.nelec)
    s2p = acc._protocol(configs, wf)
    assert np.all(np.abs(s2f - s2p) <= 1e-9 * (1 + np.abs(rat).sum(axis=(1, 2)))), np.max(np.abs(s2f - s2p))
    if case == "asymmetric_jastrow":  # an exact triplet determinant times a spin-asymmetric Jastrow is no eigenfunction
        assert np.max(np.abs(s2f - 2.0)) > 1e-3


def test_no_side_effects_on_handle():
    import pyqmc_amd as pa

    mol = systems.water()
    mf = systems.random_mf(mol, nvirt=6)
    wf = helpers.gpu_wf(mol, mf, systems.random_determinants(mol, mf, 10))
    configs = _configs(mol, 256, 10)
    wf.recompute(configs)
    pa.vmc_worker(wf, configs, 0.3, 2, {}, seed=3, state_current=True)  # leaves the state in the sweep's layout
    sl, ja = wf.wf_factors

    def state():
        return [sl._get_state(0), sl._get_state(1), ja._get_state(), wf.value()]

    before = state()
    acc = pa.S2Accumulator(mol.nelec)
    acc(configs, wf)
    assert acc.last_route == "fused"
    after = state()
    for b, a in zip(before, after):
        for u, v in zip(b, a):
            assert np.array_equal(u, v)


class _Nothing:
    def avg(self, configs, wf):
        return {}

    def __call__(self, configs, wf):
        return {}

    def keys(self):
        return {}.keys()

    def shapes(self):
        return {}


def test_vmc_and_dmc_bitwise_unchanged_by_s2():
    import pyqmc_amd as pa

    mol = systems.water()
    mf = systems.random_mf(mol)
    runs = []
    for other in (pa.S2Accumulator(mol.nelec), _Nothing()):
        wf = helpers.gpu_wf(mol, mf)
        np.random.seed(6)  # (the energy accumulator's ECP draws)
        df, cfg = pa.vmc(wf, _configs(mol, 256, 11), nblocks=3, nsteps_per_block=2, tstep=0.3,
                         accumulators={"energy": pa.EnergyAccumulator(mol), "s2": other}, seed=5)
        np.random.seed(7)
        ddf, dcfg, dw = pa.rundmc(wf, cfg, tstep=0.02, nblocks=2, nsteps_per_block=2, vmc_warmup=1,
                                  accumulators={"energy": pa.EnergyAccumulator(mol), "s2": other})
        runs.append((df["energytotal"], cfg.configs.copy(), ddf["energytotal"], dcfg.configs.copy(), dw.copy()))
    for u, v in zip(*runs):
        assert np.array_equal(u, v)


def test_route_selection_three_body_and_complex():
    import pyqmc_amd as pa

    mol = systems.water()
    mf = systems.random_mf(mol)
    wf = helpers.gpu_wf3(mol, mf)
    x = _configs(mol, 16, 12).configs
    direct = _swapped(wf, x)
    configs = pa.OpenConfigs(x.copy())
    wf.recompute(configs)
    acc = pa.S2Accumulator(mol.nelec)
    s2 = acc(configs, wf)["S2"]
    assert acc.last_route == "protocol"
    assert np.max(np.abs(s2 - (4 - direct.sum(axis=(1, 2)))) / (1 + np.abs(direct).sum(axis=(1, 2)))) < 1e-9
    from pyqmc_amd._ffi import PqaError
    from pyqmc_amd.s2 import device_s2

    with pytest.raises(PqaError, match="three-body"):
        device_s2(wf.fused_device())

    from pyqmc_amd.configs import PeriodicConfigs

    sup, kmf = helpers.pbc_complex_case()
    cwf = pa.generate_wf(sup, kmf)
    lat = sup.lattice_vectors()
    xc = np.random.default_rng(13).random((4, sum(sup.nelec), 3)) @ lat
    nu, nd = sup.nelec
    s0, l0 = cwf.recompute(PeriodicConfigs(xc.copy(), lat))
    swap = np.zeros(4, dtype=complex)
    for i in range(nu):
        for j in range(nd):
            y = xc.copy()
            y[:, i], y[:, nu + j] = xc[:, nu + j], xc[:, i]
            s, l = cwf.recompute(PeriodicConfigs(y, lat))
            swap += s / s0 * np.exp(l - l0)
    cfg = PeriodicConfigs(xc.copy(), lat)
    cwf.recompute(cfg)
    acc = pa.S2Accumulator(sup.nelec)
    s2 = acc(cfg, cwf)["S2"]
    assert acc.last_route == "protocol"
    assert np.max(np.abs(s2 - (0.5 * (nu - nd) * (0.5 * (nu - nd) + 1) + nd - swap)) / (1 + np.abs(swap))) < 1e-8


def test_vmc_triplet_and_dmc_singlet_exact():
    import pyqmc_amd as pa

    mol = _water((5, 3))
    wf = _symmetric_jastrow(helpers.gpu_wf(mol, _restricted(systems.random_mf(mol))))
    df, _ = pa.vmc(wf, _configs(mol, 256, 14), nblocks=3, nsteps_per_block=2, tstep=0.3,
                   accumulators={"s2": pa.S2Accumulator(mol.nelec)}, seed=3)
    assert df["s2S2"].shape == (3,) and np.max(np.abs(df["s2S2"] - 2.0)) < 1e-9
    mol = systems.water()
    wf = _symmetric_jastrow(helpers.gpu_wf(mol, _restricted(systems.random_mf(mol))))
    np.random.seed(8)
    ddf, _, _ = pa.rundmc(wf, _configs(mol, 256, 15), tstep=0.02, nblocks=2, nsteps_per_block=2, vmc_warmup=1,
                          accumulators={"energy": pa.EnergyAccumulator(mol), "s2": pa.S2Accumulator(mol.nelec)})
    assert ddf["s2S2"].shape == (2,) and np.max(np.abs(ddf["s2S2"])) < 1e-9
