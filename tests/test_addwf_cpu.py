"""pyqmc_amd.AddWF (the protocol route: NumPy over the components' outputs) over the CPU oracle's wave functions, against the
reference's AddWF (tests/golden/g49_addwf.npz, written by tests/golden/make_golden_addwf.py) and against its own formulas.
Tolerance: the project's 1e-9, relative to max(1, |reference|)."""

import copy
import types

import numpy as np
import pytest

from tests import addwf_ref, helpers
from pyqmc_amd import AddWF
from pyqmc_amd.configs import OpenConfigs

TOL = 1e-9


def err(a, b):
    a, b = np.asarray(a), np.asarray(b)
    assert a.shape == b.shape, (a.shape, b.shape)
    return float(np.max(np.abs(a - b)) / max(1.0, float(np.max(np.abs(b))))) if b.size else 0.0


@pytest.fixture(scope="module")
def g():
    return helpers.golden(addwf_ref.GOLDEN)


def oracle_addwf(name):
    mol, wfs = addwf_ref.components(name, helpers.oracle_wf)
    return mol, AddWF(list(addwf_ref.CASES[name]["coeffs"]), wfs)


def check_entries(out, g, p):
    keys = [k for k in g.files if k.startswith(p) and k in out]
    assert len(keys) > 40
    for k in keys:
        if k.endswith("_keys"):
            assert list(out[k]) == list(g[k]), k
        elif g[k].dtype != bool:
            assert err(out[k], g[k]) < TOL, (k, err(out[k], g[k]))


@pytest.mark.parametrize("name", ["a", "b", "c"])
def test_protocol_entries_match_reference(g, name):
    _, wf = oracle_addwf(name)
    assert wf.dtype == (complex if name == "c" else float)
    out = {}
    addwf_ref.protocol_entries(wf, OpenConfigs(g[name + "_configs"].copy()), g, name + "_", out)
    check_entries(out, g, name + "_")
    assert wf.last_route == "protocol"


def test_trajectory_matches_reference(g):
    _, wf = oracle_addwf("a")
    configs = OpenConfigs(g["a_configs"].copy())
    with addwf_ref.replay(g["a_traj_gauss"], g["a_traj_unif"]):
        blk, configs = helpers.protocol_vmc_worker(wf, configs, addwf_ref.TSTEP, addwf_ref.NSWEEPS, {})
    assert np.max(np.abs(configs.configs - g["a_configs"])) > 0.1
    assert err(configs.configs, g["a_traj_final"]) < TOL
    assert abs(blk["acceptance"] - float(g["a_traj_acceptance"])) < TOL
    s, l = wf.value()
    assert err(s, g["a_traj_sign"]) < TOL and err(l, g["a_traj_log"]) < TOL
    assert err(wf.ratio_current_config(), g["a_traj_rcc"]) < TOL


def test_parameter_keys_and_pgradient_layout(g):
    _, wf = oracle_addwf("b")
    wf.recompute(OpenConfigs(g["b_configs"].copy()))
    assert list(wf.parameters.keys()) == list(g["b_param_keys"])
    assert all(k[:3] in ("wf1", "wf2", "wf3") for k in wf.parameters.keys()) and not any("coeffs" in k for k in wf.parameters.keys())
    pg = wf.pgradient()
    assert list(pg.keys()) == list(g["b_pgrad_keys"])
    for k in pg.keys():
        assert np.shape(pg[k]) == g["b_pgrad_" + k].shape and np.shape(pg[k])[0] == 24, k
    wf.parameters["wf2wf1det_coeff"] = np.array([1.0, 0.0, 0.0, 0.0])
    assert np.array_equal(wf.wf_components[1].parameters["wf1det_coeff"], [1.0, 0.0, 0.0, 0.0])


@pytest.mark.parametrize("name", ["a", "b"])
def test_gradient_and_laplacian_against_finite_differences(g, name):
    _, wf = oracle_addwf(name)
    configs = OpenConfigs(g[name + "_configs"].copy())
    wf.recompute(configs)
    d = 1e-5
    for e in addwf_ref.CASES[name]["electrons"]:
        r = g[f"{name}_e{e}_newpos"]
        tv0 = wf.testvalue(e, configs.make_irreducible(e, r))[0]
        grad, lap = wf.gradient_laplacian(e, configs.make_irreducible(e, r))
        fd_g, fd_l = np.zeros_like(grad), np.zeros_like(lap)
        for k in range(3):
            step = np.zeros(3)
            step[k] = d
            tp = wf.testvalue(e, configs.make_irreducible(e, r + step))[0]
            tm = wf.testvalue(e, configs.make_irreducible(e, r - step))[0]
            fd_g[k] = (tp - tm) / (2 * d * tv0)
            fd_l += (tp + tm - 2 * tv0) / (d * d * tv0)
        assert err(fd_g, grad) < 1e-5 and err(fd_g, wf.gradient(e, configs.make_irreducible(e, r))) < 1e-5
        assert err(fd_l, lap) < 1e-5, err(fd_l, lap)


def test_two_copies_of_one_function_reproduce_it(g):
    mol, (psi, *_) = addwf_ref.components("a", helpers.oracle_wf)
    wf = AddWF([0.3, 0.7], [addwf_ref.components("a", helpers.oracle_wf)[1][0] for _ in range(2)])
    configs = OpenConfigs(g["a_configs"].copy())
    s0, l0 = psi.recompute(configs)
    s1, l1 = wf.recompute(configs)
    assert err(s1, s0) < TOL and err(l1, l0) < TOL
    assert err(wf.ratio_current_config(), np.array([0.3, 0.7])[:, None] * np.ones((2, len(s0)))) < TOL
    e = 5
    ep = configs.make_irreducible(e, g["a_e5_newpos"])
    ea = configs.make_irreducible(e, g["a_e5_aux"])
    mask = g["a_e5_mask"]
    assert err(wf.gradient(e, ep), psi.gradient(e, ep)) < TOL
    for x, y in zip(wf.gradient_laplacian(e, ep), psi.gradient_laplacian(e, ep)):
        assert err(x, y) < TOL
    assert err(wf.testvalue(e, ep)[0], psi.testvalue(e, ep)[0]) < TOL
    assert err(wf.testvalue(e, ea, mask)[0], psi.testvalue(e, ea, mask)[0]) < TOL
    es = np.array([0, 3, 6])
    assert err(wf.testvalue_many(es, ep), psi.testvalue_many(es, ep)) < TOL
    assert err(wf.testvalue_many(es, ep, mask), psi.testvalue_many(es, ep)[mask]) < TOL
    gw, vw, _ = wf.gradient_value(e, ep)
    gp, vp, _ = psi.gradient_value(e, ep)
    assert err(gw, gp) < TOL and err(vw, vp) < TOL


def fake(sign, logv, dev=None):
    f = types.SimpleNamespace(parameters={}, dtype=float, value=lambda: (np.asarray(sign, dtype=float), np.asarray(logv, dtype=float)))
    if dev is not None:
        f._dev = dev
    return f


def test_walkers_far_apart_in_log_stay_finite():
    """Two walkers 800 apart in log|Psi| (one global reference value underflows the smaller one to 0 / 0), and components 800 apart on
    one walker."""
    a = fake([1.0, 1.0, -1.0], [0.0, -800.0, 5.0])
    b = fake([1.0, -1.0, 1.0], [-1.0, -801.0, -795.0])
    wf = AddWF([0.6, 0.4], [a, b])
    s, l = wf.value()
    w = wf.ratio_current_config()
    assert np.all(np.isfinite(s)) and np.all(np.isfinite(l)) and np.all(np.isfinite(w))
    assert err(np.sum(w, axis=0), np.ones(3)) < TOL
    assert err(l[:2], np.array([np.log(0.6 + 0.4 * np.exp(-1.0)), -800.0 + np.log(0.6 - 0.4 * np.exp(-1.0))])) < TOL
    assert err(w[:, 2], np.array([1.0, 0.0])) < TOL and s[2] == -1.0


def test_updateinternals_without_saved_values(g):
    _, wf = oracle_addwf("a")
    _, ref = oracle_addwf("a")
    configs, configs2 = OpenConfigs(g["a_configs"].copy()), OpenConfigs(g["a_configs"].copy())
    wf.recompute(configs)
    ref.recompute(configs2)
    e, accept = 1, g["a_e1_accept"]
    ep = configs.make_irreducible(e, g["a_e1_newpos"])
    configs.move(e, ep, accept)
    wf.updateinternals(e, ep, configs, mask=accept)
    _, _, saved = ref.gradient_value(e, ep)
    configs2.move(e, ep, accept)
    ref.updateinternals(e, ep, configs2, mask=accept, saved_values=saved)
    assert err(wf.value()[1], ref.value()[1]) < TOL
    assert err(wf.value()[1], g["a_e1_post_log"]) < TOL


def test_components_sharing_a_handle_are_refused():
    handle = object()
    with pytest.raises(ValueError, match="handle of its own"):
        AddWF([0.5, 0.5], [fake([1.0], [0.0], dev=handle), fake([1.0], [0.0], dev=handle)])
    product = types.SimpleNamespace(wf_factors=[fake([1.0], [0.0], dev=handle)], parameters={}, dtype=float)
    with pytest.raises(ValueError, match="handle of its own"):
        AddWF([0.5, 0.5], [product, fake([1.0], [0.0], dev=handle)])
    AddWF([0.5, 0.5], [fake([1.0], [0.0], dev=object()), fake([1.0], [0.0], dev=object())])
    with pytest.raises(ValueError, match="route"):
        AddWF([1.0], [fake([1.0], [0.0])], route="device")
    with pytest.raises(ValueError, match="out of scope"):
        AddWF([1.0], [fake([1.0], [0.0])], route="fused")


def test_copy_rebinds_parameters(g):
    _, wf = oracle_addwf("a")
    for other in (copy.copy(wf), copy.deepcopy(wf)):
        assert other.wf_components[0] is not wf.wf_components[0] and list(other.parameters.keys()) == list(wf.parameters.keys())
        other.parameters["wf1wf2bcoeff"] = np.zeros((4, 3))
        assert np.array_equal(other.wf_components[0].parameters["wf2bcoeff"], np.zeros((4, 3)))
        assert np.any(np.asarray(wf.parameters["wf1wf2bcoeff"]) != 0)
