"""GeminalJastrow on the device (pqa_geminal.hip) against the reference's golden vectors (g48_geminal.npz, cases a, b, c of
tests/geminal_ref.py), the update / ratio / recompute triangle, the saved-row route, parameters, copies, the product with Slater and
JastrowSpin, and no side effect on another wave function of the device.

Metric and bound: helpers.relerr < 1e-10, the project's bound for device factors against goldens (tests/test_gpu_gps.py): fp64 AOs
pinned to the reference at 1e-12 and contractions over at most 184 x 184 terms of mixed sign."""

import copy
import pickle

import numpy as np
import pytest

import geminal_ref
from pyqmc_amd import _ffi, systems
from pyqmc_amd.configs import OpenConfigs, OpenElectron, PeriodicConfigs
from tests import helpers

pytestmark = pytest.mark.gpu

TOL = 1e-10


@pytest.fixture(scope="module")
def g():
    return helpers.golden(geminal_ref.GOLDEN)


def _configs(g, name, x=None):
    x = np.array(g[name + "_configs"] if x is None else x)
    return PeriodicConfigs(x, g[name + "_lattice"]) if name == "c" else OpenConfigs(x)


def _wf(g, name, gcoeff=None):
    import pyqmc_amd as pa

    wf = pa.GeminalJastrow(geminal_ref.case_mol(name))
    wf.parameters["gcoeff"] = g[name + "_gcoeff"] if gcoeff is None else gcoeff
    return wf


def _check(err):
    bad = {k: v for k, v in err.items() if not v < TOL}
    assert not bad, bad


@pytest.mark.parametrize("name", list(geminal_ref.CASES))
def test_golden_arrays(g, name):
    p = name + "_"
    W, electrons, many, keep = geminal_ref.CASES[name]
    ksl = slice(None) if keep is None else slice(0, keep)
    fsl = slice(None) if keep is None else slice(None, None, 8)
    wf = _wf(g, name)
    configs = _configs(g, name)
    sign, val = wf.recompute(configs)
    assert np.array_equal(sign, np.ones(W)) and wf.dtype is float and val.shape == (W,)
    err = {"value": helpers.relerr(val, g[p + "value"]), "ao_val": helpers.relerr(wf._get_state()[0][ksl], g[p + "ao_val"])}
    for e in electrons:
        q = p + f"e{e}_"
        mask, accept = g[q + "mask"], g[q + "accept"]
        ep, ea = configs.make_irreducible(e, g[q + "newpos"]), configs.make_irreducible(e, g[q + "aux"])
        gr, v, saved = wf.gradient_value(e, ep)
        assert saved is not None and gr.shape == (3, W) and v.shape == (W,)
        err[q + "gv_grad"], err[q + "gv_val"] = helpers.relerr(gr, g[q + "gv_grad"]), helpers.relerr(v, g[q + "gv_val"])
        err[q + "grad"] = helpers.relerr(wf.gradient(e, ep), g[q + "grad"])
        gr, lap = wf.gradient_laplacian(e, ep)
        err[q + "gl_grad"], err[q + "gl_lap"] = helpers.relerr(gr, g[q + "gl_grad"]), helpers.relerr(lap, g[q + "gl_lap"])
        tv, none = wf.testvalue(e, ep)
        assert none is None and tv.shape == (W,)
        err[q + "testvalue"] = helpers.relerr(tv, g[q + "testvalue"])
        err[q + "testvalue_mask"] = helpers.relerr(wf.testvalue(e, ep, mask)[0], g[q + "testvalue_mask"])
        err[q + "testvalue_aux"] = helpers.relerr(wf.testvalue(e, ea)[0], g[q + "testvalue_aux"])
        err[q + "testvalue_aux_mask"] = helpers.relerr(wf.testvalue(e, ea, mask)[0], g[q + "testvalue_aux_mask"])
        tm = wf.testvalue_many(list(many), ep)
        assert tm.shape == (W, 3)
        err[q + "testvalue_many"] = helpers.relerr(tm, g[q + "testvalue_many"])
        err[q + "testvalue_many_mask"] = helpers.relerr(wf.testvalue_many(list(many), ep, mask), g[q + "testvalue_many_mask"])
        # one auxiliary point per walker, an all-False mask, a single True
        r1 = wf.testvalue(e, configs.make_irreducible(e, g[q + "aux"][:, :1]))[0]
        assert r1.shape == (W, 1)
        err[q + "testvalue_aux_npt1"] = helpers.relerr(r1, g[q + "testvalue_aux"][:, :1])
        none = np.zeros(W, dtype=bool)
        assert wf.testvalue(e, ep, none)[0].shape == (0,) and wf.testvalue(e, ea, none)[0].shape == (0, 5)
        assert wf.testvalue_many(list(many), ep, none).shape == (0, 3)
        single = none.copy()
        single[W // 2] = True
        err[q + "testvalue_single"] = helpers.relerr(wf.testvalue(e, ep, single)[0], g[q + "testvalue"][W // 2 : W // 2 + 1])
        err[q + "testvalue_aux_single"] = helpers.relerr(wf.testvalue(e, ea, single)[0], g[q + "testvalue_aux"][W // 2 : W // 2 + 1])
        err[q + "testvalue_many_single"] = helpers.relerr(wf.testvalue_many(list(many), ep, single), g[q + "testvalue_many"][W // 2 : W // 2 + 1])
        wf.updateinternals(e, ep, configs, mask=accept)
        configs.move(e, ep, accept)
        err[q + "post_value"] = helpers.relerr(wf.value()[1], g[q + "post_value"])
    ao, x = wf._get_state()
    assert np.array_equal(x, configs.configs)
    err["final_ao_moved"] = helpers.relerr(ao[fsl][:, list(electrons), :], g[p + "final_ao_moved"])
    pg = wf.pgradient()
    assert sorted(pg) == ["gcoeff"] and pg["gcoeff"].shape == (W, wf.nao * (wf.nao + 1) // 2)
    err["pgrad_gcoeff"] = helpers.relerr(pg["gcoeff"][ksl], g[p + "pgrad_gcoeff"])
    err["pgrad contracted"] = helpers.relerr(pg["gcoeff"] @ g[p + "gcoeff"], wf.value()[1])
    print(name, {k: f"{v:.1e}" for k, v in err.items()})
    _check(err)


@pytest.mark.parametrize("name", ["a", "c"])
def test_single_walker(g, name):
    p = name + "_"
    wf = _wf(g, name)
    configs = _configs(g, name, g[p + "configs"][:1])
    e = int(g[p + "electrons"][0])
    q = p + f"e{e}_"
    err = {"value": helpers.relerr(wf.recompute(configs)[1], g[p + "value"][:1])}
    ep = configs.make_irreducible(e, g[q + "newpos"][:1])
    gr, lap = wf.gradient_laplacian(e, ep)
    err["gl_grad"], err["gl_lap"] = helpers.relerr(gr, g[q + "gl_grad"][:, :1]), helpers.relerr(lap, g[q + "gl_lap"][:1])
    err["testvalue_aux"] = helpers.relerr(wf.testvalue(e, configs.make_irreducible(e, g[q + "aux"][:1]))[0], g[q + "testvalue_aux"][:1])
    err["testvalue_many"] = helpers.relerr(wf.testvalue_many(list(g[p + "many"]), ep), g[q + "testvalue_many"][:1])
    wf.updateinternals(e, ep, configs)
    assert wf.pgradient()["gcoeff"].shape == (1, wf.nao * (wf.nao + 1) // 2)
    _check(err)


def test_update_ratio_recompute_triangle(g):
    """testwf.test_updateinternals on case b: two sweeps of masked moves of all 64 electrons."""
    wf = _wf(g, "b")
    configs = _configs(g, "b")
    W, N, _ = configs.configs.shape
    rng = np.random.default_rng(8)
    _, v0 = wf.recompute(configs)
    logratio = np.zeros(W)
    for _ in range(2):
        for e in range(N):
            ep = OpenElectron(configs.configs[:, e] + 0.5 * rng.standard_normal((W, 3)), configs.dist)
            mask = rng.random(W) > 0.4
            logratio[mask] += np.log(wf.testvalue(e, ep, mask)[0])
            wf.updateinternals(e, ep, configs, mask=mask)
            configs.move(e, ep, mask)
    _, v1 = wf.value()
    ao, x = wf._get_state()
    assert np.array_equal(x, configs.configs)
    fresh = _wf(g, "b")
    _, v2 = fresh.recompute(configs)
    err = {"ratio product": helpers.relerr(logratio, v1 - v0), "value": helpers.relerr(v1, v2), "ao_val": helpers.relerr(ao, fresh._get_state()[0])}
    print(err)
    assert np.max(np.abs(v1 - v0)) > 0.1
    _check(err)


@pytest.mark.parametrize("name", ["a", "c"])
def test_saved_row_update_is_bitwise_the_plain_one(g, name):
    p = name + "_"
    e = int(g[p + "electrons"][1])
    q = p + f"e{e}_"
    states = []
    for use in (True, False):
        wf = _wf(g, name)
        configs = _configs(g, name)
        wf.recompute(configs)
        ep = configs.make_irreducible(e, g[q + "newpos"])
        _, _, saved = wf.gradient_value(e, ep)
        wf.updateinternals(e, ep, configs, mask=g[q + "accept"], saved_values=saved if use else None)
        states.append((wf._get_state(), wf.value()[1]))
    (a0, x0), v0 = states[0]
    (a1, x1), v1 = states[1]
    assert np.array_equal(a0, a1) and np.array_equal(x0, x1) and np.array_equal(v0, v1)
    # a token of another evaluation, or for another electron, does not select the saved row: the plain route gives the same state
    wf = _wf(g, name)
    configs = _configs(g, name)
    wf.recompute(configs)
    ep = configs.make_irreducible(e, g[q + "newpos"])
    _, _, stale = wf.gradient_value(e, ep)
    wf.gradient_value(e, configs.electron(e))
    wf.updateinternals(e, ep, configs, mask=g[q + "accept"], saved_values=stale)
    assert np.array_equal(wf._get_state()[0], a0)


def test_parameters(g):
    import pyqmc_amd as pa

    wf = _wf(g, "a")
    configs = _configs(g, "a")
    _, v = wf.recompute(configs)
    assert set(wf.parameters) == {"gcoeff"} and wf.parameters["gcoeff"].shape == (23 * 24 // 2,)
    wf.parameters["gcoeff"] = 2 * g["a_gcoeff"]  # log Psi is linear in gcoeff, the AO values stay: no recompute needed
    assert helpers.relerr(wf.value()[1], 2 * v) < TOL
    for bad in (np.zeros(23 * 23), np.zeros(5), np.zeros((23, 23))):
        with pytest.raises(ValueError):
            wf.parameters["gcoeff"] = bad
    with pytest.raises(_ffi.PqaError, match="Wrong number of parameters.*529.*276"):
        wf._gem.call("pqa_geminal_set", _ffi.ptr(np.zeros(529)), 529)
    assert helpers.relerr(wf.recompute(configs)[1], 2 * v) < TOL
    d = pa.GeminalJastrow(geminal_ref.case_mol("a"))  # defaults of the reference: zeros
    assert np.array_equal(d.parameters["gcoeff"], np.zeros(276))
    assert np.array_equal(d.recompute(configs)[1], np.zeros(len(v)))
    assert np.array_equal(d.testvalue(1, OpenElectron(g["a_e1_newpos"]))[0], np.ones(len(v)))


def test_errors_name_what_is_missing(g):
    import pyqmc_amd as pa

    wf = _wf(g, "a")
    with pytest.raises(_ffi.PqaError, match="pqa_geminal_recompute"):
        wf._gem.call("pqa_geminal_value", _ffi.ptr(np.empty(4)))
    bare = pa.DeviceWF(geminal_ref.case_mol("a"))
    with pytest.raises(_ffi.PqaError, match="basis tables"):
        bare.call("pqa_geminal_set", _ffi.ptr(np.zeros(276)), 276)
    with pytest.raises(_ffi.PqaError, match="pqa_geminal_set"):
        bare.call("pqa_geminal_recompute", _ffi.ptr(np.zeros((2, 8, 3))), 2, _ffi.ptr(np.empty(2)))
    wf.recompute(_configs(g, "a"))
    with pytest.raises(_ffi.PqaError, match="electron index"):
        wf.gradient(8, OpenElectron(np.zeros((24, 3))))
    with pytest.raises(_ffi.PqaError, match="electron index"):
        wf.testvalue_many([0, 8], OpenElectron(np.zeros((24, 3))))
    with pytest.raises(_ffi.PqaError, match="walker index"):
        wf._gem.call("pqa_geminal_eval", 0, _ffi.ptr(np.zeros((1, 3))), 1, 1, _ffi.ptr(np.array([24], dtype=np.int32)), 0, 0, _ffi.ptr(np.empty(1)))


@pytest.mark.parametrize("case", ["twist", "complex"])
def test_twisted_and_complex_handles_raise(case):
    import pyqmc_amd as pa

    sup, mf = helpers.twist_case("prim") if case == "twist" else helpers.pbc_complex_case()
    dev = pa.Slater(sup, mf)._dev
    assert dev.twisted if case == "twist" else dev.cplx
    with pytest.raises(NotImplementedError, match="twisted and complex"):
        pa.GeminalJastrow(sup, _gem=dev)
    with pytest.raises(_ffi.PqaError, match="not implemented for twisted or complex"):
        dev.call("pqa_geminal_set", _ffi.ptr(np.zeros(3)), 3)


@pytest.mark.parametrize("how", ["copy", "pickle"])
def test_copies_are_independent(g, how):
    wf = _wf(g, "a")
    configs = _configs(g, "a")
    _, v = wf.recompute(configs)
    twin = copy.copy(wf) if how == "copy" else pickle.loads(pickle.dumps(wf))
    assert twin._gem is not wf._gem and twin._gem._h.value != wf._gem._h.value
    assert np.array_equal(twin.parameters["gcoeff"], wf.parameters["gcoeff"])
    assert helpers.relerr(twin.value()[1], v) < TOL
    e = int(g["a_electrons"][0])
    ep = OpenElectron(g[f"a_e{e}_newpos"])
    assert helpers.relerr(twin.testvalue(e, ep)[0], g[f"a_e{e}_testvalue"]) < TOL
    twin.updateinternals(e, ep, configs)
    assert np.max(np.abs(twin.value()[1] - v)) > 1e-3
    assert np.array_equal(wf.value()[1], v)
    twin.parameters["gcoeff"] = np.zeros(276)
    assert np.array_equal(wf.value()[1], v) and np.array_equal(wf.parameters["gcoeff"], g["a_gcoeff"])


def test_product_with_slater_and_jastrow(g):
    import sys

    import pyqmc_amd as pa
    from pyqmc_amd.wf import readonly_device

    mol = systems.water()
    sj = helpers.gpu_wf(mol, systems.random_mf(mol))
    sl, ja = sj.wf_factors
    gm = _wf(g, "a")
    wf = pa.MultiplyWF(sl, ja, gm)
    configs = _configs(g, "a")
    W = len(configs.configs)
    sign, logv = wf.recompute(configs)
    parts = [f.value() for f in (sl, ja, gm)]
    assert helpers.relerr(logv, sum(p[1] for p in parts)) < TOL and np.array_equal(sign, np.prod([p[0] for p in parts], axis=0))
    assert np.max(np.abs(parts[2][1])) > 0.1
    e = 5
    ep = OpenElectron(g["a_e5_newpos"])
    gs, ls = zip(*[f.gradient_laplacian(e, ep) for f in (sl, ja, gm)])
    cross = sum(np.sum(gs[i] * gs[j], axis=0) for i in range(3) for j in range(i + 1, 3))
    gr, lap = wf.gradient_laplacian(e, ep)
    assert helpers.relerr(gr, sum(gs)) < TOL and helpers.relerr(lap, sum(ls) + 2 * cross) < TOL
    assert helpers.relerr(wf.testvalue(e, ep)[0], np.prod([f.testvalue(e, ep)[0] for f in (sl, ja, gm)], axis=0)) < TOL
    assert helpers.relerr(wf.testvalue_many([1, 5], ep), np.prod([f.testvalue_many([1, 5], ep) for f in (sl, ja, gm)], axis=0)) < TOL
    # the product takes the per-factor protocol route, the fused drivers and estimators refuse it
    assert wf.fused_device() is None and readonly_device(wf) is None
    assert sys.modules["pyqmc_amd.vmc"].device_of(wf) is None and sys.modules["pyqmc_amd.vmc"].device_of(gm) is None
    with pytest.raises(NotImplementedError, match="lives on one device handle"):
        pa.vmc_worker(wf, configs, 0.3, 1, {})
    np.random.seed(3)
    blk, configs = helpers.protocol_vmc_worker(wf, configs, 0.3, 1, {})
    assert 0.1 < blk["acceptance"] < 1.0
    _, v_run = wf.value()
    _, v_new = wf.recompute(configs)
    assert helpers.relerr(v_run, v_new) < TOL
    assert wf.pgradient()["wf3gcoeff"].shape == (W, 276)


def test_unit_disturbs_nothing(g):
    """A Slater x JastrowSpin wave function gives bitwise the same recompute and energy before and after a GeminalJastrow is created
    and exercised on the same device."""
    mol = systems.water()
    sj = helpers.gpu_wf(mol, systems.random_mf(mol))
    configs = _configs(g, "a")
    dev = sj.fused_device()

    def both():
        s, v = sj.recompute(configs)
        return s.copy(), v.copy(), dev.energy(seed=5).copy()

    before = both()
    gm = _wf(g, "a")
    gm.recompute(configs)
    e = 1
    ep = OpenElectron(g["a_e1_newpos"])
    _, _, saved = gm.gradient_value(e, ep)
    gm.testvalue(e, OpenElectron(g["a_e1_aux"]), g["a_e1_mask"])
    gm.testvalue_many([0, 3, 6], ep)
    gm.updateinternals(e, ep, configs, mask=g["a_e1_accept"], saved_values=saved)
    gm.pgradient()
    after = both()
    for a, b in zip(before, after):
        assert np.array_equal(a, b)
    del gm
    for a, b in zip(before, both()):
        assert np.array_equal(a, b)
