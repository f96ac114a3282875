"""The simultaneous ensemble estimator and the Jacobi-style driver on the host: the reference's StochasticReconfigurationMultipleWF
arithmetic (g52 a, b), round_to_fixed_sum (g52 c) and one iteration of the threaded optimize_ensemble with its file and restart
(g52 d, the sampling stubbed); mix_route's decisions on stand-in objects, what a forced device route refuses, and the three deliberate
differences from the reference."""

import types

import numpy as np
import pytest

import pyqmc_amd as pa
from pyqmc_amd import blockfile, ensemble, ensemble_threaded
from pyqmc_amd.accumulators import LinearTransform, StochasticReconfigurationMultipleWF, mix_route
from pyqmc_amd.accumulators_multiwf import EnergyAccumulatorMultipleWF
from pyqmc_amd.configs import OpenConfigs
from pyqmc_amd.energy import EnergyAccumulator
from tests import helpers
from tests.test_ensemble_cpu import TOL, FakeEnacc

K = 3


def fake_wf(params, pgrad=None, index=0):
    return types.SimpleNamespace(parameters=params, pgradient=lambda: pgrad, index=index)


def _to_opts():
    det = [np.array([False, True, True]), np.zeros(3, dtype=bool), np.zeros(3, dtype=bool)]
    b = [np.ones((3, 3), dtype=bool), np.zeros((3, 3), dtype=bool), np.zeros((3, 3), dtype=bool)]
    b[0][0] = False
    b[1][1:, :2] = True
    return [{"wf1det_coeff": det[i], "wf2bcoeff": b[i]} for i in range(K)]


def _name(k):
    return k if isinstance(k, str) else f"{k[0]}_{k[1]}"


def _a_objects(g):
    params = [{"wf1det_coeff": np.array([1.0, 0.3, -0.2]) + 0.1 * i, "wf2bcoeff": g[f"a_params_b{i}"]} for i in range(K)]
    transforms = [LinearTransform(p, o) for p, o in zip(params, _to_opts())]
    table = {"total": g["a_total"], "ke": g["a_ke"]}
    sr = StochasticReconfigurationMultipleWF(FakeEnacc(table), transforms, eps=0.05)
    wfs = [fake_wf(params[i], {"wf1det_coeff": g[f"a_pg_det{i}"], "wf2bcoeff": g[f"a_pg_b{i}"]}, i) for i in range(K)]
    return sr, wfs, transforms


def test_g52a_avg():
    g = helpers.golden("g52_ensemble_multi")
    sr, wfs, transforms = _a_objects(g)
    assert [t.nparams for t in transforms] == [8, 4, 0]
    avg = sr.avg(None, wfs, g["a_weights"])
    assert sr.last_route == "protocol"
    assert sorted(_name(k) for k in avg) == sorted(k[6:] for k in g.files if k.startswith("a_avg_"))
    for k, v in avg.items():
        assert helpers.relerr(v, g["a_avg_" + _name(k)]) < TOL, k
    assert ("dp", 2) not in avg and avg[("dp", 0)].shape == (8, K) and avg[("dpipj", 1)].shape == (4, 4)


def test_g52b_block_average_terms_delta_p():
    g = helpers.golden("g52_ensemble_multi")
    sr, _, transforms = _a_objects(g)
    data = {"total": g["b_data_total"]}
    for i in (0, 1):
        for k in ("dp", "dpH", "dpipj"):
            data[(k, i)] = g[f"b_data_{k}_{i}"]
    avg, err = sr.block_average(data, g["b_ov"])
    assert sorted(_name(k) for k in avg) == sorted(k[9:] for k in g.files if k.startswith("b_ba_avg_"))
    for k, v in avg.items():
        assert helpers.relerr(v, g["b_ba_avg_" + _name(k)]) < TOL, k
    for k, v in err.items():
        assert helpers.relerr(v, g["b_ba_err_" + _name(k)]) < TOL, k
    terms = sr._collect_terms(avg, err)
    assert sorted(_name(k) for k in terms) == sorted(k[5:] for k in g.files if k.startswith("b_ct_"))
    for k, v in terms.items():
        assert helpers.relerr(v, g["b_ct_" + _name(k)]) < TOL, k
    dp, report = sr.delta_p([0.1, 0.4], avg, g["b_penalty"])
    assert len(dp) == K and [np.shape(d) for d in dp] == [(2, 8), (2, 4), (2, 0)]
    for i in (0, 1):
        assert helpers.relerr(np.asarray(dp[i]), g[f"b_dp{i}"]) < 1e-10
    assert helpers.relerr([report["pgrad"], report["SRdot"]], g["b_report"]) < 1e-10
    assert sr.keys() == {"total", "dpH", "dppsi", "dpidpj"} and sr.multiple_wf is True
    sr.update_state(None)


def test_deliberate_differences():
    g = helpers.golden("g52_ensemble_multi")
    sr, wfs, transforms = _a_objects(g)
    # shapes(): what avg returns (the reference raises on a missing attribute)
    avg = sr.avg(None, wfs, g["a_weights"])
    shapes = sr.shapes()
    assert {k: np.shape(v) for k, v in avg.items() if k != "ke"} == shapes and shapes["total"] == (K, K)
    # weights=None: a ValueError that names the argument
    with pytest.raises(ValueError, match="weights"):
        sr.avg(None, wfs)
    # no state has parameters: an empty report
    none = [LinearTransform(w.parameters, {"wf1det_coeff": np.zeros(3, dtype=bool)}) for w in wfs]
    sr0 = StochasticReconfigurationMultipleWF(FakeEnacc(), none)
    data = {"total": g["b_ba_avg_total"], "overlap": g["b_ba_avg_overlap"]}
    dp, report = sr0.delta_p([0.1], data, g["b_penalty"])
    assert report == {} and [np.shape(d) for d in dp] == [(1, 0)] * K
    with pytest.raises(ValueError):
        StochasticReconfigurationMultipleWF(FakeEnacc(), none, route="fused")


def test_g52c_round_to_fixed_sum():
    g = helpers.golden("g52_ensemble_multi")
    for n in range(int(g["c_n"])):
        y = ensemble_threaded.round_to_fixed_sum(g[f"c_x{n}"], int(g[f"c_t{n}"]))
        assert np.array_equal(y, g[f"c_y{n}"]) and y.dtype.kind == "i", n
    with pytest.raises(ValueError):
        ensemble_threaded.round_to_fixed_sum(g["c_bad_x"], int(g["c_bad_t"]))


def _d_setup(g, monkeypatch):
    base = {"wf1det_coeff": np.array([1.0, 0.3, -0.2]), "wf2bcoeff": np.array([0.1, 0.2])}
    to_opt = {"wf1det_coeff": np.array([False, True, True]), "wf2bcoeff": np.array([True, True])}
    wfs = [fake_wf({k: v.copy() for k, v in base.items()}, index=0), fake_wf({k: v + 0.05 for k, v in base.items()}, index=1)]
    updater = [[ensemble.StochasticReconfigurationWfbyWf(FakeEnacc(), LinearTransform(w.parameters, to_opt), eps=0.02)] for w in wfs]
    calls = {"norm": 0, "so": [], "vmc": [], "warm": 0, "params": []}

    def sample_overlap(wfs_, configs_, energy, **kw):
        if energy is None:
            assert len(wfs_) == 2
            calls["norm"] += 1
            return {}, {"overlap": g["d_ov_norm"]}, configs_
        i = len(wfs_) - 1
        calls["so"].append(i)
        calls["params"].append([np.array(w.parameters["wf1det_coeff"]) for w in wfs_])
        return {"wtdp": g[f"d_wtdp{i}"]}, {"overlap": g[f"d_ov_sub{i}"]}, configs_

    def vmc(wf, configs_, accumulators=None, **kw):
        if accumulators is None:
            calls["warm"] += 1
            return None, configs_
        calls["vmc"].append(wf.index)
        return {k: g[f"d_s1_{k}{wf.index}"] for k in ("total", "dppsi", "dpH", "dpidpj")}, configs_

    monkeypatch.setattr(ensemble_threaded, "_sample_overlap", sample_overlap)
    monkeypatch.setattr(ensemble_threaded, "_vmc", vmc)
    return wfs, updater, calls


def test_g52d_threaded_iteration_file_and_restart(tmp_path, monkeypatch):
    g = helpers.golden("g52_ensemble_multi")
    wfs, updater, calls = _d_setup(g, monkeypatch)
    configs = OpenConfigs(g["d_configs"].copy())
    path = str(tmp_path / "ens.hdf5")
    ensemble_threaded.optimize_ensemble(wfs, configs, updater, path, tau=0.3, max_iterations=1, overlap_penalty=g["d_penalty"], verbose=False)
    # one normalisation sampling, every VMC run before every mixture sampling, all of them before any update
    assert calls["norm"] == 1 and calls["warm"] == 1 and calls["vmc"] == [0, 1] and calls["so"] == [0, 1]
    assert np.array_equal(calls["params"][1][0], calls["params"][0][0])  # (state 1's sampling saw state 0 before its step)
    st = blockfile.BlockFile(path)
    ds = st.datasets()
    for n in range(2):
        for k in ("energy", "energy_error", "overlap"):
            assert helpers.relerr(ds[f"{k}{n}"][0], g[f"d_rec{n}_{k}{n}"]) < TOL, (n, k)
    assert list(ds["iteration"]) == [0, 0] and list(ds["wavefunction"]) == [0, 1] and list(ds["sub_iteration"]) == [0, 0]
    assert st.attrs()["tau"] == 0.3
    for i, w in enumerate(wfs):
        for k, v in w.parameters.items():
            assert helpers.relerr(v, g[f"d_rec1_wf{i}_{k}"]) < TOL, (i, k)
    assert sorted(st.load_parameters()) == ["0/wf1det_coeff", "0/wf2bcoeff", "1/wf1det_coeff", "1/wf2bcoeff"]
    # restart: parameters and walkers from the file, from iteration max(iteration) + 1 = 1, no warm-up
    fresh = [fake_wf({k: np.zeros_like(v) for k, v in w.parameters.items()}, index=i) for i, w in enumerate(wfs)]
    expect = [{k: np.array(v) for k, v in w.parameters.items()} for w in wfs]
    _, updater2, calls2 = _d_setup(g, monkeypatch)
    seen = {}
    orig = ensemble_threaded._sample_overlap

    def spy(wfs_, configs_, energy, **kw):
        seen.setdefault("params", [{k: np.array(v) for k, v in w.parameters.items()} for w in wfs_])
        seen.setdefault("configs", configs_.configs.copy())
        return orig(wfs_, configs_, energy, **kw)

    monkeypatch.setattr(ensemble_threaded, "_sample_overlap", spy)
    cfg2 = OpenConfigs(np.zeros_like(configs.configs))
    ensemble_threaded.optimize_ensemble(fresh, cfg2, updater2, path, tau=0.3, max_iterations=2, overlap_penalty=g["d_penalty"], verbose=False)
    assert calls2["warm"] == 0 and calls2["norm"] == 1 and calls2["vmc"] == [0, 1]
    for a, b in zip(seen["params"], expect):
        for k in b:
            assert np.array_equal(a[k], b[k])
    assert np.array_equal(seen["configs"], g["d_configs"])
    assert list(blockfile.BlockFile(path).datasets()["iteration"]) == [0, 0, 1, 1]
    # nothing left to do: no sampling at all
    _, updater3, calls3 = _d_setup(g, monkeypatch)
    ensemble_threaded.optimize_ensemble(fresh, cfg2, updater3, path, tau=0.3, max_iterations=2, overlap_penalty=g["d_penalty"], verbose=False)
    assert calls3["norm"] == 0 and calls3["vmc"] == []


def test_threaded_refuses_a_client():
    for kw in (dict(client=object()), dict(npartitions=2), dict(overlap_thread_weight=[1.0])):
        with pytest.raises(NotImplementedError):
            ensemble_threaded.optimize_ensemble([], None, [], None, **kw)
        with pytest.raises(NotImplementedError):
            ensemble_threaded.evaluate_gradients_threaded([], [], [], **kw)


# ---- mix_route on stand-ins ----------------------------------------------------------------------------------------------------------


def _dev(pbc=False, twisted=False, device=0):
    return types.SimpleNamespace(pbc=pbc, twisted=twisted, device=device, cplx=False)


def _wf(dev):
    return types.SimpleNamespace(_product_device=lambda: dev, fused_device=lambda: dev, parameters={})


def _acc(keys=("wf1det_coeff", "wf2bcoeff"), enacc=None, n=2):
    params = {"wf1det_coeff": np.ones(3), "wf2acoeff": np.ones((2, 2, 2)), "wf2bcoeff": np.ones((3, 3)), "wf1mo_coeff_alpha": np.ones((4, 2)),
              "wf3ccoeff": np.ones((2, 2, 2, 2, 3))}
    tr = [LinearTransform(params, {k: np.ones(params[k].shape, dtype=bool) for k in keys}) for _ in range(n)]
    enacc = EnergyAccumulator.__new__(EnergyAccumulator) if enacc is None else enacc
    return StochasticReconfigurationMultipleWF(enacc, tr)


def test_mix_route_decisions():
    wfs = [_wf(_dev()), _wf(_dev())]
    assert mix_route(wfs, _acc())[0] == "device"
    assert mix_route(wfs, _acc(keys=("wf2acoeff",)))[0] == "device"
    cases = [
        ([_wf(_dev(pbc=True)), _wf(_dev())], _acc(), "periodic"),
        ([_wf(_dev(twisted=True)), _wf(_dev())], _acc(), "periodic"),
        ([_wf(None), _wf(_dev())], _acc(), "not a real Slater x two-body Jastrow"),
        ([_wf(_dev())] * 2, _acc(), "share a device handle"),
        ([_wf(_dev(device=0)), _wf(_dev(device=1))], _acc(), "different devices"),
        ([_wf(_dev()) for _ in range(9)], _acc(n=9), "9 wave functions"),
        (wfs, _acc(enacc=FakeEnacc()), "FakeEnacc"),
        (wfs, _acc(keys=("wf1det_coeff", "wf1mo_coeff_alpha")), "wf1mo_coeff_alpha"),
        (wfs, _acc(keys=("wf3ccoeff",)), "wf3ccoeff"),
    ]
    for w, acc, why in cases:
        route, reason = mix_route(w, acc)
        assert route == "protocol" and why in reason, (why, reason)
        assert acc.resolve_route(w) == "protocol"  # route=None falls back
        acc.route = "device"
        with pytest.raises(NotImplementedError, match=why):
            acc.resolve_route(w)
        acc.route = "protocol"
        assert acc.resolve_route(w) == "protocol"
    # a transform that is not a LinearTransform
    acc = _acc()
    acc.transforms = [types.SimpleNamespace(to_opt={}, nparams=0)] * 2
    assert mix_route(wfs, acc) == ("protocol", "transform 0 is a SimpleNamespace, not a pyqmc_amd.LinearTransform")


def test_forced_device_route_out_of_scope_raises():
    wfs = [_wf(_dev(pbc=True)), _wf(_dev())]
    weights = np.ones((2, 2, 4))
    with pytest.raises(NotImplementedError, match="periodic"):
        StochasticReconfigurationMultipleWF(EnergyAccumulator.__new__(EnergyAccumulator), _acc().transforms, route="device").avg(None, wfs, weights)
    params = {"wf1det_coeff": np.ones(3)}
    tr = LinearTransform(params)
    with pytest.raises(NotImplementedError, match="periodic"):
        ensemble.StochasticReconfigurationWfbyWf(EnergyAccumulator.__new__(EnergyAccumulator), tr, mixture_route="device").avg(None, wfs, weights)
    with pytest.raises(NotImplementedError, match="periodic"):
        EnergyAccumulatorMultipleWF(EnergyAccumulator.__new__(EnergyAccumulator), route="device").avg(None, wfs, weights)
    # the existing classes keep the protocol route unless asked: None never looks at the handles
    assert ensemble.StochasticReconfigurationWfbyWf(FakeEnacc(), tr).resolve_route(wfs) == "protocol"
    assert EnergyAccumulatorMultipleWF(FakeEnacc()).resolve_route(wfs) == "protocol"
    assert pa.StochasticReconfigurationMultipleWF is StochasticReconfigurationMultipleWF and pa.mix_route is mix_route
    for bad in (dict(mixture_route="fused"),):
        with pytest.raises(ValueError):
            ensemble.StochasticReconfigurationWfbyWf(FakeEnacc(), tr, **bad)
    with pytest.raises(ValueError):
        EnergyAccumulatorMultipleWF(FakeEnacc(), route="fused")
