"""Ensemble optimisation on the host: the reference's StochasticReconfigurationWfbyWf arithmetic, renormalize and one
optimize_ensemble iteration (g44 b, c, d), the multiple-wave-function accumulators, what sample_overlap refuses, and the block /
optimisation files with their restarts on both BlockFile back ends (the sampling stubbed)."""

import os
import types

import numpy as np
import pytest

from pyqmc_amd import blockfile, ensemble, sample_many
from pyqmc_amd.accumulators import LinearTransform
from pyqmc_amd.accumulators_multiwf import AdaptSingleAccumulator, EnergyAccumulatorMultipleWF
from pyqmc_amd.configs import OpenConfigs
from tests import helpers

TOL = 1e-12


class FakeEnacc:
    def __init__(self, table=None):
        self.table = table

    def __call__(self, configs, wf):
        return {k: v[wf.index] for k, v in self.table.items()}

    def keys(self):
        return {"total"}

    def shapes(self):
        return {"total": ()}


def fake_wf(params, pgrad=None, index=0):
    return types.SimpleNamespace(parameters=params, pgradient=lambda: pgrad, index=index)


def _b_objects(g):
    params = {"wf1det_coeff": np.array([1.0, 0.3, -0.2]), "wf2bcoeff": g["b_params_b"]}
    to_opt = {"wf1det_coeff": np.array([False, True, True]), "wf2bcoeff": np.ones((3, 3), dtype=bool)}
    to_opt["wf2bcoeff"][0] = False
    tr = LinearTransform(params, to_opt)
    return params, tr, ensemble.StochasticReconfigurationWfbyWf(FakeEnacc(), tr, eps=0.05)


def test_g44b_sr_wfbywf():
    g = helpers.golden("g44_ensemble")
    params, tr, sr = _b_objects(g)
    pgrad = {"wf1det_coeff": g["b_pg_det"], "wf2bcoeff": g["b_pg_b"]}
    wfs = [fake_wf(params), fake_wf(params), fake_wf(params, pgrad)]
    assert helpers.relerr(sr.avg(None, wfs, g["b_weights"])["wtdp"], g["b_avg_wtdp"]) < TOL
    s1 = {k: g["b_s1_" + k] for k in ("total", "dppsi", "dpH", "dpidpj")}
    avg, err = sr.block_average(s1, {"wtdp": g["b_wtdp"]}, g["b_ov"])
    for k, v in avg.items():
        assert helpers.relerr(v, g["b_ba_avg_" + k]) < TOL, k
    for k, v in err.items():
        assert helpers.relerr(v, g["b_ba_err_" + k]) < TOL, k
    terms = sr._collect_terms(avg, err)
    assert sorted(terms) == sorted(k[5:] for k in g.files if k.startswith("b_ct_"))
    for k, v in terms.items():
        assert helpers.relerr(v, g["b_ct_" + k]) < TOL, k
    dp, report = sr.delta_p([0.1, 0.4], avg, g["b_penalty"])
    assert helpers.relerr(np.asarray(dp), g["b_dp"]) < 1e-10
    assert helpers.relerr([report["pgrad"], report["SRdot"]], g["b_report"]) < 1e-10
    assert sr.keys() == {"total", "dpH", "dppsi", "dpidpj"} and sr.shapes() == {"dppsi": (tr.nparams,), "total": ()}
    assert sr.allwfs() is sr and sr.onewf().nodal_cutoff == 0.05  # (the reference's positional eps lands on nodal_cutoff)


def test_g44c_renormalize():
    g = helpers.golden("g44_ensemble")
    for key in ("wf1det_coeff", "det_coeff"):
        wfs = [fake_wf({key: np.array([1.0, 0.5 * i, -0.25])}) for i in range(3)]
        ensemble.renormalize(wfs, g["c_norms"], pivot=1, N=1.5)
        assert helpers.relerr(np.array([w.parameters[key] for w in wfs]), g["c_" + key]) < TOL
    with pytest.raises(NotImplementedError):
        ensemble.renormalize([fake_wf({"x": 1.0}), fake_wf({"x": 1.0})], [1.0, 2.0])


def _d_setup(g, monkeypatch):
    base = {"wf1det_coeff": np.array([1.0, 0.3, -0.2]), "wf2bcoeff": np.array([0.1, 0.2])}
    to_opt = {"wf1det_coeff": np.array([False, True, True]), "wf2bcoeff": np.array([True, True])}
    wfs = [fake_wf({k: v.copy() for k, v in base.items()}), fake_wf({k: v + 0.05 for k, v in base.items()})]
    updater = [[ensemble.StochasticReconfigurationWfbyWf(FakeEnacc(), LinearTransform(w.parameters, to_opt), eps=0.02)] for w in wfs]
    calls = {"so": 0, "vmc": 0, "warm": 0}

    def sample_overlap(wfs_, configs_, energy, **kw):
        i, first = calls["so"] // 2, calls["so"] % 2 == 0
        calls["so"] += 1
        assert (energy is None) == first and len(wfs_) == (2 if first else i + 1)
        if first:
            return {}, {"overlap": g[f"d_ov_all{i}"]}, configs_
        return {"wtdp": g[f"d_wtdp{i}"]}, {"overlap": g[f"d_ov_sub{i}"]}, configs_

    def vmc(wf, configs_, accumulators=None, **kw):
        if accumulators is None:
            calls["warm"] += 1
            return None, configs_
        i = calls["vmc"]
        calls["vmc"] += 1
        return {k: g[f"d_s1_{k}{i}"] for k in ("total", "dppsi", "dpH", "dpidpj")}, configs_

    monkeypatch.setattr(ensemble, "_sample_overlap", sample_overlap)
    monkeypatch.setattr(ensemble, "_vmc", vmc)
    return wfs, updater, calls


@pytest.fixture(params=["npz", "h5py"])
def backend(request, monkeypatch):
    if request.param == "h5py":
        import sys

        sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
        import fake_h5py

        monkeypatch.setattr(blockfile, "h5py", fake_h5py)
        monkeypatch.setattr(blockfile.BlockFile.__init__, "__defaults__", ("h5py",))
        yield "h5py"
        fake_h5py.forget()
    else:
        monkeypatch.setattr(blockfile.BlockFile.__init__, "__defaults__", ("npz",))
        yield "npz"


def test_g44d_one_iteration_file_and_restart(tmp_path, backend, monkeypatch):
    g = helpers.golden("g44_ensemble")
    wfs, updater, calls = _d_setup(g, monkeypatch)
    configs = OpenConfigs(g["d_configs"].copy())
    path = str(tmp_path / "ens.hdf5")
    ensemble.optimize_ensemble(wfs, configs, updater, path, tau=0.3, max_iterations=1, overlap_penalty=g["d_penalty"])
    assert calls == {"so": 4, "vmc": 2, "warm": 1}
    st = blockfile.BlockFile(path)
    ds = st.datasets()
    for n in range(2):
        for k in ("energy", "energy_error", "overlap"):
            v = ds[f"{k}{n}"][0]
            assert helpers.relerr(v, g[f"d_rec{n}_{k}{n}"]) < TOL, (n, k)
    assert list(ds["iteration"]) == [0, 0] and list(ds["wavefunction"]) == [0, 1] and list(ds["sub_iteration"]) == [0, 0]
    assert st.attrs()["tau"] == 0.3
    for i, w in enumerate(wfs):
        for k, v in w.parameters.items():
            assert helpers.relerr(v, g[f"d_rec1_wf{i}_{k}"]) < 1e-12, (i, k)
    stored = st.load_parameters()
    assert sorted(stored) == ["0/wf1det_coeff", "0/wf2bcoeff", "1/wf1det_coeff", "1/wf2bcoeff"]
    # restart (ensemble_optimization_wfbywf.py:251-268): iteration max(iteration) = 0, state wavefunction[-1] = 1, sub-iteration
    # sub_iteration[-1] + 1 = 1: state 1 has one sub-iteration, so iteration 0 has nothing left, and iteration 1 runs both states
    fresh = [fake_wf({k: np.zeros_like(v) for k, v in w.parameters.items()}) for w in wfs]
    _, updater2, calls2 = _d_setup(g, monkeypatch)
    cfg2 = OpenConfigs(np.zeros_like(configs.configs))
    seen = {}
    orig = ensemble._sample_overlap

    def spy(wfs_, configs_, energy, **kw):
        seen.setdefault("params", [{k: np.array(v) for k, v in w.parameters.items()} for w in wfs_])
        seen.setdefault("configs", configs_.configs.copy())
        return orig(wfs_, configs_, energy, **kw)

    monkeypatch.setattr(ensemble, "_sample_overlap", spy)
    ensemble.optimize_ensemble(fresh, cfg2, updater2, path, tau=0.3, max_iterations=2, overlap_penalty=g["d_penalty"])
    assert calls2["warm"] == 0 and calls2["vmc"] == 2
    for i in range(2):
        for k in ("wf1det_coeff", "wf2bcoeff"):
            assert np.array_equal(seen["params"][i][k], stored[f"{i}/{k}"])
    assert np.array_equal(seen["configs"], configs.configs)
    ds = blockfile.BlockFile(path).datasets()
    assert list(ds["iteration"]) == [0, 0, 1, 1] and list(ds["wavefunction"]) == [0, 1, 0, 1]


def test_optimize_ensemble_refuses_client():
    with pytest.raises(NotImplementedError):
        ensemble.optimize_ensemble([], None, [], None, client=object())
    with pytest.raises(NotImplementedError):
        ensemble.optimize_ensemble([], None, [], None, npartitions=2)


def test_multiwf_accumulators():
    rng = np.random.default_rng(3)
    K, W = 3, 9
    table = {"total": rng.standard_normal((K, W)), "ke": rng.standard_normal((K, W))}
    weights = rng.standard_normal((K, K, W))
    wfs = [fake_wf({}, index=k) for k in range(K)]
    cfg = OpenConfigs(np.zeros((W, 2, 3)))
    acc = EnergyAccumulatorMultipleWF(FakeEnacc(table), offset=-2.5)
    d = acc.avg(cfg, wfs, weights)
    for k in table:
        ref = np.array([[np.sum((table[k][j] + 2.5) * weights[i, j]) / W for j in range(K)] for i in range(K)])
        assert np.abs(d[k] - ref).max() < TOL
    assert float(d["offset"]) == -2.5 and d["offset"].dtype == float
    assert acc.keys() == {"total"} and acc.shapes() == {"total": ()}
    ad = AdaptSingleAccumulator(FakeEnacc(table))
    d2 = ad.avg(cfg, wfs, weights)
    assert "offset" not in d2 and np.abs(d2["total"] - (d["total"] - 2.5 * np.einsum("ijc->ij", weights) / W)).max() < 1e-12
    assert ad.keys() == {"total"} and ad.shapes() == {"total": ()}  # (read from .acc; the reference reads a missing .enacc)
    # the int default offset accumulates like the reference's blocks would need it to
    blk = {}
    sample_many.rolling_average(blk, EnergyAccumulatorMultipleWF(FakeEnacc(table)).avg(cfg, wfs, weights), 2)
    assert float(blk["offset"]) == 0.0


def test_sample_overlap_refusals():
    from pyqmc_amd.energy import EnergyAccumulator

    cfg = OpenConfigs(np.zeros((2, 2, 3)))
    single = EnergyAccumulator.__new__(EnergyAccumulator)
    with pytest.raises(NotImplementedError, match="EnergyAccumulatorMultipleWF"):
        sample_many.sample_overlap_worker([], cfg, 0.5, 1, single)
    with pytest.raises(NotImplementedError, match="EnergyAccumulatorMultipleWF"):
        sample_many.sample_overlap([], cfg, single)
    with pytest.raises(NotImplementedError, match="client"):
        sample_many.sample_overlap([], cfg, None, client=object())
    with pytest.raises(NotImplementedError, match="npartitions"):
        sample_many.sample_overlap([], cfg, None, npartitions=2)
    with pytest.raises(ValueError, match="route"):
        sample_many.sample_overlap_worker([], cfg, 0.5, 1, None, route="elsewhere")
    with pytest.raises(ValueError, match="fused"):
        sample_many.sample_overlap_worker([types.SimpleNamespace()], cfg, 0.5, 1, None, route="fused")


def test_normalize():
    rng = np.random.default_rng(4)
    ov = np.eye(2) * np.array([1.2, 0.7]) + 0.01 * rng.standard_normal((5, 2, 2))
    tot = rng.standard_normal((5, 2, 2))
    avg, err = sample_many.normalize({"total": tot}, {"overlap": ov})
    N = np.abs(np.mean(ov, axis=0).diagonal())
    assert np.abs(avg["total"] - np.mean(tot, axis=0) / np.sqrt(np.outer(N, N))).max() < TOL
    assert np.abs(err["overlap"] - np.std(ov, axis=0, ddof=1) / np.sqrt(5)).max() < TOL


def test_sample_overlap_file_and_restart(tmp_path, backend, monkeypatch):
    """The block file of sample_many.py:27-39 (groups weighted / unweighted, one record per block, the walkers) and its restart
    (:205-210): an existing file gives the starting walkers."""
    starts = []

    def worker(wfs, configs, tstep, nsteps, energy, route=None):
        starts.append(configs.configs.copy())
        configs.configs = configs.configs + 1.0
        n = len(starts)
        return {"total": np.full((2, 2), float(n)), "offset": np.asarray(0.0)}, {"acceptance": 0.0, "overlap": np.eye(2) * n}, configs

    monkeypatch.setattr(sample_many, "sample_overlap_worker", worker)
    path = str(tmp_path / "so.hdf5")
    cfg = OpenConfigs(np.zeros((3, 2, 3)))
    energy = EnergyAccumulatorMultipleWF(FakeEnacc())
    w, u, cfg = sample_many.sample_overlap([None, None], cfg, energy, nblocks=3, hdf_file=path)
    assert w["total"].shape == (3, 2, 2) and u["overlap"].shape == (3, 2, 2)
    st = blockfile.BlockFile(path)
    ds = st.datasets()
    assert sorted(ds) == ["unweighted/acceptance", "unweighted/overlap", "weighted/offset", "weighted/total"]
    assert np.array_equal(ds["weighted/total"][:, 0, 0], [1.0, 2.0, 3.0]) and ds["unweighted/overlap"].shape == (3, 2, 2)
    assert st.attrs()["tstep"] == 0.5
    back = OpenConfigs(np.zeros((3, 2, 3)))
    st.load_walkers(back)
    assert np.array_equal(back.configs, np.full((3, 2, 3), 3.0))
    # restart: the walkers come from the file
    cfg2 = OpenConfigs(np.full((3, 2, 3), -7.0))
    sample_many.sample_overlap([None, None], cfg2, None, nblocks=1, hdf_file=path)
    assert np.array_equal(starts[-1], np.full((3, 2, 3), 3.0))
    assert blockfile.BlockFile(path).datasets()["unweighted/overlap"].shape == (4, 2, 2)
