"""One-body density matrix of three-body wave functions on the fused route (pqa_obdm_sweeps_j3 /
OBDMAccumulator(three_body_device=True)): the ratios against wf.testvalue_many on the same points, the whole accumulator against the
protocol route, chunking and determinism, handles without a three-body factor against the existing entries, no side effects on the
wave function's handle, the resident driver path and route selection.

Metrics and bounds: err = max |a - b| / (1 + |b|) < 1e-10 for device against protocol on the same walkers and draws;
helpers.relerr < 1e-9 where only the summation order of a walker mean differs; bitwise where stated.  Every comparison covers every
walker and every listed electron.  Sizes follow test_gpu_obdm_fused.py: 70 walkers, 3 sweeps, 37 auxiliary walkers."""

import copy
import importlib

import numpy as np
import pytest

from pyqmc_amd import systems
from pyqmc_amd.configs import OpenConfigs, PeriodicConfigs
from tests import helpers
from test_gpu_obdm_fused import LISTS, NAUX, NSW, W70, _accumulator, _basis, _electrons, _evaluator, _numpy_estimator, _place
from test_gpu_tbdm_fused import _configs, _err, _no_jastrow

pytestmark = pytest.mark.gpu


def _check_ratios(mol, wf, ev, W, seed, lists, make=OpenConfigs, x=None, start=None, reference_points=None):
    """The ratios of pqa_obdm_sweeps_j3 against wf.testvalue_many at the same points, and both modes of the estimator against NumPy
    on those ratios, for every electron list."""
    from pyqmc_amd.obdm import device_obdm_sweeps_j3

    rng = np.random.default_rng(seed)
    if x is None:
        x = _configs(mol, W, seed).configs
    N = x.shape[1]
    if start is None:
        start = x[rng.integers(0, W, NAUX), rng.integers(0, N, NAUX)] + 0.5 * rng.standard_normal((NAUX, 3))
    naux = len(start)
    kept = _place(ev, start, NSW, rng)
    pick = rng.integers(0, naux, (NSW, W)).astype(np.int32)
    dev = wf.fused_device()
    assert dev.has_j3 and dev.na3 == 4 and dev.nb3 == 4
    wf.recompute(make(x.copy()))
    worst = 0.0
    for name, kw in lists.items():
        es = _electrons(mol, **kw)
        pts = kept if reference_points is None else reference_points(kept)
        ref = np.stack([wf.testvalue_many(es, ev.container(pts[s][pick[s]]).electron(0)) for s in range(NSW)])
        assert np.all(np.isfinite(ref)) and np.max(np.abs(ref)) > 1e-6
        out = device_obdm_sweeps_j3(dev, ev, es, NSW, assign=pick, with_ratios=True)
        err = _err(out["ratio"], ref)
        value, norm = _numpy_estimator(ev, x, es, kept, pick, ref)
        got_v = ev.fetch(0, W, (ev.norb, ev.norb), 1.0, False)
        got_n = ev.fetch(1, W, (ev.norb,), 1.0, False)
        ev_err = max(_err(got_v, value), _err(got_n, norm))
        m = device_obdm_sweeps_j3(dev, ev, es, NSW, assign=pick, mean=True)
        m_err = max(_err(m["value"] * NSW, value.mean(axis=0)), _err(m["norm"] * NSW, norm.mean(axis=0)))
        print(f"obdm j3 {name}: ratios {err:.2e} (max |ref| {np.max(np.abs(ref)):.2e}) per-walker {ev_err:.2e} mean {m_err:.2e}")
        assert err < 1e-10 and ev_err < 1e-10 and m_err < 1e-10, (name, err, ev_err, m_err)
        worst = max(worst, err)
    return x, kept, pick, worst


def _three_body_matters(wf, x, make=OpenConfigs):
    """The three-body factor moves the ratios by far more than the bound (the comparison is not one of a factor of 1)."""
    wf.recompute(make(x.copy()))
    q = make(x[:, :1].copy() + 0.3).electron(0)
    r3 = wf.wf_factors[2].testvalue(0, q)[0]
    assert np.max(np.abs(r3 - 1.0)) > 1e-4


# ------------------------------------------------------------------------------------------------------------ 1. ratios
@pytest.mark.parametrize("jastrow", [True, False])
def test_water_every_list(jastrow):
    """70 walkers (no multiple of 64 or 16), 3 sweeps, 37 auxiliary walkers; both spins, all electrons, an unordered mixed list; with
    the two-body coefficients zeroed."""
    mol = systems.water()
    mf = systems.random_mf(mol)
    wf = helpers.gpu_wf3(mol, mf)
    if not jastrow:
        _no_jastrow(wf)
    x, *_ = _check_ratios(mol, wf, _evaluator(mol, mf, 3), W70, 1, LISTS)
    _three_body_matters(wf, x)


def test_six_determinants():
    """The C4 shape: several determinants x two-body x three-body."""
    mol = systems.water()
    mf = systems.random_mf(mol, nvirt=6)
    wf = helpers.gpu_wf3(mol, mf, systems.random_determinants(mol, mf, 6))
    assert wf.fused_device().ndet == 6
    _check_ratios(mol, wf, _evaluator(mol, mf, 3), W70, 3, {"all": dict(), "mixed": dict(electrons=[5, 1, 6])})


def test_chain_longer_than_the_cutoffs():
    """water_cluster(5, 1, 1): 40 electrons and 15 atoms, several passes of the item loop; the chain is longer than both cutoffs, so
    ions and pairs on both sides of rcut_a3 and rcut_b3 occur (asserted from the host coordinates)."""
    mol = systems.water_cluster(5, 1, 1)
    assert mol.nelec == (20, 20) and mol.natm == 15
    mf = systems.random_mf(mol)
    wf = helpers.gpu_wf3(mol, mf)
    dev = wf.fused_device()
    rca, rcb = dev._ctor["a3_basis"][0].rcut, dev._ctor["b3_basis"][0].rcut
    x, kept, pick, _ = _check_ratios(mol, wf, _evaluator(mol, mf, 3), W70, 4, {"up": dict(spin=0), "mixed": dict(electrons=[25, 3, 39, 0])})
    d_ion = np.linalg.norm(x[:, :, None, :] - np.asarray(mol.atom_coords())[None, None], axis=-1)
    d_pair = np.linalg.norm(x[:, :, None, :] - x[:, None, :, :], axis=-1)[:, np.triu_indices(x.shape[1], 1)[0], np.triu_indices(x.shape[1], 1)[1]]
    q = kept[0][pick[0]]
    q_ion = np.linalg.norm(q[:, None, :] - np.asarray(mol.atom_coords())[None], axis=-1)
    q_pair = np.linalg.norm(q[:, None, :] - x, axis=-1)
    for d, rc in ((d_ion, rca), (q_ion, rca), (d_pair, rcb), (q_pair, rcb)):
        assert np.any(d < rc) and np.any(d > rc), (d.min(), d.max(), rc)


def test_periodic_unfolded_points_equal_folded():
    """diamond_primitive at Gamma with a three-body factor: auxiliary points pushed out of the cell by whole lattice vectors against
    testvalue_many at the folded points."""
    import pyqmc_amd as pa

    sup, wf = helpers.gpu_pbc_wf("gamma", jastrow3=True)
    wf.parameters["wf3ccoeff"] = helpers.ccoeff_params(sup)
    _, kmf = helpers.pbc_slater_case("gamma")
    kpts = np.asarray(kmf.kpts)
    orb = [np.asarray(kmf.mo_coeff[0][k])[:, :3] for k in range(len(kpts))]
    ev = pa.obdm.OrbitalEvaluator(sup, orb, kpts=kpts)
    lat = sup.lattice_vectors()
    W, N = 16, sum(sup.nelec)
    rng = np.random.default_rng(5)
    x = rng.random((W, N, 3)) @ lat
    start = rng.random((NAUX, 3)) @ lat + rng.integers(-2, 3, (NAUX, 3)).astype(float) @ lat
    inv = np.linalg.inv(lat)

    def folded(kept):
        f = kept @ inv
        assert np.max(np.abs(np.floor(f))) >= 1.0  # (points outside the cell are among them)
        return (f - np.floor(f)) @ lat

    make = lambda y: PeriodicConfigs(y, lat)  # noqa: E731
    _check_ratios(sup, wf, ev, W, 6, {"all": dict(), "down": dict(spin=1)}, make=make, x=x, start=start, reference_points=folded)
    _three_body_matters(wf, x, make)


# ------------------------------------------------------------------------------------------------------------ 2. whole accumulator
@pytest.mark.parametrize("case", ["up", "mixed_naux"])
def test_fused_matches_protocol(case):
    mol = systems.water()
    mf = systems.random_mf(mol)
    wf = helpers.gpu_wf3(mol, mf)
    configs = _configs(mol, W70, 7)
    wf.recompute(configs)
    kw = dict(spin=0) if case == "up" else dict(spin=None, electrons=np.array([5, 1, 6]), naux=NAUX)
    wts = np.random.default_rng(3).random(W70) + 0.2
    out, states = {}, {}
    for route, flag in ((None, True), ("protocol", False)):
        make = lambda: _accumulator(mol, mf, route, three_body_device=flag, **kw)  # noqa: E731
        acc, acc2 = make(), make()
        np.random.seed(23)
        first, second = acc(configs, wf), acc(configs, wf)
        states[flag] = np.random.get_state()
        np.random.seed(23)
        avg = acc2.avg(configs, wf)
        name = "fused" if flag else "protocol"
        assert acc.last_route == name and acc2.last_route == name
        out[name] = (first, second, avg)
        if flag:
            acc3, acc4 = make(), make()
            np.random.seed(23)
            res = acc3.avg_resident(wf)
            np.random.seed(23)
            resw = acc4.avg_resident(wf, weights=wts)
            assert acc3.last_route == "fused" and acc4.last_route == "fused"
            for k in ("value", "norm"):
                assert np.array_equal(res[k], avg[k]), k  # (one entry, the same arguments)
                e = helpers.relerr(resw[k], np.tensordot(wts, first[k], axes=(0, 0)) / wts.sum())
                print(f"obdm j3 {case} avg_resident(weights) against the weighted mean of __call__ {k}: {e:.2e}")
                assert e < 1e-9, (k, e)
    for a, b in zip(states[True], states[False]):
        assert np.array_equal(a, b)
    for call in (0, 1):
        f, p = out["fused"][call], out["protocol"][call]
        err = _err(f["value"], p["value"])
        print(f"obdm j3 fused vs protocol {case} call {call}: value {err:.2e}")
        assert f["value"].shape == p["value"].shape == (W70, 4, 4) and err < 1e-10
        assert np.array_equal(f["norm"], p["norm"])  # (formed by k_obdm_acc from the same kept rows on both routes)
    for route in ("fused", "protocol"):
        per, avg = out[route][0], out[route][2]
        for k in ("value", "norm"):
            err = helpers.relerr(avg[k], per[k].mean(axis=0))
            print(f"obdm j3 {route} {case} avg against mean(__call__) {k}: {err:.2e}")
            assert err < 1e-9, (route, k, err)
    assert _err(out["fused"][2]["value"], out["protocol"][2]["value"]) < 1e-10


def test_device_rng():
    mol = systems.water()
    mf = systems.random_mf(mol)
    wf = helpers.gpu_wf3(mol, mf)
    configs = _configs(mol, W70, 10)
    wf.recompute(configs)
    runs = []
    for seed in (31, 31, 32):
        acc = _accumulator(mol, mf, None, rng="device", naux=NAUX, three_body_device=True)
        np.random.seed(seed)
        d = acc.avg(configs, wf)
        assert acc.last_route == "fused" and acc.last_assign.shape == (NSW, W70)
        assert acc.last_assign.min() >= 0 and acc.last_assign.max() < NAUX
        runs.append((d, acc.last_assign.copy()))
    assert np.array_equal(runs[0][1], runs[1][1]) and not np.array_equal(runs[0][1], runs[2][1])
    for k in ("value", "norm"):
        assert np.array_equal(runs[0][0][k], runs[1][0][k]) and not np.array_equal(runs[0][0][k], runs[2][0][k])


# ------------------------------------------------------------------------------------------------------------ 3. determinism
def test_chunking_and_two_calls_are_bitwise():
    """walker_chunk = 24 at 70 walkers against one chunk, in both modes (the mean mode takes whole 64-walker slices); a second call."""
    from pyqmc_amd.obdm import device_obdm_sweeps_j3

    mol = systems.water()
    mf = systems.random_mf(mol)
    wf = helpers.gpu_wf3(mol, mf)
    ev = _evaluator(mol, mf, 4)
    x, kept, pick, _ = _check_ratios(mol, wf, ev, W70, 8, {})
    dev, es = wf.fused_device(), np.arange(8)
    out = []
    for chunk in (0, 24, 0):
        r = device_obdm_sweeps_j3(dev, ev, es, NSW, assign=pick, walker_chunk=chunk, with_ratios=True)
        per = (ev.fetch(0, W70, (4, 4), 1.0, False), ev.fetch(1, W70, (4,), 1.0, False))
        m = device_obdm_sweeps_j3(dev, ev, es, NSW, assign=pick, walker_chunk=chunk, mean=True)
        out.append((r["ratio"], per[0], per[1], m["value"], m["norm"]))
    for other in out[1:]:
        for a, b in zip(out[0], other):
            assert np.array_equal(a, b)
    assert np.max(np.abs(out[0][0])) > 1e-6


def test_without_three_body_factor_equals_the_existing_entries():
    """A handle without a three-body factor through pqa_obdm_sweeps_j3: the bits of pqa_obdm_sweeps and pqa_obdm_sweeps_w."""
    from pyqmc_amd.obdm import device_obdm_sweeps, device_obdm_sweeps_j3, device_obdm_sweeps_w

    mol = systems.water()
    mf = systems.random_mf(mol, nvirt=6)
    wf = helpers.gpu_wf(mol, mf, systems.random_determinants(mol, mf, 6))
    ev = _evaluator(mol, mf, 4)
    rng = np.random.default_rng(12)
    x = _configs(mol, W70, 12).configs
    start = x[rng.integers(0, W70, NAUX), rng.integers(0, 8, NAUX)] + 0.5 * rng.standard_normal((NAUX, 3))
    _place(ev, start, NSW, rng)
    pick = rng.integers(0, NAUX, (NSW, W70)).astype(np.int32)
    wts = rng.random(W70) + 0.2
    dev, es = wf.fused_device(), np.array([5, 1, 6, 2])
    assert not dev.has_j3
    wf.recompute(OpenConfigs(x.copy()))
    got = []
    for fn in (device_obdm_sweeps, device_obdm_sweeps_j3):
        r = fn(dev, ev, es, NSW, assign=pick, with_ratios=True, walker_chunk=24)
        per = (ev.fetch(0, W70, (4, 4), 1.0, False), ev.fetch(1, W70, (4,), 1.0, False))
        m = fn(dev, ev, es, NSW, assign=pick, mean=True)
        w = device_obdm_sweeps_w(dev, ev, es, NSW, wts, assign=pick) if fn is device_obdm_sweeps else fn(dev, ev, es, NSW, assign=pick, mean=True, weights=wts)
        got.append((r["ratio"], per[0], per[1], m["value"], m["norm"], w["value"], w["norm"]))
    for a, b in zip(*got):
        assert np.array_equal(a, b)
    assert np.max(np.abs(got[0][0])) > 1e-6


# ------------------------------------------------------------------------------------------------------------ 4. no side effects
def test_no_side_effects_on_handle():
    import pyqmc_amd as pa

    mol = systems.water()
    mf = systems.random_mf(mol, nvirt=6)
    dets = systems.random_determinants(mol, mf, 6)
    runs = []
    for evaluate in (True, False):
        wf = helpers.gpu_wf3(mol, mf, dets)
        configs = _configs(mol, 96, 10)
        wf.recompute(configs)
        _, configs = pa.vmc_worker(wf, configs, 0.3, 2, {}, seed=3, state_current=True)  # leaves the state in the sweep's layout
        sl, ja, j3 = wf.wf_factors

        def state():
            return [sl._get_state(0), sl._get_state(1), ja._get_state(), wf.value(), j3.value(), [wf.fused_device().configs()]]

        if evaluate:
            before = state()
            for kw in (dict(spin=0), dict(spin=None)):
                acc = _accumulator(mol, mf, None, three_body_device=True, **kw)
                np.random.seed(5)
                acc(configs, wf)
                acc.avg(configs, wf)
                assert acc.last_route == "fused"
            for b, a in zip(before, state()):
                for u, v in zip(b, a):
                    assert np.array_equal(u, v)
        else:
            state()  # (the same reads of the state, so that the two runs differ by the evaluation alone)
        blk, after = pa.vmc_worker(wf, configs, 0.3, 2, {}, seed=4, state_current=True)
        runs.append((after.configs.copy(), blk["acceptance"]))
    assert np.array_equal(runs[0][0], runs[1][0]) and runs[0][1] == runs[1][1]


# ------------------------------------------------------------------------------------------------------------ 5. driver
def test_driver_takes_the_resident_path(monkeypatch):
    """{energy, rdm1_up, rdm1_down} of a three-body wave function, 96 walkers, 3 sweeps: the resident path with the flag, the host path
    without; energy keys and walkers bitwise equal, density matrices within the bound."""
    import pyqmc_amd as pa
    pvmc = importlib.import_module("pyqmc_amd.vmc")  # (the package exports the function vmc under that name)

    mol = systems.water()
    mf = systems.random_mf(mol)
    wf = helpers.gpu_wf3(mol, mf)
    start = _configs(mol, 96, 12)
    taken = []
    for name in ("_vmc_worker_resident_accumulators", "_vmc_worker_host_accumulators"):
        inner = getattr(pvmc, name)
        monkeypatch.setattr(pvmc, name, lambda *a, _n=name, _f=inner, **k: (taken.append(_n), _f(*a, **k))[1])
    out = {}
    for flag in (True, False):
        accs = {"energy": pa.EnergyAccumulator(mol), "rdm1_up": _accumulator(mol, mf, None, spin=0, three_body_device=flag),
                "rdm1_down": _accumulator(mol, mf, None, spin=1, three_body_device=flag)}
        np.random.seed(11)
        blk, cfg = pa.vmc_worker(wf, copy.deepcopy(start), 0.3, 3, accs, seed=5)
        out[flag] = (blk, cfg, np.random.get_state())
        want = "fused" if flag else "protocol"
        assert accs["rdm1_up"].last_route == want and accs["rdm1_down"].last_route == want
    assert taken == ["_vmc_worker_resident_accumulators", "_vmc_worker_host_accumulators"]
    bf, bp = out[True][0], out[False][0]
    assert set(bf) == set(bp)
    for k in bf:
        if k.startswith("energy") or k == "acceptance":
            assert np.array_equal(bf[k], bp[k]), k
        elif k.startswith("rdm1"):
            err = _err(bf[k], bp[k])
            print(f"obdm j3 driver {k}: {err:.2e}")
            assert err < 1e-10, (k, err)
    assert np.array_equal(out[True][1].configs, out[False][1].configs)
    for a, b in zip(out[True][2], out[False][2]):
        assert np.array_equal(a, b)


# ------------------------------------------------------------------------------------------------------------ 6. routing
def test_flag_off_behaves_as_today():
    mol = systems.water()
    mf = systems.random_mf(mol)
    wf = helpers.gpu_wf3(mol, mf)
    configs = _configs(mol, 6, 11)
    wf.recompute(configs)
    acc = _accumulator(mol, mf, None)
    assert acc.three_body_device is False and acc.resolve_route(wf, 6) == "protocol"
    np.random.seed(2)
    d = acc(configs, wf)
    assert acc.last_route == "protocol" and np.all(np.isfinite(d["value"]))
    with pytest.raises(ValueError, match="real Slater \\(x two-body Jastrow\\) product"):
        _accumulator(mol, mf, "fused")(configs, wf)
    on = _accumulator(mol, mf, None, three_body_device=True)
    assert on.resolve_route(wf, 6) == "fused" and _accumulator(mol, mf, "fused", three_body_device=True).resolve_route(wf, 6) == "fused"
    assert on.resolve_route(wf, 5) == "protocol"  # (the resident walkers are not the configurations)
    # a wave function without a three-body factor keeps the existing entry with the flag on
    wf2 = helpers.gpu_wf(mol, mf)
    wf2.recompute(configs)
    outs = []
    for flag in (False, True):
        a = _accumulator(mol, mf, None, three_body_device=flag)
        np.random.seed(2)
        outs.append(a(configs, wf2))
        assert a.last_route == "fused" and not a._j3_entry(wf2.fused_device())
    assert np.array_equal(outs[0]["value"], outs[1]["value"]) and np.array_equal(outs[0]["norm"], outs[1]["norm"])


@pytest.mark.parametrize("kind", ["complex", "twisted"])
def test_complex_and_twisted_are_refused(kind):
    import pyqmc_amd as pa
    from pyqmc_amd._ffi import PqaError
    from pyqmc_amd.obdm import device_obdm_sweeps_j3

    sup, kmf = helpers.pbc_complex_case() if kind == "complex" else helpers.twist_case("prim")
    wf = pa.generate_wf(sup, kmf, jastrow3=True)
    a, b = helpers.pbc_jastrow_coeffs(sup)
    wf.parameters["wf2acoeff"], wf.parameters["wf2bcoeff"] = a, b
    wf.parameters["wf3ccoeff"] = helpers.ccoeff_params(sup)
    dev = wf.fused_device()
    assert dev.cplx and dev.has_j3 and dev.twisted == (kind == "twisted")
    kpts = np.asarray(kmf.kpts)
    orb = [np.asarray(kmf.mo_coeff[0][k])[:, :2] for k in range(len(kpts))]
    W = 4
    configs = pa.initial_guess(sup, W, rng=np.random.default_rng(12))
    wf.recompute(configs)
    # both flags on: a complex or twisted three-body handle stays on the protocol route, with a reason
    acc = pa.OBDMAccumulator(sup, orb, kpts=kpts, nsweeps=1, warmup=2, spin=0, complex_device=True, three_body_device=True)
    assert acc.resolve_route(wf, W) == "protocol" and "complex or twisted" in acc._out_of_scope(wf, W)
    np.random.seed(3)
    d = acc(configs, wf)
    assert acc.last_route == "protocol" and np.all(np.isfinite(d["value"]))
    with pytest.raises(ValueError, match="complex or twisted"):
        pa.OBDMAccumulator(sup, orb, kpts=kpts, nsweeps=1, warmup=2, spin=0, route="fused", three_body_device=True)(configs, wf)
    # the entry itself
    with pytest.raises(PqaError, match="complex orbitals / twisted cell") as info:
        device_obdm_sweeps_j3(dev, acc.orbitals, [0], 1, assign=np.zeros((1, W), dtype=np.int32))
    assert "pqa_obdm_sweeps_j3" in str(info.value) and "protocol route" in str(info.value)
