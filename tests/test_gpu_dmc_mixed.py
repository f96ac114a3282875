"""DMC mixed estimators from the resident walkers: the weighted walker means sum_w w_w res_w / sum_w w_w of every accumulator with a
read-only fused route (pqa_obdm_sweeps_w, pqa_dm_points_resident + pqa_dm_fetch_w, pqa_sq_w, S^2 and the symmetry ratios weighted on
the host) and the "resident" accumulator route of dmc_propagate / rundmc against the "host" route.

Bounds: sums computed in the same order are compared bitwise (np.array_equal); where only the summation order differs the bound is
helpers.relerr < 1e-9 (tests/test_gpu_sr_moments.py, tests/test_gpu_obdm_fused.py).  Every figure is printed before it is asserted."""

import copy
import ctypes
import importlib

import numpy as np
import pytest

from pyqmc_amd import systems
from pyqmc_amd.configs import OpenConfigs, PeriodicConfigs
from tests import helpers
from test_gpu_obdm_fused import _accumulator, _evaluator, _place
from test_gpu_symmetry import GENERIC, SIGMA_X
from test_gpu_tbdm_fused import _configs

pytestmark = pytest.mark.gpu

W70, NSW, NAUX, TOL = 70, 3, 37, 1e-9
LISTS = {"up": dict(spin=0), "down": dict(spin=1), "mixed": dict(spin=None, electrons=np.array([5, 1, 6]))}


def _weights(W, seed):
    """exp(N(0, 1)) with two of them exactly 0."""
    w = np.exp(np.random.default_rng(seed).standard_normal(W))
    w[[3, W - 2]] = 0.0
    return w


def _wmean(w, res):
    return np.einsum("i,i...->...", w, res) / w.sum()


def _check(tag, got, ref):
    err = helpers.relerr(got, ref)
    print(f"dmc mixed {tag}: relerr {err:.2e}")
    assert np.max(np.abs(ref)) > 1e-8, tag  # (the comparison is not one of zeros)
    assert err < TOL, (tag, err)
    return err


def _weighted_obdm_against_call(mol, wf, configs, make, w, seed):
    """avg_resident(wf, w) against sum w res / sum w in NumPy on the fused __call__ from equal seeds; unit weights against avg."""
    wf.recompute(configs)
    a, b, c, d = (make() for _ in range(4))
    np.random.seed(seed)
    per = a(configs, wf)
    sa = np.random.get_state()
    np.random.seed(seed)
    got = b.avg_resident(wf, weights=w)
    sb = np.random.get_state()
    assert a.last_route == "fused" and b.last_route == "fused"
    for u, v in zip(sa, sb):
        assert np.array_equal(u, v)
    for k in ("value", "norm"):
        _check(f"obdm {k}", got[k], _wmean(w, per[k]))
    np.random.seed(seed)
    plain = c.avg(configs, wf)
    np.random.seed(seed)
    unit = d.avg_resident(wf, weights=np.ones(len(w)))
    for k in ("value", "norm"):
        assert np.array_equal(plain[k], unit[k]), k


# ------------------------------------------------------------------------------------------------------------ 1. weighted OBDM
@pytest.mark.parametrize("which", list(LISTS))
def test_obdm_weighted_water(which):
    mol = systems.water()
    mf = systems.random_mf(mol)
    wf = helpers.gpu_wf(mol, mf)
    _weighted_obdm_against_call(mol, wf, _configs(mol, W70, 7), lambda: _accumulator(mol, mf, None, naux=NAUX, **LISTS[which]), _weights(W70, 1), 23)


def test_obdm_weighted_chunks_and_repeat_bitwise():
    """200 walkers with walker_chunk = 64 (slices 64, 64, 64, 8) against one chunk, and two calls, bit for bit; unit weights give
    the bits of pqa_obdm_sweeps(mean=1); an evaluator that has only run the weighted mode holds no per-walker accumulator."""
    from pyqmc_amd import _ffi
    from pyqmc_amd.obdm import device_obdm_sweeps, device_obdm_sweeps_w

    mol = systems.water()
    mf = systems.random_mf(mol)
    wf = helpers.gpu_wf(mol, mf)
    W = 200
    ev = _evaluator(mol, mf, 4)
    rng = np.random.default_rng(8)
    x = _configs(mol, W, 8).configs
    wf.recompute(OpenConfigs(x.copy()))
    start = x[rng.integers(0, W, NAUX), rng.integers(0, 8, NAUX)] + 0.5 * rng.standard_normal((NAUX, 3))
    _place(ev, start, NSW, rng)
    pick = rng.integers(0, NAUX, (NSW, W)).astype(np.int32)
    dev, es, w = wf.fused_device(), np.arange(8), _weights(W, 2)
    one = device_obdm_sweeps_w(dev, ev, es, NSW, w, assign=pick)
    a, b = ctypes.c_int64(0), ctypes.c_int64(0)
    _ffi.check(ev.dev._h, _ffi.lib().pqa_obdm_bytes(ev.dev._h, ctypes.byref(a), ctypes.byref(b)))
    assert b.value == 0 and a.value > 0
    many = device_obdm_sweeps_w(dev, ev, es, NSW, w, assign=pick, walker_chunk=64)
    again = device_obdm_sweeps_w(dev, ev, es, NSW, w, assign=pick)
    for k in ("value", "norm"):
        assert np.array_equal(one[k], many[k]) and np.array_equal(one[k], again[k]), k
    unit = device_obdm_sweeps_w(dev, ev, es, NSW, np.ones(W), assign=pick, walker_chunk=64)
    plain = device_obdm_sweeps(dev, ev, es, NSW, assign=pick, mean=True)
    for k in ("value", "norm"):
        assert np.array_equal(unit[k], plain[k]), k
    # and against NumPy on the per-walker mode
    device_obdm_sweeps(dev, ev, es, NSW, assign=pick)
    _check("obdm 200 walkers value", one["value"], _wmean(w, ev.fetch(0, W, (4, 4), 1.0 / NSW, False)))
    _check("obdm 200 walkers norm", one["norm"], _wmean(w, ev.fetch(1, W, (4,), 1.0 / NSW, False)))


def test_obdm_weighted_twenty_orbitals():
    """water_cluster(5, 1, 1) with 20 orbitals: two MFMA tiles each way, tail 4."""
    mol = systems.water_cluster(5, 1, 1)
    mf = systems.random_mf(mol)
    wf = helpers.gpu_wf(mol, mf)
    _weighted_obdm_against_call(mol, wf, _configs(mol, W70, 4), lambda: _accumulator(mol, mf, None, norb=20, naux=NAUX, spin=0), _weights(W70, 3), 5)


def test_obdm_weighted_six_determinants():
    mol = systems.water()
    mf = systems.random_mf(mol, nvirt=6)
    wf = helpers.gpu_wf(mol, mf, systems.random_determinants(mol, mf, 6))
    _weighted_obdm_against_call(mol, wf, _configs(mol, W70, 3), lambda: _accumulator(mol, mf, None, naux=NAUX, spin=None), _weights(W70, 4), 6)


def _gamma_obdm(sup, kmf, spin):
    import pyqmc_amd as pa

    kpts = np.asarray(kmf.kpts)
    orb = [np.asarray(kmf.mo_coeff[0][k])[:, :3] for k in range(len(kpts))]
    return pa.obdm.OBDMAccumulator(sup, orb, nsweeps=2, warmup=3, tstep=0.4, spin=spin, kpts=kpts)


def test_obdm_weighted_gamma_cell():
    sup, wf = helpers.gpu_pbc_wf("gamma")
    _, kmf = helpers.pbc_slater_case("gamma")
    lat = sup.lattice_vectors()
    W = 32
    configs = PeriodicConfigs(np.random.default_rng(5).random((W, sum(sup.nelec), 3)) @ lat, lat)
    _weighted_obdm_against_call(sup, wf, configs, lambda: _gamma_obdm(sup, kmf, 0), _weights(W, 5), 7)


def test_obdm_weighted_device_rng():
    """rng="device": the weighted call draws the assignments the per-walker call draws from the same numpy seed."""
    mol = systems.water()
    mf = systems.random_mf(mol)
    wf = helpers.gpu_wf(mol, mf)
    configs = _configs(mol, W70, 10)
    wf.recompute(configs)
    w = _weights(W70, 6)
    a, b = (_accumulator(mol, mf, None, rng="device", naux=NAUX) for _ in range(2))
    assert b.resident_scope(wf) is None
    np.random.seed(31)
    per = a(configs, wf)
    np.random.seed(31)
    got = b.avg_resident(wf, weights=w)
    assert np.array_equal(a.last_assign, b.last_assign) and b.last_assign.max() < NAUX
    for k in ("value", "norm"):
        _check(f"obdm device rng {k}", got[k], _wmean(w, per[k]))


# ------------------------------------------------------------------------------------------------------------ 2. TBDM
def _tbdm(mol, mf, spin, **kw):
    import pyqmc_amd as pa

    C = np.asarray(mf.mo_coeff)
    return pa.TBDMAccumulator(mol, [C[0][:, :4], C[1][:, :3]], spin=spin, nsweeps=2, tstep=0.4, warmup=4, **kw)


FIVE = [(0, 1, 2, 0), (3, 3, 1, 1), (1, 0, 0, 2), (2, 2, 2, 2), (0, 3, 1, 0)]


@pytest.mark.parametrize("spin,ijkl", [((0, 0), None), ((0, 1), None), ((0, 1), FIVE)], ids=["upup-full", "updown-full", "updown-five"])
def test_tbdm_resident_weighted(spin, ijkl):
    mol = systems.water()
    mf = systems.random_mf(mol)
    wf = helpers.gpu_wf(mol, mf)
    configs = _configs(mol, W70, 9)
    wf.recompute(configs)
    w = _weights(W70, 7)
    a, b, c, d = (_tbdm(mol, mf, spin, ijkl=ijkl) for _ in range(4))
    assert b.resident_scope(wf) is None
    np.random.seed(17)
    per = a(configs, wf)
    sa = np.random.get_state()
    np.random.seed(17)
    got = b.avg_resident(wf, weights=w)
    sb = np.random.get_state()
    assert a.last_route == "fused" and b.last_route == "fused"
    for u, v in zip(sa, sb):
        assert np.array_equal(u, v)
    assert set(got) == {"value", "norm_a", "norm_b"} and got["value"].shape == per["value"].shape[1:]
    for k in got:
        _check(f"tbdm {spin} {k}", got[k], _wmean(w, per[k]))
    np.random.seed(17)
    plain = c.avg(configs, wf)
    np.random.seed(17)
    res = d.avg_resident(wf)
    for k in plain:  # (the plain mean of the resident evaluation: the per-walker accumulators hold the same bits)
        assert np.array_equal(plain[k], res[k]), k
    again = b.orbitals.fetch_w(0, W70, got["value"].shape, 0.5, w)
    assert np.array_equal(again, got["value"])


@pytest.mark.parametrize("periodic", [False, True])
def test_points_resident_bitwise(periodic):
    """pqa_dm_points_resident leaves the slot rows pqa_dm_points writes from the fetched coordinates: the following per-walker sweep
    accumulates the same bits."""
    from pyqmc_amd.obdm import device_obdm_sweeps
    from pyqmc_amd.tbdm import device_tbdm_sweep

    import pyqmc_amd as pa

    rng = np.random.default_rng(12)
    if periodic:
        sup, wf = helpers.gpu_pbc_wf("gamma")
        _, kmf = helpers.pbc_slater_case("gamma")
        kpts = np.asarray(kmf.kpts)
        orb = [np.asarray(kmf.mo_coeff[0][k])[:, :3] for k in range(len(kpts))]
        ev = pa.obdm.OrbitalEvaluator(sup, orb, kpts=kpts)
        lat = sup.lattice_vectors()
        W, mol = 16, sup
        configs = PeriodicConfigs(rng.random((W, sum(sup.nelec), 3)) @ lat, lat)
    else:
        mol = systems.water()
        mf = systems.random_mf(mol)
        wf = helpers.gpu_wf(mol, mf)
        ev = _evaluator(mol, mf, 3)
        W = W70
        configs = _configs(mol, W, 12)
    wf.recompute(configs)
    dev = wf.fused_device()
    nup, N = mol.nelec[0], sum(mol.nelec)
    es = [np.arange(nup), np.arange(nup, N)]
    x = dev.configs()
    start = x[rng.integers(0, W, NAUX), rng.integers(0, N, NAUX)] + 0.3 * rng.standard_normal((NAUX, 3))
    for slot in (0, 1):
        pos = np.ascontiguousarray(start).copy()
        ev.walk(slot, slot, pos, 0.3 * rng.standard_normal((1, NAUX, 3)), np.zeros((1, NAUX)), 1.0, 1)
    pick = rng.integers(0, NAUX, (2, W)).astype(np.int32)
    ijkl = np.array(FIVE, dtype=np.int32).T % 3
    out = []
    for resident in (False, True):
        for slot in (0, 1):
            if resident:
                ev.points_resident(slot, dev, es[slot])
            else:
                ev.points(slot, slot, x[:, es[slot]])
        device_tbdm_sweep(dev, ev, 0, (0, 1), pick[0], pick[1], ijkl, True)
        out.append([ev.fetch(i, W, sh, 1.0, False) for i, sh in enumerate(((5,), (3,), (3,)))])
    for u, v in zip(*out):
        assert np.array_equal(u, v) and np.max(np.abs(u)) > 0
    assert np.array_equal(dev.configs(), x)


# ------------------------------------------------------------------------------------------------------------ 3. S(q)
@pytest.mark.parametrize("case", ["water-qlist", "gamma-grid", "gamma-qlist"])
def test_sq_weighted(case):
    import pyqmc_amd as pa
    from pyqmc_amd.sq import device_sq, device_sq_w

    rng = np.random.default_rng(14)
    if case == "water-qlist":
        mol = systems.water()
        wf = helpers.gpu_wf(mol, systems.random_mf(mol))
        W = W70
        configs = _configs(mol, W, 14)
        acc = pa.SqAccumulator(mol, qlist=rng.standard_normal((7, 3)))
    else:
        mol, wf = helpers.gpu_pbc_wf("gamma")
        lat = mol.lattice_vectors()
        W = 70
        configs = PeriodicConfigs(rng.random((W, sum(mol.nelec), 3)) @ lat, lat)
        acc = pa.SqAccumulator(mol, nq=2) if case == "gamma-grid" else pa.SqAccumulator(mol, qlist=rng.standard_normal((5, 3)))
    wf.recompute(configs)
    dev, w = wf.fused_device(), _weights(W, 8)
    assert acc.resident_scope(wf) is None
    per = acc(configs, wf)
    got = acc.avg_resident(wf, weights=w)
    assert acc.last_route == "fused"
    for k in ("Sq", "spinSq"):
        _check(f"sq {case} {k}", got[k], _wmean(w, per[k]))
    unit = device_sq_w(dev, acc.qlist, np.ones(W), acc.qn, acc.recip)
    plain = device_sq(dev, acc.qlist, acc.qn, acc.recip, mean=True)
    for u, v, k in zip(unit, plain, ("Sq", "spinSq")):
        _check(f"sq {case} unit weights {k}", u, v)
    again = acc.avg_resident(wf, weights=w)
    assert all(np.array_equal(again[k], got[k]) for k in got)
    mean = acc.avg_resident(wf)
    assert all(np.array_equal(mean[k], p) for k, p in zip(("Sq", "spinSq"), plain))


# ------------------------------------------------------------------------------------------------------------ 4. S^2, symmetry
def test_s2_and_symmetry_weighted():
    import pyqmc_amd as pa

    mol = systems.water()
    wf = helpers.gpu_wf(mol, systems.random_mf(mol))
    configs = _configs(mol, W70, 15)
    wf.recompute(configs)
    w = _weights(W70, 9)
    for acc in (pa.S2Accumulator(mol.nelec), pa.SymmetryAccumulator({"sx": SIGMA_X, "g": GENERIC})):
        assert acc.resident_scope(wf) is None
        per, got, mean = acc(configs, wf), acc.avg_resident(wf, weights=w), acc.avg_resident(wf)
        assert acc.last_route == "fused" and set(got) == set(per)
        for k in per:
            _check(f"{type(acc).__name__} {k}", got[k], _wmean(w, per[k]))
            _check(f"{type(acc).__name__} {k} plain", mean[k], np.mean(per[k]))
    sup, pwf = helpers.gpu_pbc_wf("gamma")
    lat = sup.lattice_vectors()
    W = 32
    pconf = PeriodicConfigs(np.random.default_rng(9).random((W, sum(sup.nelec), 3)) @ lat, lat)
    pwf.recompute(pconf)
    a = sup.atom_coords()
    acc = pa.SymmetryAccumulatorPBC({"i": -np.eye(3), "g": GENERIC}, {"i": 0.5 * (a[0] + a[1]), "g": np.array([0.7, -0.3, 1.9])})
    w = _weights(W, 10)
    per, got = acc(pconf, pwf), acc.avg_resident(pwf, weights=w)
    for k in per:
        _check(f"SymmetryAccumulatorPBC {k}", got[k], _wmean(w, per[k]))


# ------------------------------------------------------------------------------------------------------------ 5. driver
def _dictionary(mol, mf):
    import pyqmc_amd as pa

    return {"energy": pa.EnergyAccumulator(mol), "rdm1_up": _accumulator(mol, mf, None, spin=0), "rdm1_down": _accumulator(mol, mf, None, spin=1),
            "tbdm_updown": _tbdm(mol, mf, (0, 1)), "s2": pa.S2Accumulator(mol.nelec),
            "sq": pa.SqAccumulator(mol, qlist=np.random.default_rng(1).standard_normal((5, 3))),
            "symmetry": pa.SymmetryAccumulator({"sx": SIGMA_X, "g": GENERIC})}


def _compare_blocks(br, bh, tag):
    assert set(br) == set(bh)
    worst = 0.0
    for k in br:
        if k.startswith("energy") or k in ("weight", "acceptance", "tmove_acceptance"):
            assert np.array_equal(br[k], bh[k]), k
        else:
            worst = max(worst, _check(f"{tag} {k}", br[k], bh[k]))
    return worst


def _propagate_both(wf, start, accs_of, nsteps, monkeypatch, tstep=0.02):
    import pyqmc_amd as pa

    dev = wf.fused_device()
    out = {}
    for route in ("resident", "host"):
        accs = accs_of()
        assert pa.dmc_accumulator_route(wf, accs)[0] == "resident"
        calls = []
        inner = type(dev).configs
        monkeypatch.setattr(type(dev), "configs", lambda self, _f=inner: (calls.append(1), _f(self))[1])
        np.random.seed(11)
        cfg = copy.deepcopy(start)
        weights = np.exp(0.1 * np.random.default_rng(2).standard_normal(cfg.configs.shape[0]))
        blk, cfg, weights = pa.dmc_propagate(wf, cfg, weights, tstep, 10.0, -17.0, -17.0, nsteps=nsteps, accumulators=accs, accumulator_route=route)
        monkeypatch.setattr(type(dev), "configs", inner)
        out[route] = (blk, cfg, weights, len(calls), np.random.get_state())
    r, h = out["resident"], out["host"]
    assert np.array_equal(r[1].configs, h[1].configs) and np.array_equal(r[2], h[2])
    assert np.array_equal(r[1].configs, dev.configs())
    for a, b in zip(r[4], h[4]):
        assert np.array_equal(a, b)
    return out


def test_driver_water(monkeypatch):
    mol = systems.water()
    mf = systems.random_mf(mol)
    wf = helpers.gpu_wf(mol, mf)
    out = _propagate_both(wf, _configs(mol, 96, 12), lambda: _dictionary(mol, mf), 3, monkeypatch)
    _compare_blocks(out["resident"][0], out["host"][0], "driver water")
    assert out["resident"][3] == 1 and out["host"][3] == 3  # one walker fetch against three


def test_driver_default_route_and_state(monkeypatch):
    """accumulator_route=None takes the resident route, and a seeded vmc_worker after the block is the one after the host route."""
    import pyqmc_amd as pa
    pdmc = importlib.import_module("pyqmc_amd.dmc")

    mol = systems.water()
    mf = systems.random_mf(mol)
    runs = []
    for route in (None, "host"):
        wf = helpers.gpu_wf(mol, mf)
        taken = []
        for name in ("_propagate_resident_accumulators", "_propagate_host_accumulators", "_propagate_fused"):
            inner = getattr(pdmc, name)
            monkeypatch.setattr(pdmc, name, lambda *a, _n=name, _f=inner, **k: (taken.append(_n), _f(*a, **k))[1])
        np.random.seed(3)
        cfg = _configs(mol, 96, 13)
        blk, cfg, w = pa.dmc_propagate(wf, cfg, np.ones(96), 0.02, 10.0, -17.0, -17.0, nsteps=2, accumulators=_dictionary(mol, mf),
                                       accumulator_route=route)
        assert taken == ["_propagate_resident_accumulators" if route is None else "_propagate_host_accumulators"]
        sl, ja = wf.wf_factors
        state = [sl._get_state(0), sl._get_state(1), ja._get_state(), wf.value()]
        vblk, after = pa.vmc_worker(wf, cfg, 0.3, 2, {}, seed=4, state_current=True)
        runs.append((state, after.configs.copy(), vblk["acceptance"], w.copy()))
        pa.dmc_propagate(wf, after, np.ones(96), 0.02, 10.0, -17.0, -17.0, nsteps=1, accumulators={"energy": pa.EnergyAccumulator(mol)})
        assert taken[-1] == "_propagate_fused"
        monkeypatch.undo()
    for b, a in zip(runs[0][0], runs[1][0]):
        for u, v in zip(b, a):
            assert np.array_equal(u, v)
    assert np.array_equal(runs[0][1], runs[1][1]) and runs[0][2] == runs[1][2] and np.array_equal(runs[0][3], runs[1][3])


def test_driver_gamma_cell(monkeypatch):
    import pyqmc_amd as pa

    sup, wf = helpers.gpu_pbc_wf("gamma")
    _, kmf = helpers.pbc_slater_case("gamma")
    x = systems.initial_guess(sup, 32, rng=np.random.default_rng(8)).configs.copy()
    start = PeriodicConfigs(x, sup.lattice_vectors())

    def accs():
        return {"energy": pa.EnergyAccumulator(sup), "rdm1_up": _gamma_obdm(sup, kmf, 0), "rdm1_down": _gamma_obdm(sup, kmf, 1),
                "sq": pa.SqAccumulator(sup, nq=1)}

    out = _propagate_both(wf, start, accs, 2, monkeypatch, tstep=0.05)
    _compare_blocks(out["resident"][0], out["host"][0], "driver gamma")
    assert np.array_equal(out["resident"][1].wrap, out["host"][1].wrap)


def test_rundmc_two_blocks():
    """2 blocks x 2 steps with device branching on both routes."""
    import pyqmc_amd as pa

    mol = systems.water()
    mf = systems.random_mf(mol)
    runs = {}
    for route in ("resident", "host"):
        wf = helpers.gpu_wf(mol, mf)
        np.random.seed(7)
        df, cfg, w = pa.rundmc(wf, _configs(mol, 96, 11), tstep=0.02, nblocks=2, nsteps_per_block=2, vmc_warmup=1, accumulators=_dictionary(mol, mf),
                               accumulator_route=route)
        runs[route] = (df, cfg.configs.copy(), w.copy(), np.random.get_state())
    r, h = runs["resident"], runs["host"]
    assert np.array_equal(r[1], h[1]) and np.array_equal(r[2], h[2])
    for a, b in zip(r[3], h[3]):
        assert np.array_equal(a, b)
    assert set(r[0]) == set(h[0])
    for k in r[0]:
        if k.startswith(("rdm1", "tbdm", "s2", "sq", "symmetry")):
            _check(f"rundmc {k}", r[0][k], h[0][k])
        else:
            assert np.array_equal(r[0][k], h[0][k]), k


class _Nothing:
    def avg(self, configs, wf):
        return {}

    def __call__(self, configs, wf):
        return {}

    def keys(self):
        return {}.keys()

    def shapes(self):
        return {}


def test_routing():
    import pyqmc_amd as pa

    mol = systems.water()
    mf = systems.random_mf(mol)
    wf = helpers.gpu_wf(mol, mf)
    en = pa.EnergyAccumulator(mol)
    assert pa.dmc_accumulator_route(wf, {"energy": en})[0] == "fused"
    assert pa.dmc_accumulator_route(wf, {"energy": en, "s2": pa.S2Accumulator(mol.nelec)})[0] == "resident"
    assert pa.dmc_accumulator_route(wf, {"energy": en, "rdm1": _accumulator(mol, mf, None, rng="device")})[0] == "resident"
    cases = [(wf, {"energy": en, "none": _Nothing()}, "avg_resident"),
             (wf, {"energy": en, "rdm1": _accumulator(mol, mf, "protocol")}, "protocol"),
             (helpers.gpu_wf3(mol, mf), {"energy": en, "s2": pa.S2Accumulator(mol.nelec)}, "three-body")]
    declined = pa.SqAccumulator(mol, qlist=np.ones((1, 3)))
    declined._fused = lambda configs, wf: None  # (the accumulator's own fused-route predicate decides for the resident route too)
    cases.append((wf, {"energy": en, "sq": declined}, "fused route"))
    sup, kmf = helpers.pbc_complex_case()
    cwf = pa.generate_wf(sup, kmf)
    assert cwf.fused_device().cplx
    cases.append((cwf, {"energy": pa.EnergyAccumulator(sup), "sq": pa.SqAccumulator(sup, nq=1)}, "complex"))
    for w_, accs, word in cases:
        route, why = pa.dmc_accumulator_route(w_, accs)
        print(f"dmc mixed routing: {route}: {why}")
        assert route == "host" and word in why, (route, why)
        W = 8
        cfg = pa.initial_guess(sup if w_ is cwf else mol, W, rng=np.random.default_rng(3))
        with pytest.raises(NotImplementedError, match=word):
            pa.dmc_propagate(w_, cfg, np.ones(W), 0.02, 10.0, -17.0, -17.0, nsteps=1, accumulators=accs, accumulator_route="resident")
    with pytest.raises(ValueError, match="accumulator_route"):
        pa.dmc_propagate(wf, _configs(mol, 8, 1), np.ones(8), 0.02, 10.0, -17.0, -17.0, nsteps=1, accumulators={"energy": en}, accumulator_route="device")


def test_refused_weights():
    """The library refuses weights the Python wrappers would have refused."""
    from pyqmc_amd import _ffi

    mol = systems.water()
    wf = helpers.gpu_wf(mol, systems.random_mf(mol))
    wf.recompute(_configs(mol, 8, 2))
    dev = wf.fused_device()
    q = np.ones((1, 3))
    out, out2 = np.empty(1), np.empty(1)
    for bad in (np.array([1.0] * 7 + [-1.0]), np.array([1.0] * 7 + [np.nan]), np.zeros(8)):
        with pytest.raises(_ffi.PqaError, match="weights"):
            dev.call("pqa_sq_w", 1, _ffi.ptr(q), None, None, _ffi.ptr(bad), _ffi.ptr(out), _ffi.ptr(out2))
