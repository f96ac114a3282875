"""Two-body density matrix on the fused route (pqa_tbdm_sweep / TBDMAccumulator(route="fused")): the pair ratios against recomputes
of the doubly moved configurations, chunking, agreement with the protocol route and the reference's g23, the layout sync after a
fused sweep, no side effects on the wave function's handle, and route selection.

Ground truth: ``wf.recompute`` on host copies with electron a at r1 and electron b at r2 (all pairs stacked into one recompute).
Metric and bound as in test_gpu_s2.py: max |R - direct| / (1 + |direct|) < 1e-10 (1e-9 above 32 electrons per spin)."""

import numpy as np
import pytest

from pyqmc_amd import systems
from pyqmc_amd.configs import OpenConfigs, PeriodicConfigs
from tests import helpers

pytestmark = pytest.mark.gpu

SECTORS = [(0, 1), (0, 0), (1, 0), (1, 1)]


def _water(nelec=(4, 4)):
    sym, xyz = zip(*systems._WATER)
    return systems.Mol(sym, xyz, nelec=nelec)


def _no_jastrow(wf):
    wf.parameters["wf2acoeff"] = np.zeros_like(wf.parameters["wf2acoeff"])
    wf.parameters["wf2bcoeff"] = np.zeros_like(wf.parameters["wf2bcoeff"])
    return wf


def _configs(mol, W, seed):
    import pyqmc_amd as pa

    return pa.initial_guess(mol, W, rng=np.random.default_rng(seed))


def _evaluator(mol, mf, norb=3, **kw):
    import pyqmc_amd as pa

    C = np.asarray(mf.mo_coeff)
    return pa.obdm.OrbitalEvaluator(mol, [C[0][:, :norb], C[1][:, :norb]], **kw)


def _place(ev, slot, pts):
    """``pts`` (n, 3) as the kept sample 0 of ``slot``: one walk sample whose proposal does not move (zero displacement tape)."""
    x = np.ascontiguousarray(pts, dtype=float).copy()
    n = len(x)
    _, kept = ev.walk(slot, slot, x, np.zeros((1, n, 3)), np.full((1, n), 0.5), 0.5, 1)
    assert np.array_equal(kept[0], pts)


def _direct(wf, make, x, r1, r2, sector, nel):
    """sign exp(dlog) (W, nea, neb) of one recompute of all doubly moved walkers; 0 where a and b are one electron."""
    s1, s2 = sector
    W = x.shape[0]
    pairs = [(a, b) for a in range(nel[s1]) for b in range(nel[s2]) if a + s1 * nel[0] != b + s2 * nel[0]]
    y = np.tile(x, (len(pairs) + 1, 1, 1))
    for p, (a, b) in enumerate(pairs):
        y[(p + 1) * W : (p + 2) * W, a + s1 * nel[0]] = r1
        y[(p + 1) * W : (p + 2) * W, b + s2 * nel[0]] = r2
    s, l = wf.recompute(make(y))
    out = np.zeros((W, nel[s1], nel[s2]))
    for p, (a, b) in enumerate(pairs):
        sl = slice((p + 1) * W, (p + 2) * W)
        out[:, a, b] = s[sl] / s[:W] * np.exp(l[sl] - l[:W])
    wf.recompute(make(x.copy()))
    return out


def _err(R, ref):
    return float(np.max(np.abs(R - ref) / (1 + np.abs(ref))))


def _check_sectors(mol, wf, ev, W, seed, sectors, tol=1e-10, make=OpenConfigs, spread=0.8):
    from pyqmc_amd.tbdm import device_pair_ratios

    rng = np.random.default_rng(seed)
    x = _configs(mol, W, seed).configs
    naux = W + 3  # (more auxiliary walkers than configurations: the assignment is a real indirection)
    aux = [x[rng.integers(0, W, naux), rng.integers(0, x.shape[1], naux)] + spread * rng.standard_normal((naux, 3)) for _ in (0, 1)]
    pick = [rng.integers(0, naux, W).astype(np.int32) for _ in (0, 1)]
    for s in (0, 1):
        _place(ev, s, aux[s])
    dev = wf.fused_device()
    wf.recompute(make(x.copy()))
    for sector in sectors:
        ref = _direct(wf, make, x, aux[0][pick[0]], aux[1][pick[1]], sector, mol.nelec)
        R = device_pair_ratios(dev, ev, 0, sector, pick[0], pick[1])
        err = _err(R, ref)
        print(f"tbdm fused ratios {sector}: {err:.2e} (max |direct| {np.max(np.abs(ref)):.2e})")
        assert err < tol, (sector, err)
        assert np.max(np.abs(ref)) > 1e-6
        if sector[0] == sector[1]:
            n = R.shape[1]
            assert np.all(R[:, np.arange(n), np.arange(n)] == 0.0)
    return x, aux, pick


@pytest.mark.parametrize("jastrow", [True, False])
def test_water_all_sectors(jastrow):
    """70 walkers: no multiple of a wave, a tile or a chunk."""
    mol = systems.water()
    mf = systems.random_mf(mol)
    wf = helpers.gpu_wf(mol, mf)
    if not jastrow:
        _no_jastrow(wf)
    _check_sectors(mol, wf, _evaluator(mol, mf), 70, 1, SECTORS)


def test_open_shell():
    """Restricted open shell (5, 3): nea != neb, a same-spin sector of 3."""
    mol = _water((5, 3))
    mf = systems.random_mf(mol)
    _check_sectors(mol, helpers.gpu_wf(mol, mf), _evaluator(mol, mf), 33, 2, SECTORS)


def test_multi_determinant():
    mol = systems.water()
    mf = systems.random_mf(mol, nvirt=6)
    wf = helpers.gpu_wf(mol, mf, systems.random_determinants(mol, mf, 6))
    _check_sectors(mol, wf, _evaluator(mol, mf), 32, 3, SECTORS)


def test_tile_edge():
    """20 electrons per spin: more than one 16-wide group of inverse rows and no multiple of it."""
    mol = systems.water_cluster(5, 1, 1)
    assert mol.nelec == (20, 20)
    mf = systems.random_mf(mol)
    _check_sectors(mol, helpers.gpu_wf(mol, mf), _evaluator(mol, mf), 8, 4, [(0, 0), (0, 1)])


def test_periodic_unfolded_points_equal_folded():
    """diamond_primitive at Gamma, 16 walkers: auxiliary points pushed out of the cell by whole lattice vectors give the ratios of
    the folded points (both within the bound of the ground truth, hence within twice the bound of each other: the fold of the orbital
    kernel and the minimal image round differently for a shifted point, so the two are not bitwise equal)."""
    import pyqmc_amd as pa
    from pyqmc_amd.tbdm import device_pair_ratios

    sup, wf = helpers.gpu_pbc_wf("gamma")
    _, kmf = helpers.pbc_slater_case("gamma")
    kpts = np.asarray(kmf.kpts)
    orb = [np.asarray(kmf.mo_coeff[0][k])[:, :3] for k in range(len(kpts))]
    ev = pa.obdm.OrbitalEvaluator(sup, orb, kpts=kpts)
    lat = sup.lattice_vectors()
    W, N = 16, sum(sup.nelec)
    rng = np.random.default_rng(5)
    x = rng.random((W, N, 3)) @ lat
    inside = [rng.random((W, 3)) @ lat for _ in (0, 1)]
    outside = [p + rng.integers(-2, 3, (W, 3)).astype(float) @ lat for p in inside]
    assert max(np.max(np.abs(o - p)) for o, p in zip(outside, inside)) > 1.0
    pick = np.arange(W, dtype=np.int32)
    make = lambda y: PeriodicConfigs(y, lat)  # noqa: E731
    dev = wf.fused_device()
    for sector in ((0, 1), (1, 1)):
        ref = _direct(wf, make, x, inside[0], inside[1], sector, sup.nelec)
        got = []
        for pts in (inside, outside):
            for s in (0, 1):
                x0 = np.ascontiguousarray(pts[s]).copy()
                ev.walk(s, s, x0, np.zeros((1, W, 3)), np.full((1, W), 0.5), 0.5, 1)
            got.append(device_pair_ratios(dev, ev, 0, sector, pick, pick))
        errs = [_err(g, ref) for g in got]
        print(f"tbdm fused periodic {sector}: folded {errs[0]:.2e} unfolded {errs[1]:.2e} between {_err(got[1], got[0]):.2e}")
        assert max(errs) < 1e-10, errs
        assert _err(got[1], got[0]) < 2e-10


def _accumulator(mol, mf, spin, route, **kw):
    import pyqmc_amd as pa

    C = np.asarray(mf.mo_coeff)
    return pa.TBDMAccumulator(mol, [C[0][:, :4], C[1][:, :3]], spin=spin, nsweeps=2, tstep=0.4, warmup=4, route=route, **kw)


def test_chunking_is_bitwise():
    """walker_chunk = 24 at 70 walkers (two whole chunks and a remainder) against one chunk: ratios and accumulators."""
    from pyqmc_amd.tbdm import device_pair_ratios

    mol = systems.water()
    mf = systems.random_mf(mol)
    wf = helpers.gpu_wf(mol, mf)
    ev = _evaluator(mol, mf)
    x, aux, pick = _check_sectors(mol, wf, ev, 70, 6, [])
    dev = wf.fused_device()
    for sector in ((0, 1), (1, 1)):
        whole = device_pair_ratios(dev, ev, 0, sector, pick[0], pick[1])
        parts = device_pair_ratios(dev, ev, 0, sector, pick[0], pick[1], walker_chunk=24)
        assert np.array_equal(whole, parts)
    configs = OpenConfigs(x.copy())
    wf.recompute(configs)
    out = []
    for chunk in (0, 24):
        acc = _accumulator(mol, mf, (0, 0), "fused", walker_chunk=chunk)
        np.random.seed(17)
        out.append((acc(configs, wf), acc.avg(configs, wf)))
        assert acc.last_route == "fused"
    for u, v in zip(*out):
        for k in ("value", "norm_a", "norm_b"):
            assert np.array_equal(u[k], v[k]), k


def _both_routes(mol, mf, wf, configs, spin, seed):
    out = {}
    for route in ("fused", "protocol"):  # (the protocol route last: its moves there and back leave round-off in the state)
        acc = _accumulator(mol, mf, spin, route)
        np.random.seed(seed)
        out[route] = (acc(configs, wf), acc.avg(configs, wf))
        assert acc.last_route == route
    for call, (f, p) in enumerate(zip(out["fused"], out["protocol"])):
        for k in ("value", "norm_a", "norm_b"):
            err = helpers.relerr(f[k], p[k])
            print(f"tbdm fused vs protocol {spin} call {call} {k}: {err:.2e}")
            assert f[k].shape == p[k].shape and err < 1e-9, (spin, call, k, err)


@pytest.mark.parametrize("case", ["water", "open_shell"])
def test_fused_matches_protocol(case):
    mol = systems.water() if case == "water" else _water((5, 3))
    mf = systems.random_mf(mol)
    wf = helpers.gpu_wf(mol, mf)
    configs = _configs(mol, 40, 7)
    wf.recompute(configs)
    for spin in ((0, 1), (1, 1)):
        _both_routes(mol, mf, wf, configs, spin, 23)


@pytest.mark.parametrize("route", ["fused", "protocol"])
def test_g23_on_each_route(route):
    from pyqmc_amd import tbdm
    from test_obdm_cpu import check_tbdm_against_golden

    g = helpers.golden("g23_tbdm")
    mol = systems.water()
    wf = helpers.gpu_wf(mol, systems.random_mf(mol))
    orb = [g["orb_up"], g["orb_dn"]]
    made = []

    def make(kw):
        made.append(tbdm.TBDMAccumulator(mol, orb, nsweeps=2, tstep=0.4, warmup=4, route=route, **kw))
        return made[-1]

    check_tbdm_against_golden(wf, g, make, 1e-8)
    assert len(made) == 3 and all(a.last_route == route for a in made)


def test_default_route_is_fused_on_g23_setup():
    mol = systems.water()
    mf = systems.random_mf(mol)
    wf = helpers.gpu_wf(mol, mf)
    configs = _configs(mol, 8, 8)
    wf.recompute(configs)
    acc = _accumulator(mol, mf, (0, 1), None)
    np.random.seed(1)
    acc(configs, wf)
    assert acc.last_route == "fused"


def test_after_a_fused_sweep():
    """The state is in the sweep's layout after pa.vmc: the fused route syncs it first."""
    import pyqmc_amd as pa

    mol = systems.water_cluster(2, 1, 1)  # (8 per spin: the lane-per-walker sweep)
    mf = systems.random_mf(mol)
    wf = helpers.gpu_wf(mol, mf)
    _, configs = pa.vmc(wf, _configs(mol, 64, 9), nblocks=2, nsteps_per_block=2, tstep=0.3, accumulators={}, seed=4)
    assert wf.fused_device().W == 64
    _both_routes(mol, mf, wf, configs, (0, 1), 29)


def test_no_side_effects_on_handle():
    import pyqmc_amd as pa

    mol = systems.water()
    mf = systems.random_mf(mol, nvirt=6)
    dets = systems.random_determinants(mol, mf, 10)
    runs = []
    for evaluate in (True, False):
        wf = helpers.gpu_wf(mol, mf, dets)
        configs = _configs(mol, 96, 10)
        wf.recompute(configs)
        _, configs = pa.vmc_worker(wf, configs, 0.3, 2, {}, seed=3, state_current=True)  # leaves the state in the sweep's layout
        sl, ja = wf.wf_factors

        def state():
            return [sl._get_state(0), sl._get_state(1), ja._get_state(), wf.value()]

        if evaluate:
            before = state()
            for spin in ((0, 1), (0, 0)):
                acc = _accumulator(mol, mf, spin, None)
                np.random.seed(5)
                acc(configs, wf)
                assert acc.last_route == "fused"
            for b, a in zip(before, state()):
                for u, v in zip(b, a):
                    assert np.array_equal(u, v)
        else:
            state()  # (the same reads of the state, so that the two runs differ by the evaluation alone)
        blk, after = pa.vmc_worker(wf, configs, 0.3, 2, {}, seed=4, state_current=True)
        runs.append((after.configs.copy(), blk["acceptance"]))
    assert np.array_equal(runs[0][0], runs[1][0]) and runs[0][1] == runs[1][1]


def _refused(wf, ev, W, match):
    from pyqmc_amd._ffi import PqaError
    from pyqmc_amd.tbdm import device_pair_ratios

    pick = np.zeros(W, dtype=np.int32)
    with pytest.raises(PqaError, match=match) as info:
        device_pair_ratios(wf.fused_device(), ev, 0, (0, 1), pick, pick)
    assert "protocol route" in str(info.value)


def test_routing_three_body():
    import pyqmc_amd as pa

    mol = systems.water()
    mf = systems.random_mf(mol)
    wf = helpers.gpu_wf3(mol, mf)
    configs = _configs(mol, 6, 11)
    wf.recompute(configs)
    acc = _accumulator(mol, mf, (0, 1), None)
    np.random.seed(2)
    d = acc(configs, wf)
    assert acc.last_route == "protocol" and np.all(np.isfinite(d["value"]))
    with pytest.raises(ValueError, match="fused"):
        _accumulator(mol, mf, (0, 1), "fused")(configs, wf)
    _refused(wf, acc.orbitals, 6, "three-body")
    with pytest.raises(ValueError, match="route"):
        pa.TBDMAccumulator(mol, np.asarray(mf.mo_coeff)[0][:, :2], spin=(0, 1), route="device")


@pytest.mark.parametrize("kind", ["complex", "twisted"])
def test_routing_complex_and_twisted(kind):
    import pyqmc_amd as pa

    sup, kmf = helpers.pbc_complex_case() if kind == "complex" else helpers.twist_case("prim")
    wf = pa.generate_wf(sup, kmf)
    a, b = helpers.pbc_jastrow_coeffs(sup)
    wf.parameters["wf2acoeff"], wf.parameters["wf2bcoeff"] = a, b
    assert wf.fused_device().cplx and wf.fused_device().twisted == (kind == "twisted")
    kpts = np.asarray(kmf.kpts)
    orb = [np.asarray(kmf.mo_coeff[0][k])[:, :2] for k in range(len(kpts))]
    W = 4
    configs = pa.initial_guess(sup, W, rng=np.random.default_rng(12))
    wf.recompute(configs)
    acc = pa.TBDMAccumulator(sup, orb, spin=(0, 1), kpts=kpts, nsweeps=1, warmup=2)
    np.random.seed(3)
    d = acc(configs, wf)
    assert acc.last_route == "protocol" and np.all(np.isfinite(d["value"]))
    with pytest.raises(ValueError, match="fused"):
        pa.TBDMAccumulator(sup, orb, spin=(0, 1), kpts=kpts, nsweeps=1, warmup=2, route="fused")(configs, wf)
    _refused(wf, acc.orbitals, W, "complex")


def test_routing_other_walker_count():
    """Configurations that are not the handle's resident walkers (another count) are outside the fused route."""
    mol = systems.water()
    mf = systems.random_mf(mol)
    wf = helpers.gpu_wf(mol, mf)
    configs = _configs(mol, 16, 13)
    wf.recompute(configs)
    fewer = OpenConfigs(configs.configs[:8].copy())
    assert _accumulator(mol, mf, (0, 1), None)._fused_device(configs, wf) is wf.fused_device()
    assert _accumulator(mol, mf, (0, 1), None)._fused_device(fewer, wf) is None
    with pytest.raises(ValueError, match="fused"):
        _accumulator(mol, mf, (0, 1), "fused")._fused_device(fewer, wf)
    wf.recompute(fewer)
    acc = _accumulator(mol, mf, (0, 1), None)
    np.random.seed(4)
    acc(fewer, wf)
    assert acc.last_route == "fused"
