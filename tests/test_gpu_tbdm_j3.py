"""Two-body density matrix of three-body wave functions on the fused route (pqa_tbdm_sweep_j3 /
TBDMAccumulator(three_body_device=True)): the pair ratios against the protocol route's (testvalue, updateinternals, testvalue_many and
back) on the same points, the whole accumulator against the protocol route, chunking and determinism, handles without a three-body
factor against pqa_tbdm_sweep, no side effects on the wave function's handle, and route selection.

Metrics and bounds: err = max |a - b| / (1 + |b|) < 1e-10 for device against protocol on the same walkers and draws;
helpers.relerr < 1e-9 where only the summation order of a walker mean differs; bitwise where stated.  Every comparison covers every
walker and every pair.  70 walkers, more auxiliary walkers than configurations."""

import numpy as np
import pytest

from pyqmc_amd import systems
from pyqmc_amd.configs import OpenConfigs, PeriodicConfigs
from tests import helpers
from test_gpu_tbdm_fused import SECTORS, _accumulator, _configs, _err, _evaluator, _no_jastrow, _place

pytestmark = pytest.mark.gpu

W70 = 70


def _protocol_ratios(mol, wf, ev, make, x, r1, r2, sector):
    """TBDMAccumulator._pair_ratios: the protocol route's pair ratios with electron a at r1 and electron b at r2."""
    import pyqmc_amd as pa

    acc = pa.TBDMAccumulator.__new__(pa.TBDMAccumulator)
    nup, ndn = mol.nelec
    acc._electrons = [np.arange(s * nup, nup + s * ndn) for s in sector]
    configs = make(x.copy())
    wf.recompute(configs)
    R = acc._pair_ratios(configs, wf, ev.container(r1).electron(0), ev.container(r2).electron(0))
    wf.recompute(make(x.copy()))
    return R


def _check_sectors(mol, wf, ev, W, seed, sectors, make=OpenConfigs, spread=0.8, x=None, aux=None, reference_points=None):
    from pyqmc_amd.tbdm import device_pair_ratios_j3

    rng = np.random.default_rng(seed)
    if x is None:
        x = _configs(mol, W, seed).configs
    naux = W + 3  # (more auxiliary walkers than configurations: the assignment is a real indirection)
    if aux is None:
        aux = [x[rng.integers(0, W, naux), rng.integers(0, x.shape[1], naux)] + spread * rng.standard_normal((naux, 3)) for _ in (0, 1)]
    pick = [rng.integers(0, naux, W).astype(np.int32) for _ in (0, 1)]
    for s in (0, 1):
        _place(ev, s, aux[s])
    dev = wf.fused_device()
    assert dev.has_j3 and dev.na3 == 4 and dev.nb3 == 4
    ref_aux = aux if reference_points is None else [reference_points(a) for a in aux]
    for sector in sectors:
        ref = _protocol_ratios(mol, wf, ev, make, x, ref_aux[0][pick[0]], ref_aux[1][pick[1]], sector)
        R = device_pair_ratios_j3(dev, ev, 0, sector, pick[0], pick[1])
        err = _err(R, ref)
        print(f"tbdm j3 ratios {sector}: {err:.2e} (max |protocol| {np.max(np.abs(ref)):.2e})")
        assert np.all(np.isfinite(ref)) and np.max(np.abs(ref)) > 1e-6
        assert err < 1e-10, (sector, err)
        if sector[0] == sector[1]:
            n = R.shape[1]
            assert np.all(R[:, np.arange(n), np.arange(n)] == 0.0)
    return x, aux, pick


def _three_body_matters(wf, x, make=OpenConfigs):
    wf.recompute(make(x.copy()))
    r3 = wf.wf_factors[2].testvalue(0, make(x[:, :1].copy() + 0.3).electron(0))[0]
    assert np.max(np.abs(r3 - 1.0)) > 1e-4


# ------------------------------------------------------------------------------------------------------------ 1. pair ratios
@pytest.mark.parametrize("jastrow", [True, False])
def test_water_all_sectors(jastrow):
    """70 walkers: no multiple of a wave, a tile or a chunk; all four sectors; with the two-body coefficients zeroed."""
    mol = systems.water()
    mf = systems.random_mf(mol)
    wf = helpers.gpu_wf3(mol, mf)
    if not jastrow:
        _no_jastrow(wf)
    x, *_ = _check_sectors(mol, wf, _evaluator(mol, mf), W70, 1, SECTORS)
    _three_body_matters(wf, x)


def test_six_determinants():
    mol = systems.water()
    mf = systems.random_mf(mol, nvirt=6)
    wf = helpers.gpu_wf3(mol, mf, systems.random_determinants(mol, mf, 6))
    assert wf.fused_device().ndet == 6
    _check_sectors(mol, wf, _evaluator(mol, mf), W70, 3, SECTORS)


def test_chain_longer_than_the_cutoffs():
    """water_cluster(5, 1, 1): 40 electrons and 15 atoms, many passes of the item loop; ions and pairs on both sides of rcut_a3 and
    rcut_b3 occur (asserted from the host coordinates), among them the two auxiliary points of a walker."""
    mol = systems.water_cluster(5, 1, 1)
    assert mol.nelec == (20, 20) and mol.natm == 15
    mf = systems.random_mf(mol)
    wf = helpers.gpu_wf3(mol, mf)
    dev = wf.fused_device()
    rca, rcb = dev._ctor["a3_basis"][0].rcut, dev._ctor["b3_basis"][0].rcut
    x, aux, pick = _check_sectors(mol, wf, _evaluator(mol, mf), W70, 4, [(0, 0), (0, 1)])
    atoms = np.asarray(mol.atom_coords())
    iu = np.triu_indices(x.shape[1], 1)
    d_ion = np.linalg.norm(x[:, :, None, :] - atoms[None, None], axis=-1)
    d_pair = np.linalg.norm(x[:, :, None, :] - x[:, None, :, :], axis=-1)[:, iu[0], iu[1]]
    r1, r2 = aux[0][pick[0]], aux[1][pick[1]]
    q_ion = np.linalg.norm(np.concatenate([r1, r2])[:, None, :] - atoms[None], axis=-1)
    q_pair = np.concatenate([np.linalg.norm(r1[:, None, :] - x, axis=-1), np.linalg.norm(r2[:, None, :] - x, axis=-1)])
    q12 = np.linalg.norm(r1 - r2, axis=-1)
    for d, rc in ((d_ion, rca), (q_ion, rca), (d_pair, rcb), (q_pair, rcb), (q12, rcb)):
        assert np.any(d < rc) and np.any(d > rc), (d.min(), d.max(), rc)


def test_periodic_unfolded_points_equal_folded():
    """diamond_primitive at Gamma with a three-body factor, 16 walkers: auxiliary points pushed out of the cell by whole lattice
    vectors against the protocol route at the folded points."""
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
    inside = [rng.random((W + 3, 3)) @ lat for _ in (0, 1)]
    outside = [p + rng.integers(-2, 3, (W + 3, 3)).astype(float) @ lat for p in inside]
    assert max(np.max(np.abs(o - p)) for o, p in zip(outside, inside)) > 1.0
    inv = np.linalg.inv(lat)

    def folded(p):
        f = p @ inv
        return (f - np.floor(f)) @ lat

    make = lambda y: PeriodicConfigs(y, lat)  # noqa: E731
    _check_sectors(sup, wf, ev, W, 6, [(0, 1), (1, 1)], make=make, x=x, aux=outside, reference_points=folded)
    _three_body_matters(wf, x, make)


# ------------------------------------------------------------------------------------------------------------ 2. whole accumulator
@pytest.mark.parametrize("spin", [(0, 1), (1, 1)])
def test_fused_matches_protocol(spin):
    mol = systems.water()
    mf = systems.random_mf(mol)
    wf = helpers.gpu_wf3(mol, mf)
    configs = _configs(mol, W70, 7)
    wf.recompute(configs)
    wts = np.random.default_rng(3).random(W70) + 0.2
    out, states = {}, {}
    for route, flag in ((None, True), ("protocol", False)):  # (the protocol route last: its moves leave round-off in the state)
        make = lambda: _accumulator(mol, mf, spin, route, three_body_device=flag, naux=37)  # noqa: E731
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
            for k in ("value", "norm_a", "norm_b"):
                e = helpers.relerr(res[k], avg[k])
                ew = helpers.relerr(resw[k], np.tensordot(wts, first[k], axes=(0, 0)) / wts.sum())
                print(f"tbdm j3 {spin} avg_resident against avg {k}: {e:.2e}; weighted against the weighted mean of __call__: {ew:.2e}")
                assert e < 1e-9 and ew < 1e-9, (k, e, ew)
    for a, b in zip(states[True], states[False]):
        assert np.array_equal(a, b)
    for call in (0, 1, 2):
        f, p = out["fused"][call], out["protocol"][call]
        err = _err(f["value"], p["value"])
        print(f"tbdm j3 fused vs protocol {spin} call {call}: value {err:.2e}")
        assert f["value"].shape == p["value"].shape and err < 1e-10, (call, err)
        if call < 2:
            assert np.array_equal(f["norm_a"], p["norm_a"]) and np.array_equal(f["norm_b"], p["norm_b"])
    for route in ("fused", "protocol"):
        per, avg = out[route][0], out[route][2]
        for k in ("value", "norm_a", "norm_b"):
            err = helpers.relerr(avg[k], per[k].mean(axis=0))
            print(f"tbdm j3 {route} {spin} avg against mean(__call__) {k}: {err:.2e}")
            assert err < 1e-9, (route, k, err)


# ------------------------------------------------------------------------------------------------------------ 3. determinism
def test_chunking_and_two_calls_are_bitwise():
    """walker_chunk = 24 at 70 walkers (two whole chunks and a remainder) against one chunk, and a second call: ratios and
    accumulators."""
    from pyqmc_amd.tbdm import device_pair_ratios_j3

    mol = systems.water()
    mf = systems.random_mf(mol)
    wf = helpers.gpu_wf3(mol, mf)
    ev = _evaluator(mol, mf)
    x, aux, pick = _check_sectors(mol, wf, ev, W70, 6, [])
    dev = wf.fused_device()
    wf.recompute(OpenConfigs(x.copy()))
    for sector in ((0, 1), (1, 1)):
        whole = device_pair_ratios_j3(dev, ev, 0, sector, pick[0], pick[1])
        parts = device_pair_ratios_j3(dev, ev, 0, sector, pick[0], pick[1], walker_chunk=24)
        again = device_pair_ratios_j3(dev, ev, 0, sector, pick[0], pick[1])
        assert np.array_equal(whole, parts) and np.array_equal(whole, again) and np.max(np.abs(whole)) > 1e-6
    configs = OpenConfigs(x.copy())
    wf.recompute(configs)
    out = []
    for chunk in (0, 24, 0):
        acc = _accumulator(mol, mf, (0, 0), None, walker_chunk=chunk, three_body_device=True)
        np.random.seed(17)
        out.append((acc(configs, wf), acc.avg(configs, wf)))
        assert acc.last_route == "fused"
    for other in out[1:]:
        for u, v in zip(out[0], other):
            for k in ("value", "norm_a", "norm_b"):
                assert np.array_equal(u[k], v[k]), k


def test_without_three_body_factor_equals_the_existing_entry():
    """A handle without a three-body factor through pqa_tbdm_sweep_j3: the bits of pqa_tbdm_sweep, ratios and accumulators."""
    from pyqmc_amd.tbdm import device_tbdm_sweep, device_tbdm_sweep_j3

    mol = systems.water()
    mf = systems.random_mf(mol, nvirt=6)
    wf = helpers.gpu_wf(mol, mf, systems.random_determinants(mol, mf, 6))
    ev = _evaluator(mol, mf)
    rng = np.random.default_rng(12)
    x = _configs(mol, W70, 12).configs
    naux = W70 + 3
    aux = [x[rng.integers(0, W70, naux), rng.integers(0, 8, naux)] + 0.8 * rng.standard_normal((naux, 3)) for _ in (0, 1)]
    pick = [rng.integers(0, naux, W70).astype(np.int32) for _ in (0, 1)]
    for s in (0, 1):
        _place(ev, s, aux[s])
    dev = wf.fused_device()
    assert not dev.has_j3
    wf.recompute(OpenConfigs(x.copy()))
    xt = ev.true_positions(OpenConfigs(x.copy()))
    ijkl = np.stack(np.meshgrid(*[np.arange(3)] * 4, indexing="ij"), -1).reshape(-1, 4).T.astype(np.int32)
    for sector in SECTORS:
        for s in (0, 1):
            ev.points(s, s, xt[:, np.arange(sector[s] * 4, 4 + sector[s] * 4)])
        got = []
        for fn in (device_tbdm_sweep, device_tbdm_sweep_j3):
            R = fn(dev, ev, 0, sector, pick[0], pick[1], ijkl=ijkl, walker_chunk=24, with_ratios=True)
            got.append((R, ev.fetch(0, W70, (81,), 1.0, False), ev.fetch(1, W70, (3,), 1.0, False), ev.fetch(2, W70, (3,), 1.0, False)))
        for a, b in zip(*got):
            assert np.array_equal(a, b)
        assert np.max(np.abs(got[0][0])) > 1e-6 and np.max(np.abs(got[0][1])) > 0


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
            for spin in ((0, 1), (0, 0)):
                acc = _accumulator(mol, mf, spin, None, three_body_device=True)
                np.random.seed(5)
                acc(configs, wf)
                acc.avg_resident(wf)
                assert acc.last_route == "fused"
            for b, a in zip(before, state()):
                for u, v in zip(b, a):
                    assert np.array_equal(u, v)
        else:
            state()  # (the same reads of the state, so that the two runs differ by the evaluation alone)
        blk, after = pa.vmc_worker(wf, configs, 0.3, 2, {}, seed=4, state_current=True)
        runs.append((after.configs.copy(), blk["acceptance"]))
    assert np.array_equal(runs[0][0], runs[1][0]) and runs[0][1] == runs[1][1]


# ------------------------------------------------------------------------------------------------------------ 5. routing
def test_flag_off_behaves_as_today():
    mol = systems.water()
    mf = systems.random_mf(mol)
    wf = helpers.gpu_wf3(mol, mf)
    configs = _configs(mol, 6, 11)
    wf.recompute(configs)
    acc = _accumulator(mol, mf, (0, 1), None)
    assert acc.three_body_device is False
    np.random.seed(2)
    d = acc(configs, wf)
    assert acc.last_route == "protocol" and np.all(np.isfinite(d["value"]))
    with pytest.raises(ValueError, match="route='fused' needs a real Slater \\(x two-body Jastrow\\) wave function"):
        _accumulator(mol, mf, (0, 1), "fused")(configs, wf)
    assert "real Slater (x two-body Jastrow)" in acc.resident_scope(wf)
    on = _accumulator(mol, mf, (0, 1), "fused", three_body_device=True)
    assert on.resident_scope(wf) is None
    np.random.seed(2)
    on(configs, wf)
    assert on.last_route == "fused"
    # a wave function without a three-body factor keeps the existing entry with the flag on
    wf2 = helpers.gpu_wf(mol, mf)
    wf2.recompute(configs)
    outs = []
    for flag in (False, True):
        a = _accumulator(mol, mf, (0, 1), None, three_body_device=flag)
        np.random.seed(2)
        outs.append(a(configs, wf2))
        assert a.last_route == "fused" and not a._j3_entry(wf2.fused_device())
    for k in ("value", "norm_a", "norm_b"):
        assert np.array_equal(outs[0][k], outs[1][k])


@pytest.mark.parametrize("kind", ["complex", "twisted"])
def test_complex_and_twisted_are_refused(kind):
    import pyqmc_amd as pa
    from pyqmc_amd._ffi import PqaError
    from pyqmc_amd.tbdm import device_pair_ratios_j3

    sup, kmf = helpers.pbc_complex_case() if kind == "complex" else helpers.twist_case("prim")
    wf = pa.generate_wf(sup, kmf, jastrow3=True)
    a, b = helpers.pbc_jastrow_coeffs(sup)
    wf.parameters["wf2acoeff"], wf.parameters["wf2bcoeff"] = a, b
    wf.parameters["wf3ccoeff"] = helpers.ccoeff_params(sup)
    dev = wf.fused_device()
    assert dev.cplx and dev.has_j3 and dev.twisted == (kind == "twisted")
    kpts = np.asarray(kmf.kpts)
    orb = [[np.asarray(kmf.mo_coeff[s][k])[:, :2] for k in range(len(kpts))] for s in (0, 1)]
    W = 4
    configs = pa.initial_guess(sup, W, rng=np.random.default_rng(12))
    wf.recompute(configs)
    # both flags on: a complex or twisted three-body handle stays on the protocol route, with a reason
    acc = pa.TBDMAccumulator(sup, orb, (0, 1), kpts=kpts, nsweeps=1, warmup=2, complex_device=True, three_body_device=True)
    assert "complex or twisted" in acc.resident_scope(wf)
    np.random.seed(3)
    d = acc(configs, wf)
    assert acc.last_route == "protocol" and np.all(np.isfinite(d["value"]))
    with pytest.raises(ValueError, match="complex or twisted"):
        pa.TBDMAccumulator(sup, orb, (0, 1), kpts=kpts, nsweeps=1, warmup=2, route="fused", three_body_device=True)(configs, wf)
    # the entry itself
    pick = np.zeros(W, dtype=np.int32)
    with pytest.raises(PqaError, match="complex orbitals / twisted cell") as info:
        device_pair_ratios_j3(dev, acc.orbitals, 0, (0, 1), pick, pick)
    assert "pqa_tbdm_sweep_j3" in str(info.value) and "protocol route" in str(info.value)
