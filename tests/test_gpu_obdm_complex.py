"""One-body density matrix of complex and twisted handles on the fused route (pqa_obdm_sweeps_c, opt-in through
OBDMAccumulator(complex_device=True)): the complex ratios against wf.testvalue_many on the same points and both modes of the estimator
against NumPy on those ratios (twisted cell, complex Bloch determinants, a real handle with a complex evaluator, a complex handle with a
real evaluator, more than 16 orbitals), the behaviour under whole lattice vectors, the whole accumulator against the protocol route,
a real handle against pqa_obdm_sweeps, weights, chunking and repeatability, the device's own draws, no side effects, the resident
driver path and the scope.

Metrics and bounds are those of tests/test_gpu_obdm_fused.py: _err = max |a - b| / (1 + |b|) < 1e-10 where the two sides share inputs
and differ in formula and summation order; helpers.relerr < 1e-9 where only the summation order differs; bitwise equality where stated.
Every comparison covers every walker and every listed electron."""

import copy
import importlib

import numpy as np
import pytest

from pyqmc_amd import pbc, systems
from pyqmc_amd.configs import PeriodicConfigs
from tests import helpers
from test_gpu_obdm_fused import _place
from test_gpu_tbdm_fused import _err, _no_jastrow

pytestmark = pytest.mark.gpu

W70, NSW, NAUX = 70, 3, 37
LISTS = {"up": dict(spin=0), "down": dict(spin=1), "all": dict(), "mixed": dict(electrons=[5, 1, 6])}


def _electrons(mol, spin=None, electrons=None):
    nup, ntot = mol.nelec[0], sum(mol.nelec)
    if spin is not None:
        return np.arange(0, nup) if spin == 0 else np.arange(nup, ntot)
    return np.arange(ntot) if electrons is None else np.asarray(electrons)


def _twisted_walkers(sup, W, seed):
    """Walkers of a periodic cell placed partly outside it (the container folds them and counts the crossings)."""
    lat = sup.lattice_vectors()
    frac = np.random.default_rng(seed).random((W, sum(sup.nelec), 3)) * 2.4 - 0.7
    cfg = PeriodicConfigs(frac @ lat, lat)
    assert np.any(cfg.wrap != 0)
    return cfg


def _kblocks(kmf, norb):
    """The leading ``norb`` columns of the mean field's spin-up block at every k-point."""
    return [np.asarray(kmf.mo_coeff[0][k])[:, :norb] for k in range(len(kmf.kpts))]


def _twisted_case(tag="prim"):
    sup, kmf = helpers.twist_case(tag)
    sup, wf = helpers.gpu_pbc_wf(tag, case=(sup, kmf))
    assert wf.fused_device().twisted and wf.fused_device().cplx
    return sup, kmf, wf


def _bloch_case():
    """The complex 3 x 1 x 1 cell with three determinants (test_gpu_sr_complex.py::bloch)."""
    sup = helpers.pbc_complex_case()[0]
    mf = pbc.random_kmf(sup, complex_coeff=True, nvirt=1)
    base = [5 * k + i for k in range(3) for i in range(4)]
    ex1, ex2 = sorted(set(base) - {3} | {4}), sorted(set(base) - {13} | {14})
    dets = [(1.0, [base, base]), (0.3, [ex2, base]), (-0.2, [ex1, ex2])]
    sup, wf = helpers.gpu_pbc_wf("cplx", case=(sup, mf), determinants=dets)
    dev = wf.fused_device()
    assert dev.ndet == 3 and dev.cplx and not dev.twisted
    return sup, mf, wf


def _numpy_estimator(ev, xt, es, kept, pick, R):
    """value (W, norb, norb) complex and norm (W, norb) real summed over the sweeps, from the ratios R (nsweeps, W, ne), in NumPy:
    value[j, k] = b[j] conj(sum_e R_e phi_k(r_e)) at the true (unfolded) positions xt of the walkers."""
    W, norb = xt.shape[0], ev.norb
    at_e = ev.mos(xt[:, es].reshape(-1, 3)).reshape(W, len(es), norb)
    value, norm = np.zeros((W, norb, norb), dtype=complex), np.zeros((W, norb))
    for s in range(len(R)):
        phi = ev.mos(kept[s])[pick[s]]
        F = np.sum(np.abs(phi) ** 2, axis=1, keepdims=True) / norb
        value += (phi / F)[:, :, None] * np.conj(np.einsum("we,wej->wj", R[s], at_e))[:, None, :]
        norm += np.abs(phi) ** 2 / F
    return value, norm


def _check_ratios(mol, wf, ev, configs, seed, lists, start=None, reference=None):
    """The ratios of pqa_obdm_sweeps_c against wf.testvalue_many at the same points (``reference(kept, pick, es)``: another
    reference), and both modes of the estimator against NumPy on those ratios, for every electron list.  Returns the pieces and the
    worst errors (ratios, per-walker, mean)."""
    from pyqmc_amd.obdm import device_obdm_sweeps_c

    rng = np.random.default_rng(seed)
    xt = ev.true_positions(configs)
    W, N = xt.shape[:2]
    if start is None:
        start = xt[rng.integers(0, W, NAUX), rng.integers(0, N, NAUX)] + 0.5 * rng.standard_normal((NAUX, 3))
    kept = _place(ev, start, NSW, rng)
    pick = rng.integers(0, len(start), (NSW, W)).astype(np.int32)
    dev = wf.fused_device()
    wf.recompute(copy.deepcopy(configs))
    norb, worst = ev.norb, np.zeros(3)
    for name, kw in lists.items():
        es = _electrons(mol, **kw)
        if reference is None:
            ref = np.stack([wf.testvalue_many(es, ev.container(kept[s][pick[s]]).electron(0)) for s in range(NSW)])
        else:
            ref = reference(kept, pick, es)
        assert np.all(np.isfinite(ref)) and np.max(np.abs(ref)) > 1e-6
        out = device_obdm_sweeps_c(dev, ev, es, NSW, assign=pick, with_ratios=True)
        assert out["ratio"].dtype == complex and out["ratio"].shape == (NSW, W, len(es))
        if not dev.cplx:
            assert np.all(out["ratio"].imag == 0)  # (a real handle: the imaginary parts are exactly 0)
        err = _err(out["ratio"], ref)
        value, norm = _numpy_estimator(ev, xt, es, kept, pick, ref)
        got_v = ev.fetch(0, W, (norb, norb), 1.0, False, cplx=True)
        got_n = ev.fetch(1, W, (norb,), 1.0, False)
        ev_err = max(_err(got_v, value), _err(got_n, norm))
        m = device_obdm_sweeps_c(dev, ev, es, NSW, assign=pick, mean=True)
        assert m["value"].dtype == complex and m["norm"].dtype == float
        m_err = max(_err(m["value"] * NSW, value.mean(axis=0)), _err(m["norm"] * NSW, norm.mean(axis=0)))
        print(f"obdm complex {name}: ratios {err:.2e} (max |ref| {np.max(np.abs(ref)):.2e}, max |Im| {np.max(np.abs(np.imag(ref))):.2e}) "
              f"per-walker {ev_err:.2e} mean {m_err:.2e}")
        assert err < 1e-10 and ev_err < 1e-10 and m_err < 1e-10, (name, err, ev_err, m_err)
        worst = np.maximum(worst, (err, ev_err, m_err))
    return xt, kept, pick, worst


# ------------------------------------------------------------------------------------------------------------ 1. ratios, both modes
@pytest.mark.parametrize("jastrow", [True, False])
def test_twisted_cell_every_list(jastrow):
    """(a) the twisted primitive cell, 4 + 4 electrons, a twisted evaluator: 70 walkers partly outside the cell, both spins, all
    electrons, an unordered mixed list."""
    import pyqmc_amd as pa

    sup, kmf, wf = _twisted_case()
    if not jastrow:
        _no_jastrow(wf)
    ev = pa.obdm.OrbitalEvaluator(sup, _kblocks(kmf, 3), kpts=kmf.kpts)
    assert ev.dev.twisted and ev.norb == 3
    _check_ratios(sup, wf, ev, _twisted_walkers(sup, W70, 1), 1, LISTS)


def test_complex_determinants():
    """(b) the complex 3 x 1 x 1 cell with three determinants and its own (untwisted, complex) Bloch orbitals, 12 + 12 electrons."""
    import pyqmc_amd as pa

    sup, mf, wf = _bloch_case()
    ev = pa.obdm.OrbitalEvaluator(sup, _kblocks(mf, 2), kpts=mf.kpts)
    assert ev.dev.cplx and not ev.dev.twisted and ev.norb == 6
    configs = pa.initial_guess(sup, W70, rng=np.random.default_rng(2))
    _check_ratios(sup, wf, ev, configs, 2, {"all": dict(), "mixed": dict(electrons=[13, 1, 22, 6]), "down": dict(spin=1)})


def test_complex_handle_real_evaluator():
    """A complex handle (the primitive cell at Gamma with complex coefficients) with a REAL evaluator: complex T, real B, the
    two-MFMA instance of the mean product."""
    import pyqmc_amd as pa

    sup, _ = helpers.pbc_slater_case("gamma")
    kmf = pbc.random_kmf(sup, complex_coeff=True)
    sup, wf = helpers.gpu_pbc_wf("gamma", case=(sup, kmf))
    assert wf.fused_device().cplx and not wf.fused_device().twisted
    nao = np.asarray(kmf.mo_coeff[0][0]).shape[0]
    ev = pa.obdm.OrbitalEvaluator(sup, [0.4 * np.random.default_rng(3).standard_normal((nao, 5))], kpts=np.zeros((1, 3)))
    assert not ev.dev.cplx and ev.norb == 5
    configs = pa.initial_guess(sup, W70, rng=np.random.default_rng(4))
    _check_ratios(sup, wf, ev, configs, 3, {"up": dict(spin=0), "mixed": dict(electrons=[5, 1, 6])})


def test_real_handle_complex_evaluator():
    """(c) a real Gamma handle with a complex untwisted evaluator: the ratios' imaginary parts are exactly 0 (asserted in
    _check_ratios), B is complex."""
    import pyqmc_amd as pa

    sup, wf = helpers.gpu_pbc_wf("gamma")
    assert not wf.fused_device().cplx
    kmf = pbc.random_kmf(sup, complex_coeff=True)
    ev = pa.obdm.OrbitalEvaluator(sup, _kblocks(kmf, 3), kpts=kmf.kpts)
    assert ev.dev.cplx and not ev.dev.twisted
    lat = sup.lattice_vectors()
    x = np.random.default_rng(5).random((W70, sum(sup.nelec), 3)) @ lat
    _check_ratios(sup, wf, ev, PeriodicConfigs(x, lat), 4, {"all": dict(), "down": dict(spin=1)})


def test_s211_two_tiles():
    """(d) the twisted 2 x 1 x 1 cell with 18 evaluator orbitals (random complex coefficients, 9 per k-point): two MFMA tiles each
    way, the second one padded."""
    import pyqmc_amd as pa

    sup, kmf, wf = _twisted_case("s211")
    nao = np.asarray(kmf.mo_coeff[0][0]).shape[0]
    rng = np.random.default_rng(6)
    orb = [0.4 * (rng.standard_normal((nao, 9)) + 1j * rng.standard_normal((nao, 9))) for _ in range(len(kmf.kpts))]
    ev = pa.obdm.OrbitalEvaluator(sup, orb, kpts=kmf.kpts)
    assert ev.dev.twisted and ev.norb == 18
    _check_ratios(sup, wf, ev, _twisted_walkers(sup, W70, 5), 5, {"up": dict(spin=0), "mixed": dict(electrons=[9, 3, 15, 0])})


# ------------------------------------------------------------------------------------------------------------ 2. lattice vectors
def test_twisted_points_moved_by_lattice_vectors():
    """The twisted analogue of test_periodic_unfolded_points_equal_folded.  An auxiliary point pushed out of the cell by the lattice
    vector n . L has the ratio of the folded point times the Bloch phase exp(i k_t . n . L) of the moved electron, and the estimator
    (b carries the same phase, the ratio enters conjugated) is that of the folded points: the reference is testvalue_many at the
    FOLDED points, times the phase."""
    import pyqmc_amd as pa

    sup, kmf, wf = _twisted_case()
    ev = pa.obdm.OrbitalEvaluator(sup, _kblocks(kmf, 3), kpts=kmf.kpts)
    lat = sup.lattice_vectors()
    kt = pbc.common_twist(sup, kmf.kpts)
    rng = np.random.default_rng(7)
    start = rng.random((NAUX, 3)) @ lat + rng.integers(-2, 3, (NAUX, 3)).astype(float) @ lat
    inv = np.linalg.inv(lat)

    def reference(kept, pick, es):
        out = []
        for s in range(NSW):
            pts = kept[s][pick[s]]
            n = np.floor(pts @ inv)
            assert np.max(np.abs(n)) >= 1.0  # (points outside the cell are among them)
            folded = PeriodicConfigs((pts - n @ lat).reshape(-1, 1, 3), lat)
            assert np.all(folded.wrap == 0)
            out.append(wf.testvalue_many(es, folded.electron(0)) * np.exp(1j * (n @ lat) @ kt)[:, None])
        return np.stack(out)

    _check_ratios(sup, wf, ev, _twisted_walkers(sup, 16, 8), 8, {"all": dict(), "down": dict(spin=1)}, start=start, reference=reference)


# ------------------------------------------------------------------------------------------------------------ 3. whole accumulator
def _accumulator(sup, orb, kpts, fused, norb=None, **kw):
    import pyqmc_amd as pa

    kw.setdefault("spin", 0)
    if kw["spin"] is None:
        del kw["spin"]
    extra = dict(complex_device=True) if fused else dict(route="protocol")
    return pa.obdm.OBDMAccumulator(sup, orb, kpts=kpts, nsweeps=NSW, tstep=0.4, warmup=4, **extra, **kw)


@pytest.mark.parametrize("case", ["twisted_up", "twisted_mixed_naux", "bloch_down"])
def test_fused_matches_protocol(case):
    import pyqmc_amd as pa

    if case.startswith("twisted"):
        sup, kmf, wf = _twisted_case()
        configs = _twisted_walkers(sup, W70, 9)
        kw = dict(spin=0) if case == "twisted_up" else dict(spin=None, electrons=np.array([5, 1, 6]), naux=NAUX)
    else:
        sup, kmf, wf = _bloch_case()
        configs = pa.initial_guess(sup, W70, rng=np.random.default_rng(9))
        kw = dict(spin=1)
    orb, norb = _kblocks(kmf, 2), 2 * len(kmf.kpts)
    wf.recompute(configs)
    out, states = {}, {}
    for route in ("fused", "protocol"):
        acc, acc2 = (_accumulator(sup, orb, kmf.kpts, route == "fused", **kw) for _ in (0, 1))
        np.random.seed(23)
        first, second = acc(configs, wf), acc(configs, wf)
        states[route] = np.random.get_state()
        np.random.seed(23)
        out[route] = (first, second, acc2.avg(configs, wf))
        assert acc.last_route == route and acc2.last_route == route
    for a, b in zip(states["fused"], states["protocol"]):
        assert np.array_equal(a, b)
    for call in (0, 1, 2):
        f, p = out["fused"][call], out["protocol"][call]
        for k in ("value", "norm"):
            assert f[k].dtype == p[k].dtype and f[k].shape == p[k].shape, (call, k)
        err = _err(f["value"], p["value"])
        print(f"obdm complex fused vs protocol {case} call {call}: value {err:.2e}")
        assert err < 1e-10 and f["value"].dtype == complex
        if call < 2:
            assert f["value"].shape == (W70, norb, norb)
            assert np.array_equal(f["norm"], p["norm"])  # (formed by k_obdm_acc from the same kept rows on both routes)
    for route in ("fused", "protocol"):
        per, avg = out[route][0], out[route][2]
        for k in ("value", "norm"):
            err = helpers.relerr(avg[k], per[k].mean(axis=0))
            print(f"obdm complex {route} {case} avg against mean(__call__) {k}: {err:.2e}")
            assert err < 1e-9, (route, k, err)


# ------------------------------------------------------------------------------------------------------------ 4. a real handle
def test_real_handle_through_the_complex_entry():
    """Water 4 + 4 with 4 determinants through pqa_obdm_sweeps_c against pqa_obdm_sweeps.  Bitwise: the norms (per walker: the same
    kernel reads the same rows; mean: the same column sums) and the drawn assignments.  Not bitwise: the ratios and the values — the
    complex kernel rounds each product of the inverse-row and determinant sums on its own where the real one fuses it into the
    running sum, and divides by the complex weight sum — so those are held to 1e-10, with imaginary parts exactly 0."""
    import pyqmc_amd as pa
    from pyqmc_amd.obdm import device_obdm_sweeps, device_obdm_sweeps_c
    from test_gpu_obdm_fused import _evaluator

    mol = systems.water()
    mf = systems.random_mf(mol, nvirt=6)
    wf = helpers.gpu_wf(mol, mf, systems.random_determinants(mol, mf, 4))
    ev = _evaluator(mol, mf, 5)
    configs = pa.initial_guess(mol, W70, rng=np.random.default_rng(10))
    xt, kept, pick, _ = _check_ratios(mol, wf, ev, configs, 10, {"all": dict()})
    dev, es = wf.fused_device(), np.array([5, 1, 6, 2])
    r = device_obdm_sweeps(dev, ev, es, NSW, assign=pick, with_ratios=True)
    rv, rn = ev.fetch(0, W70, (5, 5), 1.0, False), ev.fetch(1, W70, (5,), 1.0, False)
    rm = device_obdm_sweeps(dev, ev, es, NSW, assign=pick, mean=True)
    c = device_obdm_sweeps_c(dev, ev, es, NSW, assign=pick, with_ratios=True)
    cv, cn = ev.fetch(0, W70, (5, 5), 1.0, False, cplx=True), ev.fetch(1, W70, (5,), 1.0, False)
    cm = device_obdm_sweeps_c(dev, ev, es, NSW, assign=pick, mean=True)
    assert np.all(c["ratio"].imag == 0) and np.all(cv.imag == 0) and np.all(cm["value"].imag == 0)
    errs = _err(c["ratio"].real, r["ratio"]), _err(cv.real, rv), _err(cm["value"].real, rm["value"])
    print(f"obdm real handle through the complex entry: ratios {errs[0]:.2e} per-walker {errs[1]:.2e} mean {errs[2]:.2e}")
    assert max(errs) < 1e-10
    assert np.array_equal(cn, rn) and np.array_equal(cm["norm"], rm["norm"])
    a = device_obdm_sweeps(dev, ev, es, NSW, seed=77, mean=True)["assign"]
    b = device_obdm_sweeps_c(dev, ev, es, NSW, seed=77, mean=True)["assign"]
    assert np.array_equal(a, b) and len(np.unique(a)) > NAUX // 2


# ------------------------------------------------------------------------------------------------------------ 5. weights
def test_weighted_mean():
    sup, kmf, wf = _twisted_case()
    configs = _twisted_walkers(sup, W70, 11)
    wf.recompute(configs)
    orb = _kblocks(kmf, 2)
    w = 0.5 + np.random.default_rng(12).random(W70)
    out = {}
    for name, wts in (("per", None), ("weighted", w), ("unit", np.ones(W70)), ("avg", None)):
        acc = _accumulator(sup, orb, kmf.kpts, True, spin=None)
        np.random.seed(31)
        out[name] = acc(configs, wf) if name == "per" else (acc.avg(configs, wf) if name == "avg" else acc.avg_resident(wf, weights=wts))
        assert acc.last_route == "fused"
    for k in ("value", "norm"):
        ref = np.tensordot(w, out["per"][k], axes=(0, 0)) / w.sum()
        err = helpers.relerr(out["weighted"][k], ref)
        print(f"obdm complex weighted {k}: {err:.2e}")
        assert err < 1e-9 and out["weighted"][k].dtype == out["avg"][k].dtype
        assert np.array_equal(out["unit"][k], out["avg"][k])  # (a weight of 1 leaves every bit)
    with pytest.raises(ValueError):
        _accumulator(sup, orb, kmf.kpts, True).avg_resident(wf, weights=-w)


# ------------------------------------------------------------------------------------------------------------ 6. repeatability
def test_chunking_and_repeats_are_bitwise():
    """walker_chunk = 24 at 70 walkers against one chunk in both modes (the mean mode takes whole 64-walker slices); two mean calls."""
    import pyqmc_amd as pa
    from pyqmc_amd.obdm import device_obdm_sweeps_c

    sup, kmf, wf = _twisted_case()
    ev = pa.obdm.OrbitalEvaluator(sup, _kblocks(kmf, 3), kpts=kmf.kpts)
    xt, kept, pick, _ = _check_ratios(sup, wf, ev, _twisted_walkers(sup, W70, 13), 13, {})
    dev, es = wf.fused_device(), np.arange(8)
    out = []
    for chunk in (0, 24):
        r = device_obdm_sweeps_c(dev, ev, es, NSW, assign=pick, walker_chunk=chunk, with_ratios=True)
        per = (ev.fetch(0, W70, (3, 3), 1.0, False, cplx=True), ev.fetch(1, W70, (3,), 1.0, False))
        m = device_obdm_sweeps_c(dev, ev, es, NSW, assign=pick, walker_chunk=chunk, mean=True)
        out.append((r["ratio"], per[0], per[1], m["value"], m["norm"]))
    for a, b in zip(*out):
        assert np.array_equal(a, b)
    again = device_obdm_sweeps_c(dev, ev, es, NSW, assign=pick, mean=True)
    assert np.array_equal(again["value"], out[0][3]) and np.array_equal(again["norm"], out[0][4])
    assert np.abs(out[0][3].imag).max() > 0


def test_sixteen_slices():
    """1 024 walkers (16 slices): the mean mode against the mean of the per-walker mode."""
    import pyqmc_amd as pa
    from pyqmc_amd.obdm import device_obdm_sweeps_c

    sup, kmf, wf = _twisted_case()
    ev = pa.obdm.OrbitalEvaluator(sup, _kblocks(kmf, 3), kpts=kmf.kpts)
    W, nsw = 1024, 2
    configs = _twisted_walkers(sup, W, 14)
    wf.recompute(configs)
    rng = np.random.default_rng(14)
    xt = ev.true_positions(configs)
    start = xt[rng.integers(0, W, 200), rng.integers(0, 8, 200)] + 0.5 * rng.standard_normal((200, 3))
    _place(ev, start, nsw, rng)
    pick = rng.integers(0, 200, (nsw, W)).astype(np.int32)
    dev, es = wf.fused_device(), np.arange(4)
    m = device_obdm_sweeps_c(dev, ev, es, nsw, assign=pick, mean=True)
    m2 = device_obdm_sweeps_c(dev, ev, es, nsw, assign=pick, mean=True)
    assert np.array_equal(m["value"], m2["value"]) and np.array_equal(m["norm"], m2["norm"])
    device_obdm_sweeps_c(dev, ev, es, nsw, assign=pick)
    value = ev.fetch(0, W, (3, 3), 1.0 / nsw, True, cplx=True)
    norm = ev.fetch(1, W, (3,), 1.0 / nsw, True)
    errs = helpers.relerr(m["value"], value), helpers.relerr(m["norm"], norm)
    print(f"obdm complex mean mode at {W} walkers against the mean of the per-walker mode: value {errs[0]:.2e} norm {errs[1]:.2e}")
    assert max(errs) < 1e-9


# ------------------------------------------------------------------------------------------------------------ 7. rng="device"
def test_device_rng():
    from pyqmc_amd.obdm import device_obdm_sweeps_c

    sup, kmf, wf = _twisted_case()
    configs = _twisted_walkers(sup, W70, 15)
    wf.recompute(configs)
    orb = _kblocks(kmf, 2)
    runs = []
    for seed in (31, 31, 32):
        acc = _accumulator(sup, orb, kmf.kpts, True, rng="device", naux=NAUX)
        np.random.seed(seed)
        d = acc.avg(configs, wf)
        assert acc.last_route == "fused" and acc.last_assign.shape == (NSW, W70)
        assert acc.last_assign.min() >= 0 and acc.last_assign.max() < NAUX and len(np.unique(acc.last_assign)) > NAUX // 2
        runs.append((d, acc.last_assign.copy(), acc))
    assert np.array_equal(runs[0][1], runs[1][1]) and not np.array_equal(runs[0][1], runs[2][1])
    for k in ("value", "norm"):
        assert np.array_equal(runs[0][0][k], runs[1][0][k]) and not np.array_equal(runs[0][0][k], runs[2][0][k])
    d, used, acc = runs[2]  # its kept samples are still in the slot: the same evaluation with the assignment handed back in
    back = device_obdm_sweeps_c(wf.fused_device(), acc.orbitals, acc._electrons, NSW, assign=used, mean=True)
    assert np.array_equal(back["value"], d["value"]) and np.array_equal(back["norm"], d["norm"])


# ------------------------------------------------------------------------------------------------------------ 8. no side effects
def test_no_side_effects_on_handle():
    import pyqmc_amd as pa

    sup, kmf, wf = _twisted_case()
    configs = _twisted_walkers(sup, 96, 16)
    wf.recompute(configs)
    twin = copy.deepcopy(wf)  # (rebuilt from the same walkers: the same state)
    dev, tdev = wf.fused_device(), twin.fused_device()
    for d in (dev, tdev):
        d.vmc_sweeps(0.3, 2, seed=9, energy=False)  # (state after a fused sweep: layouts and stale sums as a driver leaves them)
    orb = _kblocks(kmf, 2)
    for kw in (dict(spin=0), dict(spin=None)):
        acc = _accumulator(sup, orb, kmf.kpts, True, **kw)
        np.random.seed(5)
        acc.avg_resident(wf)
        acc.avg_resident(wf, weights=np.arange(1.0, 97.0))
        assert acc.last_route == "fused"
    v, tv = wf.value(), twin.value()
    assert np.array_equal(v[0], tv[0]) and np.array_equal(v[1], tv[1])
    assert np.array_equal(dev.configs(), tdev.configs())
    pvmc = importlib.import_module("pyqmc_amd.vmc")  # (the package exports the function vmc under that name)
    out = []
    for w in (wf, twin):
        c = copy.deepcopy(configs)
        pvmc._fetch(w.fused_device(), c)
        blk, after = pa.vmc_worker(w, c, 0.3, 2, {}, seed=4, state_current=True)
        out.append((after.configs.copy(), after.wrap.copy(), blk["acceptance"]))
    assert np.array_equal(out[0][0], out[1][0]) and np.array_equal(out[0][1], out[1][1]) and out[0][2] == out[1][2]


# ------------------------------------------------------------------------------------------------------------ 9. driver
def test_driver_twisted_cell(monkeypatch):
    """vmc_worker with {energy, rdm1_up} on the twisted cell, 64 walkers, 2 sweeps: the resident path (complex_device=True) against
    the host-accumulator path (the OBDM bound to route="protocol")."""
    import pyqmc_amd as pa
    pvmc = importlib.import_module("pyqmc_amd.vmc")  # (the package exports the function vmc under that name)

    sup, kmf, wf = _twisted_case()
    start = _twisted_walkers(sup, 64, 17)
    orb = _kblocks(kmf, 2)
    taken = []
    for name in ("_vmc_worker_resident_accumulators", "_vmc_worker_host_accumulators"):
        inner = getattr(pvmc, name)
        monkeypatch.setattr(pvmc, name, lambda *a, _n=name, _f=inner, **k: (taken.append(_n), _f(*a, **k))[1])
    out = {}
    for fused in (True, False):
        accs = {"energy": pa.EnergyAccumulator(sup), "rdm1_up": _accumulator(sup, orb, kmf.kpts, fused, spin=0)}
        np.random.seed(11)
        blk, cfg = pa.vmc_worker(wf, copy.deepcopy(start), 0.3, 2, accs, seed=5)
        assert accs["rdm1_up"].last_route == ("fused" if fused else "protocol")
        out[fused] = (blk, cfg, np.random.get_state())
    assert taken == ["_vmc_worker_resident_accumulators", "_vmc_worker_host_accumulators"]
    bf, bp = out[True][0], out[False][0]
    assert set(bf) == set(bp) and {"rdm1_upvalue", "rdm1_upnorm", "energytotal"} <= set(bf)
    for k in bp:
        if "time" in k:
            continue
        err = helpers.relerr(bf[k], bp[k])
        print(f"obdm complex driver {k}: {err:.2e}")
        assert err < 1e-9, (k, err)
        assert np.iscomplexobj(bf[k]) == np.iscomplexobj(bp[k]), k  # (energy keys complex where EnergyAccumulator returns them so)
    assert np.iscomplexobj(bf["rdm1_upvalue"]) and not np.iscomplexobj(bf["rdm1_upnorm"])
    assert np.array_equal(out[True][1].configs, out[False][1].configs) and np.array_equal(out[True][1].wrap, out[False][1].wrap)
    for a, b in zip(out[True][2], out[False][2]):
        assert np.array_equal(a, b)


# ------------------------------------------------------------------------------------------------------------ 10. scope
def _refused(wf, ev, match, electrons=(0,), nsweeps=1, **kw):
    from pyqmc_amd._ffi import PqaError
    from pyqmc_amd.obdm import device_obdm_sweeps_c

    W = wf.fused_device().W
    x = np.zeros((W, 3)) + 0.1
    ev.walk(0, 0, x, np.zeros((1, W, 3)), np.full((1, W), 0.5), 0.5, 1)
    with pytest.raises(PqaError, match=match) as info:
        device_obdm_sweeps_c(wf.fused_device(), ev, electrons, nsweeps, assign=np.zeros((nsweeps, W), dtype=np.int32), **kw)
    assert "protocol route" in str(info.value) and "pqa_obdm_sweeps_c" in str(info.value)


def test_scope_default_is_todays():
    import pyqmc_amd as pa

    sup, kmf, wf = _twisted_case()
    configs = _twisted_walkers(sup, 4, 18)
    wf.recompute(configs)
    orb = _kblocks(kmf, 2)
    acc = pa.OBDMAccumulator(sup, orb, kpts=kmf.kpts, nsweeps=1, warmup=2, spin=0)
    assert acc.complex_device is False and acc.resolve_route(wf, 4) == "protocol" and acc.resident_scope(wf) is not None
    assert acc._out_of_scope(wf) == "the wave function is not a real Slater (x two-body Jastrow) product on one device handle"
    with pytest.raises(ValueError, match="fused"):
        pa.OBDMAccumulator(sup, orb, kpts=kmf.kpts, nsweeps=1, warmup=2, spin=0, route="fused")(configs, wf)
    on = pa.OBDMAccumulator(sup, orb, kpts=kmf.kpts, nsweeps=1, warmup=2, spin=0, complex_device=True)
    assert on.resolve_route(wf, 4) == "fused" and on.resident_scope(wf) is None and on.resolve_route(wf, 5) == "protocol"
    np.random.seed(3)
    d = on(configs, wf)
    assert on.last_route == "fused" and d["value"].dtype == complex and d["value"].shape == (4, 2, 2)


def test_scope_twisted_evaluator_untwisted_handle():
    import pyqmc_amd as pa

    sup, wf = helpers.gpu_pbc_wf("gamma")
    _, kmf = helpers.twist_case("prim")
    orb = _kblocks(kmf, 2)
    configs = pa.initial_guess(sup, 4, rng=np.random.default_rng(14))
    wf.recompute(configs)
    acc = pa.OBDMAccumulator(sup, orb, kpts=kmf.kpts, nsweeps=1, warmup=2, spin=0, complex_device=True)
    assert acc.orbitals.dev.twisted and not wf.fused_device().twisted
    assert acc.resolve_route(wf, 4) == "protocol" and "twisted" in acc._out_of_scope(wf)
    np.random.seed(3)
    d = acc(configs, wf)
    assert acc.last_route == "protocol" and np.all(np.isfinite(d["value"]))
    with pytest.raises(ValueError, match="twisted"):
        pa.OBDMAccumulator(sup, orb, kpts=kmf.kpts, nsweeps=1, warmup=2, spin=0, complex_device=True, route="fused")(configs, wf)
    _refused(wf, acc.orbitals, "twisted orbital evaluator")
    # the complex UNTWISTED evaluator of the same handle is in scope
    kmf0 = pbc.random_kmf(sup, complex_coeff=True)
    ok = pa.OBDMAccumulator(sup, _kblocks(kmf0, 2), kpts=kmf0.kpts, nsweeps=1, warmup=2, spin=0, complex_device=True)
    assert ok.orbitals.dev.cplx and ok.resolve_route(wf, 4) == "fused"


def test_scope_library_refusals():
    import pyqmc_amd as pa
    from pyqmc_amd._ffi import PqaError
    from pyqmc_amd.obdm import device_obdm_sweeps_c
    from test_gpu_obdm_fused import _evaluator

    mol = systems.water()
    mf = systems.random_mf(mol)
    ev = _evaluator(mol, mf, 3)
    wf3 = helpers.gpu_wf3(mol, mf)
    wf3.recompute(pa.initial_guess(mol, 6, rng=np.random.default_rng(11)))
    _refused(wf3, ev, "three-body")
    acc = pa.obdm.OBDMAccumulator(mol, np.asarray(mf.mo_coeff)[0][:, :3], complex_device=True)
    assert acc.resolve_route(wf3, 6) == "protocol"
    sup, kmf, wf = _twisted_case()
    wf.recompute(_twisted_walkers(sup, 16, 19))
    tev = pa.obdm.OrbitalEvaluator(sup, _kblocks(kmf, 2), kpts=kmf.kpts)
    _refused(wf, tev, "listed twice", electrons=(1, 3, 1))
    _refused(wf, tev, "more sweeps", nsweeps=2)
    with pytest.raises(ValueError, match="mean mode"):
        device_obdm_sweeps_c(wf.fused_device(), tev, [0], 1, weights=np.ones(16))
    with pytest.raises(PqaError, match="mean mode"):  # (the library itself: walker weights without the mean mode)
        wf.fused_device().call("pqa_obdm_sweeps_c", tev.dev._h, 0, pa._ffi.ptr(np.zeros(1, dtype=np.int32)), 1, 1, None, 0, 0, 1, 0,
                               pa._ffi.ptr(np.ones(16)), None, None, None, None)
    # accumulators started for 16 walkers cannot take the sweeps of a handle that holds 8
    device_obdm_sweeps_c(wf.fused_device(), tev, [0, 5], 1, assign=np.zeros((1, 16), dtype=np.int32))
    wf.recompute(_twisted_walkers(sup, 8, 20))
    with pytest.raises(PqaError, match="another number of walkers"):
        device_obdm_sweeps_c(wf.fused_device(), tev, [0, 5], 1, assign=np.zeros((1, 8), dtype=np.int32), first=False)
