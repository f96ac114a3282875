"""Two-body density matrix of complex and twisted handles on the fused route (pqa_tbdm_sweep_c, opt-in through
TBDMAccumulator(complex_device=True)): the complex pair ratios against recomputes of all doubly moved walkers and against the
protocol route's own ratios (twisted cell, complex Bloch determinants, the twisted 2 x 1 x 1 cell with 18 evaluator orbitals), mixed
pairs of real and complex handles, real handles against pqa_tbdm_sweep, whole lattice vectors, the whole accumulator against the
protocol route, chunking and repeatability, the resident mean and its weights, no side effects, and the scope.

Metrics and bounds are those of tests/test_gpu_tbdm_fused.py and tests/test_gpu_obdm_complex.py: _err = max |a - b| / (1 + |b|) < 1e-10
where the two sides differ in formula and summation order; helpers.relerr < 1e-9 where only the summation order differs; bitwise equality
where stated.  Every comparison covers every walker and every pair; references are finite with max |ref| > 1e-6."""

import copy
import importlib

import numpy as np
import pytest

from pyqmc_amd import pbc, systems
from pyqmc_amd.configs import OpenConfigs, PeriodicConfigs
from tests import helpers
from test_gpu_obdm_complex import _bloch_case, _kblocks, _twisted_case, _twisted_walkers
from test_gpu_tbdm_fused import SECTORS, _err, _no_jastrow, _place

pytestmark = pytest.mark.gpu

W70 = 70


def _direct_c(wf, make, x, r1, r2, sector, nel):
    """test_gpu_tbdm_fused._direct with complex phases: phase exp(dlog) (W, nea, neb) of ONE recompute of all doubly moved walkers
    (true coordinates ``x``: ``make`` folds them and counts the crossings, which carry the Bloch phase); 0 where a and b are one
    electron.  (_direct itself stores the ratios in a real array.)"""
    s1, s2 = sector
    W = x.shape[0]
    pairs = [(a, b) for a in range(nel[s1]) for b in range(nel[s2]) if a + s1 * nel[0] != b + s2 * nel[0]]
    y = np.tile(x, (len(pairs) + 1, 1, 1))
    for p, (a, b) in enumerate(pairs):
        y[(p + 1) * W : (p + 2) * W, a + s1 * nel[0]] = r1
        y[(p + 1) * W : (p + 2) * W, b + s2 * nel[0]] = r2
    s, l = wf.recompute(make(y))
    out = np.zeros((W, nel[s1], nel[s2]), dtype=complex)
    for p, (a, b) in enumerate(pairs):
        sl = slice((p + 1) * W, (p + 2) * W)
        out[:, a, b] = s[sl] / s[:W] * np.exp(l[sl] - l[:W])
    wf.recompute(make(x.copy()))
    return out


def _accumulator(sup, orb, kpts, spin, fused=True, **kw):
    import pyqmc_amd as pa

    extra = dict(complex_device=True) if fused else dict(route="protocol")
    return pa.TBDMAccumulator(sup, orb, spin=spin, kpts=kpts, nsweeps=2, tstep=0.4, warmup=4, **extra, **kw)


def _check_sectors(sup, wf, acc, configs, seed, sectors, spread=0.5):
    """The ratios of pqa_tbdm_sweep_c in every listed sector against one recompute of all doubly moved walkers; in the accumulator's own
    sector also against its _pair_ratios (the protocol route), and one accumulating sweep against pqa_tbdm_accumulate fed with the same
    ratios (bitwise: one kernel, the same operands).  W + 3 auxiliary points per slot, placed around the (unfolded) electrons."""
    from pyqmc_amd import _ffi
    from pyqmc_amd.tbdm import device_pair_ratios_c, device_tbdm_sweep_c

    ev, lat = acc.orbitals, sup.lattice_vectors()
    make = lambda y: PeriodicConfigs(y, lat)  # noqa: E731
    rng = np.random.default_rng(seed)
    x = ev.true_positions(configs)
    W, N = x.shape[:2]
    naux = W + 3  # (more auxiliary walkers than configurations: the assignment is a real indirection)
    aux = [x[rng.integers(0, W, naux), rng.integers(0, N, naux)] + spread * rng.standard_normal((naux, 3)) for _ in (0, 1)]
    pick = [rng.integers(0, naux, W).astype(np.int32) for _ in (0, 1)]
    for s in (0, 1):
        _place(ev, s, aux[s])
    r1, r2 = aux[0][pick[0]], aux[1][pick[1]]
    dev = wf.fused_device()
    wf.recompute(make(x.copy()))
    worst = 0.0
    for sector in sectors:
        ref = _direct_c(wf, make, x, r1, r2, sector, sup.nelec)
        R = device_pair_ratios_c(dev, ev, 0, sector, pick[0], pick[1])
        err = _err(R, ref)
        print(f"tbdm complex ratios {sector}: {err:.2e} (max |direct| {np.max(np.abs(ref)):.2e}, max |Im| {np.max(np.abs(ref.imag)):.2e})")
        assert R.dtype == complex and R.shape == ref.shape
        assert np.all(np.isfinite(ref)) and np.max(np.abs(ref)) > 1e-6
        assert err < 1e-10, (sector, err)
        if sector[0] == sector[1]:
            n = R.shape[1]
            d = R[:, np.arange(n), np.arange(n)]
            assert np.all(d.real == 0.0) and np.all(d.imag == 0.0)
        worst = max(worst, err)
    sector = acc._spin_sector
    if sector in sectors:
        for s in (0, 1):
            ev.points(s, s, x[:, acc._electrons[s]])
        ijkl = acc._ijkl[:, :: max(1, acc._ijkl.shape[1] // 97)]  # (a spread of index tuples)
        ijkl = np.ascontiguousarray(ijkl)
        na, nb = ev.nmo()
        R = device_tbdm_sweep_c(dev, ev, 0, sector, pick[0], pick[1], ijkl, True, with_ratios=True)
        fused = [ev.fetch(0, W, (ijkl.shape[1],), 1.0, False, True), ev.fetch(1, W, (na,), 1.0, False), ev.fetch(2, W, (nb,), 1.0, False)]
        ev.dev.call("pqa_tbdm_accumulate", 0, W, R.shape[1], R.shape[2], _ffi.ptr(pick[0]), _ffi.ptr(pick[1]), _ffi.ptr(R), 1, _ffi.ptr(ijkl),
                    ijkl.shape[1], 1)
        host = [ev.fetch(0, W, (ijkl.shape[1],), 1.0, False, True), ev.fetch(1, W, (na,), 1.0, False), ev.fetch(2, W, (nb,), 1.0, False)]
        assert np.max(np.abs(host[0])) > 1e-6 and np.all(np.isfinite(host[0]))
        for f, h in zip(fused, host):
            assert np.array_equal(f, h)
        # last: the protocol route's moves there and back leave round-off in the state
        there = [ev.container(p).electron(0) for p in (r1, r2)]
        proto = acc._pair_ratios(make(x.copy()), wf, *there)
        err = _err(R, proto)
        print(f"tbdm complex ratios {sector} against _pair_ratios: {err:.2e}")
        assert np.iscomplexobj(proto) == bool(dev.cplx) and np.max(np.abs(proto)) > 1e-6 and err < 1e-10, (sector, err)
        wf.recompute(make(x.copy()))
    return x, aux, pick, worst


# ------------------------------------------------------------------------------------------------------------ 1. ratios
@pytest.mark.parametrize("jastrow", [True, False])
def test_twisted_cell_all_sectors(jastrow):
    """The twisted primitive cell, 4 + 4 electrons (groups of 4 lanes, 16 inverse rows per pass), a twisted evaluator: 70 walkers partly
    outside the cell."""
    sup, kmf, wf = _twisted_case()
    if not jastrow:
        _no_jastrow(wf)
    acc = _accumulator(sup, _kblocks(kmf, 3), kmf.kpts, (0, 1))
    assert acc.orbitals.dev.twisted
    _check_sectors(sup, wf, acc, _twisted_walkers(sup, W70, 1), 1, SECTORS)


def test_complex_determinants_all_sectors():
    """The complex 3 x 1 x 1 cell, 12 + 12 electrons, three determinants: groups of 16 lanes with masked lanes, D n rows no multiple of
    the rows per pass, complex determinant weights."""
    import pyqmc_amd as pa

    sup, mf, wf = _bloch_case()
    acc = _accumulator(sup, _kblocks(mf, 2), mf.kpts, (1, 1))
    assert acc.orbitals.dev.cplx and not acc.orbitals.dev.twisted
    _check_sectors(sup, wf, acc, pa.initial_guess(sup, W70, rng=np.random.default_rng(2)), 2, SECTORS)


def test_s211_eighteen_orbitals():
    """The twisted 2 x 1 x 1 cell, 8 + 8 electrons, an evaluator with 18 orbitals (random complex coefficients, 9 per k-point)."""
    sup, kmf, wf = _twisted_case("s211")
    nao = np.asarray(kmf.mo_coeff[0][0]).shape[0]
    rng = np.random.default_rng(6)
    orb = [0.4 * (rng.standard_normal((nao, 9)) + 1j * rng.standard_normal((nao, 9))) for _ in range(len(kmf.kpts))]
    acc = _accumulator(sup, orb, kmf.kpts, (0, 0))
    assert acc.orbitals.dev.twisted and acc.orbitals.nmo() == [18, 18]
    _check_sectors(sup, wf, acc, _twisted_walkers(sup, W70, 5), 5, SECTORS)


# ------------------------------------------------------------------------------------------------------------ 2. mixed pairs
def test_complex_handle_real_evaluator():
    """A complex Gamma handle with a REAL evaluator."""
    import pyqmc_amd as pa

    sup, _ = helpers.pbc_slater_case("gamma")
    kmf = pbc.random_kmf(sup, complex_coeff=True)
    sup, wf = helpers.gpu_pbc_wf("gamma", case=(sup, kmf))
    assert wf.fused_device().cplx and not wf.fused_device().twisted
    nao = np.asarray(kmf.mo_coeff[0][0]).shape[0]
    acc = _accumulator(sup, [0.4 * np.random.default_rng(3).standard_normal((nao, 5))], np.zeros((1, 3)), (0, 1))
    assert not acc.orbitals.dev.cplx and acc._complex_entry(wf.fused_device())
    _check_sectors(sup, wf, acc, pa.initial_guess(sup, W70, rng=np.random.default_rng(4)), 3, [(0, 1), (1, 1)])


def test_real_handle_complex_evaluator():
    """A real Gamma handle with a complex untwisted evaluator: Im R is exactly 0, the accumulated value is complex."""
    from pyqmc_amd.tbdm import device_pair_ratios_c

    sup, wf = helpers.gpu_pbc_wf("gamma")
    assert not wf.fused_device().cplx
    kmf = pbc.random_kmf(sup, complex_coeff=True)
    acc = _accumulator(sup, _kblocks(kmf, 3), kmf.kpts, (0, 0))
    assert acc.orbitals.dev.cplx and not acc.orbitals.dev.twisted and acc._complex_entry(wf.fused_device())
    lat = sup.lattice_vectors()
    x = np.random.default_rng(5).random((W70, sum(sup.nelec), 3)) @ lat
    _, _, pick, _ = _check_sectors(sup, wf, acc, PeriodicConfigs(x, lat), 4, [(0, 0), (1, 0)])
    for sector in SECTORS:
        R = device_pair_ratios_c(wf.fused_device(), acc.orbitals, 0, sector, pick[0], pick[1])
        assert np.all(R.imag == 0.0) and np.max(np.abs(R.real)) > 1e-6


@pytest.mark.parametrize("case", ["open_shell", "six_determinants"])
def test_real_handle_through_the_complex_entry(case):
    """Water (5, 3) and a 6-determinant water through pqa_tbdm_sweep_c against pqa_tbdm_sweep.  Bitwise: the norms (k_tbdm_acc reads
    the same kept rows).  Not bitwise: the ratios and the values — the complex kernel rounds each product of the inverse-row and
    determinant sums on its own where the real one fuses it into the running sum, and divides by the complex weight sum — so those are
    held to 1e-10, with imaginary parts exactly 0."""
    import pyqmc_amd as pa
    from pyqmc_amd.tbdm import device_tbdm_sweep, device_tbdm_sweep_c
    from test_gpu_tbdm_fused import _evaluator, _water

    if case == "open_shell":
        mol = _water((5, 3))
        mf = systems.random_mf(mol)
        wf = helpers.gpu_wf(mol, mf)
    else:
        mol = systems.water()
        mf = systems.random_mf(mol, nvirt=6)
        wf = helpers.gpu_wf(mol, mf, systems.random_determinants(mol, mf, 6))
    ev = _evaluator(mol, mf, 3)
    rng = np.random.default_rng(8)
    x = pa.initial_guess(mol, W70, rng=rng).configs
    naux = W70 + 3
    aux = [x[rng.integers(0, W70, naux), rng.integers(0, x.shape[1], naux)] + 0.8 * rng.standard_normal((naux, 3)) for _ in (0, 1)]
    pick = [rng.integers(0, naux, W70).astype(np.int32) for _ in (0, 1)]
    for s in (0, 1):
        _place(ev, s, aux[s])
    wf.recompute(OpenConfigs(x.copy()))
    dev = wf.fused_device()
    ijkl = np.stack(np.meshgrid(*[np.arange(3)] * 4, indexing="ij"), -1).reshape(-1, 4).T
    for sector in SECTORS:
        nea, neb = mol.nelec[sector[0]], mol.nelec[sector[1]]
        for s in (0, 1):
            ev.points(s, s, x[:, np.arange(sector[s] * mol.nelec[0], mol.nelec[0] + sector[s] * mol.nelec[1])])
        out = []
        for sweep, cplx in ((device_tbdm_sweep, False), (device_tbdm_sweep_c, True)):
            R = sweep(dev, ev, 0, sector, pick[0], pick[1], ijkl, True, with_ratios=True)
            out.append((R, ev.fetch(0, W70, (81,), 1.0, False, cplx), ev.fetch(1, W70, (3,), 1.0, False), ev.fetch(2, W70, (3,), 1.0, False)))
        (Rr, vr, nar, nbr), (Rc, vc, nac, nbc) = out
        assert Rr.shape == (W70, nea, neb) and Rc.dtype == complex and vc.dtype == complex
        assert np.all(Rc.imag == 0.0) and np.all(vc.imag == 0.0)
        errs = _err(Rc.real, Rr), _err(vc.real, vr)
        print(f"tbdm real handle through the complex entry {case} {sector}: ratios {errs[0]:.2e} values {errs[1]:.2e}")
        assert np.max(np.abs(Rr)) > 1e-6 and np.max(np.abs(vr)) > 1e-6 and max(errs) < 1e-10
        assert np.array_equal(nac, nar) and np.array_equal(nbc, nbr)


# ------------------------------------------------------------------------------------------------------------ 3. lattice vectors
def test_twisted_points_moved_by_lattice_vectors():
    """Auxiliary points pushed out of the cell by the lattice vectors n1 . L and n2 . L have the ratios of the folded points times the
    Bloch phases exp(i k_t . (n1 + n2) . L) of the two moved electrons: the reference is the recompute at the FOLDED points, times the
    phase."""
    from pyqmc_amd.tbdm import device_pair_ratios_c

    sup, kmf, wf = _twisted_case()
    acc = _accumulator(sup, _kblocks(kmf, 3), kmf.kpts, (0, 1))
    ev, lat, kt = acc.orbitals, sup.lattice_vectors(), pbc.common_twist(sup, kmf.kpts)
    make = lambda y: PeriodicConfigs(y, lat)  # noqa: E731
    W = 16
    rng = np.random.default_rng(7)
    x = ev.true_positions(_twisted_walkers(sup, W, 8))
    inside = [rng.random((W, 3)) @ lat for _ in (0, 1)]
    n = [rng.integers(-2, 3, (W, 3)).astype(float) for _ in (0, 1)]
    outside = [p + m @ lat for p, m in zip(inside, n)]
    assert max(np.max(np.abs(o - p)) for o, p in zip(outside, inside)) > 1.0
    phase = np.exp(1j * ((n[0] + n[1]) @ lat) @ kt)
    assert np.max(np.abs(phase - 1)) > 1e-3
    pick = np.arange(W, dtype=np.int32)
    dev = wf.fused_device()
    wf.recompute(make(x.copy()))
    for sector in SECTORS:
        ref = _direct_c(wf, make, x, inside[0], inside[1], sector, sup.nelec)
        got = []
        for pts in (inside, outside):
            for s in (0, 1):
                _place(ev, s, pts[s])
            got.append(device_pair_ratios_c(dev, ev, 0, sector, pick, pick))
        errs = _err(got[0], ref), _err(got[1], ref * phase[:, None, None])
        print(f"tbdm complex lattice vectors {sector}: folded {errs[0]:.2e} moved {errs[1]:.2e}")
        assert np.all(np.isfinite(ref)) and np.max(np.abs(ref)) > 1e-6 and max(errs) < 1e-10, (sector, errs)


# ------------------------------------------------------------------------------------------------------------ 4. whole accumulator
CASES = {"twisted_ud": ("twisted", (0, 1), {}), "twisted_uu": ("twisted", (0, 0), {}), "bloch_dd": ("bloch", (1, 1), {}),
         "twisted_ud_naux": ("twisted", (0, 1), dict(naux=37))}


def _system(kind, seed):
    import pyqmc_amd as pa

    if kind == "twisted":
        sup, kmf, wf = _twisted_case()
        return sup, kmf, wf, _twisted_walkers(sup, W70, seed)
    sup, kmf, wf = _bloch_case()
    return sup, kmf, wf, pa.initial_guess(sup, W70, rng=np.random.default_rng(seed))


@pytest.mark.parametrize("case", list(CASES))
def test_fused_matches_protocol(case):
    kind, spin, kw = CASES[case]
    sup, kmf, wf, configs = _system(kind, 9)
    orb = _kblocks(kmf, 2)
    wf.recompute(configs)
    out, states = {}, {}
    for route in ("fused", "protocol"):  # (the protocol route last: its moves there and back leave round-off in the state)
        acc, acc2 = (_accumulator(sup, orb, kmf.kpts, spin, route == "fused", **kw) for _ in (0, 1))
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
        for k in ("value", "norm_a", "norm_b"):
            assert f[k].dtype == p[k].dtype and f[k].shape == p[k].shape, (call, k)
            assert np.all(np.isfinite(p[k])) and np.max(np.abs(p[k])) > 1e-6
        err = _err(f["value"], p["value"])
        print(f"tbdm complex fused vs protocol {case} call {call}: value {err:.2e} (max |value| {np.max(np.abs(p['value'])):.2e})")
        assert err < 1e-10 and f["value"].dtype == complex and f["norm_a"].dtype == float and f["norm_b"].dtype == float
        for k in ("norm_a", "norm_b"):  # (formed by k_tbdm_acc from the same kept rows on both routes)
            assert np.array_equal(f[k], p[k]), (call, k)
        if call < 2:
            assert f["value"].shape[0] == W70


# ------------------------------------------------------------------------------------------------------------ 5. / 6. repeatability
def test_chunking_and_repeats_are_bitwise():
    """walker_chunk = 24 at 70 walkers (two whole chunks and a remainder) against one chunk: ratios and accumulators; two calls."""
    from pyqmc_amd.tbdm import device_pair_ratios_c

    sup, kmf, wf = _twisted_case()
    orb = _kblocks(kmf, 2)
    acc0 = _accumulator(sup, orb, kmf.kpts, (0, 1))
    configs = _twisted_walkers(sup, W70, 13)
    x, aux, pick, _ = _check_sectors(sup, wf, acc0, configs, 13, [])
    dev = wf.fused_device()
    for sector in ((0, 1), (1, 1)):
        whole = device_pair_ratios_c(dev, acc0.orbitals, 0, sector, pick[0], pick[1])
        parts = device_pair_ratios_c(dev, acc0.orbitals, 0, sector, pick[0], pick[1], walker_chunk=24)
        again = device_pair_ratios_c(dev, acc0.orbitals, 0, sector, pick[0], pick[1])
        assert np.array_equal(whole, parts) and np.array_equal(whole, again)
        assert np.max(np.abs(whole.imag)) > 1e-6
    wf.recompute(configs)
    out = []
    for chunk in (0, 24, 0):
        acc = _accumulator(sup, orb, kmf.kpts, (0, 0), walker_chunk=chunk)
        np.random.seed(17)
        out.append((acc(configs, wf), acc.avg(configs, wf)))
        assert acc.last_route == "fused"
    for other in out[1:]:
        for u, v in zip(out[0], other):
            for k in ("value", "norm_a", "norm_b"):
                assert np.array_equal(u[k], v[k]), k
    assert out[0][0]["value"].dtype == complex and np.max(np.abs(out[0][0]["value"].imag)) > 1e-6


# ------------------------------------------------------------------------------------------------------------ 7. resident mean
def test_resident_mean_and_weights():
    sup, kmf, wf = _twisted_case()
    configs = _twisted_walkers(sup, W70, 11)
    wf.recompute(configs)
    orb = _kblocks(kmf, 2)
    w = 0.5 + np.random.default_rng(12).random(W70)
    out, states = {}, {}
    for name, wts in (("per", None), ("avg", None), ("resident", None), ("weighted", w), ("unit", np.ones(W70))):
        acc = _accumulator(sup, orb, kmf.kpts, (0, 1))
        assert acc.resident_scope(wf) is None
        np.random.seed(31)
        out[name] = acc(configs, wf) if name == "per" else (acc.avg(configs, wf) if name == "avg" else acc.avg_resident(wf, weights=wts))
        states[name] = np.random.get_state()
        assert acc.last_route == "fused"
    for name in states:
        for a, b in zip(states["per"], states[name]):
            assert np.array_equal(a, b)
    for k in ("value", "norm_a", "norm_b"):
        assert np.all(np.isfinite(out["avg"][k])) and np.max(np.abs(out["avg"][k])) > 1e-6
        errs = helpers.relerr(out["resident"][k], out["avg"][k]), helpers.relerr(out["weighted"][k], np.tensordot(w, out["per"][k], axes=(0, 0)) / w.sum())
        print(f"tbdm complex resident {k}: against avg {errs[0]:.2e}, weighted against sum w res / sum w {errs[1]:.2e}")
        assert max(errs) < 1e-9
        for name in ("resident", "weighted", "unit"):
            assert out[name][k].dtype == out["avg"][k].dtype and out[name][k].shape == out["avg"][k].shape
        assert np.array_equal(out["unit"][k], out["resident"][k])  # (a weight of 1 leaves every bit of the unweighted mean)
    assert out["resident"]["value"].dtype == complex and out["resident"]["norm_a"].dtype == float
    with pytest.raises(ValueError):
        _accumulator(sup, orb, kmf.kpts, (0, 1)).avg_resident(wf, weights=-w)


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
    for spin in ((0, 1), (0, 0)):
        acc = _accumulator(sup, orb, kmf.kpts, spin)
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


# ------------------------------------------------------------------------------------------------------------ 9. scope
def _refused(entry, wf, ev, match):
    from pyqmc_amd._ffi import PqaError

    W = wf.fused_device().W
    pick = np.zeros(W, dtype=np.int32)
    for s in (0, 1):
        _place(ev, s, np.zeros((W, 3)) + 0.1)
    with pytest.raises(PqaError, match=match) as info:
        entry(wf.fused_device(), ev, 0, (0, 1), pick, pick)
    assert "protocol route" in str(info.value)
    return str(info.value)


def test_scope_default_is_todays():
    import pyqmc_amd as pa
    from pyqmc_amd.tbdm import device_pair_ratios

    sup, kmf, wf = _twisted_case()
    configs = _twisted_walkers(sup, 4, 18)
    wf.recompute(configs)
    orb = _kblocks(kmf, 2)
    acc = pa.TBDMAccumulator(sup, orb, spin=(0, 1), kpts=kmf.kpts, nsweeps=1, warmup=2)
    assert acc.complex_device is False and acc._fused_device(configs, wf) is None
    assert acc.resident_scope(wf) == "the wave function is not a real Slater (x two-body Jastrow) product on one device handle"
    np.random.seed(3)
    d = acc(configs, wf)
    assert acc.last_route == "protocol" and np.all(np.isfinite(d["value"]))
    with pytest.raises(ValueError, match="real Slater"):
        pa.TBDMAccumulator(sup, orb, spin=(0, 1), kpts=kmf.kpts, nsweeps=1, warmup=2, route="fused")(configs, wf)
    with pytest.raises(ValueError, match="real Slater"):
        acc.avg_resident(wf)
    # pqa_tbdm_sweep itself still refuses the complex handle, with its present text
    text = _refused(device_pair_ratios, wf, acc.orbitals, "complex orbitals / twisted cell")
    assert "pqa_tbdm_sweep: complex orbitals / twisted cell (outside the fused scope: use the protocol route)" in text
    on = pa.TBDMAccumulator(sup, orb, spin=(0, 1), kpts=kmf.kpts, nsweeps=1, warmup=2, complex_device=True)
    assert on._fused_device(configs, wf) is wf.fused_device() and on.resident_scope(wf) is None
    np.random.seed(3)
    f = on(configs, wf)
    assert on.last_route == "fused" and f["value"].dtype == complex and f["value"].shape == d["value"].shape
    for bad in (1, "yes", None):
        with pytest.raises(ValueError, match="complex_device"):
            pa.TBDMAccumulator(sup, orb, spin=(0, 1), kpts=kmf.kpts, complex_device=bad)


def test_scope_twisted_evaluator_untwisted_handle():
    import pyqmc_amd as pa
    from pyqmc_amd.tbdm import device_pair_ratios_c

    sup, wf = helpers.gpu_pbc_wf("gamma")
    _, kmf = helpers.twist_case("prim")
    orb = _kblocks(kmf, 2)
    configs = pa.initial_guess(sup, 4, rng=np.random.default_rng(14))
    wf.recompute(configs)
    acc = pa.TBDMAccumulator(sup, orb, spin=(0, 1), kpts=kmf.kpts, nsweeps=1, warmup=2, complex_device=True)
    assert acc.orbitals.dev.twisted and not wf.fused_device().twisted
    assert acc._fused_device(configs, wf) is None and "twisted" in acc.resident_scope(wf)
    np.random.seed(3)
    d = acc(configs, wf)
    assert acc.last_route == "protocol" and np.all(np.isfinite(d["value"]))
    with pytest.raises(ValueError, match="twisted"):
        pa.TBDMAccumulator(sup, orb, spin=(0, 1), kpts=kmf.kpts, nsweeps=1, warmup=2, complex_device=True, route="fused")(configs, wf)
    with pytest.raises(ValueError, match="twisted"):
        acc.avg_resident(wf)
    text = _refused(device_pair_ratios_c, wf, acc.orbitals, "twisted orbital evaluator")
    assert "pqa_tbdm_sweep_c" in text
    # the complex UNTWISTED evaluator of the same handle is in scope
    kmf0 = pbc.random_kmf(sup, complex_coeff=True)
    ok = pa.TBDMAccumulator(sup, _kblocks(kmf0, 2), spin=(0, 1), kpts=kmf0.kpts, nsweeps=1, warmup=2, complex_device=True)
    assert ok.orbitals.dev.cplx and ok._fused_device(configs, wf) is wf.fused_device()


def test_scope_three_body_and_real_pairs():
    import pyqmc_amd as pa
    from pyqmc_amd.tbdm import device_pair_ratios_c
    from test_gpu_tbdm_fused import _evaluator

    mol = systems.water()
    mf = systems.random_mf(mol)
    ev = _evaluator(mol, mf, 3)
    wf3 = helpers.gpu_wf3(mol, mf)
    configs = pa.initial_guess(mol, 6, rng=np.random.default_rng(11))
    wf3.recompute(configs)
    assert "pqa_tbdm_sweep_c" in _refused(device_pair_ratios_c, wf3, ev, "three-body")
    C = np.asarray(mf.mo_coeff)
    acc = pa.TBDMAccumulator(mol, [C[0][:, :3], C[1][:, :3]], spin=(0, 1), nsweeps=1, warmup=2, complex_device=True)
    assert acc._fused_device(configs, wf3) is None
    with pytest.raises(ValueError, match="fused"):
        pa.TBDMAccumulator(mol, [C[0][:, :3], C[1][:, :3]], spin=(0, 1), nsweeps=1, warmup=2, complex_device=True, route="fused")(configs, wf3)
    # two real handles with complex_device=True: pqa_tbdm_sweep, the bits of the default
    wf = helpers.gpu_wf(mol, mf)
    wf.recompute(configs)
    out = []
    for kw in (dict(), dict(complex_device=True)):
        a = pa.TBDMAccumulator(mol, [C[0][:, :3], C[1][:, :3]], spin=(0, 1), nsweeps=1, warmup=2, **kw)
        np.random.seed(6)
        out.append(a(configs, wf))
        assert a.last_route == "fused" and not a._complex_entry(wf.fused_device())
    for k in ("value", "norm_a", "norm_b"):
        assert out[0][k].dtype == float and np.array_equal(out[0][k], out[1][k])
