"""Stochastic-reconfiguration moments of complex and twisted handles from the resident state (pqa_sr_moments_c, opt-in through
complex_device=True) against the protocol route of the same accumulator (pgradient, energy, four pqa_gram products) on the same
walkers and energy draws: a twisted cell whose columns are all real, complex determinant columns beside real Jastrow blocks (one, two
and four matrix instructions per step), the imaginary-part tail against NumPy, a real handle against pqa_sr_moments, repeatability and
chunking, the handle left as it was, a gradient-VMC block, and the scope.

Tolerance: both routes use the same per-walker numbers and differ in summation order only (~ W 2^-53), checked at the 1e-9 of
test_gpu_sr_moments.py; two device calls give the same bits."""

import copy
import importlib

import numpy as np
import pytest

import pyqmc_amd as pa
from pyqmc_amd import pbc, systems
from pyqmc_amd import wf as pwf
from pyqmc_amd.accumulators import LinearTransform, gradient_generator, nodal_regularization, sr_columns, sr_columns_c, sr_route
from pyqmc_amd.configs import OpenConfigs, PeriodicConfigs
from tests import helpers

pytestmark = pytest.mark.gpu

TOL = 1e-9
pvmc = importlib.import_module("pyqmc_amd.vmc")


def _twisted_walkers(sup, W, seed):
    """Walkers of a periodic cell placed partly outside it (the container folds them and counts the crossings)."""
    lat = sup.lattice_vectors()
    frac = np.random.default_rng(seed).random((W, sum(sup.nelec), 3)) * 2.4 - 0.7
    cfg = PeriodicConfigs(frac @ lat, lat)
    assert np.any(cfg.wrap != 0)
    return cfg


@pytest.fixture(scope="module")
def twisted():
    sup, kmf = helpers.twist_case("prim")
    sup, wf = helpers.gpu_pbc_wf("prim", case=(sup, kmf))
    dev = wf.fused_device()
    assert dev.twisted and dev.cplx and sum(sup.nelec) == 8
    return sup, wf


@pytest.fixture(scope="module")
def bloch():
    """The complex 3 x 1 x 1 cell with three determinants (one virtual orbital per k-point)."""
    sup = helpers.pbc_complex_case()[0]
    mf = pbc.random_kmf(sup, complex_coeff=True, nvirt=1)
    base = [5 * k + i for k in range(3) for i in range(4)]  # flat indices into the per-k blocks of 4 + 1 orbitals
    ex1, ex2 = sorted(set(base) - {3} | {4}), sorted(set(base) - {13} | {14})  # (the last column in use: no orbital is cut off)
    dets = [(1.0, [base, base]), (0.3, [ex2, base]), (-0.2, [ex1, ex2])]
    sup, wf = helpers.gpu_pbc_wf("cplx", case=(sup, mf), determinants=dets)
    dev = wf.fused_device()
    assert dev.ndet == 3 and dev.cplx and not dev.twisted
    return sup, wf


def _pair(mol, wf, to_opt=None, seed=100):
    """The same accumulator once per route, with the same energy key sequence."""
    out = []
    for route in ("device", "protocol"):
        sr = gradient_generator(mol, wf, to_opt or pwf.default_to_opt(wf), route=route, complex_device=True)
        sr.enacc.seed = seed
        out.append(sr)
    return out


def _agree(d, p):
    assert sorted(d) == sorted(p)
    worst = 0.0
    for k in p:
        err = helpers.relerr(d[k], p[k])
        print(k, err)
        worst = max(worst, err)
        assert np.shape(d[k]) == np.shape(p[k]) and err < TOL, (k, err)
        assert np.iscomplexobj(d[k]) == np.iscomplexobj(p[k]), k
    return worst


def test_twisted_cell_real_columns(twisted):
    sup, wf = twisted
    configs = _twisted_walkers(sup, 70, 1)  # one 64-walker slice plus a tail
    wf.recompute(configs)
    sd, sp = _pair(sup, wf)
    assert "wf1det_coeff" not in sd.transform.to_opt  # one determinant: every column is a (real) Jastrow sum
    for wts in (None, 0.5 + np.random.default_rng(2).random(70)):
        d, p = sd.avg(configs, wf, weights=wts), sp.avg(configs, wf, weights=wts)
        _agree(d, p)
        assert sd.last_route == "device" and sp.last_route == "protocol"
        if wf.fused_device().necp:
            assert np.abs(np.imag(d["dpH"])).max() > 0 and np.imag(d["total"]) != 0
        assert np.all(np.imag(d["dpidpj"]) == 0) and np.all(np.imag(d["dppsi"]) == 0)
        assert all(np.isrealobj(d[k]) for k in ("ke", "ee", "ei", "grad2"))
    # the walkers are compared unfolded: a container that differs is refused
    other = copy.deepcopy(configs)
    other.configs[3, 2] += 1e-3
    with pytest.raises(ValueError, match="differ"):
        sd.avg(other, wf)


def _bloch_to_opt(wf):
    """default_to_opt with the determinant columns between the Jastrow keys: column block 0 is real, block 1 holds the complex
    columns and E - block pairs with one, two (either side) and four matrix instructions per step."""
    t = pwf.default_to_opt(wf)
    return {k: t[k] for k in ("wf2acoeff", "wf1det_coeff", "wf2bcoeff")}


def test_complex_determinants(bloch):
    sup, wf = bloch
    W = 96
    configs = pa.initial_guess(sup, W, rng=np.random.default_rng(3))
    wf.recompute(configs)
    to_opt = _bloch_to_opt(wf)
    sd, sp = _pair(sup, wf, to_opt)
    tr = sd.transform
    P = tr.nparams
    src, pos, tail = sr_columns_c(tr)
    first_det = int(np.flatnonzero(src == 0)[0])
    assert P > 32 and P % 16 != 0 and first_det >= 32 and len(tail) == 0
    d, p = sd.avg(configs, wf), sp.avg(configs, wf)
    _agree(d, p)
    assert sd.last_route == "device" and sp.last_route == "protocol"
    assert np.abs(np.imag(d["dpidpj"])).max() > 0
    assert np.array_equal(d["dpidpj"], d["dpidpj"].T)
    dev = wf.fused_device()
    dp = dev.sr_moments_c(src, pos, tail, 1e-3, seed=5, dp_walker=True)[2]
    ref = tr.serialize_gradients(wf.pgradient())
    err = helpers.relerr(dp, ref)
    print("dp_walker", err)
    assert dp.shape == ref.shape and err < TOL
    assert np.all(dp[:, src != 0].imag == 0) and np.abs(dp[:, src == 0].imag).max() > 0


def test_tail_columns_against_numpy(bloch):
    sup, wf = bloch
    W = 96
    configs = pa.initial_guess(sup, W, rng=np.random.default_rng(4))
    wf.recompute(configs)
    dev = wf.fused_device()
    tr = LinearTransform(wf.parameters, _bloch_to_opt(wf))
    src, pos = sr_columns(tr)
    P = len(src)
    tail = np.flatnonzero(src == 0)[::-1].astype(np.int32)  # the determinant columns, not in primary order
    assert len(tail) == 2
    en = dev.energy(10.0, seed=77)
    cut = float(np.median(en[4].real) ** -0.5)
    near, f = nodal_regularization(en[4].real, cut)
    assert near.any() and (~near).any()
    wts = 0.5 + np.random.default_rng(6).random(W)
    mean, mom, enw, dp = dev.sr_moments_c(src, pos, tail, cut, weights=wts, seed=77, per_walker=True, dp_walker=True)
    assert np.array_equal(enw.T, en) and dp.shape == (W, P + 2) and mom.shape == (P + 4, P + 2)
    for t in range(2):
        assert np.array_equal(dp[:, P + t], 1j * dp[:, tail[t]])
    w = wts / wts.sum()
    A = np.concatenate((dp, enw[:, 5:6], np.ones((W, 1))), axis=1)
    ref = A.T @ ((w * f)[:, None] * dp)
    for name, a, b in (("dpidpj", mom[:-2], ref[:-2]), ("dpH", mom[-2], ref[-2]), ("dppsi", mom[-1], ref[-1]), ("means", mean, w @ enw)):
        err = helpers.relerr(a, b)
        print(name, err)
        assert err < TOL, (name, err)
    assert np.array_equal(mom[:-2], mom[:-2].T)
    # the weight really acts: the unregularised moments differ
    assert helpers.relerr(dev.sr_moments_c(src, pos, tail, 1e-3, weights=wts, seed=77)[1][-1], ref[-1]) > 1e-3
    # the handle's det_coeff is a real-dtype parameter, so no transform built from its parameters has a tail of its own
    assert not np.iscomplexobj(wf.parameters["wf1det_coeff"])


def test_real_handle_through_the_complex_entry():
    mol = systems.water()
    mf = systems.random_mf(mol, nvirt=6)
    wf = helpers.gpu_wf(mol, mf, determinants=systems.random_determinants(mol, mf, 4))
    W = 200
    wf.recompute(OpenConfigs(systems.initial_guess(mol, W, rng=np.random.default_rng(1)).configs.copy()))
    dev = wf.fused_device()
    src, pos = sr_columns(gradient_generator(mol, wf, pwf.default_to_opt(wf)).transform)
    wts = 0.5 + np.random.default_rng(2).random(W)
    mr, momr, enr = dev.sr_moments(src, pos, 1e-3, weights=wts, seed=9, per_walker=True)
    mc, momc, enc = dev.sr_moments_c(src, pos, [], 1e-3, weights=wts, seed=9, per_walker=True)
    for name, a, b in (("moments", momc.real, momr), ("means", mc.real, mr)):
        err = helpers.relerr(a, b)
        print(name, err)
        assert err < TOL, (name, err)
    assert np.all(momc.imag == 0) and np.all(mc.imag == 0) and np.all(enc.imag == 0)
    assert np.array_equal(enc.real, enr)
    # with tail columns of a real handle: i times real columns
    dp = dev.sr_moments_c(src, pos, [0, 2], 1e-3, seed=9, dp_walker=True)[2]
    assert np.all(dp[:, : len(src)].imag == 0) and np.array_equal(dp[:, len(src):], 1j * dp[:, [0, 2]])


def test_repeatability_and_chunks(twisted):
    sup, wf = twisted
    configs = _twisted_walkers(sup, 70, 7)
    wf.recompute(configs)
    dev = wf.fused_device()
    src, pos, tail = sr_columns_c(LinearTransform(wf.parameters, pwf.default_to_opt(wf)))
    a = dev.sr_moments_c(src, pos, tail, 1e-3, seed=3, per_walker=True, dp_walker=True)
    b = dev.sr_moments_c(src, pos, tail, 1e-3, seed=3, per_walker=True, dp_walker=True)
    assert all(np.array_equal(x, y) for x, y in zip(a, b))
    c = dev.sr_moments_c(src, pos, tail, 1e-3, seed=3, per_walker=True, dp_walker=True, walker_chunk=24)  # 24 + 24 + 22 walkers
    assert np.array_equal(a[3], c[3]) and np.array_equal(a[2], c[2]) and np.array_equal(a[0], c[0])
    err = helpers.relerr(c[1], a[1])
    print("chunked moments", err)
    assert err < TOL
    # 16 slices
    configs = _twisted_walkers(sup, 1024, 8)
    wf.recompute(configs)
    sd, sp = _pair(sup, wf)
    _agree(sd.avg(configs, wf), sp.avg(configs, wf))


def test_state_untouched(twisted):
    sup, wf = twisted
    dev = wf.fused_device()
    configs = _twisted_walkers(sup, 128, 9)
    wf.recompute(configs)
    twin = copy.deepcopy(wf)  # (rebuilt from the same walkers: the same state)
    for d in (dev, twin.fused_device()):
        d.vmc_sweeps(0.3, 2, seed=9, energy=False)  # (state after a fused sweep: layouts and stale sums as a driver leaves them)
    src, pos, tail = sr_columns_c(LinearTransform(wf.parameters, pwf.default_to_opt(wf)))
    dev.sr_moments_c(src, pos, tail, 1e-3, seed=21)
    v, tv = wf.value(), twin.value()
    assert np.array_equal(v[0], tv[0]) and np.array_equal(v[1], tv[1])
    assert np.array_equal(dev.configs(), twin.fused_device().configs())
    # a VMC trajectory after the call is the one the untouched twin makes
    r1 = dev.vmc_sweeps(0.3, 2, seed=33)
    r2 = twin.fused_device().vmc_sweeps(0.3, 2, seed=33)
    assert np.array_equal(r1[0], r2[0]) and np.array_equal(r1[1], r2[1])
    assert np.array_equal(dev.configs(), twin.fused_device().configs())


def test_vmc_worker_block(twisted):
    sup, wf = twisted
    start = _twisted_walkers(sup, 64, 10)
    out = {}
    for sr in _pair(sup, wf):
        assert sr.resolve_route(wf) == sr.route
        np.random.seed(11)
        blk, cfg = pa.vmc_worker(wf, copy.deepcopy(start), 0.3, 2, {"pgrad": sr}, seed=5)
        assert sr.last_route == sr.route
        out[sr.route] = (blk, cfg)
    bd, bp = out["device"][0], out["protocol"][0]
    assert sorted(bd) == sorted(bp) and {"pgraddpidpj", "pgradtotal", "acceptance", "move time", "accumulator time"} <= set(bd)
    for k in bp:
        if "time" not in k:
            err = helpers.relerr(bd[k], bp[k])
            print(k, err)
            assert err < TOL, (k, err)
    assert np.array_equal(out["device"][1].configs, out["protocol"][1].configs)
    assert np.array_equal(out["device"][1].wrap, out["protocol"][1].wrap)


def test_scope(twisted):
    sup, wf = twisted
    # the default is today's: protocol, and route="device" raises
    sr = gradient_generator(sup, wf, pwf.default_to_opt(wf))
    assert sr.complex_device is False and sr.resolve_route(wf) == "protocol" and "complex" in sr_route(wf, sr)[1]
    with pytest.raises(NotImplementedError, match="complex"):
        gradient_generator(sup, wf, pwf.default_to_opt(wf), route="device")
    assert gradient_generator(sup, wf, pwf.default_to_opt(wf), complex_device=True).resolve_route(wf) == "device"
    # orbital keys of such a handle stay on the protocol route
    orb = pwf.default_to_opt(wf, optimize_orbitals=True)
    assert gradient_generator(sup, wf, orb, complex_device=True).resolve_route(wf) == "protocol"
    with pytest.raises(NotImplementedError, match="complex"):
        gradient_generator(sup, wf, orb, complex_device=True, route="device")
    # the library refuses what the Python side would not send
    dev = wf.fused_device()
    wf.recompute(_twisted_walkers(sup, 64, 11))
    nb = int(np.size(wf.parameters["wf2bcoeff"]))
    for src, pos, tail in (([2, 2], [3, 4], [2]), ([2, 2], [3, 4], [-1]), ([2, 2], [3, 4], [1, 1]), ([4], [0], []), ([5], [0], []),
                           ([2], [nb], []), ([0], [1], []), ([3], [0], []), ([], [], [])):
        with pytest.raises(pa._ffi.PqaError, match="pqa_sr_moments_c"):
            dev.sr_moments_c(src, pos, tail, 1e-3)
