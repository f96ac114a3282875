"""The identities behind the fused density matrices of three-body wave functions (pqa_obdm_sweeps_j3, pqa_tbdm_sweep_j3,
csrc/pqa_j3dm.hpp), stated in NumPy on the oracle's three-body factor, the entry points' ABI and the argument rules of
three_body_device.  No GPU: this pins the mathematics.

With C symmetrised in (k, l) the pair term is symmetric,

    t(x, s; y, u) = sum_I sum_klm C[I][k][l][m][s + u] a_k(|x - R_I|) a_l(|y - R_I|) b_m(|x - y|)
    U3 = sum_{i<j} t(r_i, s_i; r_j, s_j),   P_e = sum_{j != e} t(r_e, s_e; r_j, s_j)

and with one table per point q and moving spin s, G_s(q)[j] = t(q, s; r_j, s_j), SG_s(q) = sum_j G_s(q)[j]:

    one-body   A3_e(r')  = SG_{s_e}(r') - G_{s_e}(r')[e] - P_e
    two-body   dU3_ab    = SG_{s1}(r1) + SG_{s2}(r2) + t(r1, s1; r2, s2) - G_{s1}(r1)[a] - G_{s1}(r1)[b] - G_{s2}(r2)[a] - G_{s2}(r2)[b]
                           - P_a - P_b + t(r_a, s1; r_b, s2)                      (a != b)

Bound: the project's err = max |a - b| / (1 + |b|) < 1e-10."""

import inspect
import os
import re
import types

import numpy as np
import pytest

import helpers
from oracle import jastrow_basis
from pyqmc_amd import systems
from pyqmc_amd.configs import OpenConfigs

W = 6
DETS2 = [(1.0, [[0, 1, 2, 3], [0, 1, 2, 3]]), (-0.4, [[0, 1, 2, 4], [0, 1, 2, 5]])]


def _err(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return float(np.max(np.abs(a - b) / (1.0 + np.abs(b))))


def _wf(ndet):
    mol = systems.water()
    mf = systems.random_mf(mol, nvirt=6)
    wf = helpers.oracle_wf3(mol, mf, None if ndet == 1 else DETS2)
    x = np.random.default_rng(5).standard_normal((W, sum(mol.nelec), 3)) * 1.1
    wf.recompute(OpenConfigs(x.copy()))
    return mol, wf, x


class Tables:
    """t, G and P of the three-body factor ``j3`` for the walkers ``x`` (W, N, 3)."""

    def __init__(self, j3, x, nup):
        self.j3, self.x, self.nup, self.N = j3, x, nup, x.shape[1]
        self.C = j3._C()  # (A, k, l, m, 3), symmetric in (k, l)
        assert np.array_equal(self.C, self.C.swapaxes(1, 2))

    def a(self, p):
        d = self.j3._mi(p[:, None, :] - self.j3.atoms[None])
        return jastrow_basis.evaluate(self.j3.a_basis, self.j3.rcut, d, np.linalg.norm(d, axis=-1), "value")  # (W, A, k)

    def t(self, p, sp, q, sq):
        d = self.j3._mi(p - q)
        b = jastrow_basis.evaluate(self.j3.b_basis, self.j3.rcut, d, np.linalg.norm(d, axis=-1), "value")  # (W, m)
        return np.einsum("wIk,wIl,wm,Iklm->w", self.a(p), self.a(q), b, self.C[..., sp + sq])

    def spin(self, j):
        return int(j >= self.nup)

    def G(self, q, s):
        return np.stack([self.t(q, s, self.x[:, j], self.spin(j)) for j in range(self.N)], axis=1)  # (W, N)

    def P(self, e):
        return sum(self.t(self.x[:, e], self.spin(e), self.x[:, j], self.spin(j)) for j in range(self.N) if j != e)


@pytest.mark.parametrize("ndet", [1, 2])
def test_one_body_difference(ndet):
    mol, wf, x = _wf(ndet)
    j3 = wf.wf_factors[2]
    tb = Tables(j3, x, mol.nelec[0])
    rng = np.random.default_rng(8)
    worst = 0.0
    for _ in range(3):  # several points, every electron
        q = rng.standard_normal((W, 3)) * 1.2
        G = [tb.G(q, 0), tb.G(q, 1)]
        for e in range(tb.N):
            s = tb.spin(e)
            A3 = G[s].sum(axis=1) - G[s][:, e] - tb.P(e)
            ref = np.log(j3.testvalue(e, types.SimpleNamespace(configs=q))[0])
            assert np.all(np.isfinite(ref)) and np.max(np.abs(ref)) > 1e-6
            worst = max(worst, _err(A3, ref))
    print(f"j3 one-body identity, {ndet} determinant(s): worst {worst:.2e}")
    assert worst < 1e-10


@pytest.mark.parametrize("ndet", [1, 2])
@pytest.mark.parametrize("sector", [(0, 0), (0, 1), (1, 1)], ids=["uu", "ud", "dd"])
def test_two_body_difference(ndet, sector):
    mol, wf, x = _wf(ndet)
    j3 = wf.wf_factors[2]
    nup, ndn = mol.nelec
    tb = Tables(j3, x, nup)
    s1, s2 = sector
    rng = np.random.default_rng(9)
    r1, r2 = rng.standard_normal((W, 3)) * 1.2, rng.standard_normal((W, 3)) * 1.2
    G1, G2, t12 = tb.G(r1, s1), tb.G(r2, s2), tb.t(r1, s1, r2, s2)
    u0 = j3.recompute(OpenConfigs(x.copy()))[1]
    worst, npair = 0.0, 0
    for a in range(s1 * nup, nup + s1 * ndn):
        for b in range(s2 * nup, nup + s2 * ndn):
            if a == b:
                continue
            dU3 = (G1.sum(axis=1) + G2.sum(axis=1) + t12 - G1[:, a] - G1[:, b] - G2[:, a] - G2[:, b] - tb.P(a) - tb.P(b)
                   + tb.t(x[:, a], s1, x[:, b], s2))
            y = x.copy()
            y[:, a], y[:, b] = r1, r2
            ref = j3.recompute(OpenConfigs(y))[1] - u0
            assert np.all(np.isfinite(ref)) and np.max(np.abs(ref)) > 1e-6
            worst, npair = max(worst, _err(dU3, ref)), npair + 1
    j3.recompute(OpenConfigs(x.copy()))
    print(f"j3 two-body identity, {ndet} determinant(s), sector {sector}: {npair} pairs, worst {worst:.2e}")
    nea, neb = (ndn if s1 else nup), (ndn if s2 else nup)
    assert npair == nea * neb - (nea if s1 == s2 else 0)
    assert worst < 1e-10


def test_pair_sum_is_u3():
    """U3 = sum_{i<j} t(i, j) = 1/2 sum_e P_e: the tables describe the factor the oracle evaluates."""
    mol, wf, x = _wf(1)
    j3 = wf.wf_factors[2]
    tb = Tables(j3, x, mol.nelec[0])
    u3 = sum(tb.t(x[:, i], tb.spin(i), x[:, j], tb.spin(j)) for i in range(tb.N) for j in range(i + 1, tb.N))
    assert _err(u3, j3.recompute(OpenConfigs(x.copy()))[1]) < 1e-10
    assert _err(0.5 * sum(tb.P(e) for e in range(tb.N)), u3) < 1e-10


# ---- host logic ----------------------------------------------------------------------------------------------------------------

def _params(header, name):
    decl = re.search(r"int " + name + r"\(([^;]*)\);", header).group(1)
    return [p.strip() for p in decl.replace("\n", " ").split(",")]


@pytest.mark.parametrize("name,sibling", [("pqa_obdm_sweeps_j3", "pqa_obdm_sweeps_c"), ("pqa_tbdm_sweep_j3", "pqa_tbdm_sweep"),
                                          ("pqa_dm_points_resident_j3", "pqa_dm_points_resident")])
def test_abi(name, sibling):
    """The entries are declared with their siblings' parameter lists, prototyped with the same arguments, and exported when the
    library is built."""
    import ctypes as C

    import __graft_entry__ as ge
    from pyqmc_amd import _ffi

    assert name in _ffi._PROTOTYPES and name in _ffi.header_symbols()
    res, args = _ffi._PROTOTYPES[name]
    assert res is C.c_int and args == _ffi._PROTOTYPES[sibling][1]
    header = open(os.path.join(ge.ROOT, "include", "pyqmc_amd.h")).read()
    params = _params(header, name)
    assert params == _params(header, sibling) and len(params) == len(args)
    for p, a in zip(params, args):
        if "*" in p:
            assert a in (_ffi._H, C.c_void_p), p
        elif p.startswith("uint64_t"):
            assert a is C.c_uint64, p
        elif p.startswith("int64_t"):
            assert a is C.c_int64, p
        else:
            assert a is C.c_int, p
    assert "pqa_obdm" in ge.UNITS and "pqa_tbdm" in ge.UNITS and not any("j3dm" in u for u in ge.UNITS)  # (no new translation unit)
    if os.path.exists(ge.LIB):
        assert hasattr(_ffi.lib(), name)


def test_three_body_device_arguments():
    from pyqmc_amd import obdm, tbdm

    mol = systems.water()
    for bad in ("yes", 1, None):
        with pytest.raises(ValueError, match="three_body_device"):
            obdm.OBDMAccumulator(mol, None, three_body_device=bad)
        with pytest.raises(ValueError, match="three_body_device"):
            tbdm.TBDMAccumulator(mol, None, (0, 1), three_body_device=bad)
    # the existing rules come first and are unchanged
    with pytest.raises(ValueError, match="route"):
        obdm.OBDMAccumulator(mol, None, route="device", three_body_device=True)
    with pytest.raises(ValueError, match="fused"):
        obdm.OBDMAccumulator(mol, None, rng="device", route="protocol", three_body_device=True)
    with pytest.raises(ValueError, match="complex_device"):
        obdm.OBDMAccumulator(mol, None, complex_device=1, three_body_device=True)
    with pytest.raises(ValueError, match="route"):
        tbdm.TBDMAccumulator(mol, None, (0, 1), route="device", three_body_device=True)
    assert inspect.signature(obdm.OBDMAccumulator.__init__).parameters["three_body_device"].default is False
    assert inspect.signature(tbdm.TBDMAccumulator.__init__).parameters["three_body_device"].default is False
    assert list(inspect.signature(obdm.device_obdm_sweeps_j3).parameters) == list(inspect.signature(obdm.device_obdm_sweeps_c).parameters)
    assert list(inspect.signature(tbdm.device_tbdm_sweep_j3).parameters) == list(inspect.signature(tbdm.device_tbdm_sweep).parameters)
    assert list(inspect.signature(tbdm.device_pair_ratios_j3).parameters) == list(inspect.signature(tbdm.device_pair_ratios).parameters)


class _Handle:
    """Stand-in for a DeviceWF: the attributes the scope rules read."""

    def __init__(self, j2=True, j3=True, cplx=False, twisted=False):
        self.has_slater, self.has_jastrow, self.has_j3, self.cplx, self.twisted = True, j2, j3, cplx, twisted

    def vmc_sweeps(self, *a, **k):
        raise AssertionError("the scope rules must not evaluate anything")


def _product(dev, kinds):
    from pyqmc_amd import wf as pwf

    factors = []
    for cls in kinds:
        f = object.__new__(getattr(pwf, cls))
        f._dev, f.dtype, f.parameters = dev, float, {}
        factors.append(f)
    return pwf.MultiplyWF(*factors) if len(factors) > 1 else factors[0]


def test_readonly_device_j3():
    from pyqmc_amd.wf import readonly_device, readonly_device_c, readonly_device_j3

    S, J2, J3 = "Slater", "JastrowSpin", "ThreeBodyJastrow"
    dev = _Handle()
    wf = _product(dev, [S, J2, J3])
    assert readonly_device_j3(wf) is dev
    assert readonly_device(wf) is None and readonly_device_c(wf) is None  # (the existing rules keep refusing it)
    d = _Handle(j2=False)
    assert readonly_device_j3(_product(d, [S, J3])) is d  # without the two-body factor
    d = _Handle(j3=False)
    assert readonly_device_j3(_product(d, [S, J2])) is d and readonly_device(_product(d, [S, J2])) is d  # readonly_device's own scope
    d = _Handle(j2=False, j3=False)
    assert readonly_device_j3(_product(d, [S])) is d
    # dev.has_j3 / the two-body flag must match the factor list
    assert readonly_device_j3(_product(_Handle(), [S, J2])) is None
    assert readonly_device_j3(_product(_Handle(j3=False), [S, J2, J3])) is None
    assert readonly_device_j3(_product(_Handle(j2=False), [S, J2, J3])) is None
    assert readonly_device_j3(_product(_Handle(), [S, J3])) is None
    # no Slater factor, a factor twice, complex, twisted
    assert readonly_device_j3(_product(_Handle(), [J2, J3])) is None
    assert readonly_device_j3(_product(_Handle(), [S, J2, J3, J3])) is None
    assert readonly_device_j3(_product(_Handle(cplx=True), [S, J2, J3])) is None
    assert readonly_device_j3(_product(_Handle(twisted=True), [S, J2, J3])) is None
    # factors on different handles
    from pyqmc_amd import wf as pwf

    a, b = _product(_Handle(), [S]), _product(_Handle(), [J3])
    assert readonly_device_j3(pwf.MultiplyWF(a, b)) is None
