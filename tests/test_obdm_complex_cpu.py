"""The identities behind the fused one-body density matrix of complex and twisted handles (pqa_obdm_sweeps_c, csrc/pqa_obdm.hip),
stated in NumPy on the oracle's objects, the entry point's ABI and the argument rules of complex_device.  No GPU: this pins the
mathematics.

For configuration w and sweep s, r' the auxiliary walker assign[s][w] of kept sample s, e over the listed electrons:

    b[w][j]   = phi_j(r') / F,   F = sum_i |phi_i(r')|^2 / norb                      (complex, F real)
    R[w][e]   = (sum_D w_D v_D(r')[e] / sum_D w_D) exp(A_e(r'))                       (complex; A_e real)
    w_D       = c_D phase_up,D phase_dn,D exp(log_up,D + log_dn,D - ref)              (complex)
    v_D(q)[e] = sum_k phi^s_occ[k](q) Dinv^s_D[k][e]
    t[w][k]   = conj(sum_e R[w][e] phi_k(r_e))
    value[w] += b[w] (x) t[w],   norm[w][j] += |phi_j(r')|^2 / F
    mean over walkers: B^T T / W,   Re = Br^T Tr - Bi^T Ti,   Im = Br^T Ti + Bi^T Tr

Everything is stated in TRUE (unfolded) coordinates, which is what a twisted device handle keeps: the oracle's periodic orbitals fold a
point themselves and derive the wrap phase from the fold, and the Jastrow factor takes minimal images."""

import re
import types

import numpy as np
import pytest

import helpers
from oracle import dm as odm
from oracle import jastrow_basis
from oracle import wf as owf
from oracle.pbc import PeriodicOrbitals
from pyqmc_amd import pbc
from pyqmc_amd.configs import OpenConfigs
from test_obdm_fused_cpu import _err, closed_form

W, NSWEEPS, WARMUP, TSTEP = 5, 2, 3, 0.4


class _OpenView:
    """A cell without its lattice attribute ``a``: seeds open containers, so the oracle's auxiliary walk stays in true coordinates."""

    def __init__(self, cell):
        object.__setattr__(self, "_cell", cell)

    def __getattr__(self, name):
        if name == "a":
            raise AttributeError(name)
        return getattr(object.__getattribute__(self, "_cell"), name)


class OraclePeriodicOrbitals:
    """mos(points) from the oracle's periodic orbital evaluator at true positions: the CPU stand-in for obdm.OrbitalEvaluator(kpts=)."""

    def __init__(self, sup, kpts, blocks, Ls):
        self._orb = PeriodicOrbitals(sup, kpts, [blocks, blocks], Ls)
        self.mol, self.norb, self.mo_dtype = _OpenView(sup), sum(b.shape[1] for b in blocks), complex

    def nmo(self):
        return [self.norb, self.norb]

    def mos(self, points, spin=0):
        return self._orb.mos(self._orb.aos(np.asarray(points, dtype=float).reshape(-1, 3), 1), spin)[0]


def _case(kind):
    """(supercell, k-point mean field, oracle Slater x Jastrow, lattice sums) of the twisted primitive cell / the complex 3 x 1 x 1
    cell with the three determinants of test_gpu_sr_complex.py::bloch."""
    if kind == "twisted":
        sup, kmf = helpers.twist_case("prim")
        Ls = pbc.lattice_points_within(sup.original_cell.lattice_vectors(), 30.0)
        return sup, kmf, helpers.oracle_pbc_wf("prim", Ls=Ls, case=(sup, kmf))[1], Ls
    sup = helpers.pbc_complex_case()[0]
    kmf = pbc.random_kmf(sup, complex_coeff=True, nvirt=1)
    base = [5 * k + i for k in range(3) for i in range(4)]
    ex1, ex2 = sorted(set(base) - {3} | {4}), sorted(set(base) - {13} | {14})
    dets = [(1.0, [base, base]), (0.3, [ex2, base]), (-0.2, [ex1, ex2])]
    Ls = pbc.lattice_points_within(sup.original_cell.lattice_vectors(), 30.0)
    sl = owf.Slater.periodic(sup, kmf.kpts, kmf.mo_coeff, Ls, determinants=dets)
    rcut = float(np.amin(np.pi / np.linalg.norm(sup.reciprocal_vectors(), axis=1)))
    ab, bb, rcut = jastrow_basis.default_basis(ion_cusp=False, rcut=rcut)
    ja = owf.JastrowSpin(sup, ab, bb, rcut)
    ja.parameters["acoeff"], ja.parameters["bcoeff"] = helpers.pbc_jastrow_coeffs(sup)
    return sup, kmf, owf.MultiplyWF(sl, ja), Ls


def _true_walkers(sup, n, seed):
    """Walkers partly outside the cell, in true coordinates."""
    return (np.random.default_rng(seed).random((n, sum(sup.nelec), 3)) * 2.4 - 0.7) @ sup.lattice_vectors()


CASES = [("twisted", dict(spin=0)), ("twisted", dict(electrons=np.array([5, 1, 6]), naux=7)), ("bloch", dict(spin=1)),
         ("bloch", dict(electrons=np.array([13, 1, 22, 6]), naux=7))]


@pytest.mark.parametrize("kind,kw", CASES, ids=[f"{k}-{'-'.join(sorted(d))}" for k, d in CASES])
def test_identity(kind, kw):
    sup, kmf, wf, Ls = _case(kind)
    assert wf.wf_factors[0].dtype is complex
    ev = OraclePeriodicOrbitals(sup, kmf.kpts, [np.asarray(kmf.mo_coeff[0][k])[:, :2] for k in range(len(kmf.kpts))], Ls)
    norb = ev.norb
    x = _true_walkers(sup, W, 3)
    configs = OpenConfigs(x.copy())
    wf.recompute(OpenConfigs(x.copy()))
    acc = odm.OBDM(ev.mol, ev, nsweeps=NSWEEPS, tstep=TSTEP, warmup=WARMUP, **kw)
    np.random.seed(11)
    ref = acc(configs, wf)
    assert ref["value"].dtype == complex and ref["norm"].dtype == float
    # the same draws again, by hand: seeding, warm-up, assignment, walk (oracle/dm.py: OBDM.__call__)
    es = acc._electrons
    np.random.seed(11)
    aux = odm.seed_walkers(ev.mol, kw.get("naux", W), len(es))
    aux = odm.density_walk(aux, ev, 0, WARMUP, TSTEP)[1][-1]
    naux = aux.configs.shape[0]
    pick = np.random.randint(0, naux, size=(NSWEEPS, W))
    _, snaps, vals = odm.density_walk(aux, ev, 0, NSWEEPS, TSTEP)
    at_e = ev.mos(x[:, es].reshape(-1, 3), 0).reshape(W, len(es), norb)
    value, norm, mean = np.zeros((W, norb, norb), dtype=complex), np.zeros((W, norb)), np.zeros((norb, norb), dtype=complex)
    worst, planar = 0.0, 0.0
    for s in range(NSWEEPS):
        q = snaps[s].configs[pick[s], 0]
        direct = wf.testvalue_many(es, types.SimpleNamespace(configs=q))
        assert np.all(np.isfinite(direct)) and np.max(np.abs(direct)) > 1e-6 and np.max(np.abs(direct.imag)) > 1e-6
        R = closed_form(wf, es, q)
        worst = max(worst, _err(R, direct))
        if s == 0:  # and against recomputes of the moved configurations
            rec = recomputed_c(wf, x, es, q)
            assert _err(R, rec) < 1e-10, _err(R, rec)
        phi = vals[s][pick[s]]
        F = np.sum(np.abs(phi) ** 2, axis=1, keepdims=True) / norb
        B, T = phi / F, np.conj(np.einsum("we,wej->wj", R, at_e))
        value += B[:, :, None] * T[:, None, :]
        norm += np.abs(phi) ** 2 / F
        full = B.T @ T / W  # (no conjugation of B: a plain transpose)
        four = (B.real.T @ T.real - B.imag.T @ T.imag) + 1j * (B.real.T @ T.imag + B.imag.T @ T.real)
        planar = max(planar, _err(four / W, full))
        mean += full
    print(f"obdm complex identity {kind} {sorted(kw)}: closed-form ratio against testvalue_many {worst:.2e}, planar product {planar:.2e}")
    assert worst < 1e-10 and planar < 1e-12
    assert _err(value / NSWEEPS, ref["value"]) < 1e-10 and _err(norm / NSWEEPS, ref["norm"]) < 1e-10
    assert _err(mean / NSWEEPS, ref["value"].mean(axis=0)) < 1e-10
    assert np.max(np.abs(ref["value"].imag)) > 1e-3  # (the comparison is not one of zeros, nor of real numbers)


def recomputed_c(wf, x, es, q):
    """phase exp(dlog) of recomputes with electron e at q, for every listed electron (complex phases)."""
    s0, l0 = wf.recompute(OpenConfigs(x.copy()))
    out = np.zeros((x.shape[0], len(es)), dtype=complex)
    for t, e in enumerate(es):
        y = x.copy()
        y[:, e] = q
        s, l = wf.recompute(OpenConfigs(y))
        out[:, t] = s / s0 * np.exp(l - l0)
    wf.recompute(OpenConfigs(x.copy()))
    return out


def test_abi():
    """The entry point is declared and prototyped with the same arguments, and exported when the library is built."""
    import os

    import __graft_entry__ as ge
    from pyqmc_amd import _ffi

    name = "pqa_obdm_sweeps_c"
    assert name in _ffi._PROTOTYPES and name in _ffi.header_symbols()
    res, args = _ffi._PROTOTYPES[name]
    # wf, ev, slot, es, ne, nsweeps, assign, seed, mean, first, walker_chunk, weights, ratio, assign_out, value_mean, norm_mean
    assert len(args) == 16 and len(_ffi._PROTOTYPES["pqa_obdm_sweeps"][1]) == 15
    header = open(os.path.join(ge.ROOT, "include", "pyqmc_amd.h")).read()
    decl = re.search(r"int pqa_obdm_sweeps_c\(([^;]*)\);", header).group(1)
    params = [p.strip() for p in decl.replace("\n", " ").split(",")]
    assert len(params) == len(args)
    names = [p.split()[-1].lstrip("*") for p in params]
    assert names == ["wf", "ev", "slot", "es", "ne", "nsweeps", "assign", "seed", "mean", "first", "walker_chunk", "weights", "ratio",
                     "assign_out", "value_mean", "norm_mean"]
    import ctypes as C

    for p, a in zip(params, args):
        if "*" in p:
            assert a in (_ffi._H, C.c_void_p), p
        elif p.startswith("uint64_t"):
            assert a is C.c_uint64, p
        elif p.startswith("int64_t"):
            assert a is C.c_int64, p
        else:
            assert a is C.c_int, p
    assert "pqa_obdm" in ge.UNITS
    if os.path.exists(ge.LIB):
        assert hasattr(_ffi.lib(), name)


def test_complex_device_arguments():
    from pyqmc_amd import obdm, systems
    from pyqmc_amd import wf as pwf

    mol = systems.water()
    with pytest.raises(ValueError, match="complex_device"):
        obdm.OBDMAccumulator(mol, None, complex_device="yes")
    with pytest.raises(ValueError, match="complex_device"):
        obdm.OBDMAccumulator(mol, None, complex_device=1)
    # the existing rules come first and are unchanged
    with pytest.raises(ValueError, match="route"):
        obdm.OBDMAccumulator(mol, None, route="device", complex_device=True)
    with pytest.raises(ValueError, match="fused"):
        obdm.OBDMAccumulator(mol, None, rng="device", route="protocol", complex_device=True)
    assert callable(pwf.readonly_device_c) and callable(obdm.device_obdm_sweeps_c)
    import inspect

    sig = inspect.signature(obdm.device_obdm_sweeps_c)
    assert list(sig.parameters) == ["dev", "ev", "electrons", "nsweeps", "assign", "seed", "mean", "first", "walker_chunk", "with_ratios", "weights"]
    assert inspect.signature(obdm.OBDMAccumulator.__init__).parameters["complex_device"].default is False
