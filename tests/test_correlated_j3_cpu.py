"""The identity pqa_correlated_j3 rests on, stated in NumPy on the oracle's objects, its ABI, and the argument and route rules of
three_body_device in pyqmc_amd.linemin.  No GPU.

U3 is linear in C = (c + c^T_kl) / 2, and C enters only through its contraction with the moving electron's a-functions.  With the
C-independent tables of electron e (spin s_e) at r = r_e and the a-triples of r_eI,

    M_c[I][l][m][s'] = sum_{j != e, spin s'} a_l(r_jI) {b_m, grad b_m (x, y, z), lap b_m}(r_e - r_j)        c = 0 .. 4
    t_c[I][k]        = sum_{l m s'} C[I][k][l][m][s_e + s'] M_c[I][l][m][s']
    P_e = sum_{I k} a_k t_0,   grad P_e = sum_{I k} grad a_k t_0 + a_k t_{1..3},
    lap P_e = sum_{I k} lap a_k t_0 + 2 grad a_k . t_{1..3} + a_k t_4,

every set has grad U3 = grad P_e, lap U3 = lap P_e and U3 = 1/2 sum_e P_e(r_e); they join the two-body and determinant parts as in
tests/test_correlated_md_cpu.py."""

import inspect
import os
import re

import numpy as np
import pytest

from oracle import energy as oenergy
from oracle import jastrow_basis
from oracle import wf as owf
from pyqmc_amd import systems
from pyqmc_amd.configs import OpenConfigs
from tests import helpers

BOUND = 1e-12  # relative: both sides are the same fp64 sums reordered (tests/test_correlated_md_cpu.py)
DETS2 = [(1.0, [[0, 1, 2, 3], [0, 1, 2, 3]]), (-0.4, [[0, 1, 2, 4], [0, 1, 2, 5]])]


def _tables(j3, x, e, nup):
    """M (5, W, A, l, m, 2) and the a-triples (a (W, A, k), grad a (W, A, k, 3), lap a (W, A, k)) of electron e at its own position."""
    N = x.shape[1]
    pos = x[:, e]
    de_I = j3._mi(pos[:, None, :] - j3.atoms[None])
    ga, a = jastrow_basis.evaluate(j3.a_basis, j3.rcut, de_I, np.linalg.norm(de_I, axis=-1), "gradient_value")
    _, la = jastrow_basis.evaluate(j3.a_basis, j3.rcut, de_I, np.linalg.norm(de_I, axis=-1), "gradient_laplacian")
    W, A, nb = x.shape[0], len(j3.atoms), len(j3.b_basis)
    M = np.zeros((5, W, A, len(j3.a_basis), nb, 2))
    for j in range(N):
        if j == e:
            continue
        dj_I = j3._mi(x[:, j, None, :] - j3.atoms[None])
        aj = jastrow_basis.evaluate(j3.a_basis, j3.rcut, dj_I, np.linalg.norm(dj_I, axis=-1), "value")  # (W, A, l)
        d = j3._mi(pos - x[:, j])
        r = np.linalg.norm(d, axis=-1)
        gb, b = jastrow_basis.evaluate(j3.b_basis, j3.rcut, d, r, "gradient_value")  # (W, m, 3), (W, m)
        _, lb = jastrow_basis.evaluate(j3.b_basis, j3.rcut, d, r, "gradient_laplacian")
        comps = [b, gb[..., 0], gb[..., 1], gb[..., 2], lb]
        for c in range(5):
            M[c, ..., int(j >= nup)] += np.einsum("wIl,wm->wIlm", aj, comps[c])
    return M, (a, ga, la)


def _p_terms(C, M, trip, edown):
    """P_e (W), grad P_e (3, W), lap P_e (W) of one set's symmetrised C (A, k, l, m, 3)."""
    a, ga, la = trip
    t = np.einsum("Iklms,cwIlms->cwIk", C[..., edown:edown + 2], M)
    P = np.einsum("wIk,wIk->w", a, t[0])
    grad = np.einsum("wIkx,wIk->xw", ga, t[0]) + np.einsum("wIk,xwIk->xw", a, t[1:4])
    lap = np.einsum("wIk,wIk->w", la, t[0]) + 2.0 * np.einsum("wIkx,xwIk->w", ga, t[1:4]) + np.einsum("wIk,wIk->w", a, t[4])
    return P, grad, lap


@pytest.mark.parametrize("ndet", [1, 2])
def test_linear_in_three_body_coefficients(ndet):
    mol = systems.water()
    mf = systems.random_mf(mol, nvirt=6)
    dets = [(1.0, DETS2[0][1])] if ndet == 1 else DETS2
    W, K, N, nup = 6, 3, sum(mol.nelec), mol.nelec[0]
    configs = OpenConfigs(systems.initial_guess(mol, W, rng=np.random.default_rng(1)).configs.copy())
    x = configs.configs
    rng = np.random.default_rng(2)
    a0, b0 = helpers.jastrow_params(mol)
    c30 = helpers.ccoeff_params(mol)
    d0 = np.array([c for c, _ in dets])
    sets = [tuple(v + 0.05 * rng.standard_normal(v.shape) for v in (d0, a0, b0, c30)) for _ in range(K)]
    ab, bb, rcut = jastrow_basis.default_basis(ion_cusp=False)

    # set-independent: per-determinant (sign, log, gradient and laplacian ratios), the three-body tables of every electron
    sign, logd, rho = [], [], []
    for _, occ in dets:
        sl = owf.Slater(mol, mf.mo_coeff, [(1.0, occ)])
        s, l = sl.recompute(configs)
        sign.append(s)
        logd.append(l)
        rho.append([np.vstack([g, lap[None]]) for g, lap in (sl.gradient_laplacian(e, configs.electron(e)) for e in range(N))])
    sign, logd, rho = np.array(sign), np.array(logd), np.array(rho)
    ref = logd.max(axis=0)
    omega = sign * np.exp(logd - ref)
    j3 = owf.ThreeBodyJastrow(mol, ab, bb, rcut)
    tabs = [_tables(j3, x, e, nup) for e in range(N)]

    def full(s):
        w = owf.MultiplyWF(owf.Slater(mol, mf.mo_coeff, [(ck, occ) for ck, (_, occ) in zip(s[0], dets)]), owf.JastrowSpin(mol, ab, bb, rcut),
                           owf.ThreeBodyJastrow(mol, ab, bb, rcut))
        w.wf_factors[1].parameters["acoeff"], w.wf_factors[1].parameters["bcoeff"] = s[1], s[2]
        w.wf_factors[2].parameters["ccoeff"] = s[3]
        return w

    worst, kes = 0.0, []
    for s in sets:
        c, a, b, c3 = s
        C = 0.5 * (c3 + c3.swapaxes(1, 2))
        S = np.einsum("d,dw->w", c, omega)
        G = np.einsum("d,dw,dncw->ncw", c, omega, rho) / S
        ja = owf.JastrowSpin(mol, ab, bb, rcut)
        ja.parameters["acoeff"], ja.parameters["bcoeff"] = a, b
        _, U2 = ja.recompute(configs)
        ke, grad2, U3 = np.zeros(W), np.zeros(W), np.zeros(W)
        for e in range(N):
            P, g3, l3 = _p_terms(C, *tabs[e], int(e >= nup))
            U3 += 0.5 * P
            g2, lJ = ja.gradient_laplacian(e, configs.electron(e))  # lJ = lap U2 + |grad U2|^2
            gU = g2 + g3
            lapU = lJ - np.sum(g2**2, axis=0) + l3
            lap = G[e, 3] + lapU + np.sum(gU**2, axis=0) + 2 * np.sum(G[e, :3] * gU, axis=0)
            ke += -0.5 * lap
            grad2 += np.sum((G[e, :3] + gU) ** 2, axis=0)
        logpsi = np.log(np.abs(S)) + ref + U2 + U3
        w = full(s)
        _, rl = w.recompute(configs)
        rke, rg2 = oenergy.kinetic(configs, w)
        kes.append(rke)
        errs = [helpers.relerr(logpsi, rl), helpers.relerr(ke, rke), helpers.relerr(grad2, rg2)]
        print("relative differences: logpsi, ke, grad2", errs)
        worst = max(worst, *errs)
    assert worst < BOUND, worst
    assert np.abs(kes[0] - kes[1]).max() > 1e-6  # (the sets really differ)
    # ... and the three-body coefficients alone move the energy
    only_c = full((sets[0][0], sets[0][1], sets[0][2], sets[1][3]))
    only_c.recompute(configs)
    assert np.abs(oenergy.kinetic(configs, only_c)[0] - kes[0]).max() > 1e-6


# ---- ABI -----------------------------------------------------------------------------------------------------------------------

def _params(header, name):
    decl = re.search(r"int " + name + r"\(([^;]*)\);", header).group(1)
    return [p.strip() for p in decl.replace("\n", " ").split(",")]


def test_abi():
    """pqa_correlated_j3 is declared with pqa_correlated_md's parameter list plus ccoeff after bcoeff, prototyped with matching
    ctypes kinds, lives in the existing unit and is exported when the library is built."""
    import ctypes as C

    import __graft_entry__ as ge
    from pyqmc_amd import _ffi

    name, sibling = "pqa_correlated_j3", "pqa_correlated_md"
    assert name in _ffi._PROTOTYPES and name in _ffi.header_symbols()
    res, args = _ffi._PROTOTYPES[name]
    sargs = _ffi._PROTOTYPES[sibling][1]
    header = open(os.path.join(ge.ROOT, "include", "pyqmc_amd.h")).read()
    params, sparams = _params(header, name), _params(header, sibling)
    at = sparams.index("const double* bcoeff") + 1
    assert params == sparams[:at] + ["const double* ccoeff"] + sparams[at:]
    assert res is C.c_int and args == sargs[:at] + [C.c_void_p] + sargs[at:] and len(params) == len(args)
    for p, a in zip(params, args):
        if "*" in p:
            assert a in (_ffi._H, C.c_void_p), p
        elif p.startswith("uint64_t"):
            assert a is C.c_uint64, p
        elif p.startswith("long"):
            assert a is C.c_long, p
        elif p.startswith("double"):
            assert a is C.c_double, p
        else:
            assert a is C.c_int, p
    assert "pqa_correlated" in ge.UNITS and not any("j3" in u for u in ge.UNITS)  # (no new translation unit)
    if os.path.exists(ge.LIB):
        assert hasattr(_ffi.lib(), name)


# ---- argument and route rules ----------------------------------------------------------------------------------------------------

FIVE = ("correlated_route", "correlated_compute_worker", "correlated_compute", "correlated_sampling_minimum", "line_minimization")


class _Handle:
    """Stand-in for a DeviceWF: the attributes the scope rules read."""

    def __init__(self, j3=True, cplx=False, twisted=False, ndet=1):
        self.has_slater, self.has_jastrow, self.has_j3, self.cplx, self.twisted, self.ndet = True, True, j3, cplx, twisted, ndet

    def correlated_j3(self, *a, **k):
        raise AssertionError("the route rules must not evaluate anything")

    correlated_md = correlated = vmc_sweeps = correlated_j3


def _product(dev, kinds):
    from pyqmc_amd import wf as pwf

    factors = []
    for cls in kinds:
        f = object.__new__(getattr(pwf, cls))
        f._dev, f.dtype, f.parameters = dev, float, {}
        factors.append(f)
    return pwf.MultiplyWF(*factors)


class _Transform:
    def __init__(self, keys):
        self.to_opt = {k: np.ones(2, dtype=bool) for k in keys}


class _PGrad:
    def __init__(self, keys, enacc=None):
        from pyqmc_amd.energy import EnergyAccumulator

        self.transform = _Transform(keys)
        self.enacc = EnergyAccumulator(systems.water()) if enacc is None else enacc


S3 = ["Slater", "JastrowSpin", "ThreeBodyJastrow"]
KEYS3 = ("wf1det_coeff", "wf2acoeff", "wf2bcoeff", "wf3ccoeff")


def test_three_body_device_arguments():
    from pyqmc_amd import linemin

    for name in FIVE:
        assert inspect.signature(getattr(linemin, name)).parameters["three_body_device"].default is False, name
    wf, pg = _product(_Handle(), S3), _PGrad(KEYS3)
    for bad in ("yes", 1, None):
        with pytest.raises(ValueError, match="three_body_device"):
            linemin.correlated_route(wf, pg, three_body_device=bad)
        with pytest.raises(ValueError, match="three_body_device"):
            linemin.correlated_compute_worker(wf, None, [], pg, [0, 1], three_body_device=bad)
        with pytest.raises(ValueError, match="three_body_device"):
            linemin.correlated_compute(wf, None, [], pg, three_body_device=bad)
        with pytest.raises(ValueError, match="three_body_device"):
            linemin.correlated_sampling_minimum(0.2, 5, 3.0, [0, 1], pg, wf, {}, np.zeros(2), None, None, None, three_body_device=bad)
        with pytest.raises(ValueError, match="three_body_device"):
            linemin.line_minimization(wf, None, pg, three_body_device=bad)
    with pytest.raises(ValueError, match="evaluation route"):  # the existing rule is unchanged
        linemin.correlated_route(wf, pg, "device", three_body_device=True)


def test_linear_j3_device():
    from pyqmc_amd import wf as pwf

    assert pwf.LINEAR_J3_KEYS == pwf.LINEAR_DET_KEYS | {"wf3ccoeff"}
    dev = _Handle()
    wf = _product(dev, S3)
    assert pwf.linear_j3_device(wf, KEYS3) is dev and pwf.linear_j3_device(wf, ()) is dev
    assert pwf.linear_j3_device(_product(_Handle(ndet=4), S3), KEYS3) is not None
    for bad, kinds, keys, text in ((_Handle(), S3[:2], KEYS3, "ThreeBodyJastrow"), (_Handle(), [S3[0], S3[2], S3[1]], KEYS3, "ThreeBodyJastrow"),
                                   (_Handle(cplx=True), S3, KEYS3, "complex"), (_Handle(twisted=True), S3, KEYS3, "twisted"),
                                   (_Handle(j3=False), S3, KEYS3, "three-body"), (_Handle(), S3, KEYS3 + ("wf1mo_coeff_alpha",), "wf1mo_coeff_alpha")):
        why = []
        assert pwf.linear_j3_device(_product(bad, kinds), keys, why) is None
        assert len(why) == 1 and text in why[0], why
    a, b = _product(_Handle(), S3[:2]), _product(_Handle(), S3[2:])
    assert pwf.linear_j3_device(pwf.MultiplyWF(*a.wf_factors, *b.wf_factors), KEYS3) is None  # factors on different handles


def test_routes():
    from pyqmc_amd import linemin
    from pyqmc_amd.energy import EnergyAccumulator

    pg = _PGrad(KEYS3)
    for ndet in (1, 4):
        wf3 = _product(_Handle(ndet=ndet), S3)
        # the flag off: unchanged
        assert linemin.correlated_route(wf3, pg) == "protocol" and linemin.correlated_route(wf3, pg, three_body_device=False) == "protocol"
        with pytest.raises(NotImplementedError, match="evaluation_route='protocol'"):
            linemin.correlated_route(wf3, pg, "fused")
        # the flag on
        assert linemin.correlated_route(wf3, pg, three_body_device=True) == "fused"
        assert linemin.correlated_route(wf3, pg, "fused", three_body_device=True) == "fused"
        assert linemin.correlated_route(wf3, pg, "protocol", three_body_device=True) == "protocol"
    # out of scope with the flag on: protocol by default, the reason on request
    mol = systems.water()
    cases = ((_product(_Handle(twisted=True), S3), pg, "twisted"), (_product(_Handle(cplx=True), S3), pg, "complex"),
             (_product(_Handle(), S3), _PGrad(KEYS3 + ("wf1mo_coeff_alpha",)), "wf1mo_coeff_alpha"),
             (_product(_Handle(), S3), _PGrad(KEYS3, EnergyAccumulator(mol, use_old_ecp=False)), "use_old_ecp"))
    for wf, p, text in cases:
        assert linemin.correlated_route(wf, p, three_body_device=True) == "protocol"
        with pytest.raises(NotImplementedError, match=text) as ei:
            linemin.correlated_route(wf, p, "fused", three_body_device=True)
        assert "evaluation_route='protocol'" in str(ei.value)
    # without a three-body factor the flag changes nothing
    pg2 = _PGrad(KEYS3[1:3])
    pgd = _PGrad(KEYS3[:3])
    for flag in (False, True):
        w1, w4, wt = _product(_Handle(j3=False), S3[:2]), _product(_Handle(j3=False, ndet=4), S3[:2]), _product(_Handle(j3=False, twisted=True), S3[:2])
        assert linemin.correlated_route(w1, pg2, three_body_device=flag) == "fused"
        assert linemin.correlated_route(w1, pgd, three_body_device=flag) == "protocol"
        assert linemin.correlated_route(w4, pgd, three_body_device=flag) == "protocol"
        assert linemin.correlated_route(w4, pgd, "fused", three_body_device=flag) == "fused"
        with pytest.raises(NotImplementedError, match="twisted"):
            linemin.correlated_route(wt, pgd, "fused", three_body_device=flag)
