"""The identity pqa_correlated_md rests on, stated in NumPy on the oracle's objects: the values and kinetic terms of a
multi-determinant Slater x Jastrow wave function at K sets of (det_coeff, acoeff, bcoeff) from per-determinant quantities that do
not depend on the set (omega_d, rho_d) and the Jastrow derivatives of the set, against set -> recompute -> value / kinetic."""

import numpy as np

from oracle import energy as oenergy
from oracle import jastrow_basis
from oracle import wf as owf
from pyqmc_amd import systems
from pyqmc_amd.configs import OpenConfigs
from tests import helpers

BOUND = 1e-12  # relative: both sides are the same fp64 sums reordered


def test_linear_in_det_coeff_and_jastrow_coefficients():
    mol = systems.water()
    mf = systems.random_mf(mol, nvirt=6)
    dets = systems.random_determinants(mol, mf, 5)
    W, K, N = 6, 3, sum(mol.nelec)
    configs = OpenConfigs(systems.initial_guess(mol, W, rng=np.random.default_rng(1)).configs.copy())
    rng = np.random.default_rng(2)
    a0, b0 = helpers.jastrow_params(mol)
    c0 = np.array([c for c, _ in dets])
    sets = [(c0 + 0.05 * rng.standard_normal(c0.shape), a0 + 0.05 * rng.standard_normal(a0.shape), b0 + 0.05 * rng.standard_normal(b0.shape))
            for _ in range(K)]

    # set-independent: one single-determinant Slater per determinant -> (sign, log), rho_d[e] = (grad, lap) ratios
    sign, logd, rho = [], [], []
    for _, occ in dets:
        sl = owf.Slater(mol, mf.mo_coeff, [(1.0, occ)])
        s, l = sl.recompute(configs)
        sign.append(s)
        logd.append(l)
        rows = []
        for e in range(N):
            g, lap = sl.gradient_laplacian(e, configs.electron(e))
            rows.append(np.vstack([g, lap[None]]))
        rho.append(rows)
    sign, logd, rho = np.array(sign), np.array(logd), np.array(rho)  # (D, W), (D, W), (D, N, 4, W)
    ref = logd.max(axis=0)
    omega = sign * np.exp(logd - ref)  # (D, W)

    ab, bb, rcut = jastrow_basis.default_basis(ion_cusp=False)
    worst = 0.0
    for c, a, b in sets:
        # the formulas of the kernel's header
        S = np.einsum("d,dw->w", c, omega)
        G = np.einsum("d,dw,dncw->ncw", c, omega, rho) / S
        ja = owf.JastrowSpin(mol, ab, bb, rcut)
        ja.parameters["acoeff"], ja.parameters["bcoeff"] = a, b
        _, U = ja.recompute(configs)
        logpsi = np.log(np.abs(S)) + ref + U
        ke, grad2 = np.zeros(W), np.zeros(W)
        for e in range(N):
            gU, lJ = ja.gradient_laplacian(e, configs.electron(e))  # lJ = lap U + |grad U|^2
            lapU = lJ - np.sum(gU**2, axis=0)
            lap = G[e, 3] + lapU + np.sum(gU**2, axis=0) + 2 * np.sum(G[e, :3] * gU, axis=0)
            ke += -0.5 * lap
            grad2 += np.sum((G[e, :3] + gU) ** 2, axis=0)
        # set -> recompute -> value / kinetic of the multi-determinant wave function
        full = owf.MultiplyWF(owf.Slater(mol, mf.mo_coeff, [(ck, occ) for ck, (_, occ) in zip(c, dets)]), owf.JastrowSpin(mol, ab, bb, rcut))
        full.wf_factors[1].parameters["acoeff"], full.wf_factors[1].parameters["bcoeff"] = a, b
        _, rl = full.recompute(configs)
        rke, rg2 = oenergy.kinetic(configs, full)
        errs = [helpers.relerr(logpsi, rl), helpers.relerr(ke, rke), helpers.relerr(grad2, rg2)]
        print("relative differences: logpsi, ke, grad2", errs)
        worst = max(worst, *errs)
    assert worst < BOUND, worst
    k0, k1 = (oenergy.kinetic(configs, _full(mol, mf, dets, s, ab, bb, rcut, configs))[0] for s in sets[:2])
    assert np.abs(k0 - k1).max() > 1e-6  # (the sets really differ)


def _full(mol, mf, dets, s, ab, bb, rcut, configs):
    w = owf.MultiplyWF(owf.Slater(mol, mf.mo_coeff, [(ck, occ) for ck, (_, occ) in zip(s[0], dets)]), owf.JastrowSpin(mol, ab, bb, rcut))
    w.wf_factors[1].parameters["acoeff"], w.wf_factors[1].parameters["bcoeff"] = s[1], s[2]
    w.recompute(configs)
    return w
