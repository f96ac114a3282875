"""The closed form of the two-body density matrix's pair ratios (pqa_tbdm.hip), stated in NumPy on the oracle's
wave-function objects and compared with recomputes of the doubly moved configurations.  No GPU: this pins the mathematics.

    R_ab = Psi(r_a -> r1, r_b -> r2) / Psi = S_ab exp(dU_ab)
    S_ab  = v_s1(r1)[a] v_s2(r2)[b]                             (s1 != s2)
          = v(r1)[a] v(r2)[b] - v(r2)[a] v(r1)[b],  S_aa = 0    (s1 == s2)
          per determinant, v_s(q)[i] = sum_k phi^s_occ[k](q) Dinv^s[k][i]; several determinants: sum_D w_D S_ab(D) / sum_D w_D
    dU_ab = A_a(r1) + A_b(r2) + u(r1, r2) + u(r_a, r_b) - u(r1, r_b) - u(r_a, r2),   A_e(q) = U(e -> q) - U
"""

import types

import numpy as np
import pytest

import helpers
from oracle import wf as owf
from pyqmc_amd import systems
from pyqmc_amd.configs import OpenConfigs

W = 6


def closed_form(wf, r1, r2, s1, s2):
    """R (W, nea, neb) from the state ``wf`` holds after ``recompute``; r1, r2 (W, 3)."""
    factors = wf.wf_factors if hasattr(wf, "wf_factors") else [wf]
    sl = next(f for f in factors if isinstance(f, owf.Slater))
    ja = next((f for f in factors if isinstance(f, owf.JastrowSpin)), None)
    nel = sl._nelec
    nea, neb = nel[s1], nel[s2]

    def v(s, q):  # (W, D_s, n_s): single-move ratios of every unique determinant of spin s
        phi = sl._mo(q, s, 1)[1][0]  # (W, nmo)
        return np.einsum("wdj,wdji->wdi", phi[:, sl._det_occup[s]], sl._inverse[s])

    wts = sl._det_weights()  # (W, D)
    da, db = sl._det_map[s1], sl._det_map[s2]
    if s1 != s2:
        S = np.einsum("wd,wda,wdb->wab", wts, v(s1, r1)[:, da], v(s2, r2)[:, db])
    else:
        v1, v2 = v(s1, r1)[:, da], v(s1, r2)[:, da]
        S = np.einsum("wd,wda,wdb->wab", wts, v1, v2) - np.einsum("wd,wda,wdb->wab", wts, v2, v1)
        S[:, np.arange(nea), np.arange(nea)] = 0.0
    S = S / wts.sum(axis=1)[:, None, None]
    if ja is None:
        return S
    ea, eb = np.arange(nea) + s1 * nel[0], np.arange(neb) + s2 * nel[0]
    x = ja._x

    def u(d):  # two-body term of channel (s1, s2) at displacements d (..., 3)
        return ja._b(d, "value") @ ja.parameters["bcoeff"][:, s1 + s2]

    def A(e, q):
        return np.log(ja.testvalue(e, types.SimpleNamespace(configs=q))[0])

    A1 = np.stack([A(e, r1) for e in ea], axis=1)
    A2 = np.stack([A(e, r2) for e in eb], axis=1)
    xa, xb = x[:, ea], x[:, eb]
    dU = (A1[:, :, None] + A2[:, None, :] + u(r1 - r2)[:, None, None] + u(xa[:, :, None, :] - xb[:, None, :, :])
          - u(r1[:, None, :] - xb)[:, None, :] - u(xa - r2[:, None, :])[:, :, None])
    with np.errstate(invalid="ignore"):  # (the diagonal of a same-spin sector: one electron at distance 0 from itself)
        R = S * np.exp(np.where(S == 0.0, 0.0, dU))
    return R


def direct(wf, x, r1, r2, s1, s2, nel):
    """sign exp(dlog) of recomputes with a at r1 and b at r2; 0 where a and b are one electron."""
    s0, l0 = wf.recompute(OpenConfigs(x.copy()))
    out = np.zeros((x.shape[0], nel[s1], nel[s2]))
    for a in range(nel[s1]):
        for b in range(nel[s2]):
            ia, ib = a + s1 * nel[0], b + s2 * nel[0]
            if ia == ib:
                continue
            y = x.copy()
            y[:, ia], y[:, ib] = r1, r2
            s, l = wf.recompute(OpenConfigs(y))
            out[:, a, b] = s / s0 * np.exp(l - l0)
    wf.recompute(OpenConfigs(x.copy()))
    return out


def _case(kind):
    import pyqmc_amd as pa

    mol = systems.water()
    if kind == "twodet":
        mf = systems.random_mf(mol, nvirt=2)
        wf = helpers.oracle_wf(mol, mf, [(1.0, [[0, 1, 2, 3], [0, 1, 2, 3]]), (-0.4, [[0, 1, 2, 4], [0, 1, 3, 5]])])
    else:
        wf = helpers.oracle_wf(mol, systems.random_mf(mol))
        if kind == "slater":
            wf = wf.wf_factors[0]
    rng = np.random.default_rng(3)
    x = pa.initial_guess(mol, W, rng=rng).configs
    r1, r2 = (x[:, 0] + 0.7 * rng.standard_normal((W, 3)) for _ in (0, 1))  # near the molecule, inside the Jastrow cut-off
    return mol, wf, x, r1, r2


@pytest.mark.parametrize("sector", [(0, 1), (0, 0), (1, 0), (1, 1)])
@pytest.mark.parametrize("kind", ["jastrow", "slater", "twodet"])
def test_closed_form_matches_recompute(kind, sector):
    mol, wf, x, r1, r2 = _case(kind)
    ref = direct(wf, x, r1, r2, *sector, mol.nelec)
    R = closed_form(wf, r1, r2, *sector)
    err = float(np.max(np.abs(R - ref) / (1 + np.abs(ref))))
    print(f"tbdm pairs {kind} {sector}: {err:.2e}")
    assert err < 1e-10
    if sector[0] == sector[1]:
        assert np.all(R[:, np.arange(R.shape[1]), np.arange(R.shape[1])] == 0.0)
    assert np.max(np.abs(ref)) > 1e-3  # (the comparison is not one of zeros)
