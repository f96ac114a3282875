"""The identity behind the fused one-body density matrix (pqa_obdm_sweeps, csrc/pqa_obdm.hip), stated in NumPy on
the oracle's objects, and the entry point's ABI.  No GPU: this pins the mathematics.

For configuration w and sweep s, r' the auxiliary walker assign[s][w] of kept sample s, F = f(r') / norb, e over the listed electrons:

    b[w][i]   = phi_i(r') / F
    R[w][e]   = Psi(r_e -> r') / Psi = (sum_D w_D v_D(r')[e] / sum_D w_D) exp(A_e(r'))
    v_D(q)[e] = sum_k phi^s_occ[k](q) Dinv^s_D[k][e],   A_e(q) = U(e -> q) - U
    t[w][j]   = sum_e R[w][e] phi_j(r_e)
    value[w] += b[w] (x) t[w],   norm[w][i] += phi_i(r')^2 / F,   mean over walkers: B^T T / W
"""

import types

import numpy as np
import pytest

import helpers
from oracle import dm as odm
from oracle import wf as owf
from pyqmc_amd import systems
from pyqmc_amd.configs import OpenConfigs
from test_obdm_cpu import OracleOrbitals

W, NORB, NSWEEPS, WARMUP, TSTEP = 6, 5, 3, 4, 0.4
CASES = [("jastrow", dict(spin=0)), ("jastrow", dict(electrons=np.array([5, 1, 6]), naux=10)), ("slater", dict()), ("slater", dict(spin=1)),
         ("twodet", dict()), ("twodet", dict(electrons=np.array([5, 1, 6]), naux=10))]


def closed_form(wf, es, q):
    """R (W, ne) = Psi(r_e -> q_w) / Psi for the listed electrons from the state ``wf`` holds after ``recompute``; q (W, 3)."""
    factors = wf.wf_factors if hasattr(wf, "wf_factors") else [wf]
    sl = next(f for f in factors if isinstance(f, owf.Slater))
    ja = next((f for f in factors if isinstance(f, owf.JastrowSpin)), None)
    nup = sl._nelec[0]
    wts = sl._det_weights()  # (W, D)
    v = []
    for s in (0, 1):  # (W, D, n_s): single-move ratios of the determinants, each spin's unique ones spread over the expansion
        phi = sl._mo(q, s, 1)[1][0]
        v.append(np.einsum("wdj,wdji->wdi", phi[:, sl._det_occup[s]], sl._inverse[s])[:, sl._det_map[s]])
    R = np.stack([np.einsum("wd,wd->w", wts, v[int(e >= nup)][:, :, e - nup * int(e >= nup)]) for e in es], axis=1) / wts.sum(axis=1)[:, None]
    if ja is not None:
        R = R * np.stack([ja.testvalue(e, types.SimpleNamespace(configs=q))[0] for e in es], axis=1)  # exp(A_e(q))
    return R


def _wf(kind, mol):
    if kind == "twodet":
        mf = systems.random_mf(mol, nvirt=2)
        return mf, helpers.oracle_wf(mol, mf, [(1.0, [[0, 1, 2, 3], [0, 1, 2, 3]]), (-0.4, [[0, 1, 2, 4], [0, 1, 3, 5]])])
    mf = systems.random_mf(mol)
    wf = helpers.oracle_wf(mol, mf)
    return mf, (wf.wf_factors[0] if kind == "slater" else wf)


def recomputed(wf, x, es, q):
    """sign exp(dlog) of recomputes with electron e at q, for every listed electron: the ratios from nothing but ``recompute``."""
    s0, l0 = wf.recompute(OpenConfigs(x.copy()))
    out = np.zeros((x.shape[0], len(es)))
    for t, e in enumerate(es):
        y = x.copy()
        y[:, e] = q
        s, l = wf.recompute(OpenConfigs(y))
        out[:, t] = s / s0 * np.exp(l - l0)
    wf.recompute(OpenConfigs(x.copy()))
    return out


def _err(a, b):
    return float(np.max(np.abs(a - b) / (1 + np.abs(b))))


@pytest.mark.parametrize("kind,kw", CASES, ids=[f"{k}-{'-'.join(sorted(d)) or 'all'}" for k, d in CASES])
def test_identity(kind, kw):
    import pyqmc_amd as pa

    mol = systems.water()
    mf, wf = _wf(kind, mol)
    nao = np.asarray(mf.mo_coeff[0]).shape[0]
    ev = OracleOrbitals(mol, 0.4 * np.random.default_rng(2).standard_normal((nao, NORB)))  # (the estimator's basis: any orbitals)
    configs = pa.initial_guess(mol, W, rng=np.random.default_rng(3))
    wf.recompute(OpenConfigs(configs.configs.copy()))
    acc = odm.OBDM(mol, ev, nsweeps=NSWEEPS, tstep=TSTEP, warmup=WARMUP, **kw)
    np.random.seed(11)
    ref = acc(configs, wf)
    # the same draws again, by hand: seeding, warm-up, assignment, walk (oracle/dm.py: OBDM.__call__)
    es = acc._electrons
    np.random.seed(11)
    aux = odm.seed_walkers(mol, kw.get("naux", W), len(es))
    aux = odm.density_walk(aux, ev, 0, WARMUP, TSTEP)[1][-1]
    naux = aux.configs.shape[0]
    pick = np.random.randint(0, naux, size=(NSWEEPS, W))
    _, snaps, vals = odm.density_walk(aux, ev, 0, NSWEEPS, TSTEP)
    at_e = ev.mos(configs.configs[:, es].reshape(-1, 3), 0).reshape(W, len(es), NORB)
    value, norm, mean = np.zeros((W, NORB, NORB)), np.zeros((W, NORB)), np.zeros((NORB, NORB))
    worst = 0.0
    for s in range(NSWEEPS):
        q = snaps[s].configs[pick[s], 0]
        direct = wf.testvalue_many(es, types.SimpleNamespace(configs=q))
        assert np.all(np.isfinite(direct))
        R = closed_form(wf, es, q)
        worst = max(worst, _err(R, direct))
        if s == 0:  # and against recomputes of the moved configurations (bound of test_tbdm_pairs_cpu.py)
            assert _err(R, recomputed(wf, configs.configs, es, q)) < 1e-10
        phi = vals[s][pick[s]]
        F = np.sum(phi**2, axis=1, keepdims=True) / NORB
        B, T = phi / F, np.einsum("we,wej->wj", R, at_e)
        value += B[:, :, None] * T[:, None, :]
        norm += phi**2 / F
        mean += B.T @ T / W
    print(f"obdm identity {kind} {sorted(kw)}: closed-form ratio against testvalue_many {worst:.2e}")
    assert worst < 1e-12
    assert _err(value / NSWEEPS, ref["value"]) < 1e-12 and _err(norm / NSWEEPS, ref["norm"]) < 1e-12
    assert _err(mean / NSWEEPS, ref["value"].mean(axis=0)) < 1e-12
    assert np.max(np.abs(ref["value"])) > 1e-3  # (the comparison is not one of zeros)


def test_abi():
    """The entry point is declared, prototyped, built and exported."""
    import __graft_entry__ as ge
    from pyqmc_amd import _ffi

    for name in ("pqa_obdm_sweeps", "pqa_obdm_bytes"):
        assert name in _ffi._PROTOTYPES and name in _ffi.header_symbols()
        assert hasattr(_ffi.lib(), name)
    res, args = _ffi._PROTOTYPES["pqa_obdm_sweeps"]
    assert len(args) == 15  # wf, ev, slot, es, ne, nsweeps, assign, seed, mean, first, walker_chunk, ratio, assign_out, value_mean, norm_mean
    assert "pqa_obdm" in ge.UNITS


def test_route_arguments():
    from pyqmc_amd import obdm

    mol = systems.water()
    with pytest.raises(ValueError, match="route"):
        obdm.OBDMAccumulator(mol, None, route="device")
    with pytest.raises(ValueError, match="rng"):
        obdm.OBDMAccumulator(mol, None, rng="philox")
    with pytest.raises(ValueError, match="fused"):
        obdm.OBDMAccumulator(mol, None, rng="device", route="protocol")
