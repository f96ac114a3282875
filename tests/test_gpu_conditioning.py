"""The fused sweeps on ill-conditioned determinants and long chains without a recompute.

Every other wave function of the suite has orthonormal random orbitals (cond(D) ~ 10 .. 1e3) and no chain longer than 15 sweeps.  Here
two occupied orbitals of each spin are parallel up to eps (tests/conditioning.py: cond(D) 1e6 .. 1e8 on every walker), chains run up to
100 sweeps, and forced acceptances put walkers next to nodes.  Judged: the state each single-determinant sweep carries (inverse, log|Psi|,
the value sum q_e that k_sweep_r8's drift and the quad-cooperative k_kinetic_lw take as 1), the energies formed from it, and the
independence of walkers that share a block.  The yardstick is always the ORACLE's own error on the same chain (computed here, or read
from the fixture g50 for the cluster), never anything the device produced; test_conditioning_cpu.py pins the inputs and the margin 8.

Measured on an MI355X (every figure is printed, and written to $PQA_TEST_REPORT_DIR/parity_report_conditioning.json where that is set;
DESIGN.md section 33 has the table): largest
device / oracle ratio 5.3 through k_sweep_r8, 4.7 through k_sweep_res, 7.6 through the launch-per-move sweep, 3.1 in the DMC chains.

(e) - (g) and the last two cases of (d): the same for periodic cells (real, complex, twisted: launch-per-move sweep, wave-per-walker
launches, k_sweep_res<PBC> and <PBC, CX> on the cells that sweep takes), for multi-determinant handles with two- and three-body Jastrow
factors (k_sweep_ww and the k_propose / k_accept launches; every unique determinant's inverse is judged) and for periodic DMC chains on
host tapes (launch-per-move sweep and k_sweep_res<DMC, PBC>); their oracle side is the fixture g51 or runs live.  Largest device / oracle ratio: 4.5 through k_sweep_res<PBC[, CX]>, 6.3
through the periodic launch-per-move sweep, 4.5 through the wave-per-walker launches, 6.3 through k_sweep_ww, 3.9 through k_propose /
k_accept, 4.4 in the periodic DMC chains (2.5 through k_sweep_res<DMC, PBC>).  Which sweep ran is asserted from the profiler's bracket
counts (_sweep_launches) or, for the resident sweeps, the route every handle reports under PQA_RES_DEBUG (conditioning.reported_routes).
"""

import json
import os

import numpy as np
import pytest

import conditioning as cond
import helpers
from pyqmc_amd.configs import OpenConfigs

pytestmark = pytest.mark.gpu

MARGIN = 8.0  # device error <= 8 x the oracle's own (test_conditioning_cpu.py::test_summation_order_spread)
NQ = 4  # walkers of the 16 384 that the oracle replays in (c)
PATHS = cond.PATHS
_report = {}


def note(key, value):
    _report[key] = float(value)
    print(f"[conditioning] {key} = {float(value):.4g}")
    return value


@pytest.fixture(scope="module", autouse=True)
def _write_report():
    yield
    out = os.environ.get("PQA_TEST_REPORT_DIR")
    if out:
        os.makedirs(out, exist_ok=True)
        with open(os.path.join(out, "parity_report_conditioning.json"), "w") as f:
            json.dump(_report, f, indent=1, sort_keys=True)


def _handle(mol, mf, path, monkeypatch, capfd=None):
    for k, v in PATHS[path].items():
        monkeypatch.setenv(k, v)  # read when the handle is created
    if capfd is not None:
        monkeypatch.setenv("PQA_RES_DEBUG", "1")
    wf = cond.gpu_wf(mol, mf)
    return wf, wf.fused_device()


def _assert_only_route(capfd, setup_tag, kernel):
    """PQA_RES_DEBUG makes a resident sweep's setup report its plan once it has accepted the system (``setup_tag``), and every handle
    report the kernel a sweep runs whenever it is not the one its last sweep ran: ``kernel`` was reported and no other."""
    out, err = capfd.readouterr()
    print(out, end="")
    assert setup_tag in err
    routes = cond.reported_routes(err)
    assert routes and set(routes) == {kernel}, routes


def _assert_r8_ran(capfd):
    """The 'r8' cases did run k_sweep_r8 and not a sweep the handle falls back to."""
    _assert_only_route(capfd, "[pqa_res8]", "k_sweep_r8")


def _device_errors(mol, mf, wf, dev):
    """Chain-error summary of the resident state, against the oracle's Slater matrices at the device's coordinates."""
    x = dev.configs()
    inv, logpsi = cond.device_state(wf, dev)
    owf = helpers.oracle_wf(mol, mf)
    err = cond.chain_errors(cond.oracle_slater_matrix(owf), inv, logpsi - cond.fresh_jastrow(mol, mf, x), x)
    return x, err


def _fresh_kinetic(mol, mf, x):
    from oracle import energy as oen

    owf = helpers.oracle_wf(mol, mf)
    owf.recompute(OpenConfigs(x.copy()))
    return oen.kinetic(OpenConfigs(x.copy()), owf)


def _check(ratios):
    """All figures are noted before any is asserted."""
    bad = {k: v for k, v in ratios.items() if not v <= MARGIN}
    assert not bad, bad


# ---------------------------------------------------------------- (a) tape replay through each single-determinant sweep
@pytest.mark.parametrize("path", list(PATHS))
@pytest.mark.parametrize("name", list(cond.CASES))
def test_chain_on_tapes_against_the_oracle(name, path, monkeypatch, capfd):
    """Each case of tests/conditioning.py (100 sweeps of the three water cases, 12 of the cluster, no recompute, forced sweeps) through
    k_sweep_r8, k_sweep_res and the launch-per-move sweep on the oracle's tapes.  Every decision is the oracle's (no walker excused: the
    oracle's unforced |ratio - u| is > 1e-6 everywhere).  In units of the oracle's own figure for the same chain, each <= 8: the error of
    the inverse (both spins) against a refined inverse of the oracle's Slater matrix at the device's coordinates, of the resident log|Psi|
    against a fresh one, max |q_e - 1|; the final coordinates in units of what two float64 oracle runs differ by; the per-walker ke and
    grad2 rows of the standalone energy pass against the oracle on a fresh state at the device's coordinates, in units of the oracle's
    updated-against-fresh difference; for the water cases the fused per-sweep means of ke and grad2, averaged over the chain, against the
    oracle's block value in units of what the two oracle runs' block values differ by."""
    mol, mf, W, ns, forced = cond.case_inputs(name)
    o = cond.oracle_case(name)
    wf, dev = _handle(mol, mf, path, monkeypatch, capfd)
    start, gauss, unif, tstep = cond.tapes(mol, W, ns, forced)
    wf.recompute(start)
    live = name in cond.LIVE
    N, necp = gauss.shape[1], getattr(dev, "necp", 0)
    kw = {"ecp_rot": np.tile(np.eye(3), (ns, N, necp, 1, 1)), "ecp_unif": np.ones((ns, N, necp, W))} if (live and necp) else {}
    acc, en, rec = dev.vmc_sweeps(tstep, ns, gauss=gauss, unif=unif, energy=live, record=True, **kw)
    rows = np.real(dev.energy(10.0, seed=9))
    if path == "r8":
        _assert_r8_ran(capfd)
    for k, v in o.items():
        if isinstance(v, float):
            note(f"{name}_oracle_{k}", v)  # the yardsticks themselves
    same = rec == o["decisions"]
    note(f"{name}_{path}_decisions_equal", same.mean())
    assert same.all(), (int((~same).sum()), np.argwhere(~same)[:4].tolist())
    x, err = _device_errors(mol, mf, wf, dev)
    dev_err = cond.summary(err)
    note(f"{name}_{path}_cond", err["cond"].max())
    r = {}
    for k in ("inv", "log", "q0m1"):
        note(f"{name}_{path}_{k}", dev_err[k])
        r[k] = note(f"{name}_{path}_{k}_over_oracle", dev_err[k] / o[k])
    r["x"] = note(f"{name}_{path}_x_over_oracle_spread", float(np.max(np.abs(x - o["x"]))) / o["spread_x"])
    ke_f, g2_f = _fresh_kinetic(mol, mf, x)
    r["ke"] = note(f"{name}_{path}_ke_rows_over_oracle", cond.rel_rows(rows[0], ke_f) / o["ke_upd_vs_fresh"])
    r["grad2"] = note(f"{name}_{path}_grad2_rows_over_oracle", cond.rel_rows(rows[4], g2_f) / o["grad2_upd_vs_fresh"])
    if live:
        en = np.real(en)
        r["block_ke"] = note(f"{name}_{path}_block_ke_over_oracle_spread", abs(en[:, 0].mean() - o["block_ke"]) / o["spread_block_ke"])
        r["block_grad2"] = note(f"{name}_{path}_block_grad2_over_oracle_spread", abs(en[:, 4].mean() - o["block_grad2"]) / o["spread_block_grad2"])
    _check(r)


# ---------------------------------------------------------------- (b) the DMC instantiation
_dmc_oracle = {}


@pytest.mark.parametrize("path", ["r8", "launches"])
def test_dmc_chain_against_the_oracle(path, monkeypatch, capfd):
    """water-1e-5, 13 walkers, 30 DMC steps at tstep 0.02 (T-moves, Umrigar's drift limiter, fixed-node rejection; 480 moves per walker
    without a recompute) through k_sweep_r8's DMC instantiation and the launch-per-move sweep on device Philox draws, which the oracle's
    dmc_propagate replays (philox_dmc_tapes -> DeviceDmcTape).  A walker is excused only where the oracle itself had |ratio - u| < 1e-7
    in one of its tests, and at most one of the 13 may be.  The device reports no per-move masks for DMC steps: the decisions are compared
    as each step's count of accepted drift-diffusion moves and of accepted T-moves (exact), and through the coordinates — one flipped
    decision displaces an electron by ~sqrt(3 tstep) = 0.2 bohr.  Coordinates and weights in units of what two float64 oracle runs (occupied
    columns permuted) differ by, the chain errors of the resident state in units of the oracle's own: each <= 8."""
    mol, mf, W, _, _ = cond.case_inputs("water-1e-5")
    wf, dev = _handle(mol, mf, path, monkeypatch, capfd)
    start, *_ = cond.tapes(mol, W, 1)
    x0 = np.array(start.configs)
    wf.recompute(start)
    w = np.ones(W)
    avg, acc = dev.dmc_steps(cond.DMC_TSTEP, cond.DMC_STEPS, w, cond.DMC_BRANCHCUT, cond.DMC_ETRIAL, cond.DMC_ETRIAL, seed=cond.DMC_SEED)
    if path == "r8":
        _assert_r8_ran(capfd)
    if not _dmc_oracle:  # the draws depend on the seed alone: one oracle side for both paths
        t = dev.philox_dmc_tapes(cond.DMC_SEED, cond.DMC_STEPS, W)
        _dmc_oracle["a"] = cond.oracle_dmc(mol, mf, x0, t)
        _dmc_oracle["b"] = cond.oracle_dmc(mol, cond.permuted_mf(mf, 1), x0, t)
    o, p = _dmc_oracle["a"], _dmc_oracle["b"]
    good = o["min_margin"] >= 1e-7
    note(f"dmc_{path}_walkers_excused", (~good).sum())
    note(f"dmc_{path}_oracle_min_margin", o["min_margin"].min())
    assert (~good).sum() <= 1
    N = x0.shape[1]
    assert o["accepted"][:, 0].sum() < 0.999 * cond.DMC_STEPS * N * W and o["accepted"][:, 1].sum() >= 1  # rejections and T-moves do occur
    if good.all():
        assert np.array_equal(np.rint(acc * W * N), o["accepted"].sum(axis=2)), (acc * W * N, o["accepted"].sum(axis=2))
    x, err = _device_errors(mol, mf, wf, dev)
    assert np.max(np.abs(x - o["x"])[good]) < 1e-6  # every decision and T-move the oracle's
    r = {}
    sx = float(np.max(np.abs(p["x"] - o["x"])[good]))
    sw = float(np.max(np.abs(p["weights"] / o["weights"] - 1)[good]))
    r["x"] = note(f"dmc_{path}_x_over_oracle_spread", float(np.max(np.abs(x - o["x"])[good])) / sx)
    r["weights"] = note(f"dmc_{path}_weights_over_oracle_spread", float(np.max(np.abs(w / o["weights"] - 1)[good])) / sw)
    dev_err = {"inv": float(err["inv"][good].max()), "log": float(err["log"][good].max()), "q0m1": float(np.abs(err["q0m1"][good]).max())}
    note(f"dmc_{path}_cond", err["cond"].max())
    for k in ("inv", "log", "q0m1"):
        note(f"dmc_{path}_{k}", dev_err[k])
        r[k] = note(f"dmc_{path}_{k}_over_oracle", dev_err[k] / o[k])
    _check(r)


# ---------------------------------------------------------------- (c) the quad-cooperative kinetic pass
def test_quad_kinetic_pass_within_its_first_order_bound():
    """Shards of 16 384 walkers take k_kinetic_lw<.., QUAD>, which does not read the value block: it forms ke and grad2 with q_e = 1.  On
    (H2O)8 with cond(D) ~ 1e7, 6 sweeps without a recompute: the fused pass's walker means differ from the means of the standalone rows
    (pqa_energy, which divides) by no more than 2 B + 1e-13 |mean|, B = mean_w sum_e |q_we - 1| |s_we| being the first-order size of what
    the kernel drops (test_conditioning_cpu.py::test_first_order_formula_of_the_unit_value_sum; s_e = -1/2 (ls_e + 2 gs_e.gj_e) for ke,
    2 gs_e.(gs_e + gj_e) for grad2).  B is formed on the host from the device's inverse and its 5-component orbital rows (eval_mo) and the
    device's Jastrow gradients; q and s of the first walkers are cross-checked with oracle-evaluated rows.  1e-11 < max |q - 1| < 1e-6:
    below, the test has no teeth; above, the inverse itself is broken.  The first walkers' chain is replayed by the oracle on the device's
    draws (same decisions), and their standalone rows are compared with the oracle on a fresh state at the device's coordinates, in units
    of the oracle's own updated-against-fresh difference on that chain (<= 8, as in (a))."""
    import pyqmc_amd as pa

    make, eps, _, _, _ = cond.CASES["cluster-1e-5"]
    mol, W = make(), 16384
    mf = cond.near_degenerate_mf(mol, eps)
    wf = cond.gpu_wf(mol, mf)
    dev = wf.fused_device()
    start = pa.initial_guess(mol, W, rng=np.random.default_rng(77))
    x0 = np.array(start.configs[:NQ])
    wf.recompute(start)
    acc, en, rec = dev.vmc_sweeps(0.3, 6, seed=5, energy=True, record=True)
    rows = np.real(dev.energy(10.0, seed=9))
    x = dev.configs()
    nup, ndn = mol.nelec
    N = nup + ndn
    cfg = OpenConfigs(x.copy())
    ja = wf.wf_factors[1]
    gj = np.array([np.real(ja.gradient(e, cfg.electron(e))) for e in range(N)])  # (N, 3, W)
    q, ls, gs = np.empty((N, W)), np.empty((N, W)), np.empty((N, 3, W))
    Ts = [wf.wf_factors[0]._get_state(s)[0][:, 0] for s in (0, 1)]  # (W, n, n) [orbital, electron]
    for s, (b, n) in enumerate(((0, nup), (nup, ndn))):
        T = Ts[s]
        for w0 in range(0, W, 2048):  # (the 5-component rows of all walkers at once are 0.7 GB per spin)
            sl = slice(w0, w0 + 2048)
            mo = dev.eval_mo(s, x[sl, b:b + n], 5)[..., :n].reshape(5, -1, n, n)  # (5, w, electron, orbital)
            r = np.einsum("cwej,wje->cew", mo, T[sl])
            q[b:b + n, sl], ls[b:b + n, sl], gs[b:b + n, :, sl] = r[0], r[4] / r[0], np.moveaxis(r[1:4] / r[0], 0, 1)
    gsgj, gs2 = np.sum(gs * gj, axis=1), np.sum(gs * gs, axis=1)
    dq = np.abs(q - 1.0)
    B = {"ke": float(np.mean(np.sum(dq * np.abs(-0.5 * (ls + 2 * gsgj)), axis=0))),
         "grad2": float(np.mean(np.sum(dq * np.abs(2 * (gs2 + gsgj)), axis=0)))}
    note("quad_max_q0m1", dq.max())
    # q and s of the first walkers from oracle-evaluated orbital rows and Jastrow gradients (the device's inverse: it is the state under test)
    owf = helpers.oracle_wf(mol, mf)
    sl_o, ja_o = owf.wf_factors[0], owf.wf_factors[1]
    ja_o.recompute(OpenConfigs(x[:NQ].copy()))
    c8 = OpenConfigs(x[:NQ].copy())
    for e in range(N):
        s, i = sl_o._spin(e)
        _, mo = sl_o._mo(x[:NQ, e], s, 5)
        col = Ts[s][:NQ, :, i]
        r = np.einsum("cwj,wj->cw", mo[..., sl_o._det_occup[s][0]], col)
        g_o = np.real(ja_o.gradient(e, c8.electron(e)))
        s_o = -0.5 * (r[4] / r[0] + 2 * np.sum(r[1:4] / r[0] * g_o, axis=0))
        s_d = -0.5 * (ls[e, :NQ] + 2 * gsgj[e, :NQ])
        # an orbital value is a sum of nao products |ao c| <= 1, so the two evaluators' rows differ by <= 2 nao eps, and the sums over the
        # inverse column by that times sum_j |T_je| (~1e-8 here, where s is O(1..100): a wrong index or layout would show as O(1))
        tol = 2 * dev.nao * np.finfo(float).eps * np.sum(np.abs(col), axis=1)
        assert np.all(np.abs(r[0] - q[e, :NQ]) <= tol), (e, np.abs(r[0] - q[e, :NQ]).max(), tol.max())
        assert np.all(np.abs(s_o - s_d) <= 1e-6 * np.maximum(1.0, np.abs(s_o))), (e, s_o, s_d)
    assert 1e-11 < dq.max() < 1e-6
    for name, row in (("ke", 0), ("grad2", 4)):
        fused, alone = float(np.real(en[-1][row])), float(rows[row].mean())
        note(f"quad_{name}_fused_minus_standalone", abs(fused - alone))
        note(f"quad_{name}_B", B[name])
        assert abs(fused - alone) <= 2 * B[name] + 1e-13 * abs(alone), (name, fused, alone, B[name])
    # the first walkers' chain replayed by the oracle on the device's draws: the yardstick of (a) for exactly this trajectory
    from oracle import energy as oen, vmc as ovmc

    gauss, unif = dev.philox_tapes(5, 6, NQ)
    record, margins = [], []
    _, ocfg = ovmc.vmc_worker(mol, owf, OpenConfigs(x0), 0.3, gauss, unif, with_energy=False, record=record, margins=margins)
    note("quad_oracle_min_margin", np.abs(margins).min())
    assert np.abs(margins).min() > 1e-6 and np.array_equal(np.asarray(record).reshape(6, N, NQ), rec[:, :, :NQ])
    ke_u, g2_u = oen.kinetic(ocfg, owf)
    ke_o, g2_o = _fresh_kinetic(mol, mf, np.array(ocfg.configs))
    ke_f, g2_f = _fresh_kinetic(mol, mf, x[:NQ])
    _check({"ke": note("quad_standalone_ke_rows_over_oracle", cond.rel_rows(rows[0][:NQ], ke_f) / cond.rel_rows(ke_u, ke_o)),
            "grad2": note("quad_standalone_grad2_rows_over_oracle", cond.rel_rows(rows[4][:NQ], g2_f) / cond.rel_rows(g2_u, g2_o))})


# ---------------------------------------------------------------- (e) periodic, complex and twisted sweeps
PBC_PATHS = {"res": {"PQA_RES": "1"},                            # k_sweep_res<.., PBC> / <.., PBC, CX>
             "launches": {"PQA_RES": "0"},                       # k_step_lw<PBC, CX, ..>, blocked update and k_flush_lw
             "ww-launches": {"PQA_RES": "0", "PQA_LW": "0"}}     # wave per walker: k_propose<CX> / k_accept<CX>


def _pbc_handle(c, path, monkeypatch):
    for k in ("PQA_RES", "PQA_R8", "PQA_LW", "PQA_WW"):
        monkeypatch.delenv(k, raising=False)
    for k, v in PBC_PATHS[path].items():
        monkeypatch.setenv(k, v)  # read when the handle is created
    monkeypatch.setenv("PQA_RES_DEBUG", "1")
    wf = c.gpu_wf()
    return wf, wf.fused_device()


def _assert_res_ran(capfd):
    """With PQA_RES=1 on a cell that res_setup accepts every sweep is k_sweep_res."""
    _assert_only_route(capfd, "[pqa_res]", "k_sweep_res")


def _sweep_launches(dev):
    """(bracketed orbital launches at proposals, bracketed k_step_lw launches) of the sweeps since ``profile_enable`` — which sweep ran:
    k_sweep_ww launches no orbital kernel at all (0, 0); k_propose -> orbitals -> k_accept one per move, of which every 4th is bracketed
    (> 0, 0); the lane-per-walker launch-per-move sweep also brackets a sample of its k_step_lw launches (> 0, > 0); a resident sweep
    brackets its one launch per sweep (sweeps, 0).  (test_gpu_pbc.py::test_event_brackets_do_not_change_the_sweep: the brackets leave
    the numbers alone.)"""
    dev.sync()
    n_orb, n_part = dev.profile_query()[0], dev.profile_query_part()[0]
    dev.profile_enable(False)
    return n_orb, n_part


def _device_configs(c, dev, start):
    """The device's walkers as the container of their kind: for a cell folded coordinates and wrap counters (start wraps plus the
    sweeps' wrap deltas), fetched as the VMC driver does."""
    if not c.periodic:
        return c.configs(dev.configs())
    from pyqmc_amd.vmc import _fetch

    cfg = start.copy()
    _fetch(dev, cfg)
    return cfg


def _chain_ratios(c, o, tag, wf, dev, cfg, rows, nrows=None):
    """The device's chain errors and kinetic rows over the oracle's own, noted; -> {key: ratio}."""
    inv, phase, logpsi = cond.device_state_all(wf, dev)
    err = c.judge(inv, phase, logpsi, cfg)
    dev_err = cond.summary(err)
    note(f"{tag}_cond", err["cond"].max())
    note(f"{tag}_cond_min", err["cond_min"].min())
    r = {}
    for k in dev_err:
        note(f"{tag}_{k}", dev_err[k])
        r[k] = note(f"{tag}_{k}_over_oracle", dev_err[k] / o[k])
    r["x"] = note(f"{tag}_x_over_oracle_spread", float(np.max(np.abs(cfg.configs - o["x"]))) / o["spread_x"])
    n = c.W if nrows is None else nrows
    sub = c.configs(cfg.configs[:n], cfg.wrap[:n]) if c.periodic else c.configs(cfg.configs[:n])
    ke_f, g2_f = c.fresh_kinetic(sub)
    r["ke"] = note(f"{tag}_ke_rows_over_oracle", cond.rel_rows(rows[0][:n], ke_f) / o["ke_upd_vs_fresh"])
    r["grad2"] = note(f"{tag}_grad2_rows_over_oracle", cond.rel_rows(rows[4][:n], g2_f) / o["grad2_upd_vs_fresh"])
    return r


def _pbc_params():
    """Every periodic case through the launch-per-move sweep; the two primitive cells also through the wave-per-walker launches; the
    resident sweep on the cells it takes (res_setup refuses more than 128 lattice-sum candidates: the primitive cells have 249, 3x1x1
    has 183 — with PQA_RES=1 those handles run the launch-per-move sweep again)."""
    return [(n, p) for n in cond.PBC_CASES for p in PBC_PATHS
            if (p == "launches" or (p == "res" and n in cond.RES_ELIGIBLE) or (p == "ww-launches" and n in ("gamma-1e-5", "twist-1e-5")))]


@pytest.mark.parametrize("name,path", _pbc_params())
def test_periodic_chain_on_tapes_against_the_oracle(name, path, monkeypatch, capfd):
    """The periodic cases of tests/conditioning.py (diamond at Gamma and twisted: 100 sweeps; 3x1x1 with complex coefficients: 30; 2x2x2:
    12; the conventional cell, real and twisted: 20; no recompute, forced sweeps) through the launch-per-move sweep (k_step_lw, blocked
    update, k_flush_lw), the resident sweep k_sweep_res<PBC> (2x2x2: two orbital tiles; conventional cell: one) and k_sweep_res<PBC, CX>
    (twisted conventional cell) and, for the two primitive cells, the wave-per-walker launches (k_propose / k_accept), on the oracle's tapes.
    Every decision is the oracle's (fixture g51; its unforced |ratio - u| is > 1e-5 everywhere) and so is every wrap counter.  In units of
    the oracle's own figure for the same chain, each <= 8: the inverse of both spins against a refined inverse of the oracle's Slater
    matrix on the device's PeriodicConfigs (coordinates and wraps), log|Psi| and, for complex cases, the phase of Psi against fresh ones,
    max |q_e - 1|; the folded coordinates in units of what two float64 oracle runs differ by; the per-walker ke and grad2 rows of the
    standalone energy pass against the oracle on a fresh state at the device's configs (k222: the first 4 walkers), in units of the
    oracle's updated-against-fresh difference."""
    c, o = cond.case(name), cond.oracle_case(name)
    wf, dev = _pbc_handle(c, path, monkeypatch)
    dev.set_ewald(10, 1)
    start, gauss, unif, tstep = c.tapes()
    wf.recompute(start)
    dev.profile_enable(True)
    acc, en, rec = dev.vmc_sweeps(tstep, c.ns, gauss=gauss, unif=unif, energy=False, record=True)
    n_orb, n_part = _sweep_launches(dev)
    rows = np.real(dev.energy(10.0, seed=9))
    tag = f"{name}_{path}"
    note(f"{tag}_bracketed_orbital_launches", n_orb), note(f"{tag}_bracketed_step_lw_launches", n_part)
    if path == "res":
        _assert_res_ran(capfd)
        assert (n_orb, n_part) == (c.ns, 0)
    elif path == "launches":
        assert n_orb > c.ns and n_part > 0  # k_orb per move, k_step_lw
    else:
        assert n_orb > c.ns and n_part == 0  # PQA_LW=0 took effect: k_propose / k_accept around the orbital launches
    assert dev.pbc and bool(dev.cplx) == c.complex
    for k, v in o.items():
        if isinstance(v, float):
            note(f"{name}_oracle_{k}", v)  # the yardsticks themselves
    same = rec == o["decisions"]
    note(f"{tag}_decisions_equal", same.mean())
    assert same.all(), (int((~same).sum()), np.argwhere(~same)[:4].tolist())
    cfg = _device_configs(c, dev, start)
    wraps = cfg.wrap == o["wrap"]
    note(f"{tag}_wraps_equal", wraps.mean())
    r = _chain_ratios(c, o, tag, wf, dev, cfg, rows, nrows=4 if name == "k222-1e-5" else None)
    assert wraps.all(), np.argwhere(~wraps)[:4].tolist()
    _check(r)


# ---------------------------------------------------------------- (f) multi-determinant and three-body handles
@pytest.mark.parametrize("ww", ["1", "0"])
@pytest.mark.parametrize("name", list(cond.MD_CASES))
def test_multidet_chain_on_tapes_against_the_oracle(name, ww, monkeypatch):
    """The multi-determinant cases (H2O with 6 'all-ill' determinants and a two-body Jastrow; with the 'mixed' list of g8 and two- plus
    three-body Jastrow factors; 100 sweeps, forced sweeps 5 and 50) through the fused wave-per-walker sweep k_sweep_ww (PQA_WW=1) and the
    k_propose -> orbitals -> k_accept launches (PQA_WW=0), on the oracle's tapes against the oracle run live.  Every decision is the
    oracle's.  In units of the oracle's own figures, each <= 8: the inverse of EVERY unique determinant of both spins (the largest error
    counts), log|Psi| against the long-double log-determinants, the coefficients and freshly evaluated Jastrow exponents, max |q_e - 1|,
    the coordinates, the ke and grad2 rows.  c4-mixed: the resident three-body exponent equals a fresh one to 1e-12 relative — that
    factor keeps no partial sums, nothing may drift."""
    c, o = cond.case(name), cond.oracle_case(name)
    for k in ("PQA_RES", "PQA_R8", "PQA_LW"):
        monkeypatch.delenv(k, raising=False)
    monkeypatch.setenv("PQA_WW", ww)
    wf = c.gpu_wf()
    dev = wf.fused_device()
    assert max(dev.ndet_s) > 1  # a wave-per-walker handle (which of its two sweeps ran: _sweep_launches below)
    start, gauss, unif, tstep = c.tapes()
    wf.recompute(start)
    dev.profile_enable(True)
    acc, en, rec = dev.vmc_sweeps(tstep, c.ns, gauss=gauss, unif=unif, energy=False, record=True)
    n_orb, n_part = _sweep_launches(dev)
    rows = np.real(dev.energy(10.0, seed=9))
    tag = f"{name}_ww{ww}"
    note(f"{tag}_bracketed_orbital_launches", n_orb)
    assert n_part == 0
    assert n_orb == 0 if ww == "1" else n_orb > c.ns  # k_sweep_ww did run (no orbital launch) / the launches did (one per move)
    for k, v in o.items():
        if isinstance(v, float):
            note(f"{name}_oracle_{k}", v)
    same = rec == o["decisions"]
    note(f"{tag}_decisions_equal", same.mean())
    assert same.all(), (int((~same).sum()), np.argwhere(~same)[:4].tolist())
    cfg = _device_configs(c, dev, start)
    r = _chain_ratios(c, o, tag, wf, dev, cfg, rows)
    if c.three:
        j3 = wf.wf_factors[2]
        u_res = j3.value()[1]
        u_fresh = j3.recompute(cfg)[1]  # (last: this replaces the factor's resident state)
        drift = note(f"{tag}_j3_exponent_resident_vs_fresh", helpers.relerr(u_res, u_fresh))
        assert drift <= 1e-12
    _check(r)


# ---------------------------------------------------------------- (g) the periodic DMC instantiation
@pytest.mark.parametrize("name,path", [("gamma-1e-5", "launches"), ("cubic-1e-5", "launches"), ("cubic-1e-5", "res")])
def test_periodic_dmc_chain_against_the_oracle(name, path, monkeypatch, capfd):
    """DMC chains at tstep 0.02 on 13 walkers: gamma-1e-5, 30 steps, through the launch-per-move sweep (the primitive cell's handle
    refuses the resident one); cubic-1e-5, 12 steps (384 moves and 384 T-move proposals per walker), through the launch-per-move sweep
    and through k_sweep_res<DMC, PBC>.  T-move candidates folded into the cell, wrap counters, Ewald energies in the weights.  Unlike the
    open case the draws are HOST tapes (conditioning.host_dmc_tapes), so the oracle side (oracle.dmc.dmc_propagate over PeriodicConfigs,
    twice, occupied columns permuted) is the committed fixture g51.  The conditions of test_dmc_chain_against_the_oracle: a walker is
    excused only where the oracle itself had |margin| < 1e-7, at most one of the 13; the oracle alone shows rejections and T-moves;
    per-step accepted counts exact; coordinates, wrap counters, weights and chain errors within 8 x the oracle's own."""
    import pyqmc_amd as pa

    c, o = cond.case(name), cond.oracle_pbc_dmc_case(name)
    _, nsteps, e_trial = cond.PBC_DMC[name]
    wf, dev = _pbc_handle(c, path, monkeypatch)
    pa.EnergyAccumulator(c.mol).bind(dev)  # the Ewald tables and quadrature rule of the oracle's defaults
    start, *_ = c.tapes(1, ())
    wf.recompute(start)
    w = np.ones(c.W)
    avg, acc = dev.dmc_steps(cond.DMC_TSTEP, nsteps, w, cond.DMC_BRANCHCUT, e_trial, e_trial, tapes=cond.pbc_dmc_tapes(name))
    if path == "res":
        _assert_res_ran(capfd)
    good = o["min_margin"] >= 1e-7
    tag = f"pbc_dmc_{name}_{path}"
    note(f"{tag}_walkers_excused", (~good).sum())
    note(f"{tag}_oracle_min_margin", o["min_margin"].min())
    assert (~good).sum() <= 1
    N, W = start.configs.shape[1], c.W
    assert o["accepted"][:, 0].sum() < 0.999 * nsteps * N * W and o["accepted"][:, 1].sum() >= 1  # rejections and T-moves do occur
    if good.all():
        assert np.array_equal(np.rint(acc * W * N), o["accepted"].sum(axis=2)), (acc * W * N, o["accepted"].sum(axis=2))
    cfg = _device_configs(c, dev, start)
    x = cfg.configs
    assert np.max(np.abs(x - o["x"])[good]) < 1e-6  # every decision and T-move the oracle's
    wraps = (cfg.wrap == o["wrap"])[good]
    note(f"{tag}_wraps_equal", wraps.mean())
    r = {}
    r["x"] = note(f"{tag}_x_over_oracle_spread", float(np.max(np.abs(x - o["x"])[good])) / o["spread_x"])
    r["weights"] = note(f"{tag}_weights_over_oracle_spread", float(np.max(np.abs(w / o["weights"] - 1)[good])) / o["spread_weights"])
    err = c.judge(*cond.device_state_all(wf, dev), cfg)
    dev_err = {"inv": float(err["inv"][good].max()), "log": float(err["log"][good].max()), "q0m1": float(np.abs(err["q0m1"][good]).max())}
    note(f"{tag}_cond", err["cond"].max())
    for k in ("inv", "log", "q0m1"):
        note(f"{tag}_{k}", dev_err[k])
        r[k] = note(f"{tag}_{k}_over_oracle", dev_err[k] / o[k])
    assert wraps.all()
    _check(r)


# ---------------------------------------------------------------- (d) walker independence
@pytest.mark.parametrize("path", ["r8", "res16", "k222-res", "c3-res"])
def test_walkers_that_share_a_block_are_independent(path, monkeypatch, capfd):
    """The resident sweeps run 8 (k_sweep_r8) or 16 (k_sweep_res) walkers per block through shared LDS tiles and cross-lane sums.  The 13
    walkers of water-1e-5, 3 sweeps on tapes, once as they are and once with walkers and tapes permuted: every walker meets other
    block-mates and another slot, the partly filled block included.  Per walker, after un-permuting, bit for bit: decisions, coordinates,
    log|Psi|, the inverse of both spins, the rows of the standalone energy pass.  (The walker means are sums in another order and are
    not compared.)  'k222-res' / 'c3-res': the same for k222-1e-5 and c3-1e-5 through k_sweep_res<PBC> and <PBC, CX> (image lists and
    lattice sums in shared LDS), with the wrap deltas and the phase of Psi — the cells the resident sweep takes; the primitive cells'
    handles refuse it.  (k_sweep_ww runs one wave per walker with no shared tile.)"""
    name, path = (path.split("-")[0] + "-1e-5", "res") if "-" in path else ("water-1e-5", path)
    c = cond.case(name)
    W = c.W
    start, gauss, unif, tstep = c.tapes(3, (1,))
    perm = np.random.default_rng(1).permutation(W)
    assert not np.array_equal(perm // 8, np.arange(W) // 8)
    outs = []
    for order in (np.arange(W), perm):
        if c.periodic:
            wf, dev = _pbc_handle(c, path, monkeypatch)
            dev.set_ewald(10, 1)
            wf.recompute(c.configs(start.configs[order], start.wrap[order]))
        else:
            wf, dev = _handle(c.mol, c.mf, path, monkeypatch, capfd)
            wf.recompute(OpenConfigs(start.configs[order].copy()))
        _, _, rec = dev.vmc_sweeps(tstep, 3, gauss=gauss[:, :, order].copy(), unif=unif[:, :, order].copy(), energy=False, record=True)
        inv, phase, logpsi = cond.device_state_all(wf, dev)
        got = {"rec": np.moveaxis(rec, 2, 0), "x": dev.configs(), "logpsi": logpsi, "inv_up": inv[0][:, 0], "inv_dn": inv[1][:, 0],
               "rows": np.real(dev.energy(10.0, seed=9))[[0, 1, 2, 4]].T}  # ke, ee, ei, grad2 (the ECP row draws its grid per walker index: test_gpu_ecp_shapes.py)
        if c.periodic:
            got["wrap_delta"], got["phase"] = dev.wrap_delta(), phase
        back = np.argsort(order)
        outs.append({k: v[back] for k, v in got.items()})
    if path == "r8":
        _assert_r8_ran(capfd)
    if c.periodic:
        _assert_res_ran(capfd)
    a, b = outs
    assert 0.1 < a["rec"].mean() < 1.0
    tag = path if not c.periodic else name.split("-")[0] + "_" + path
    for k in a:
        diff = a[k] != b[k]
        note(f"independence_{tag}_{k}_unequal", diff.sum())
        assert not diff.any(), (k, np.argwhere(diff)[:4].tolist())
