"""Shared code of the conditioning tests (test_conditioning_cpu.py, test_gpu_conditioning.py, golden/make_golden_conditioning.py):
wave functions whose Slater matrices are ill-conditioned on EVERY walker, random-number tapes with forced acceptances, an inverse
accurate enough to judge a Sherman-Morrison chain at cond(D) ~ 1e8, and the oracle side of every case.  Plain module, no GPU.

The quantity under test is the state a sweep kernel carries through a chain of Sherman-Morrison updates without a recompute:
T (the inverse, [orbital j, electron e]), log|Psi|, and q_e = sum_j phi_j(r_e) T_je — the value sum at the electron's own position, which
the reference divides its derivative sums by and two device kernels take as 1 (k_sweep_r8's next-proposal drift, the quad-cooperative
k_kinetic_lw).  All three are judged against an inverse / determinant of the Slater matrix that the ORACLE evaluates at the judged
state's own coordinates: two float64 trajectories differ by ~1e-9 bohr, and cond(D) times that is more than what is measured.
"""

import copy
import functools
import os

import numpy as np

import helpers
from pyqmc_amd import systems
from pyqmc_amd.configs import OpenConfigs

LD = np.longdouble
TSTEP = 0.3
FIXTURE = "g50_conditioning"

# name -> (molecule, eps, walkers, sweeps, forced sweeps)
CASES = {
    "water-1e-5": (systems.water, 1e-5, 13, 100, (5, 50)),           # n = 4 per spin, 23 AOs: one padding row in k_sweep_r8's tile
    "water-1e-7": (systems.water, 1e-7, 13, 100, (5, 50)),
    "general-1e-5": (systems.water_general, 1e-5, 13, 100, (5, 50)),  # 5 + 5 all-electron, 24 AOs
    "cluster-1e-5": (systems.water_cluster, 1e-5, 13, 12, (3,)),      # n = 32: two orbital tiles; one full + one partly filled r8 block
}
# max cond(D) over the final walkers, measured with the oracle (asserted within a decade by test_conditioning_cpu.py)
COND = {"water-1e-5": 3e6, "water-1e-7": 3e8, "general-1e-5": 2e7, "cluster-1e-5": 9e6}
LIVE = ("water-1e-5", "water-1e-7", "general-1e-5")  # the cluster's oracle side (~9 s a run) is the committed fixture


def near_degenerate_mf(mol, eps):
    """``systems.random_mf`` with occupied orbital 1 of each spin replaced by orbital 0 + eps * (a unit vector): columns 0 and 1 of every
    walker's Slater matrix are parallel up to eps, cond(D) ~ O(10) / eps wherever the walker is."""
    mf = systems.random_mf(mol)
    mo = np.array(mf.mo_coeff, dtype=float)
    g = np.random.default_rng(5)
    for s in (0, 1):
        d = g.standard_normal(mo.shape[1])
        d /= np.linalg.norm(d)
        mo[s][:, 1] = mo[s][:, 0] + eps * d
    return systems.MeanField(mo, np.array(mf.mo_occ))


def permuted_mf(mf, seed):
    """The same determinant (up to its sign) with the occupied columns in another order: every sum over orbitals runs in another order."""
    r = np.random.default_rng(seed)
    mo = np.array(mf.mo_coeff)
    return systems.MeanField(np.stack([mo[s][:, r.permutation(mo.shape[2])] for s in (0, 1)]), np.array(mf.mo_occ))


def tapes(mol, W, nsteps, forced=()):
    """-> (start configs, gauss (nsteps,N,W,3), unif (nsteps,N,W), tstep).  Sweeps in ``forced`` have uniforms 0: every proposal is
    accepted whatever its ratio, which is how walkers land next to nodes."""
    import pyqmc_amd as pa

    N = int(np.sum(mol.nelec))
    r = np.random.default_rng(3)
    gauss = r.standard_normal((nsteps, N, W, 3))
    unif = r.random((nsteps, N, W))
    for k in forced:
        unif[k] = 0.0
    return pa.initial_guess(mol, W, rng=np.random.default_rng(11)), gauss, unif, TSTEP


def refined_inverse(D):
    """(..., n, n) float64 -> longdouble inverse: ``np.linalg.inv`` refined by Newton-Schulz steps X <- X (2 I - D X) in longdouble until
    max |D X - I| < 1e-16 or the residual stops falling.  (A residual EVALUATED in longdouble cannot fall below ~ eps_ld * |D| |X| ~ 1e-19 *
    cond(D), which is above 1e-16 for cond(D) > 1e3; the iteration has converged when it reaches that floor.  What counts is the
    forward error, which test_conditioning_cpu.py measures against 50-digit arithmetic: < 1e-11 relative at cond 3e8, 1e-13 at 3e6 —
    three orders below the chain errors judged with it.  float64 ``inv`` alone is off by cond * 1e-16 and would not do.)"""
    D = np.asarray(D, dtype=float)
    Dl = D.astype(LD)
    X = np.linalg.inv(D).astype(LD)
    I2 = 2 * np.eye(D.shape[-1], dtype=LD)
    last = np.inf
    for _ in range(30):
        P = Dl @ X
        res = float(np.max(np.abs(P - 0.5 * I2))) if P.size else 0.0
        if res < 1e-16 or res > 0.5 * last:
            break
        last = res
        X = X @ (I2 - P)
    return X


def logabsdet(D):
    """(W, n, n) float64 -> (W,) log |det D| by Gaussian elimination with partial pivoting in longdouble (float64 slogdet is off by
    cond * 1e-16, the size of what it would be compared with)."""
    A = np.array(D, dtype=LD)
    W, n, _ = A.shape
    out = np.zeros(W, dtype=LD)
    ar = np.arange(W)
    for k in range(n):
        p = k + np.argmax(np.abs(A[:, k:, k]), axis=1)
        rows = A[ar, p].copy()
        A[ar, p] = A[:, k]
        A[:, k] = rows
        piv = A[:, k, k]
        out += np.log(np.abs(piv))
        if k + 1 < n:
            f = A[:, k + 1:, k] / piv[:, None]
            A[:, k + 1:, k:] -= f[:, :, None] * A[:, k, None, k:]
    return out


def chain_errors(slater_matrix_fn, inverse, logdet, coords):
    """The errors a chain of updates has left in one state (the device's or the oracle's), per walker.

    slater_matrix_fn(coords, s) -> (W, n_s, n_s) [electron, orbital]: the oracle's Slater matrix of spin s at ``coords``;
    inverse: per spin (W, n_s, n_s) [orbital, electron]; logdet: (W,) the state's log |det up| + log |det dn| (its log |Psi| less a
    freshly evaluated Jastrow exponent); coords: (W, N, 3), the judged state's own.
    -> {"inv": (W,) max over spins of max |T - X| / max |X| against ``refined_inverse``, "log": (W,) |logdet - fresh|,
        "q0m1": (W, N) q_e - 1 with q_e = sum_j D_ej T_je, "cond": (W,) max over spins of cond(D)}."""
    coords = np.asarray(coords, dtype=float)
    W = coords.shape[0]
    inv_err, cond, fresh, q = np.zeros(W), np.zeros(W), np.zeros(W, dtype=LD), []
    for s in (0, 1):
        D = np.asarray(slater_matrix_fn(coords, s), dtype=float)
        if D.shape[1] == 0:
            continue
        X = refined_inverse(D)
        T = np.asarray(inverse[s], dtype=float).astype(LD)
        err = np.max(np.abs(T - X), axis=(1, 2)) / np.max(np.abs(X), axis=(1, 2))
        inv_err = np.maximum(inv_err, err.astype(float))
        cond = np.maximum(cond, np.linalg.cond(D))
        fresh += logabsdet(D)
        q.append((np.einsum("wej,wje->we", D.astype(LD), T) - 1).astype(float))
    return {"inv": inv_err, "log": np.abs((np.asarray(logdet, dtype=LD) - fresh).astype(float)), "q0m1": np.concatenate(q, axis=1),
            "cond": cond}


def summary(err):
    """The three figures the tests bound: max over walkers (and electrons) of each chain error."""
    return {"inv": float(err["inv"].max()), "log": float(err["log"].max()), "q0m1": float(np.abs(err["q0m1"]).max())}


# ---------------------------------------------------------------- oracle side
def oracle_slater_matrix(owf):
    sl = owf.wf_factors[0]
    nup, ndn = sl._nelec

    def fn(x, s):
        b, e = nup * s, nup + ndn * s
        _, mo = sl._mo(np.asarray(x)[:, b:e].reshape(-1, 3), s, 1)
        return mo[0].reshape(len(x), e - b, -1)[:, :, sl._det_occup[s][0]]

    return fn


def fresh_jastrow(mol, mf, x):
    """(W,) Jastrow exponent of a freshly built oracle factor at x."""
    return helpers.oracle_wf(mol, mf).wf_factors[1].recompute(OpenConfigs(np.array(x)))[1]


def gpu_wf(mol, mf):
    """``helpers.gpu_wf`` with the Jastrow basis of ``helpers.oracle_wf`` (no electron-ion cusp function, which the library would add
    for the all-electron molecule)."""
    return helpers.gpu_wf(mol, mf, jastrow_kws={"ion_cusp": False})


def oracle_state(owf):
    """(inverse per spin, log|Psi|) of the oracle's current (updated) state."""
    sl = owf.wf_factors[0]
    return [sl._inverse[s][:, 0] for s in (0, 1)], owf.value()[1]


def device_state(wf, dev):
    """(inverse per spin, log|Psi|) of the device's resident state."""
    return [wf.wf_factors[0]._get_state(s)[0][:, 0] for s in (0, 1)], dev.value()[1]


def kinetic_rows(owf, x):
    """Per-electron pieces of the kinetic sum on the oracle's CURRENT state at its coordinates x, as k_kinetic_lw forms them
    (pqa_lw.hpp): with r_c = sum_j d_c phi_j(r_e) T_je (c = value, x, y, z, laplacian), q_e = r_0, the Slater ratios gs = r_xyz / q,
    ls = r_lap / q and the Jastrow's gj, lj (its Laplacian ratio, |gj|^2 included),
        ke = -1/2 sum_e (ls + lj + 2 gs.gj),        grad2 = sum_e |gs + gj|^2.
    -> dict of (N, W) arrays q, ls, gs.gj, |gs|^2, lj, |gj|^2."""
    sl, ja = owf.wf_factors[0], owf.wf_factors[1]
    cfg = OpenConfigs(np.array(x))
    out = {k: [] for k in ("q", "ls", "gsgj", "gs2", "lj", "gj2")}
    for e in range(x.shape[1]):
        s, _ = sl._spin(e)
        _, mo = sl._mo(sl._r(cfg.electron(e)), s, 5)
        r = sl._row_ratios(e, mo)
        gj, lj = ja.gradient_laplacian(e, cfg.electron(e))
        gs = r[1:4] / r[0]
        out["q"].append(r[0]), out["ls"].append(r[4] / r[0]), out["gsgj"].append(np.sum(gs * gj, axis=0))
        out["gs2"].append(np.sum(gs * gs, axis=0)), out["lj"].append(np.real(lj)), out["gj2"].append(np.sum(gj * gj, axis=0))
    return {k: np.array(v) for k, v in out.items()}


def kinetic_sums(rows, unit_q):
    """(ke (W,), grad2 (W,)) from ``kinetic_rows``; ``unit_q``: the value sum q_e taken as 1 (the derivative sums are then q_e times
    the ratios), as the two device kernels do."""
    q = rows["q"] if unit_q else 1.0
    ke = -0.5 * np.sum(q * rows["ls"] + rows["lj"] + 2 * q * rows["gsgj"], axis=0)
    grad2 = np.sum(q * q * rows["gs2"] + 2 * q * rows["gsgj"] + rows["gj2"], axis=0)
    return ke, grad2


def shortcut_terms(rows):
    """First-order change of (ke, grad2) when q_e is taken as 1, per electron: (q_e - 1) s_e with
        s_e[ke] = -1/2 (ls_e + 2 gs_e.gj_e)   (exact: ke is linear in the Slater sums),
        s_e[grad2] = 2 gs_e.(gs_e + gj_e)     (+ (q_e - 1)^2 |gs_e|^2, second order).
    -> (N, W) arrays q - 1, s_ke, s_grad2."""
    return rows["q"] - 1.0, -0.5 * (rows["ls"] + 2 * rows["gsgj"]), 2 * (rows["gs2"] + rows["gsgj"])


def rel_rows(a, b):
    """max over walkers of |a - b| / max(1, |b|): the measure of the per-walker ke and grad2 comparisons."""
    a, b = np.asarray(a, dtype=float), np.asarray(b, dtype=float)
    return float(np.max(np.abs(a - b) / np.maximum(1.0, np.abs(b))))


def case_inputs(name):
    make, eps, W, nsteps, forced = CASES[name]
    mol = make()
    return mol, near_degenerate_mf(mol, eps), W, nsteps, forced


def oracle_run(name, mf=None, nsteps=None, with_energy=False):
    """One oracle chain of case ``name`` (optionally with another mean field of the same wave function, or cut short).
    -> dict: decisions (nsteps, N, W), margins (same shape, ratio - u), x (final coordinates), chain-error summary ``inv`` / ``log`` /
    ``q0m1`` / ``cond``, ``ke_upd_vs_fresh`` / ``grad2_upd_vs_fresh`` (rel_rows of the updated state's kinetic rows against a fresh
    state's at the same coordinates), and with ``with_energy`` the block means ``block_ke`` / ``block_grad2`` of vmc_worker."""
    from oracle import energy as oen, vmc as ovmc

    mol, mf0, W, ns, forced = case_inputs(name)
    mf = mf0 if mf is None else mf
    start, gauss, unif, tstep = tapes(mol, W, ns, forced)
    ns = ns if nsteps is None else nsteps
    owf = helpers.oracle_wf(mol, mf)
    N = gauss.shape[1]
    record, margins = [], []
    emol = copy.copy(mol)
    emol._ecp = {}  # only the kinetic rows of vmc_worker's energies are used: spare the oracle its ECP pass
    blk, cfg = ovmc.vmc_worker(emol, owf, start, tstep, gauss[:ns], unif[:ns], with_energy=with_energy, record=record, margins=margins)
    x = np.array(cfg.configs)
    inv, logpsi = oracle_state(owf)
    err = chain_errors(oracle_slater_matrix(owf), inv, logpsi - fresh_jastrow(mol, mf, x), x)
    out = {"decisions": np.asarray(record).reshape(ns, N, W), "margins": np.asarray(margins).reshape(ns, N, W), "x": x,
           "cond": float(err["cond"].max()), **summary(err)}
    ke_u, g2_u = oen.kinetic(cfg, owf)
    fresh = helpers.oracle_wf(mol, mf)
    fresh.recompute(OpenConfigs(x.copy()))
    ke_f, g2_f = oen.kinetic(OpenConfigs(x.copy()), fresh)
    out["ke_upd_vs_fresh"], out["grad2_upd_vs_fresh"] = rel_rows(ke_u, ke_f), rel_rows(g2_u, g2_f)
    out["owf"] = owf
    if with_energy:
        out["block_ke"], out["block_grad2"] = float(blk["energyke"]), float(blk["energygrad2"])
    return out


FIXTURE_KEYS = ("decisions", "x", "inv", "log", "q0m1", "cond", "ke_upd_vs_fresh", "grad2_upd_vs_fresh", "min_margin", "forced_min_ratio",
                "spread_x", "spread_inv", "spread_log", "spread_q0m1")


def unforced_min_margin(run, forced):
    m = np.abs(run["margins"])
    keep = np.ones(m.shape[0], dtype=bool)
    keep[list(forced)] = False
    return float(m[keep].min())


def compute_case(name):
    """The whole oracle side of a case: the run, a second run with the occupied columns permuted (what two float64 evaluations of one
    chain differ by), and the precondition figures.  The cluster's is stored by golden/make_golden_conditioning.py."""
    mol, mf, W, ns, forced = case_inputs(name)
    a = oracle_run(name, with_energy=name in LIVE)
    b = oracle_run(name, mf=permuted_mf(mf, 1), with_energy=name in LIVE)
    out = {k: a[k] for k in a if k not in ("margins", "owf")}
    out["min_margin"] = unforced_min_margin(a, forced)
    out["forced_min_ratio"] = float(min(a["margins"][k].min() for k in forced))  # (u = 0: the margin is the ratio)
    out["decisions_equal_permuted"] = bool(np.array_equal(a["decisions"], b["decisions"]))
    out["spread_x"] = float(np.max(np.abs(a["x"] - b["x"])))
    for k in ("inv", "log", "q0m1"):
        out["spread_" + k] = b[k] / a[k]
    if name in LIVE:
        out["spread_block_ke"] = abs(a["block_ke"] - b["block_ke"])
        out["spread_block_grad2"] = abs(a["block_grad2"] - b["block_grad2"])
    return out


@functools.lru_cache(maxsize=None)
def oracle_case(name):
    """The oracle side of a case, computed once per process (water cases) or read from the fixture (cluster)."""
    if name in LIVE:
        return compute_case(name)
    g = np.load(os.path.join(helpers.GOLDEN, FIXTURE + ".npz"), allow_pickle=False)
    out = {k: (g[k] if g[k].ndim else g[k].item()) for k in FIXTURE_KEYS}
    out["decisions"] = out["decisions"].astype(bool)
    out["decisions_equal_permuted"] = bool(g["decisions_equal_permuted"])
    return out


# ---------------------------------------------------------------- DMC
DMC_TSTEP, DMC_STEPS, DMC_SEED = 0.02, 30, 77
DMC_ETRIAL, DMC_BRANCHCUT = -5.0, 50.0  # fixed inputs of both sides (the local energies of this trial function scatter around it: weights stay O(1))


def oracle_dmc(mol, mf, x0, device_tapes, tmoves=True):
    """``oracle.dmc.dmc_propagate`` on the draws of a device-RNG DMC block (``DeviceWF.philox_dmc_tapes``), from coordinates x0 with unit
    weights.  -> dict: per-walker ``min_margin`` (smallest |margin| of any of its tests), ``accepted`` (steps, 2) counts of accepted
    drift-diffusion moves / T-moves per step, x, weights, the chain-error summary and cond."""
    from oracle import dmc as odmc, energy as oen

    W, N = x0.shape[:2]
    owf = helpers.oracle_wf(mol, mf)
    tape = helpers.DeviceDmcTape(device_tapes, N, len(oen.ecp_atoms(mol)), tmoves)
    nsteps = device_tapes["gauss"].shape[0]
    record, margins = [], []
    _, cfg, wts = odmc.dmc_propagate(mol, owf, OpenConfigs(np.array(x0)), np.ones(W), DMC_TSTEP, DMC_BRANCHCUT, DMC_ETRIAL, DMC_ETRIAL,
                                     nsteps, tape, record=record, margins=margins)
    x = np.array(cfg.configs)
    inv, logpsi = oracle_state(owf)
    err = chain_errors(oracle_slater_matrix(owf), inv, logpsi - fresh_jastrow(mol, mf, x), x)
    per_step = len(record) // nsteps
    acc = np.zeros((nsteps, 2, W))
    for k, (kind, _, a) in enumerate(record):
        acc[k // per_step, 0 if kind == "d" else 1] += a
    return {"min_margin": np.min([np.abs(m) for _, _, m in margins], axis=0), "accepted": acc, "x": x, "weights": np.asarray(wts),
            "cond": float(err["cond"].max()), **summary(err)}
