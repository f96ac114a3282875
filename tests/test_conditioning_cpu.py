"""The inputs of test_gpu_conditioning.py, pinned with the CPU oracle alone: ill-conditioned Slater matrices on every walker, long chains
of Sherman-Morrison updates, no Metropolis near-tie — and the two facts its bounds rest on (what two float64 evaluations of one chain
differ by, and the first-order size of taking the value sum q_e as 1)."""

import numpy as np
import pytest

import conditioning as cond
import helpers
from pyqmc_amd.configs import OpenConfigs


def _slater_matrices(name):
    c = cond.case(name)
    start, *_ = c.tapes()
    return cond.oracle_slater_matrices(c.oracle_wf())(start, 0)[:, 0]


def _mp(v):
    """A longdouble (or clongdouble) as an mpmath number: the sum of two doubles per component."""
    import mpmath

    if np.iscomplexobj(v):
        return mpmath.mpc(_mp(v.real), _mp(v.imag))
    hi = float(v)
    return mpmath.mpf(hi) + mpmath.mpf(float(v - np.longdouble(hi)))


@pytest.mark.parametrize("name,nwalk,bound", [("water-1e-5", 13, 1e-13), ("water-1e-7", 13, 1e-11), ("cluster-1e-5", 1, 1e-12),
                                              ("cx311-1e-5", 2, 1e-13)])
def test_refined_inverse_against_50_digit_arithmetic(name, nwalk, bound):
    """The truth the chain errors are measured against: forward error of ``refined_inverse`` (and of ``logabsdet``) against mpmath at 50
    digits, relative to max |X|.  ``bound`` is three orders below the smallest chain error the case is used to judge (4e-11, 2e-9,
    4e-10 in the inverse; cx311, the complex case with n = 12: 1.1e-10; measured 1.6e-14 there, float64 ``inv`` 9e-11), and float64 ``inv`` alone misses it."""
    import mpmath

    D = _slater_matrices(name)[:nwalk]
    X = cond.refined_inverse(D)
    ph, ld = cond.slogdet_ld(D)
    n = D.shape[-1]
    worst = worst64 = worst_log = worst_ph = 0.0
    with mpmath.workdps(50):
        for w in range(nwalk):
            Dm = mpmath.matrix(D[w].tolist())
            Xm = Dm ** -1
            scale = max(abs(Xm[i, j]) for i in range(n) for j in range(n))
            X64 = np.linalg.inv(D[w])
            for i in range(n):
                for j in range(n):
                    worst = max(worst, float(abs(Xm[i, j] - _mp(X[w, i, j])) / scale))
            worst64 = max(worst64, float(max(abs(Xm[i, j] - complex(X64[i, j])) for i in range(n) for j in range(n)) / scale))
            det = mpmath.det(Dm)
            worst_log = max(worst_log, float(abs(mpmath.log(abs(det)) - _mp(ld[w]))))
            worst_ph = max(worst_ph, float(abs(det / abs(det) - _mp(ph[w]))))
    print(f"[conditioning] {name}: refined_inverse {worst:.2e}, float64 inv {worst64:.2e}, logabsdet {worst_log:.2e}, phase {worst_ph:.2e}")
    assert worst < bound and worst_log < bound and worst_ph < bound
    assert worst64 > bound


@pytest.mark.parametrize("name", list(cond.ALL_CASES))
def test_case_is_ill_conditioned_and_far_from_ties(name):
    """Each case of the GPU tests: cond(D) within a decade of its nominal value, every unforced Metropolis test further than 1e-6 from a
    tie (so every decision must be reproduced: no walker is ever excused), and the oracle's own chain error non-zero and below 1e-6 —
    hard, not broken.  Measured (max cond / min |ratio - u| / chain error of inverse, log): water-1e-5 3.0e6 / 1.5e-4 / 4.2e-11, 5.0e-10;
    water-1e-7 3.0e8 / 1.5e-4 / 2.4e-9, 6.1e-8; general-1e-5 2.3e7 / 1.8e-4 / 7.2e-11, 1.4e-9 (smallest forced ratio 3.1e-8);
    cluster-1e-5 (fixture) 8.6e6 / 6.0e-6 / 3.8e-10, 5.7e-8 (smallest forced ratio 4.6e-7).
    The periodic, complex and multi-determinant cases (cond is the largest over walkers AND unique determinants; their smallest forced
    ratio is below 1e-3): gamma-1e-5 2.5e6 / 1.9e-5 / 7.0e-11, 2.6e-8;
    twist-1e-5 9.8e5 / 2.9e-5 / 8.7e-11, 6.7e-10 (phase 9.5e-10); cx311-1e-5 3.2e6 / 3.4e-5 / 1.1e-10, 1.4e-9 (3.1e-10); k222-1e-5 5.8e6 /
    1.5e-4 / 1.0e-9, 4.4e-9; cubic-1e-5 3.1e6 / 2.1e-4 / 1.5e-10, 6.3e-9; c3-1e-5 2.3e6 / 2.5e-5 / 2.2e-10, 7.2e-10 (5.4e-10);
    multidet-all-1e-5 4.0e7 (smallest 2.1e5) / 3.0e-4 / 3.8e-9, 3.1e-8; c4-mixed-1e-5 4.1e7 (smallest 2.6) / 3.8e-5 / 3.0e-9, 1.2e-7.
    The tape seeds of twist-1e-5 and cx311-1e-5 were changed for the forced-ratio condition (conditioning.PBC_CASES)."""
    o = cond.oracle_case(name)
    print(f"[conditioning] {name}: " + ", ".join(f"{k} {v:.3e}" for k, v in o.items() if isinstance(v, float)))
    new = name not in cond.CASES
    assert cond.COND[name] / 10 < o["cond"] < cond.COND[name] * 10
    assert o["min_margin"] > 1e-6
    for k in ("inv", "log", "q0m1") + (("phase",) if "phase" in o else ()):
        assert 0.0 < o[k] < 1e-6, (k, o[k])
    assert 0.0 < o["forced_min_ratio"] < (1e-3 if new else 1e-2)  # a forced sweep did put a walker next to a node
    assert o["decisions_equal_permuted"]
    c = cond.case(name)
    assert o["decisions"].shape == (c.ns, int(np.sum(c.mol.nelec)), c.W) and o["decisions"][list(c.forced)].all()
    assert 0.2 < o["decisions"].mean() < 0.95
    if c.periodic:
        assert o["wrap"].shape == o["x"].shape and np.abs(o["wrap"]).sum() > 0  # walkers did leave the cell
    if c.complex:
        assert np.allclose(np.abs(o["psi_phase"]), 1.0, atol=1e-12) and np.abs(np.imag(o["psi_phase"])).max() > 0.1


def test_cluster_fixture_belongs_to_these_inputs():
    """The committed oracle side of the cluster case is the trajectory of today's inputs: its first sweeps, run live (the whole chain takes
    ~9 s), give the fixture's decisions."""
    g = cond.oracle_case("cluster-1e-5")
    live = cond.oracle_run("cluster-1e-5", nsteps=2)
    assert np.array_equal(live["decisions"], g["decisions"][:2])
    assert cond.unforced_min_margin(live, ()) >= g["min_margin"]


@pytest.mark.parametrize("name", list(cond.PBC_CASES))
def test_periodic_fixture_belongs_to_these_inputs(name):
    """The committed oracle side of each periodic case (g51) is the trajectory of today's inputs: its first sweeps (two; one of k222 and of the conventional cells),
    run live, give the fixture's decisions.  On the twisted cell also: the truth — Slater rows evaluated on the state's PeriodicConfigs,
    folded coordinates and wrap counters — gives the oracle's own state an inverse error below 1e-8, live and over the whole chain,
    while rows evaluated at the folded coordinates alone (their phase e^{ik.L.wrap} missing) call the same correct state wrong by O(1)."""
    g = cond.oracle_case(name)
    k = 2 if name in ("gamma-1e-5", "twist-1e-5", "cx311-1e-5") else 1
    live = cond.oracle_run(name, nsteps=k)
    assert np.array_equal(live["decisions"], g["decisions"][:k])
    assert cond.unforced_min_margin(live, ()) >= g["min_margin"]
    if name == "twist-1e-5":
        print(f"[conditioning] twist: oracle inverse error {live['inv']:.2e} after {k} sweeps, {g['inv']:.2e} after the chain")
        assert live["inv"] < 1e-8 and g["inv"] < 1e-8
        c, cfg = cond.case(name), live["cfg"]
        assert np.abs(cfg.wrap).sum() > 0
        inv, ph, lg = cond.oracle_state_all(live["owf"])
        folded = cond.summary(c.judge(inv, ph, lg, c.configs(cfg.configs)))
        print(f"[conditioning] twist: the same state judged at the folded coordinates alone: inverse 'error' {folded['inv']:.2e}")
        assert folded["inv"] > 1e-2


@pytest.mark.parametrize("name", list(cond.PBC_DMC))
def test_periodic_dmc_fixture_belongs_to_these_inputs(name):
    """The committed oracle side of each periodic DMC chain (g51, "dmc/" and "dmc_cubic/"): its first steps (2 of gamma, 1 of cubic, where
    a step takes 15 s), run live on the same host tapes, give the fixture's per-step accepted counts AND the wrap counters stored for
    that point; over the whole chain the oracle alone shows rejections and T-moves, at most one walker came within 1e-7 of a tie, and the
    weights stayed O(1) in the median (the local energies of these random trial functions scatter by tens of hartree: single walkers'
    weights fall to 5e-4)."""
    g = cond.oracle_pbc_dmc_case(name)
    k = cond.pbc_dmc_first(name)
    live = cond.oracle_pbc_dmc(name, nsteps=k)
    assert np.array_equal(live["accepted"], g["accepted"][:k])
    assert np.array_equal(live["wrap"], g["wrap_first"])
    print(f"[conditioning] periodic DMC {name}: " + ", ".join(f"{q} {g[q]:.3e}" for q in ("cond", "inv", "log", "q0m1", "spread_x", "spread_weights")),
          f"min margin {g['min_margin'].min():.2e}, weights {g['weights'].min():.2e} .. {g['weights'].max():.2f}, "
          f"median {np.median(g['weights']):.2f}, T-moves {int(g['accepted'][:, 1].sum())}")
    c = cond.case(name)
    N, nsteps = int(np.sum(c.mol.nelec)), cond.PBC_DMC[name][1]
    assert g["accepted"].shape == (nsteps, 2, c.W)
    assert g["accepted"][:, 0].sum() < 0.999 * nsteps * N * c.W and g["accepted"][:, 1].sum() >= 1
    assert (g["min_margin"] < 1e-7).sum() <= 1
    assert 0.1 < np.median(g["weights"]) < 10 and g["weights"].min() > 1e-4 and g["weights"].max() < 20
    assert cond.COND[name] / 10 < g["cond"] < cond.COND[name] * 10
    for q in ("inv", "log", "q0m1"):
        assert 0.0 < g[q] < 1e-6, (q, g[q])
    assert 0.0 < g["spread_x"] < 1e-6 and 0.0 < g["spread_weights"] < 1e-6
    assert np.abs(g["wrap"]).sum() > 0


def test_oracle_tmove_candidates_are_folded_and_leave_the_wrap_counters():
    """The reference folds its T-move candidates into the cell (eval_ecp.py:113) and propose_tmoves takes their coordinates alone
    (dmc.py:100), so a T-move across the cell boundary does not advance the wrap counters.  The oracle's ``compute_tmoves`` likewise: on
    the start walkers of gamma-1e-5 some unfolded quadrature points lie outside the cell, every candidate it hands on lies inside, and
    moving an electron to such a candidate through ``make_irreducible`` / ``move`` leaves its counters where they were."""
    from oracle import dmc as odmc, energy as oen

    c = cond.case("gamma-1e-5")
    start, *_ = c.tapes(1, ())
    owf = c.oracle_wf()
    owf.recompute(start)
    W = c.W
    inv_lat = np.linalg.inv(c.mol.lattice_vectors())
    ia = oen.ecp_atoms(c.mol)[0]
    raw = oen.ecp_ea(c.mol, start, owf, 0, ia, 10.0, np.eye(3), np.zeros(W))
    frac_raw = raw["epos"][raw["mask"]] @ inv_lat
    crossing = (frac_raw < 0).any(axis=-1) | (frac_raw >= 1).any(axis=-1)  # (masked walkers, points)
    assert crossing.any()

    class Tape:
        def random(self, n):
            return np.zeros(n)

        def rot(self):
            return np.eye(3)

    ratio, weight, pos = odmc.compute_tmoves(c.mol, start, owf, 0, 10.0, cond.DMC_TSTEP, Tape())
    frac = pos @ inv_lat
    assert frac.min() > -1e-12 and frac.max() < 1 + 1e-12
    w_idx = np.nonzero(raw["mask"])[0][np.nonzero(crossing.any(axis=1))[0][0]]
    p_idx = int(np.nonzero(crossing[np.nonzero(raw["mask"])[0].tolist().index(w_idx)])[0][0])
    newpos = start.configs[:, 0, :].copy()
    newpos[w_idx] = pos[w_idx, p_idx]
    before = start.wrap.copy()
    cfg = start.copy()
    accept = np.zeros(W, dtype=bool)
    accept[w_idx] = True
    cfg.move(0, cfg.make_irreducible(0, newpos), accept)
    assert np.max(np.abs(cfg.configs[w_idx, 0] - pos[w_idx, p_idx])) < 1e-12 and np.array_equal(cfg.wrap, before)


# chain-error ratios between two float64 evaluations of one chain must lie inside [1 / margin, margin]: 8 (the GPU tests' MARGIN) unless a
# case's measured spread asks for a margin of its own (largest spread x 8 / 2.8, the headroom the 8 has over water's 2.8)
SPREAD_MARGIN = {}


def test_summation_order_spread():
    """What two float64 evaluations of ONE chain differ by: the oracle on water-1e-5 (20 sweeps, forced sweep 5) with the occupied orbital
    columns in six other orders — the same wave function, every sum over orbitals in another order.  Decisions identical; the chain errors
    of the permuted runs lie within 0.5 .. 2.6 times the original's (measured, with the 100-sweep cases' 0.6 .. 2.8 of
    test_case_is_ill_conditioned_and_far_from_ties).  The GPU tests allow the device 8 times the oracle's own error: a factor ~3 of such
    spread either way, and the device's fused multiply-adds and AO rounding on top.  Asserted here: the spread stays inside that 8.
    Likewise gamma-1e-5 (20 sweeps, the columns of the k-point's block in two other orders: a run takes half a minute) and
    multidet-all-1e-5 (20 sweeps, six orders, the occupied columns permuted alike in every determinant).  Measured: water 0.55 .. 1.83,
    gamma 0.36 .. 1.54, multidet-all 0.61 .. 3.64; over the full chains of the new cases 0.24 .. 1.88: no case needs a margin of its own.
    Final coordinates of the runs differ by 2.6e-10 bohr (water), 1.5e-9 (gamma), 7.3e-9 (multidet-all,
    whose cond(D) is 13 times water's): bounded by 1e-8 for water as before and by 1e-7 for the other two."""
    for name, seeds in (("water-1e-5", range(1, 7)), ("gamma-1e-5", (1, 2)), ("multidet-all-1e-5", range(1, 7))):
        base = cond.oracle_run(name, nsteps=20)
        lo, hi, dx = np.inf, 0.0, 0.0
        for seed in seeds:
            p = cond.permuted_run(name, seed, nsteps=20)
            assert np.array_equal(p["decisions"], base["decisions"])
            r = [p[k] / base[k] for k in ("inv", "log", "q0m1")]
            lo, hi, dx = min(lo, *r), max(hi, *r), max(dx, float(np.max(np.abs(p["x"] - base["x"]))))
        print(f"[conditioning] summation-order spread, {name}: chain-error ratios {lo:.2f} .. {hi:.2f}, final coordinates differ by {dx:.2e} bohr")
        m = SPREAD_MARGIN.get(name, 8)
        assert 1 / m < lo and hi < m, name
        assert 0.0 < dx < (1e-8 if name == "water-1e-5" else 1e-7), name
    for name in cond.LIVE_ALL + tuple(cond.PBC_CASES):
        o = cond.oracle_case(name)
        m = SPREAD_MARGIN.get(name, 8)
        assert all(1 / m < o["spread_" + k] < m for k in ("inv", "log", "q0m1") + (("phase",) if "phase" in o else ())), name


@pytest.mark.parametrize("name", ["water-1e-5", "water-1e-7"])
def test_first_order_formula_of_the_unit_value_sum(name):
    """k_sweep_r8's drift and the quad-cooperative k_kinetic_lw take q_e = sum_j phi_j(r_e) T_je as 1 where the reference divides by it.
    With the Slater sums r_c = sum_j d_c phi_j(r_e) T_je, gs = r_xyz / q, ls = r_lap / q and the Jastrow's gj, lj, k_kinetic_lw forms
    (pqa_lw.hpp) ke = -1/2 sum_e (ls + lj + 2 gs.gj) and grad2 = sum_e |gs + gj|^2; without the division gs and ls become q gs and q ls:
        ke[q := 1]    = ke    + sum_e (q_e - 1) s_e,       s_e = -1/2 (ls_e + 2 gs_e.gj_e)       (exact, ke is linear in them)
        grad2[q := 1] = grad2 + sum_e (q_e - 1) 2 gs_e.(gs_e + gj_e) + sum_e (q_e - 1)^2 |gs_e|^2.
    Checked on the oracle's state after the whole chain, where q - 1 is ~1e-10: the two evaluations differ by the first-order sum up to
    rounding of the sums themselves (1e-14 of sum_e |terms|: ~100 eps for sums of 8 x 3 terms) and the second-order term."""
    o = cond.oracle_run(name)
    owf, x = o["owf"], o["x"]
    rows = cond.kinetic_rows(owf, x)
    ke_d, g2_d = cond.kinetic_sums(rows, unit_q=False)
    ke_1, g2_1 = cond.kinetic_sums(rows, unit_q=True)
    from oracle import energy as oen

    ke_o, g2_o = oen.kinetic(OpenConfigs(x.copy()), owf)  # the dividing evaluation is the oracle's own accumulator
    assert np.max(np.abs(ke_d - ke_o) / np.maximum(1, np.abs(ke_o))) < 1e-13 and np.max(np.abs(g2_d - g2_o) / np.maximum(1, np.abs(g2_o))) < 1e-13
    dq, s_ke, s_g2 = cond.shortcut_terms(rows)
    assert 1e-12 < np.max(np.abs(dq)) < 1e-6
    for tag, diff, s, mag in (("ke", ke_1 - ke_d, s_ke, np.abs(rows["ls"]) + np.abs(rows["lj"]) + 2 * np.abs(rows["gsgj"])),
                              ("grad2", g2_1 - g2_d, s_g2, rows["gs2"] + 2 * np.abs(rows["gsgj"]) + rows["gj2"])):
        first = np.sum(dq * s, axis=0)
        second = np.sum(dq * dq * rows["gs2"], axis=0)
        tol = 1e-14 * np.sum(mag, axis=0) + 2 * second
        print(f"[conditioning] {name} {tag}: max |diff| {np.max(np.abs(diff)):.3e}, first-order sum {np.max(np.abs(first)):.3e}, "
              f"max |diff - first| {np.max(np.abs(diff - first)):.3e}, rounding allowance {np.max(tol):.3e}")
        assert np.all(np.abs(diff - first) <= tol)
        assert np.max(np.abs(first)) > 10 * np.median(tol)  # the check has teeth: the first-order term stands above the allowance


def test_chain_errors_see_a_small_defect():
    """The measure has teeth at the size the GPU tests bound: on the oracle's state after 20 sweeps of water-1e-5 (own chain error 1e-11 ..
    1e-10), one inverse column of one walker scaled by 1 + 1e-8 — what a single missed normalisation of relative size 1e-8 leaves — shows
    as 1e-8 in max |q - 1| (9 times the bound of 8 x the oracle's own) and as 5e-9 in the inverse error of that walker (4 times the
    bound), and nowhere else; a stale
    log|Psi| of the same size shows likewise.  The same on a COMPLEX inverse (twist-1e-5 after 2 sweeps: a column turned by the phase
    1 + 1e-8 i, a stale phase of Psi) and in a NON-REFERENCE determinant (multidet-all-1e-5 after 4 sweeps: the column with the largest
    entry of unique determinant 1 of spin up, by d = 100 x the oracle's own inverse error, at least 1e-8)."""
    o = cond.oracle_run("water-1e-5", nsteps=20)
    mol, mf, *_ = cond.case_inputs("water-1e-5")
    owf, x = o["owf"], o["x"]
    inv, logpsi = cond.oracle_state(owf)
    bad = [inv[0].copy(), inv[1].copy()]
    bad[0][3, :, 2] *= 1 + 1e-8
    logdet = logpsi - cond.fresh_jastrow(mol, mf, x)
    logdet[5] += 1e-8
    err = cond.chain_errors(cond.oracle_slater_matrix(owf), bad, logdet, x)
    assert abs(err["q0m1"][3, 2] / 1e-8 - 1) < 0.1 and err["q0m1"][3, 2] > 8 * o["q0m1"]
    others = np.ones(err["q0m1"].shape, dtype=bool)
    others[3, 2] = False
    assert np.abs(err["q0m1"][others]).max() <= o["q0m1"]
    assert err["inv"][3] > 8 * o["inv"] and np.delete(err["inv"], 3).max() <= o["inv"]
    assert abs(err["log"][5] / 1e-8 - 1) < 0.2 and np.delete(err["log"], 5).max() <= o["log"]
    # a complex inverse
    c = cond.case("twist-1e-5")
    o = cond.oracle_run("twist-1e-5", nsteps=2)
    inv, ph, lg = cond.oracle_state_all(o["owf"])
    bad = [inv[0].copy(), inv[1].copy()]
    bad[1][7, 0, :, 1] *= 1 + 1e-8j
    ph = ph.copy()
    ph[2] *= np.exp(1e-8j)
    err = c.judge(bad, ph, lg, o["cfg"])
    nup = c.mol.nelec[0]
    assert abs(err["q0m1"][7, nup + 1] / 1e-8j - 1) < 0.1 and abs(err["q0m1"][7, nup + 1]) > 8 * o["q0m1"]
    others = np.ones(err["q0m1"].shape, dtype=bool)
    others[7, nup + 1] = False
    assert np.abs(err["q0m1"][others]).max() <= o["q0m1"]
    assert err["inv"][7] > 8 * o["inv"] and np.delete(err["inv"], 7).max() <= o["inv"]
    assert abs(err["phase"][2] / 1e-8 - 1) < 0.2 and err["phase"][2] > 8 * o["phase"] and np.delete(err["phase"], 2).max() <= o["phase"]
    # a determinant that is not the reference
    c = cond.case("multidet-all-1e-5")
    o = cond.oracle_run("multidet-all-1e-5", nsteps=4)
    inv, ph, lg = cond.oracle_state_all(o["owf"])
    assert inv[0].shape[1] > 1
    d = max(1e-8, 100 * o["inv"])
    bad = [inv[0].copy(), inv[1].copy()]
    col = int(np.argmax(np.abs(inv[0][3, 1]).max(axis=0)))
    bad[0][3, 1, :, col] *= 1 + d
    err = c.judge(bad, ph, lg, o["cfg"])
    assert abs(err["q0m1"][3, col] / d - 1) < 0.1 and err["q0m1"][3, col] > 8 * o["q0m1"]
    assert abs(err["inv"][3] / d - 1) < 0.1 and err["inv"][3] > 8 * o["inv"] and np.delete(err["inv"], 3).max() <= o["inv"]


def _wrong_update(kind):
    """``oracle.wf.Slater.updateinternals`` (slater.py:262-291) with a planted defect: 'conj' conjugates the row factor of the
    Sherman-Morrison outer product (right for real matrices, wrong for complex ones), 'skip' leaves unique determinant 1 untouched."""
    from oracle.wf import _phase

    def update(self, e, epos, configs, mask=None, saved_values=None):
        s, eeff = self._spin(e)
        mask = np.ones(epos.configs.shape[0], dtype=bool) if mask is None else np.asarray(mask, dtype=bool)
        mo = saved_values[1][mask]
        vec = mo[:, self._det_occup[s]]
        old = self._inverse[s][mask]
        tmp = np.einsum("wdk,wdkj->wdj", vec, old)
        ratio = tmp[:, :, eeff]
        invr = old[:, :, :, eeff] / ratio[:, :, None]
        inv = old - np.einsum("wdi,wdj->wdij", invr, np.conj(tmp) if kind == "conj" else tmp)
        inv[:, :, :, eeff] = invr
        if kind == "skip":
            inv[:, 1], ratio = old[:, 1], ratio.copy()
            ratio[:, 1] = 1.0
        self._inverse[s][mask] = inv
        self._dets[s][0][mask] *= _phase(ratio)
        self._dets[s][1][mask] += np.log(np.abs(ratio))
        self._x_last[mask, e] = self._r(epos)[mask]

    return update


@pytest.mark.parametrize("kind,name", [("conj", "twist-1e-5"), ("skip", "multidet-all-1e-5")])
def test_chain_errors_catch_a_wrong_update(kind, name, monkeypatch):
    """A deliberately wrong build is caught: two sweeps of the oracle with a defect planted in its Sherman-Morrison update — a complex
    update that conjugates the wrong factor (twist-1e-5), a skipped update of a non-reference determinant (multidet-all-1e-5) — leave a
    state whose inverse error is far beyond 8 x the right oracle's (which is what the GPU tests allow the device); the right update on
    the same tapes is within it by construction."""
    from oracle import wf as owf

    right = cond.oracle_run(name, nsteps=2)
    monkeypatch.setattr(owf.Slater, "updateinternals", _wrong_update(kind))
    wrong = cond.oracle_run(name, nsteps=2)
    print(f"[conditioning] planted {kind}: inverse error {wrong['inv']:.2e} (right update {right['inv']:.2e}), log {wrong['log']:.2e} ({right['log']:.2e})")
    assert wrong["inv"] > 1e3 * 8 * right["inv"]
    assert wrong["log"] > 8 * right["log"]
