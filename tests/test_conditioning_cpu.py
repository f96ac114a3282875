"""The inputs of test_gpu_conditioning.py, pinned with the CPU oracle alone: ill-conditioned Slater matrices on every walker, long chains
of Sherman-Morrison updates, no Metropolis near-tie — and the two facts its bounds rest on (what two float64 evaluations of one chain
differ by, and the first-order size of taking the value sum q_e as 1)."""

import numpy as np
import pytest

import conditioning as cond
import helpers
from pyqmc_amd.configs import OpenConfigs


def _slater_matrices(name):
    mol, mf, W, ns, forced = cond.case_inputs(name)
    start, *_ = cond.tapes(mol, W, ns, forced)
    owf = helpers.oracle_wf(mol, mf)
    return cond.oracle_slater_matrix(owf)(start.configs, 0)


@pytest.mark.parametrize("name,nwalk,bound", [("water-1e-5", 13, 1e-13), ("water-1e-7", 13, 1e-11), ("cluster-1e-5", 1, 1e-12)])
def test_refined_inverse_against_50_digit_arithmetic(name, nwalk, bound):
    """The truth the chain errors are measured against: forward error of ``refined_inverse`` (and of ``logabsdet``) against mpmath at 50
    digits, relative to max |X|.  ``bound`` is three orders below the smallest chain error the case is used to judge (4e-11, 2e-9,
    4e-10 in the inverse), and float64 ``inv`` alone misses it."""
    import mpmath

    D = _slater_matrices(name)[:nwalk]
    X = cond.refined_inverse(D)
    ld = cond.logabsdet(D)
    n = D.shape[-1]
    worst = worst64 = worst_log = 0.0
    with mpmath.workdps(50):
        for w in range(nwalk):
            Dm = mpmath.matrix(D[w].tolist())
            Xm = Dm ** -1
            scale = max(abs(Xm[i, j]) for i in range(n) for j in range(n))
            for i in range(n):
                for j in range(n):
                    hi = float(X[w, i, j])  # a longdouble as the sum of two doubles
                    lo = float(X[w, i, j] - np.longdouble(hi))
                    worst = max(worst, float(abs(Xm[i, j] - hi - lo) / scale))
            worst64 = max(worst64, float(max(abs(Xm[i, j] - float(np.linalg.inv(D[w])[i, j])) for i in range(n) for j in range(n)) / scale))
            hi = float(ld[w])
            worst_log = max(worst_log, float(abs(mpmath.log(abs(mpmath.det(Dm))) - hi - float(ld[w] - np.longdouble(hi)))))
    print(f"[conditioning] {name}: refined_inverse {worst:.2e}, float64 inv {worst64:.2e}, logabsdet {worst_log:.2e}")
    assert worst < bound and worst_log < bound
    assert worst64 > bound


@pytest.mark.parametrize("name", list(cond.CASES))
def test_case_is_ill_conditioned_and_far_from_ties(name):
    """Each case of the GPU tests: cond(D) within a decade of its nominal value, every unforced Metropolis test further than 1e-6 from a
    tie (so every decision must be reproduced: no walker is ever excused), and the oracle's own chain error non-zero and below 1e-6 —
    hard, not broken.  Measured (max cond / min |ratio - u| / chain error of inverse, log): water-1e-5 3.0e6 / 1.5e-4 / 4.2e-11, 5.0e-10;
    water-1e-7 3.0e8 / 1.5e-4 / 2.4e-9, 6.1e-8; general-1e-5 2.3e7 / 1.8e-4 / 7.2e-11, 1.4e-9 (smallest forced ratio 3.1e-8);
    cluster-1e-5 (fixture) 8.6e6 / 6.0e-6 / 3.8e-10, 5.7e-8 (smallest forced ratio 4.6e-7)."""
    o = cond.oracle_case(name)
    print(f"[conditioning] {name}: " + ", ".join(f"{k} {v:.3e}" for k, v in o.items() if isinstance(v, float)))
    assert cond.COND[name] / 10 < o["cond"] < cond.COND[name] * 10
    assert o["min_margin"] > 1e-6
    for k in ("inv", "log", "q0m1"):
        assert 0.0 < o[k] < 1e-6, (k, o[k])
    assert 0.0 < o["forced_min_ratio"] < 1e-2  # a forced sweep did put a walker next to a node
    assert o["decisions_equal_permuted"]
    mol, _, W, ns, forced = cond.case_inputs(name)
    assert o["decisions"].shape == (ns, int(np.sum(mol.nelec)), W) and o["decisions"][list(forced)].all()
    assert 0.2 < o["decisions"].mean() < 0.95


def test_cluster_fixture_belongs_to_these_inputs():
    """The committed oracle side of the cluster case is the trajectory of today's inputs: its first sweeps, run live (the whole chain takes
    ~9 s), give the fixture's decisions."""
    g = cond.oracle_case("cluster-1e-5")
    live = cond.oracle_run("cluster-1e-5", nsteps=2)
    assert np.array_equal(live["decisions"], g["decisions"][:2])
    assert cond.unforced_min_margin(live, ()) >= g["min_margin"]


def test_summation_order_spread():
    """What two float64 evaluations of ONE chain differ by: the oracle on water-1e-5 (20 sweeps, forced sweep 5) with the occupied orbital
    columns in six other orders — the same wave function, every sum over orbitals in another order.  Decisions identical; the chain errors
    of the permuted runs lie within 0.5 .. 2.6 times the original's (measured, with the 100-sweep cases' 0.6 .. 2.8 of
    test_case_is_ill_conditioned_and_far_from_ties).  The GPU tests allow the device 8 times the oracle's own error: a factor ~3 of such
    spread either way, and the device's fused multiply-adds and AO rounding on top.  Asserted here: the spread stays inside that 8."""
    base = cond.oracle_run("water-1e-5", nsteps=20)
    _, mf, *_ = cond.case_inputs("water-1e-5")
    lo, hi, dx = np.inf, 0.0, 0.0
    for seed in range(1, 7):
        p = cond.oracle_run("water-1e-5", mf=cond.permuted_mf(mf, seed), nsteps=20)
        assert np.array_equal(p["decisions"], base["decisions"])
        r = [p[k] / base[k] for k in ("inv", "log", "q0m1")]
        lo, hi, dx = min(lo, *r), max(hi, *r), max(dx, float(np.max(np.abs(p["x"] - base["x"]))))
    print(f"[conditioning] summation-order spread: chain-error ratios {lo:.2f} .. {hi:.2f}, final coordinates differ by {dx:.2e} bohr")
    assert 1 / 8 < lo and hi < 8
    assert 0.0 < dx < 1e-8
    for name in cond.LIVE:
        o = cond.oracle_case(name)
        assert all(1 / 8 < o["spread_" + k] < 8 for k in ("inv", "log", "q0m1")), name


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
    log|Psi| of the same size shows likewise."""
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
