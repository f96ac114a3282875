"""The fused sweeps on the shapes no other system of the suite reaches: a basis whose highest shell is f (the LMAX = 3 instantiations of
k_sweep_r8, k_sweep_res and k_sweep_ww, and k_sweep_ww<5>), n_up != n_dn, an empty spin channel, different orbital-tile counts per
spin, more than 32 atoms, species whose atoms fill one work item and part of another, the default route of 16 .. 31 electrons per spin.
The cases and their oracle side are tests/sweep_shapes.py (13 walkers, 3 sweeps, sweep 1 forced; periodic cases: 4 walkers, 2 sweeps,
fixture g52_sweep_shapes); test_sweep_shapes_cpu.py pins the shapes and shows that no decision of the oracle is within 1e-6 of a tie, so
no walker is excused anywhere.  Which kernel ran is asserted from the route every handle reports under PQA_RES_DEBUG, or from the
profiler's bracket counts (k_sweep_ww).

The yardstick of a device figure is sweep_shapes.yardstick: the oracle's own figure on the same chain, floored at cond(D) * 2.2e-16 (the
coordinates: what two float64 oracle runs differ by, with a floor only for h-atom and h-atom-df, whose two runs are the same run); the
device may be MARGIN = 8 times that (test_conditioning_cpu.py::test_summation_order_spread).  Every figure is printed and written to
$PQA_TEST_REPORT_DIR/parity_report_sweep_shapes.json where that is set; DESIGN.md section 50 has the measured table.  Measured on an
MI355X, largest device / oracle ratio: 5.7 through k_sweep_r8, 6.3 through k_sweep_res, 4.0 through the launch-per-move sweep (all
three on w4f-1715's log|Psi| or h-atom-df's kinetic rows), 3.7 in the DMC chains, 1.8 through k_sweep_ww, 1.9 in the periodic cells; largest coordinate ratio 2.9 (h33s, k_sweep_r8).

h36 and h36-1917 are outside k_sweep_r8's scope: r8_setup (pqa_res8.hip) refuses them at ``h->r8.lds > 80 * 1024`` — the two-tile
partials take 59 136 B and 36 atoms with 15 work items 27 088 B.  Through k_sweep_r8, forced and by default, their line (natom > 32:
the second ion pass and the clamp of ion-less lanes; four full work items and a partial one; two tiles per spin) is hit by h33s and
h33s-1917, 33 atoms with one s function each (81 904 B); h36 and h36-1917 themselves run k_sweep_res and the launch-per-move sweep.
h-atom is outside k_sweep_res's scope: res_setup (pqa_res.hip) takes no basis below 20 padded rows (``kt_cap < 20``; 5 AOs are one
16-row chunk).  Through k_sweep_res N = 1 and the empty spin channel are hit by h-atom-df, the same atom with a d and an f shell (17
AOs).  c3-f has the carbon table s, s, p, f (96 AOs) and not cubic-f's 160: a twisted cell's tile holds 2 nao rows, of which res_setup
takes at most 256 (``rows4 <= rows_cap``) within 160 KB of LDS.
"""

import json
import os

import numpy as np
import pytest

import conditioning as cond
import helpers
import sweep_shapes as ss
from pyqmc_amd.configs import OpenConfigs

pytestmark = pytest.mark.gpu

MARGIN = 8.0
PATHS = dict(cond.PATHS, default={})  # default: no switch set
ROUTE = {"r8": ("[pqa_res8]", "k_sweep_r8"), "default": ("[pqa_res8]", "k_sweep_r8"), "res16": ("[pqa_res]", "k_sweep_res"),
         "launches": ("", "k_step_lw")}
_report = {}


def note(key, value):
    _report[key] = float(value)
    print(f"[sweep_shapes] {key} = {float(value):.4g}")
    return value


@pytest.fixture(scope="module", autouse=True)
def _write_report():
    yield
    out = os.environ.get("PQA_TEST_REPORT_DIR")
    if out:
        os.makedirs(out, exist_ok=True)
        with open(os.path.join(out, "parity_report_sweep_shapes.json"), "w") as f:
            json.dump(_report, f, indent=1, sort_keys=True)


def _handle(c, env, monkeypatch):
    for k in ("PQA_RES", "PQA_R8", "PQA_LW", "PQA_WW"):
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)  # read when the handle is created
    monkeypatch.setenv("PQA_RES_DEBUG", "1")
    wf = c.gpu_wf()
    return wf, wf.fused_device()


def _assert_only_route(err, path):
    """The resident sweep's setup accepted the system (it reports its plan) and every sweep ran the kernel the path names."""
    tag, kernel = ROUTE[path]
    assert tag in err, err
    routes = cond.reported_routes(err)
    assert routes and set(routes) == {kernel}, routes


def _state(c, wf, dev):
    """``conditioning.device_state_all`` that leaves an empty spin channel alone."""
    ph, lg = dev.value()
    sl = wf.wf_factors[0]
    return [sl._get_state(s)[0] if c.mol.nelec[s] else np.zeros((c.W, 1, 0, 0)) for s in (0, 1)], ph, lg


def _check(ratios):
    """All figures are noted before any is asserted."""
    bad = {k: v for k, v in ratios.items() if not v <= MARGIN}
    assert not bad, bad


def _ratios(c, o, tag, inv, phase, logpsi, cfg, rows=None):
    """The device's chain errors (and the rows of its energy pass) in units of sweep_shapes.yardstick, noted; -> {key: ratio}."""
    from oracle import energy as oen

    err = c.judge(inv, phase, logpsi, cfg)
    dev_err = cond.summary(err)
    note(f"{tag}_cond", err["cond"].max())
    r = {}
    for k in dev_err:
        note(f"{tag}_{k}", dev_err[k])
        r[k] = note(f"{tag}_{k}_over_oracle", dev_err[k] / ss.yardstick(o, k))
    r["x"] = note(f"{tag}_x_over_oracle_spread", float(np.max(np.abs(cfg.configs - o["x"]))) / ss.yardstick(o, "x"))
    if rows is not None:
        ke_f, g2_f = c.fresh_kinetic(cfg)
        r["ke"] = note(f"{tag}_ke_rows_over_oracle", cond.rel_rows(rows[0], ke_f) / ss.yardstick(o, "ke_upd_vs_fresh"))
        r["grad2"] = note(f"{tag}_grad2_rows_over_oracle", cond.rel_rows(rows[4], g2_f) / ss.yardstick(o, "grad2_upd_vs_fresh"))
        if not c.periodic:  # the Coulomb rows do not read the wave function: the oracle's updated-against-fresh difference is 0, the floor counts
            ee, ei, _ = oen.coulomb(c.mol, cfg)
            r["ee"] = note(f"{tag}_ee_rows_over_oracle", cond.rel_rows(rows[1], ee) / ss.yardstick(o, "ee"))
            r["ei"] = note(f"{tag}_ei_rows_over_oracle", cond.rel_rows(rows[2], ei) / ss.yardstick(o, "ei"))
    return r


# ---------------------------------------------------------------- (a) chains against the oracle, (b) the routes against each other
_chains = {}


def _chain(name, path, monkeypatch, capfd):
    """One device chain of an open case through one route, run once per module: decisions, state, energy rows, the reported routes."""
    if (name, path) not in _chains:
        c = ss.case(name)
        wf, dev = _handle(c, PATHS[path], monkeypatch)
        start, gauss, unif, tstep = c.tapes()
        wf.recompute(start)
        _, _, rec = dev.vmc_sweeps(tstep, c.ns, gauss=gauss, unif=unif, energy=False, record=True)
        rows = np.real(dev.energy(10.0, seed=9))
        out, err = capfd.readouterr()
        print(out + err, end="")
        inv, phase, logpsi = _state(c, wf, dev)
        _chains[(name, path)] = {"rec": rec, "rows": rows, "x": dev.configs(), "inv": inv, "phase": phase, "logpsi": logpsi, "stderr": err}
    return _chains[(name, path)]


def _chain_params():
    """Every open case through the three routes, except the pairs of sweep_shapes.REPLACEMENT (module docstring: the replacements take
    their place there); the default route, no switch set, on the two shapes with 16 .. 31 electrons per spin."""
    out = [(n, p) for n in ss.OPEN_CASES for p in cond.PATHS if (n, p) not in ss.REPLACEMENT]
    return out + [(ss.REPLACEMENT.get((n, "default"), n), "default") for n in ss.DEFAULT_ROUTE_CASES]


@pytest.mark.parametrize("name,path", _chain_params())
def test_chain_on_tapes_against_the_oracle(name, path, monkeypatch, capfd):
    """3 sweeps on the oracle's tapes (sweep 1 forced), no recompute, then the standalone energy pass.  The route ran the kernel it names.
    Every decision is the oracle's.  In units of the yardstick, each <= 8: the inverse of both spins against a refined inverse of the
    oracle's Slater matrix at the device's coordinates, the resident log|Psi| against a fresh one, max |q_e - 1|; the coordinates in units
    of what two float64 oracle runs (occupied columns permuted) differ by; the ke, ee, ei and grad2 rows against the oracle on a fresh
    state at the device's coordinates, in units of the oracle's updated-against-fresh difference."""
    c, o = ss.case(name), ss.oracle_case(name)
    d = _chain(name, path, monkeypatch, capfd)
    tag = f"{name}_{path}"
    _assert_only_route(d["stderr"], path)
    for k in ss.SCALARS:
        note(f"{name}_oracle_{k}", o[k])  # the yardsticks themselves
    same = d["rec"] == o["decisions"]
    note(f"{tag}_decisions_equal", same.mean())
    assert same.all(), (int((~same).sum()), np.argwhere(~same)[:4].tolist())
    _check(_ratios(c, o, tag, d["inv"], d["phase"], d["logpsi"], c.configs(d["x"]), d["rows"]))


@pytest.mark.parametrize("name", list(ss.OPEN_CASES))
def test_routes_agree_pairwise(name, monkeypatch, capfd):
    """The routes of a case against each other (h36, h36-1917: k_sweep_res and the launch-per-move sweep; h-atom: k_sweep_r8 and the
    launch-per-move sweep; every other case all three): the same decisions, coordinates to 1e-10 relative, log|Psi| to 1e-9 — the bounds
    of test_gpu_jastrow_merge.py, no walker excused."""
    paths = [p for p in cond.PATHS if (name, p) not in ss.REPLACEMENT]
    runs = {p: _chain(name, p, monkeypatch, capfd) for p in paths}
    bad = {}
    for i, p in enumerate(paths):
        for q in paths[i + 1:]:
            a, b = runs[p], runs[q]
            flips = int((a["rec"] != b["rec"]).sum())
            dx = note(f"{name}_{p}_vs_{q}_x", helpers.relerr(a["x"], b["x"]))
            dl = note(f"{name}_{p}_vs_{q}_log", float(np.max(np.abs(a["logpsi"] - b["logpsi"]))))
            if flips or not dx < 1e-10 or not dl < 1e-9:
                bad[(p, q)] = (flips, dx, dl)
    assert not bad, bad


# ---------------------------------------------------------------- (c) the DMC instantiations with f shells
DMC_STEPS = 3
_dmc_oracle = {}


@pytest.mark.parametrize("path", ["r8", "res16"])
def test_dmc_chain_against_the_oracle(path, monkeypatch, capfd):
    """water-f, 13 walkers, 3 DMC steps at tstep 0.02 on device Philox draws through k_sweep_r8<true, 3> and k_sweep_res<true, 3>, replayed
    by the oracle's dmc_propagate — the conditions of test_gpu_conditioning.py::test_dmc_chain_against_the_oracle: per-step counts of
    accepted drift-diffusion moves exact (the oracle rejects some: 298 of 312 accepted; none of the T-move proposals of these three
    steps is accepted, on either side), coordinates < 1e-6, coordinates and weights in units of what two float64 oracle runs differ by
    and the chain errors in units of the oracle's own (no floor), each <= 8.  No walker is excused: the oracle's smallest |margin| on
    these draws is 6.7e-3."""
    c = ss.case("water-f")
    mol, mf, W = c.mol, c.mf, c.W
    wf, dev = _handle(c, PATHS[path], monkeypatch)
    start, *_ = c.tapes()
    x0 = np.array(start.configs)
    wf.recompute(start)
    w = np.ones(W)
    avg, acc = dev.dmc_steps(cond.DMC_TSTEP, DMC_STEPS, w, cond.DMC_BRANCHCUT, cond.DMC_ETRIAL, cond.DMC_ETRIAL, seed=cond.DMC_SEED)
    out, err = capfd.readouterr()
    _assert_only_route(err, path)
    if not _dmc_oracle:  # the draws depend on the seed alone: one oracle side for both paths
        t = dev.philox_dmc_tapes(cond.DMC_SEED, DMC_STEPS, W)
        _dmc_oracle["a"] = cond.oracle_dmc(mol, mf, x0, t)
        _dmc_oracle["b"] = cond.oracle_dmc(mol, cond.permuted_mf(mf, 1), x0, t)
    o, p = _dmc_oracle["a"], _dmc_oracle["b"]
    good = o["min_margin"] >= 1e-7
    tag = f"dmc_water-f_{path}"
    note(f"{tag}_walkers_excused", (~good).sum())
    note(f"{tag}_oracle_min_margin", o["min_margin"].min())
    note(f"{tag}_oracle_accepted_moves", o["accepted"][:, 0].sum()), note(f"{tag}_oracle_accepted_tmoves", o["accepted"][:, 1].sum())
    assert good.all()
    N = x0.shape[1]
    assert o["accepted"][:, 0].sum() < 0.999 * DMC_STEPS * N * W  # rejections do occur
    if good.all():
        assert np.array_equal(np.rint(acc * W * N), o["accepted"].sum(axis=2)), (acc * W * N, o["accepted"].sum(axis=2))
    x = dev.configs()
    inv, logpsi = cond.device_state(wf, dev)
    e = cond.chain_errors(cond.oracle_slater_matrix(helpers.oracle_wf(mol, mf)), inv, logpsi - cond.fresh_jastrow(mol, mf, x), x)
    assert np.max(np.abs(x - o["x"])[good]) < 1e-6  # every decision and T-move the oracle's
    r = {}
    sx = float(np.max(np.abs(p["x"] - o["x"])[good]))
    sw = float(np.max(np.abs(p["weights"] / o["weights"] - 1)[good]))
    r["x"] = note(f"{tag}_x_over_oracle_spread", float(np.max(np.abs(x - o["x"])[good])) / sx)
    r["weights"] = note(f"{tag}_weights_over_oracle_spread", float(np.max(np.abs(w / o["weights"] - 1)[good])) / sw)
    dev_err = {"inv": float(e["inv"][good].max()), "log": float(e["log"][good].max()), "q0m1": float(np.abs(e["q0m1"][good]).max())}
    note(f"{tag}_cond", e["cond"].max())
    for k in ("inv", "log", "q0m1"):
        note(f"{tag}_{k}", dev_err[k])
        note(f"{tag}_oracle_{k}", o[k])
        r[k] = note(f"{tag}_{k}_over_oracle", dev_err[k] / o[k])
    _check(r)


# ---------------------------------------------------------------- (d) walker independence
def test_walkers_that_share_a_block_are_independent(monkeypatch, capfd):
    """w4f-1715 (LMAX 3, two tiles of one spin and one of the other) through k_sweep_r8, once as it is and once with walkers and tapes
    permuted: per walker, after un-permuting, bit for bit the decisions, coordinates, log|Psi|, the inverse of both spins and the rows of
    the standalone energy pass — test_gpu_conditioning.py::test_walkers_that_share_a_block_are_independent on this shape."""
    c = ss.case("w4f-1715")
    start, gauss, unif, tstep = c.tapes()
    perm = np.random.default_rng(1).permutation(c.W)
    assert not np.array_equal(perm // 8, np.arange(c.W) // 8)
    outs, errs = [], ""
    for order in (np.arange(c.W), perm):
        wf, dev = _handle(c, PATHS["r8"], monkeypatch)
        wf.recompute(OpenConfigs(start.configs[order].copy()))
        _, _, rec = dev.vmc_sweeps(tstep, c.ns, gauss=gauss[:, :, order].copy(), unif=unif[:, :, order].copy(), energy=False, record=True)
        inv, _, logpsi = _state(c, wf, dev)
        got = {"rec": np.moveaxis(rec, 2, 0), "x": dev.configs(), "logpsi": logpsi, "inv_up": inv[0][:, 0], "inv_dn": inv[1][:, 0],
               "rows": np.real(dev.energy(10.0, seed=9))[[0, 1, 2, 4]].T}  # ke, ee, ei, grad2 (the ECP row draws its grid per walker index: test_gpu_ecp_shapes.py)
        back = np.argsort(order)
        outs.append({k: v[back] for k, v in got.items()})
        errs += capfd.readouterr()[1]
    _assert_only_route(errs, "r8")
    a, b = outs
    assert 0.1 < a["rec"].mean() < 1.0
    for k in a:
        diff = a[k] != b[k]
        note(f"independence_w4f-1715_r8_{k}_unequal", diff.sum())
        assert not diff.any(), (k, np.argwhere(diff)[:4].tolist())


# ---------------------------------------------------------------- (e) multi-determinant handles: k_sweep_ww<3> and <5>
def _sweep_launches(dev):
    """test_gpu_conditioning.py::_sweep_launches: (bracketed orbital launches, bracketed k_step_lw launches) since profile_enable."""
    dev.sync()
    n_orb, n_part = dev.profile_query()[0], dev.profile_query_part()[0]
    dev.profile_enable(False)
    return n_orb, n_part


@pytest.mark.parametrize("ww", ["1", "0"])
@pytest.mark.parametrize("name", list(ss.MD_CASES))
def test_multidet_chain_on_tapes_against_the_oracle(name, ww, monkeypatch):
    """H2O with an f shell on O (k_sweep_ww<3>) and C2 with f, g and h shells (k_sweep_ww<5>), six determinants, through the fused
    wave-per-walker sweep (PQA_WW=1: no orbital launch at all) and the k_propose -> orbitals -> k_accept launches (PQA_WW=0), against the
    oracle run live: every decision, and in units of the yardstick the inverse of EVERY unique determinant of both spins, log|Psi|,
    max |q_e - 1|, the coordinates and the ke and grad2 rows, each <= 8."""
    c, o = ss.case(name), ss.oracle_case(name)
    wf, dev = _handle(c, {"PQA_WW": ww}, monkeypatch)
    assert max(dev.ndet_s) > 1
    start, gauss, unif, tstep = c.tapes()
    wf.recompute(start)
    dev.profile_enable(True)
    _, _, rec = dev.vmc_sweeps(tstep, c.ns, gauss=gauss, unif=unif, energy=False, record=True)
    n_orb, n_part = _sweep_launches(dev)
    rows = np.real(dev.energy(10.0, seed=9))
    tag = f"{name}_ww{ww}"
    note(f"{tag}_bracketed_orbital_launches", n_orb)
    assert n_part == 0
    assert n_orb == 0 if ww == "1" else n_orb > c.ns  # k_sweep_ww did run (no orbital launch) / the launches did (one per move)
    for k in ss.SCALARS:
        note(f"{name}_oracle_{k}", o[k])
    same = rec == o["decisions"]
    note(f"{tag}_decisions_equal", same.mean())
    assert same.all(), (int((~same).sum()), np.argwhere(~same)[:4].tolist())
    inv, phase, logpsi = _state(c, wf, dev)
    r = _ratios(c, o, tag, inv, phase, logpsi, c.configs(dev.configs()), rows)
    _check(r)


# ---------------------------------------------------------------- (f) periodic cells with f shells
@pytest.mark.parametrize("res", ["1", "0"])
@pytest.mark.parametrize("name", list(ss.PBC_CASES))
def test_periodic_chain_on_tapes_against_the_oracle(name, res, monkeypatch, capfd):
    """The conventional diamond cell with an f shell on carbon, real (cubic-f) and twisted with complex coefficients (c3-f), 4 walkers,
    2 sweeps, through k_sweep_res<false, 3, PBC> / <false, 3, PBC, CX> (PQA_RES=1) and the launch-per-move sweep (PQA_RES=0) against the
    fixture g52: every decision and wrap counter, and in units of the yardstick the inverse, log|Psi|, the phase of Psi (c3-f),
    max |q_e - 1|, the folded coordinates and the ke and grad2 rows, each <= 8."""
    from pyqmc_amd.vmc import _fetch

    c, o = ss.case(name), ss.oracle_case(name)
    wf, dev = _handle(c, {"PQA_RES": res}, monkeypatch)
    dev.set_ewald(10, 1)
    start, gauss, unif, tstep = c.tapes()
    wf.recompute(start)
    _, _, rec = dev.vmc_sweeps(tstep, c.ns, gauss=gauss, unif=unif, energy=False, record=True)
    rows = np.real(dev.energy(10.0, seed=9))
    out, err = capfd.readouterr()
    print(out + err, end="")
    _assert_only_route(err, "res16" if res == "1" else "launches")
    assert dev.pbc and bool(dev.cplx) == c.complex
    tag = f"{name}_res{res}"
    for k in ss.SCALARS + (("phase",) if c.complex else ()):
        note(f"{name}_oracle_{k}", o[k])
    same = rec == o["decisions"]
    note(f"{tag}_decisions_equal", same.mean())
    assert same.all(), (int((~same).sum()), np.argwhere(~same)[:4].tolist())
    cfg = start.copy()
    _fetch(dev, cfg)
    wraps = cfg.wrap == o["wrap"]
    note(f"{tag}_wraps_equal", wraps.mean())
    inv, phase, logpsi = _state(c, wf, dev)
    r = _ratios(c, o, tag, inv, phase, logpsi, cfg, rows)
    assert wraps.all(), np.argwhere(~wraps)[:4].tolist()
    _check(r)
