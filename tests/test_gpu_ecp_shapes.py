"""The ECP row of the energy pass on the shapes of tests/sweep_shapes.py (f-shell bases, n_up != n_dn, an empty spin channel, more than 32
atoms, uneven orbital-tile counts) and on the two ill-conditioned water cases of tests/conditioning.py after their 100-sweep chain, through
every route of energy_plan (csrc/pqa_energy.hip), against the oracle's ecp_ea at the device's own coordinates.  The cases, the
pseudopotential table under which hydrogen's non-local channel counts, the ECP tapes, the measure max_w |dev - oracle| / max(1, A_w) and the
yardstick are tests/ecp_shapes.py; test_ecp_shapes_cpu.py pins that the inputs test something.  The device may be MARGIN = 8 times the
yardstick (test_conditioning_cpu.py::test_summation_order_spread, through test_gpu_sweep_shapes.MARGIN).  13 walkers (three full
four-walker blocks of the list passes and a partial one), periodic cells 4; thresholds -1 (every point) and 10.

Which route ran is asserted from the ``[pqa] energy route:`` lines under PQA_RES_DEBUG; the route tables below are read from energy_plan.  The
standalone entry ``energy()`` works on the walker-major state whatever ran before it (pqa_energy: sync_aos, no ``soa_current``): it is the
walker-major route, also behind a sweep.  The routes that read the planes a sweep leaves (column = k_ecp_orbcol, rows with the point pass
on planes, accum x4 / x1, lists first) are reached through the sweep's own energy stage only, ``vmc_sweeps(..., energy=True, ecp_rot=,
ecp_unif=)`` — where jsx_current / coords_sweep is taken — so every after-sweep case runs through that call and reads the last step's rows
from ``energy_last()``; the evaluations of steps 2 .. ns are deferred ones (point totals left on the device).  Every open single-determinant
case fits the column route (h36: 47 744 B of the 64 KB bound), so no case needs a replacement; the multi-determinant handles have no
lane-per-walker sweep, their route behind k_sweep_ww is accum on the walker-major state.

Every ratio is printed and written to $PQA_TEST_REPORT_DIR/parity_report_ecp_shapes.json; DESIGN.md section 54 has the measured table.
Measured on an MI355X, largest device / yardstick ratio per route: walker-major 1.5 (water-f), column 3.8, rows with the point pass on
planes 3.8, accum x4 3.8, accum x1 3.8, lists first 3.8, batched 3.9 (all w4f-1715 at the deterministic mask, where the routes differ
from each other by 0.006: the oracle's own error at those coordinates); the conditioning cases 0.05 (water-1e-5) and 0.02 (water-1e-7);
the routes of a case against each other at most 0.24 (h-atom); periodic 0.04 (cubic-f) and 0.24 (c3-f).
"""

import json
import os

import numpy as np
import pytest

import ecp_shapes as es
import test_gpu_energy_route as er
from test_gpu_sweep_shapes import MARGIN

pytestmark = pytest.mark.gpu

SWITCHES = {"default": {}, "point_lw0": {"PQA_ECP_POINT_LW": "0"}, "wave": {"PQA_ECP_WAVE": "1"},
            "wave_acc1": {"PQA_ECP_WAVE": "1", "PQA_ECP_ACC_WAVES": "1"}, "lds0": {"PQA_ECP_LDS": "0"}}
WALKER_MAJOR = er.route("coulomb x4", "lds", "rows", "point walker-major")
# the route of the sweep's energy stage per switch setting: open single-determinant handles (lane-per-walker sweeps: the planes are live)
OPEN_ROUTES = {"default": er.route("lw", "lds", "column", "point_lw"), "point_lw0": er.route("lw", "lds", "rows", "point on planes"),
               "wave": er.route("lw", "lds", "rows", "accum x4"), "wave_acc1": er.route("lw", "lds", "rows", "accum x1"),
               "lds0": er.route("lw", "first", "column", "point_lw")}
# multi-determinant handles: wave-per-walker accumulation on the walker-major state, standalone and behind k_sweep_ww
MD_WALKER_MAJOR = er.route("coulomb x4", "lds", "rows", "accum x4")
MD_ROUTES = {"default": MD_WALKER_MAJOR, "wave_acc1": er.route("coulomb x1", "lds", "rows", "accum x1")}
PBC_WALKER_MAJOR = {"cubic-f": er.route("coulomb x4", "lds nseg=8", "rows", "point walker-major"),
                    "c3-f": er.route("complex coulomb x4", "lds nseg=8", "rows", "complex accum x4")}
PBC_ROUTES = {("cubic-f", "default"): er.route("periodic lw", "lds nseg=8", "rows", "point_lw"),
              ("cubic-f", "point_lw0"): er.route("periodic lw", "lds nseg=8", "rows", "point on planes"),
              ("c3-f", "default"): er.route("periodic complex lw", "lds nseg=8", "rows", "complex point_lw"),
              ("c3-f", "point_lw0"): er.route("periodic complex lw", "lds nseg=8", "rows", "complex accum x4")}
_report = {}


def note(key, value):
    _report[key] = float(value)
    print(f"[ecp_shapes] {key} = {float(value):.4g}")
    return value


@pytest.fixture(scope="module", autouse=True)
def _write_report():
    yield
    out = os.environ.get("PQA_TEST_REPORT_DIR")
    if out:
        os.makedirs(out, exist_ok=True)
        with open(os.path.join(out, "parity_report_ecp_shapes.json"), "w") as f:
            json.dump(_report, f, indent=1, sort_keys=True)


def _check(ratios, allowance=1.0):
    """All figures are noted before any is asserted."""
    bad = {k: v for k, v in ratios.items() if not v <= allowance * MARGIN}
    assert not bad, bad


def _routes(capfd):
    out, err = capfd.readouterr()
    print(out + err, end="")
    return [line[len(er.ROUTE):] for line in err.splitlines() if line.startswith(er.ROUTE)]


def expected_routes(name, switch):
    """The route lines of ``_run``'s handle, in order (a line is printed whenever the route is not the handle's last one)."""
    if name in es.MD_CASES:
        return [MD_ROUTES[switch]] if switch != "default" else [MD_WALKER_MAJOR]  # standalone and behind the sweep: the same line, once
    sweep = OPEN_ROUTES[switch]
    return [WALKER_MAJOR, sweep] * len(es.THRESHOLDS) + [WALKER_MAJOR] if switch == "default" else [sweep]


# ---------------------------------------------------------------- one handle per (case, switch setting), run once per module
_runs = {}


def _run(name, switch, capfd):
    """-> {"routes", "start": {thr: (row, points)} (default setting: ``energy`` at the start coordinates, tape step 0), "sweep": {thr:
    (row, points)} (the last step's rows of ``vmc_sweeps(energy=True)`` on the tapes), "after": {thr: (row, points)} (default setting:
    ``energy`` behind those sweeps, tape step ns - 1), "x": the final coordinates (the same bits for both thresholds)}."""
    if (name, switch) in _runs:
        return _runs[(name, switch)]
    c = es.case(name)
    start, gauss, unif, tstep = c.tapes()
    rot, eun = es.ecp_tapes(name)
    capfd.readouterr()
    out = {"start": {}, "sweep": {}, "after": {}}
    with er.environment(**SWITCHES[switch]):
        wf = c.gpu_wf()
        dev = wf.fused_device()
        assert dev.necp == es.necp(c.mol)
        xs = []
        for thr in es.THRESHOLDS:
            wf.recompute(start)
            if switch == "default":
                out["start"][thr] = (np.array(dev.energy(thr, rot=rot[0], unif=eun[0])[3]), dev.last_ecp_points())
            dev.vmc_sweeps(tstep, c.ns, gauss=gauss, unif=unif, threshold=thr, ecp_rot=rot, ecp_unif=eun, energy=True)
            out["sweep"][thr] = (np.array(dev.energy_last()[3]), dev.last_ecp_points())
            xs.append(dev.configs())
        assert np.array_equal(xs[0], xs[1])  # the chain does not depend on the threshold
        if switch == "default":
            for thr in es.THRESHOLDS:
                out["after"][thr] = (np.array(dev.energy(thr, rot=rot[-1], unif=eun[-1])[3]), dev.last_ecp_points())
    out["x"], out["routes"] = xs[0], _routes(capfd)
    _runs[(name, switch)] = out
    return out


def _judge(name, key, rows, x, step):
    """{threshold tag: measure / yardstick} of the rows ``{thr: (row, points)}`` against the oracle at ``x`` on tape step ``step``."""
    y = es.yardstick(name)
    note(f"{name}_yardstick", y)
    r = {}
    for thr, (row, _) in rows.items():
        o = es.oracle_at(name, x, thr, step)
        m = note(f"{name}_{key}_{es.tag(thr)}", es.measure(row, o))
        r[es.tag(thr)] = note(f"{name}_{key}_{es.tag(thr)}_over_yardstick", m / y)
    return r


# ---------------------------------------------------------------- (a) the walker-major route
@pytest.mark.parametrize("name", es.LIVE_CASES)
def test_walker_major_route_against_the_oracle(name, capfd):
    """``recompute(start)``, then ``energy(thr, rot=, unif=)`` for thr = -1 and 10: coulomb x4 / lds / rows / point walker-major
    (multi-determinant handles: accum x4).  Row 3 against oracle_ecp at the start coordinates."""
    d = _run(name, "default", capfd)
    assert d["routes"] == expected_routes(name, "default"), d["routes"]
    _check(_judge(name, "walker_major", d["start"], es.case(name).tapes()[0].configs, 0))


@pytest.mark.parametrize("name", es.LIVE_CASES + es.COND_CASES)
def test_walker_major_route_behind_the_sweeps(name, capfd):
    """The same entry behind the case's sweeps — the walker-major state converted back from the planes the sweep leaves, an updated
    inverse (the conditioning cases: 100 sweeps at cond(D) 3e6 and 3e8) — against the oracle at the device's final coordinates."""
    d = _run(name, "default", capfd)
    assert d["routes"] == expected_routes(name, "default"), d["routes"]
    _check(_judge(name, "walker_major_after_sweeps", d["after"], d["x"], es.case(name).ns - 1))


# ---------------------------------------------------------------- (b), (c), (d) the routes of the sweep's energy stage
def _sweep_params():
    out = [(n, s) for n in es.OPEN_CASES for s in SWITCHES]
    out += [(n, s) for n in es.MD_CASES for s in MD_ROUTES]
    return out + [(n, s) for n in es.COND_CASES for s in ("default", "point_lw0")]


@pytest.mark.parametrize("name,switch", _sweep_params())
def test_sweep_stage_routes_against_the_oracle(name, switch, capfd):
    """The case's sweeps on its tapes with the energy stage on (ECP tapes replayed), per switch setting: column (k_ecp_orbcol), rows with
    the point pass on planes, accum x4, accum x1, lists first; multi-determinant handles accum x4 and x1 behind k_sweep_ww; the two
    conditioning cases column and rows after 100 sweeps of Sherman-Morrison updates at cond(D) 3e6 and 3e8.  Row 3 of the last step's
    ``energy_last()`` against oracle_ecp at the device's own final coordinates, thresholds -1 and 10."""
    d = _run(name, switch, capfd)
    assert d["routes"] == expected_routes(name, switch), d["routes"]
    _check(_judge(name, f"sweep_{switch}", d["sweep"], d["x"], es.case(name).ns - 1))


@pytest.mark.parametrize("name", es.OPEN_CASES + es.MD_CASES + es.COND_CASES)
def test_routes_agree_pairwise(name, capfd):
    """The rows of a case's routes at the same final coordinates (bit for bit the same: the switches do not touch the sweeps) against
    each other, within the sum of their two allowances."""
    switches = [s for n, s in _sweep_params() if n == name]
    runs = {s: _run(name, s, capfd) for s in switches}
    y, r = es.yardstick(name), {}
    rows = {s: runs[s]["sweep"] for s in switches}
    rows["walker_major"] = runs["default"]["after"]
    for s in switches[1:]:
        assert np.array_equal(runs[s]["x"], runs["default"]["x"]), s
    keys = list(rows)
    for thr in es.THRESHOLDS:
        o = es.oracle_at(name, runs["default"]["x"], thr, es.case(name).ns - 1)
        for i, p in enumerate(keys):
            for q in keys[i + 1:]:
                key = f"{p}_vs_{q}_{es.tag(thr)}"
                r[key] = note(f"{name}_{key}_over_yardstick", es.measure_pair(rows[p][thr][0], rows[q][thr][0], o) / y)
    _check(r, allowance=2.0)


# ---------------------------------------------------------------- (e) point counts
@pytest.mark.parametrize("name", es.LIVE_CASES)
def test_point_counts(name, capfd):
    """``last_ecp_points()`` at the deterministic mask: at most the oracle's count (every point of every pair), at least the oracle's count
    over the pairs with a term above 1e-20 (the device leaves out an atom beyond the range where all its terms are below 1e-22), equal
    to it where no pair is out of range; at threshold 10, where only pairs far inside the range pass, equal."""
    c = es.case(name)
    bad = {}
    for switch in [s for n, s in _sweep_params() if n == name]:
        d = _run(name, switch, capfd)
        for key, x, step in (("start", c.tapes()[0].configs, 0), ("sweep", d["x"], c.ns - 1), ("after", d["x"], c.ns - 1)):
            for thr, (_, pts) in d[key].items():
                o = es.oracle_at(name, x, thr, step)
                hi, lo = int(o["points"].sum()), int(o["points_seen"].sum())
                note(f"{name}_{switch}_{key}_{es.tag(thr)}_points", pts), note(f"{name}_{switch}_{key}_{es.tag(thr)}_oracle_points", hi)
                ok = lo <= pts <= hi and (pts == hi if o["pairs_out"] == 0 or thr > 0 else True)
                if not ok:
                    bad[(switch, key, thr)] = (lo, pts, hi)
    assert not bad, bad


def test_every_route_is_reached_by_every_shape():
    """Each of walker-major, column, rows on planes, accum x4, accum x1, lists first and batched is run by an f-shell case, an n_up != n_dn
    case, a natom > 32 case and a one-electron case (no replacement is needed: every open case takes every switch setting)."""
    import sweep_shapes as ss

    params = _sweep_params()
    for switch in SWITCHES:
        names = [n for n, s in params if s == switch and n in es.OPEN_CASES]
        mols = [es.case(n).mol for n in names]
        assert any(ss.highest_l(m) == 3 for m in mols) and any(m.nelec[0] != m.nelec[1] for m in mols)
        assert any(m.natm > 32 for m in mols) and any(sum(m.nelec) == 1 for m in mols)
    # the batched integrator holds one ECP atom per lane and a table of every atom's points per electron: one electron has nothing to
    # select from (6 points, 6 kept), its line — N = 1 and the empty spin channel of the list pass — is the walker-major route's h-atom
    mols = [es.case(n).mol for n in es.BATCHED_CASES]
    assert any(ss.highest_l(m) == 3 for m in mols) and any(m.nelec[0] != m.nelec[1] for m in mols) and any(m.natm > 32 for m in mols)


# ---------------------------------------------------------------- (f) the batched integrator
BATCHED_ROUTE = er.route("coulomb x4", "batched", "rows", "point walker-major")


@pytest.mark.parametrize("name", es.BATCHED_CASES)
def test_batched_integrator(name, capfd):
    """``EnergyAccumulator(use_old_ecp=False)`` (six points an atom, the six likeliest of an electron's table kept, one of the others
    sampled) against oracle/ecp_batched.py with the rotations and selection uniforms replayed, at the start coordinates and behind the
    case's sweeps: the ECP row in the measure of the other tests, and the T-move tables of ``ecp_batched_moves`` for the first and the
    last electron of each spin — positions to 1e-12 as test_batched_ecp_golden asks, weights as max |dev - oracle| / max(1, sum_l
    |e^{-tau v_l} - 1| P_l) in units of the yardstick."""
    import pyqmc_amd as pa

    c = es.case(name)
    start, gauss, unif, tstep = c.tapes()
    rot, sel, tm_rot, tm_sel = es.batched_tapes(name)
    naip, nsd, nsr = es.batched_rule(c.mol)
    y = note(f"{name}_yardstick", es.yardstick(name))
    capfd.readouterr()
    r, dpos = {}, {}
    with er.environment():
        wf = c.gpu_wf()
        dev = wf.fused_device()
        acc = pa.EnergyAccumulator(c.mol, use_old_ecp=False)
        assert np.array_equal(acc.ecp.naip, naip) and (acc.ecp.nselect_deterministic, acc.ecp.nselect_random) == (nsd, nsr)
        assert nsd + nsr < naip.sum()  # points are dropped: the selection runs
        for key in ("start", "after_sweeps"):
            wf.recompute(start)
            if key == "after_sweeps":
                dev.vmc_sweeps(tstep, c.ns, gauss=gauss, unif=unif, energy=False)
            cfg = c.configs(dev.configs())
            o = es.batched_at(name, cfg.configs)
            row = acc(cfg, wf, rot=rot, unif=sel)["ecp"]
            r[key] = note(f"{name}_batched_{key}_over_yardstick", note(f"{name}_batched_{key}", es.measure(row, o)) / y)
            acc.ecp.bind(dev)
            try:
                for e in es.tmove_electrons(c.mol):
                    weight, pos = dev.ecp_batched_moves(e, es.BATCHED_TAU, tm_rot[e], np.ascontiguousarray(tm_sel[e]))
                    w_o, pos_o, scale = o["tmoves"][e]
                    assert weight.shape == w_o.shape == (c.W, nsd + nsr)
                    dpos[(key, e)] = note(f"{name}_batched_{key}_tmove{e}_positions", float(np.max(np.abs(pos - pos_o)) / np.max(np.abs(pos_o))))
                    m = float(np.max(np.abs(weight - w_o) / np.maximum(1.0, scale)))
                    r[f"{key}_tmove{e}"] = note(f"{name}_batched_{key}_tmove{e}_weights_over_yardstick", m / y)
            finally:
                dev.set_ecp_batched(None)
    assert _routes(capfd) == [BATCHED_ROUTE]
    assert all(v < 1e-12 for v in dpos.values()), dpos
    _check(r)


# ---------------------------------------------------------------- (g) periodic cells with f shells
@pytest.mark.parametrize("name", es.PBC_CASES)
def test_periodic_routes(name, capfd):
    """cubic-f (real, lds nseg=8, Ewald) and c3-f (twisted, the complex point pass), 4 walkers.  The walker-major route at the
    coordinates and wrap counters of the fixture g52 against the oracle rows of g53 (complex for c3-f).  The routes of the sweep's energy
    stage (periodic [complex] lw / point_lw, and PQA_ECP_POINT_LW=0) against the walker-major route at the device's own final coordinates
    (``recompute``, then ``energy`` with the same tapes), within the two allowances summed: a fixture cannot follow the device's
    last-digit coordinates."""
    import sweep_shapes as ss
    from pyqmc_amd.vmc import _fetch

    c, g = es.case(name), ss.oracle_case(name)
    start, gauss, unif, tstep = c.tapes()
    rot, eun = es.ecp_tapes(name)
    y = note(f"{name}_yardstick", es.yardstick(name))
    r, r2, routes = {}, {}, {}
    for switch in ("default", "point_lw0"):
        capfd.readouterr()
        with er.environment(**SWITCHES[switch]):
            wf = c.gpu_wf()
            dev = wf.fused_device()
            dev.set_ewald(10, 1)
            for thr in es.THRESHOLDS:
                o = es.pbc_oracle(name, thr)
                if switch == "default":
                    wf.recompute(c.configs(g["x"], g["wrap"]))
                    row = dev.energy(thr, rot=rot[0], unif=eun[0])[3]
                    assert int(o["points_seen"].sum()) <= dev.last_ecp_points() <= int(o["points"].sum())
                    m = note(f"{name}_walker_major_{es.tag(thr)}", es.measure(row if c.complex else np.real(row), o))
                    r[f"walker_major_{es.tag(thr)}"] = note(f"{name}_walker_major_{es.tag(thr)}_over_yardstick", m / y)
                wf.recompute(start)
                dev.vmc_sweeps(tstep, c.ns, gauss=gauss, unif=unif, threshold=thr, ecp_rot=rot, ecp_unif=eun, energy=True)
                row_s = np.array(dev.energy_last()[3])
                cfg = start.copy()
                _fetch(dev, cfg)
                assert np.array_equal(cfg.wrap, g["wrap"]) and np.max(np.abs(cfg.configs - g["x"])) < 1e-8
                wf.recompute(cfg)
                row_w = dev.energy(thr, rot=rot[-1], unif=eun[-1])[3]
                key = f"{switch}_vs_walker_major_{es.tag(thr)}"
                r2[key] = note(f"{name}_sweep_{key}_over_yardstick", es.measure_pair(row_s, row_w, o) / y)
        routes[switch] = _routes(capfd)
    wm = PBC_WALKER_MAJOR[name]
    assert routes["default"] == [wm, PBC_ROUTES[(name, "default")], wm, PBC_ROUTES[(name, "default")], wm], routes
    assert routes["point_lw0"] == [PBC_ROUTES[(name, "point_lw0")], wm, PBC_ROUTES[(name, "point_lw0")], wm], routes
    _check(r)
    _check(r2, allowance=2.0)
