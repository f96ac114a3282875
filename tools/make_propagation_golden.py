"""Fixture propagation_parent: everything the two propagation entries (pqa_vmc_sweeps, pqa_dmc_steps) and the per-step DMC loops of
pyqmc_amd.dmc return on small cases that reach every branch of their host code, and after each call the resident walkers, the wave
function's value, the last energy rows and (periodic handles) the wrap increments (tests/test_gpu_propagation_parent.py replays the
same calls and compares bit for bit).  Record it on the GPU from a tree of the commit BEFORE the two entries got their one call
prologue (StepCall), one MoveBuf builder and the T-move phase as functions, with that tree's library and Python; only public functions
are used, so the file runs unchanged in both:

    python tools/make_propagation_golden.py --tree <parent tree> --out tests/golden/propagation_parent.npz

--tapes records, without a GPU, the replay tapes that tree's pyqmc_amd.dmc draws (tests/golden/dmc_tapes_parent.npz,
tests/test_dmc_tapes_cpu.py)."""
import os
import sys

import numpy as np

TSTEP, DMC = 0.3, dict(tstep=0.5, branchcut=5.0)
SWITCHES = ("PQA_RES", "PQA_R8", "PQA_LW", "PQA_WW")  # read when a handle is created (tests/test_gpu_sweep_route.py)
ROUTES = {"r8": {"PQA_RES": "1", "PQA_R8": "1"}, "res": {"PQA_RES": "1", "PQA_R8": "0"}, "lw": {"PQA_RES": "0"},
          "ww": {"PQA_LW": "0", "PQA_WW": "1"}, "launches": {"PQA_LW": "0", "PQA_WW": "0"}, None: {}}
SELECTIONS = {"sel6_3": dict(nselect_deterministic=6, nselect_random=3),  # drops points, nsr > 0: selection uniforms
              "all": dict(nselect_deterministic=24, nselect_random=0)}    # drops none: no ecp_unif / tm_unif tapes
_cache = {}


def system(name, route=None):
    """(mol, wave function on a handle created under the route's switches, e_trial), built once per (system, route)."""
    import pyqmc_amd as pa
    from pyqmc_amd import systems
    from tests import helpers

    if (name, route) in _cache:
        return _cache[name, route]
    saved = {k: os.environ.pop(k, None) for k in SWITCHES}
    os.environ.update(ROUTES[route])
    e_trial = -17.0
    if name == "water":  # ECP, 4 + 4 electrons
        mol = systems.water()
        wf = helpers.gpu_wf(mol, systems.random_mf(mol))
    elif name == "general":  # all-electron water: necp = 0
        mol, e_trial = systems.water_general(), -60.0
        wf = pa.generate_wf(mol, systems.random_mf(mol))
    elif name == "water4":  # 4 determinants: the wave-per-walker kernels, k_tm_walker alone
        mol = systems.water()
        mf = systems.random_mf(mol, nvirt=6)
        wf = helpers.gpu_wf(mol, mf, systems.random_determinants(mol, mf, 4))
    elif name == "water3b":  # three-body factor
        mol = systems.water()
        wf = helpers.gpu_wf3(mol, systems.random_mf(mol))
    elif name == "waterb":  # s, p, d channels on oxygen: the system of the batched-integrator tests
        mol = systems.water_multichannel()
        wf = helpers.gpu_wf(mol, systems.random_mf(mol))
    elif name == "gamma":  # diamond primitive cell at Gamma
        mol, wf = helpers.gpu_pbc_wf("gamma")
        e_trial = -10.0
    else:  # complex Bloch coefficients (3 x 1 x 1 cell) / twisted primitive cell
        mol, wf = helpers.gpu_pbc_wf(None, case=helpers.pbc_complex_case() if name == "complex" else helpers.twist_case("prim"))
        e_trial = -30.0 if name == "complex" else -10.0
    wf.fused_device()
    for k in SWITCHES:
        os.environ.pop(k, None)
    os.environ.update({k: v for k, v in saved.items() if v is not None})
    _cache[name, route] = (mol, wf, e_trial)
    return _cache[name, route]


def V(system, W, n, route=None, tapes=False, energy=True, record=False):
    return ("vmc", system, W, n, dict(route=route, tapes=tapes, energy=energy, record=record))


def D(system, W, n, tapes=False, **kw):
    return ("dmc", system, W, n, dict(tapes=tapes, **kw))


# name -> (kind, system, walkers, steps, keywords).  Walkers: 7 (less than one block, the odd tail of the four-walker T-move blocks) and
# 300 (a tail in 256-thread grids).  Seeds are fixed by the position in the table.
CASES = {
    # the five sweep routes, with host tapes and on device draws; energy on and off; the accept record
    "vmc_r8_w7_n1": V("water", 7, 1, "r8", record=True),
    "vmc_r8_tapes_w300_n3": V("water", 300, 3, "r8", tapes=True),
    "vmc_res_w7_n3": V("water", 7, 3, "res", energy=False),
    "vmc_res_tapes_w7_n1": V("water", 7, 1, "res", tapes=True, record=True),
    "vmc_lw_w300_n3": V("water", 300, 3, "lw", record=True),
    "vmc_lw_tapes_w7_n3": V("water", 7, 3, "lw", tapes=True, energy=False),
    "vmc_ww_w7_n3": V("water", 7, 3, "ww"),
    "vmc_ww_tapes_w7_n1": V("water", 7, 1, "ww", tapes=True, energy=False, record=True),
    "vmc_launches_w7_n1": V("water", 7, 1, "launches", energy=False),
    "vmc_launches_tapes_w7_n3": V("water", 7, 3, "launches", tapes=True, record=True),
    "vmc_general_w7_n3": V("general", 7, 3),  # necp = 0: nrot counts one pseudo-atom
    "vmc_general_tapes_w7_n1": V("general", 7, 1, tapes=True),
    "vmc_water4_w7_n3": V("water4", 7, 3, record=True),
    "vmc_water3b_w7_n1": V("water3b", 7, 1, tapes=True),
    "vmc_gamma_w7_n3": V("gamma", 7, 3, record=True),  # wrap counters
    "vmc_gamma_tapes_w300_n1": V("gamma", 300, 1, tapes=True),
    "vmc_twist_w7_n3": V("twist", 7, 3),  # twisted: no wrap pointers
    # pqa_dmc_steps, semi-local ECP
    "dmc_water_w7_n1": D("water", 7, 1),
    "dmc_water_w300_n3": D("water", 300, 3),
    "dmc_water_tapes_w7_n3": D("water", 7, 3, tapes=True),
    "dmc_water_tapes_w300_n1": D("water", 300, 1, tapes=True),
    "dmc_water_split_w7_n3": D("water", 7, 3, tapes=True, split=True),  # one call of 3 steps and three calls with cont=True
    "dmc_water_split_rng_w7_n3": D("water", 7, 3, split=True),
    "dmc_water_cont_refused_w7": D("water", 7, 1, refused="cont"),  # cont after a recompute in between
    # "T-moves off in the accumulator": the device makes T-moves on every ECP handle, so all such an accumulator changes is that its tape set
    # lacks the T-move tapes (philox_dmc_tapes(tmoves=False)), which pqa_dmc_steps refuses; the tapes and the refusal's text are the record
    "dmc_water_notm_refused_w7": D("water", 7, 1, refused="notm"),  # a tape set without the T-move tapes
    "dmc_general_w7_n3": D("general", 7, 3),  # no T-moves
    "dmc_general_tapes_w7_n1": D("general", 7, 1, tapes=True),
    "dmc_water4_w7_n3": D("water4", 7, 3),  # pre false
    "dmc_water4_tapes_w7_n1": D("water4", 7, 1, tapes=True),
    "dmc_water3b_w7_n3": D("water3b", 7, 3),
    # pqa_dmc_steps, batched ECP integrator
    "dmc_sel6_3_w7_n3": D("waterb", 7, 3, batched="sel6_3"),
    "dmc_sel6_3_tapes_w300_n1": D("waterb", 300, 1, batched="sel6_3", tapes=True),
    "dmc_all_w7_n1": D("waterb", 7, 1, batched="all"),
    "dmc_all_tapes_w7_n3": D("waterb", 7, 3, batched="all", tapes=True),
    # periodic, complex, twisted
    "dmc_gamma_w7_n3": D("gamma", 7, 3),
    "dmc_gamma_tapes_w7_n1": D("gamma", 7, 1, tapes=True),
    "dmc_complex_w7_n3": D("complex", 7, 3),  # navg = 8
    "dmc_twist_w7_n1": D("twist", 7, 1),
    "dmc_twist_tapes_w7_n3": D("twist", 7, 3, tapes=True),
    # the per-step loops of dmc_propagate with one further accumulator and replayed draws
    "loop_resident_water_w7_n3": ("loop", "water", 7, 3, dict(route="resident")),
    "loop_host_water_w7_n3": ("loop", "water", 7, 3, dict(route="host")),
    "loop_resident_gamma_w7_n3": ("loop", "gamma", 7, 3, dict(route="resident")),  # the per-step fetch of periodic containers
    "loop_host_complex_w7_n1": ("loop", "complex", 7, 1, dict(route=None)),  # complex ecp / total in the shared loop
}


def _after(dev, wf):
    """The state a call leaves: resident walkers, value, last energy rows, wrap increments."""
    out = {"walkers": dev.get_walkers(np.arange(dev.W)), "energy_last": dev.energy_last()}
    out["sign"], out["log"] = wf.value()
    if dev.pbc:
        out["wrap"] = dev.wrap_delta()
    return out


def _message(fn):
    try:
        fn()
    except Exception as e:  # noqa: BLE001 (the text is the record)
        return np.frombuffer(f"{type(e).__name__}: {e}".encode(), dtype=np.uint8)
    raise AssertionError("the call was expected to be refused")


def _energy_acc(mol, batched):
    import pyqmc_amd as pa

    if batched is None:
        return pa.EnergyAccumulator(mol, **({"ewald_gmax": 10} if hasattr(mol, "lattice_vectors") else {}))
    acc = pa.EnergyAccumulator(mol, use_old_ecp=False)
    acc.ecp = pa.ECPAccumulator(mol, **SELECTIONS[batched])
    return acc


def replay(name):
    """The call of one case -> {"<name>__<output>": array}."""
    import pyqmc_amd as pa
    from tests.dmc_batched_ref import SeededDraws

    kind, sysname, W, n, kw = CASES[name]
    seed = 500 + 3 * list(CASES).index(name)
    mol, wf, e_trial = system(sysname, kw.get("route") if kind == "vmc" else None)
    start = pa.initial_guess(mol, W, rng=np.random.default_rng(seed))
    wf.recompute(start)
    dev = wf.fused_device()
    N, necp = dev.N, getattr(dev, "necp", 0)
    rng = np.random.default_rng(seed + 1)
    out = {}
    if kind == "vmc":
        acc = _energy_acc(mol, None)
        acc.bind(dev)
        t = {}
        if kw["tapes"]:
            t = dict(gauss=rng.standard_normal((n, N, W, 3)), unif=rng.random((n, N, W)))
            if necp and kw["energy"]:
                t.update(ecp_rot=np.linalg.qr(rng.standard_normal((n, N, necp, 3, 3)))[0], ecp_unif=rng.random((n, N, necp, W)))
        a, en, rec = dev.vmc_sweeps(TSTEP, n, seed=seed, energy=kw["energy"], record=kw["record"], **t)
        out = {"acceptance": a, **({"energy": en} if kw["energy"] else {}), **({"record": rec} if kw["record"] else {})}
        if not kw["energy"]:
            dev.energy(seed=seed)  # (energy_last below: of the walkers the sweeps left)
        out.update(_after(dev, wf))
    elif kind == "dmc":
        acc = _energy_acc(mol, kw.get("batched"))
        acc.bind(dev)
        args = (DMC["branchcut"], e_trial, e_trial)
        if kw.get("refused") == "cont":
            dev.dmc_steps(DMC["tstep"], 1, np.ones(W), *args, seed=seed)
            wf.recompute(start)
            out["message"] = _message(lambda: dev.dmc_steps(DMC["tstep"], 1, np.ones(W), *args, seed=seed, cont=True))
        elif kw.get("refused") == "notm":
            t = dev.philox_dmc_tapes(seed, 1, W, tmoves=False)
            out["message"] = _message(lambda: dev.dmc_steps(DMC["tstep"], 1, np.ones(W), *args, tapes=t, seed=seed))
            out.update({"tape_" + k: v for k, v in t.items()})
        else:
            t = dev.philox_dmc_tapes(seed + 2, n, W) if kw["tapes"] else None
            w = np.exp(0.1 * rng.standard_normal(W))
            out["step_avg"], out["step_acc"] = dev.dmc_steps(DMC["tstep"], n, w, *args, tapes=t, seed=seed)
            out["weights"] = w
            out.update(_after(dev, wf))
            if kw.get("split"):  # the same steps as calls of one step, sliced as pyqmc_amd.dmc slices them
                wf.recompute(start)
                w = np.exp(0.1 * np.random.default_rng(seed + 1).standard_normal(W))
                for i in range(n):
                    ti = None if t is None else {k: (np.stack([v[0 if i == 0 else i], v[i + 1]]) if k.startswith("ecp_") else v[i:i + 1]) for k, v in t.items()}
                    out[f"split_avg{i}"], out[f"split_acc{i}"] = dev.dmc_steps(DMC["tstep"], 1, w, *args, tapes=ti, seed=seed, cont=i > 0)
                out["split_weights"] = w
                out.update({"split_" + k: v for k, v in _after(dev, wf).items()})
    else:
        lat = hasattr(mol, "lattice_vectors")
        accs = {"energy": _energy_acc(mol, None), "sq": pa.SqAccumulator(mol, nq=1) if lat else pa.SqAccumulator(mol, qlist=rng.standard_normal((5, 3)))}
        np.random.seed(seed)
        w = np.exp(0.1 * rng.standard_normal(W))
        blk, cfg, w = pa.dmc_propagate(wf, start, w, DMC["tstep"], DMC["branchcut"], e_trial, e_trial, nsteps=n, accumulators=accs, rng=SeededDraws(seed),
                                       accumulator_route=kw["route"])
        out = {"blk_" + k: v for k, v in blk.items()}
        out.update(configs=cfg.configs, weights=w, **({"cfg_wrap": cfg.wrap} if lat else {}))
        out.update({k: v for k, v in _after(dev, wf).items() if k != "wrap"})  # (the loop fetched the increments)
    return {f"{name}__{k}": np.array(v) for k, v in out.items()}


# The replay tapes pyqmc_amd.dmc draws from a generator (no GPU): name -> (tmoves, batched selection (naip, nsd, nsr) or None), for
# N = 3 electrons, 2 ECP atoms, 5 walkers, 2 steps.  --tapes records them into tests/golden/dmc_tapes_parent.npz.
TAPE_SHAPE = dict(nsteps=2, N=3, necp=2, W=5)
TAPE_CASES = {"semilocal_tm": (True, None), "semilocal_notm": (False, None),
              "batched_drop": (True, ([12, 0], 6, 3)),  # the selection drops points: selection uniforms; an atom without points
              "batched_all": (True, ([12, 6], 18, 0))}  # drops none: no ecp_unif / tm_unif


def replay_tapes(name):
    from pyqmc_amd import dmc
    from tests.dmc_batched_ref import SeededDraws

    tmoves, batched = TAPE_CASES[name]
    batched = None if batched is None else (np.asarray(batched[0]), batched[1], batched[2])
    t = dmc._record_tapes(SeededDraws(40 + list(TAPE_CASES).index(name)), tmoves=tmoves, batched=batched, **TAPE_SHAPE)
    return {f"{name}__{k}": v for k, v in t.items()}


def record():
    arrays = {}
    for name in CASES:
        arrays.update(replay(name))
    return arrays


if __name__ == "__main__":
    def option(name, default):
        return sys.argv[sys.argv.index(name) + 1] if name in sys.argv else default

    root = os.path.abspath(option("--tree", os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))  # the tree whose package is used
    sys.path.insert(0, root)
    if "--tapes" in sys.argv:
        arrays = {k: v for name in TAPE_CASES for k, v in replay_tapes(name).items()}
        path = option("--out", os.path.join(root, "tests", "golden", "dmc_tapes_parent.npz"))
        np.savez_compressed(path, **arrays)
        sys.exit(print(f"wrote {path}: {len(arrays)} arrays, {os.path.getsize(path)} bytes"))
    path = option("--out", os.path.join(root, "tests", "golden", "propagation_parent.npz"))
    arrays = record()
    bad = [k for k, v in arrays.items() if not np.all(np.isfinite(v))]
    assert not bad, f"not finite: {bad}"
    for k, v in arrays.items():
        if k.endswith("__step_acc"):  # (a case that accepts no T-move does not reach the phase's back end)
            print(k, "accepted T-moves per (electron, walker):", v[:, 1].tolist())
    np.savez_compressed(path, **arrays)
    print(f"wrote {path}: {len(arrays)} arrays, {os.path.getsize(path)} bytes")
