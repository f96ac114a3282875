"""The energy pass decides its routes once (energy_plan, csrc/pqa_energy.hip) and launches from the plan.  Every case
below drives one kind of evaluation and checks two things: the route the handle reports under ``PQA_RES_DEBUG``
(``[pqa] energy route: kinetic=... lists=... orbitals=... points=...``) is the one read from the code of the commit before the plan, and
the outputs are, bit for bit, those that commit's library gave for the same call (tests/golden/energy_routes_parent.npz).

The fixture is recorded by ``record()`` of this module, run once with ``PQA_LIB`` pointing at a library built from the parent commit
(tools/make_energy_route_golden.py).  Stored per case: the per-walker rows of the last evaluation (``energy_last``), the per-step walker
means, the walkers and ``last_ecp_points``; for the two large cases the means, 64 sampled walkers with their rows, and a SHA-256 of the
whole arrays.  ECP rotations and uniforms are replayed where the entry point takes them, otherwise the call's seed fixes them."""

import contextlib
import hashlib
import os

import numpy as np
import pytest

import helpers
from helpers import pbc_jastrow_coeffs, rotations
from pyqmc_amd import systems

pytestmark = pytest.mark.gpu

SWITCHES = ("PQA_ECP_POINT_LW", "PQA_ECP_WAVE", "PQA_ECP_ACC_WAVES", "PQA_ECP_LDS", "PQA_ECP_DEFER", "PQA_RES_DEBUG")
ROUTE = "[pqa] energy route: "
CASES = {}  # name -> (the route lines expected, in order; the function that runs the case and returns its outputs)


@contextlib.contextmanager
def environment(**env):
    """The switches are read when a handle is created: every case makes its handles inside this block."""
    saved = {k: os.environ.pop(k, None) for k in SWITCHES}
    os.environ.update(env, PQA_RES_DEBUG="1")
    try:
        yield
    finally:
        for k in SWITCHES:
            os.environ.pop(k, None)
        os.environ.update({k: v for k, v in saved.items() if v is not None})


def case(name, *routes, **env):
    def register(run):
        def run_in_env():
            with environment(**env):
                return {k: np.asarray(v) for k, v in run().items()}

        CASES[name] = (list(routes), run_in_env)
        return run

    return register


def route(kinetic, lists, orbitals, points):
    return f"kinetic={kinetic} lists={lists} orbitals={orbitals} points={points}"


def ecp_tapes(dev, nsteps, seed=21):
    """ECP rotations (nsteps, N, necp, 3, 3) and mask uniforms (nsteps, N, necp, W), as pqa_vmc_sweeps replays them."""
    rng = np.random.default_rng(seed)
    return rotations(rng, nsteps, dev.N, dev.necp), rng.random((nsteps, dev.N, dev.necp, dev.W))


def sha(a):
    return np.frombuffer(hashlib.sha256(np.ascontiguousarray(a).tobytes()).digest(), dtype=np.uint8)


def outputs(dev, large=False, **more):
    rows, x = np.asarray(dev.energy_last()), dev.configs()
    out = dict(more, points=dev.last_ecp_points())
    if large:  # a fixed sample and a digest of the whole arrays: the fixture stays small
        idx = np.random.default_rng(1).choice(dev.W, 64, replace=False)
        out.update(rows=rows[:, idx], walkers=x[idx], rows_sha256=sha(rows), walkers_sha256=sha(x))
    else:
        out.update(rows=rows, walkers=x)
    return out


def water(W=13, seed=3):
    import pyqmc_amd as pa

    mol = systems.water()
    wf = helpers.gpu_wf(mol, systems.random_mf(mol))
    wf.recompute(pa.initial_guess(mol, W, rng=np.random.default_rng(seed)))
    return wf, wf.fused_device()


def sweeps(dev, nsteps=1, tapes=True, large=False, tstep=0.3, seed=21):
    rot, unif = ecp_tapes(dev, nsteps) if tapes and dev.necp else (None, None)
    acc, en, _ = dev.vmc_sweeps(tstep, nsteps, seed=seed, ecp_rot=rot, ecp_unif=unif, energy=True)
    return outputs(dev, large, means=en, acceptance=acc)


def energy(dev, seed=9):
    rot, unif = ecp_tapes(dev, 1) if dev.necp else (None, None)
    en = dev.energy(10.0, rot=None if rot is None else rot[0], unif=None if unif is None else unif[0], seed=seed)
    return outputs(dev, returned=en)


# ---------------------------------------------------------------- the water molecule, 13 walkers
WATER_SWEEP = route("lw", "lds", "column", "point_lw")
WATER_ENERGY = route("coulomb x4", "lds", "rows", "point walker-major")


@case("water_sweep", WATER_SWEEP)
def _():
    return sweeps(water()[1])


@case("water_sweep_point_lw0", route("lw", "lds", "rows", "point on planes"), PQA_ECP_POINT_LW="0")
def _():
    return sweeps(water()[1])


@case("water_sweep_wave", route("lw", "lds", "rows", "accum x4"), PQA_ECP_WAVE="1")
def _():
    return sweeps(water()[1])


@case("water_sweep_wave_acc1", route("lw", "lds", "rows", "accum x1"), PQA_ECP_WAVE="1", PQA_ECP_ACC_WAVES="1")
def _():
    return sweeps(water()[1])


@case("water_sweep_lds0", route("lw", "first", "column", "point_lw"), PQA_ECP_LDS="0")
def _():
    return sweeps(water()[1])


@case("water_energy", WATER_ENERGY)
def _():
    return energy(water()[1])


def three_steps():
    """Steps 2 and 3 are deferred evaluations (the totals stay on the device) unless PQA_ECP_DEFER=0."""
    return sweeps(water()[1], nsteps=3)


case("water_three_steps", WATER_SWEEP)(three_steps)
case("water_three_steps_defer0", WATER_SWEEP, PQA_ECP_DEFER="0")(three_steps)


@case("water_batched_energy", route("coulomb x4", "batched", "rows", "point walker-major"))
def _():
    dev = water()[1]
    dev.set_ecp_batched([12, 6, 6], 4, 3)
    rng = np.random.default_rng(22)  # replayed rotations and selection uniforms (N, W, nselect_random)
    en = dev.energy(0.0, rot=rotations(rng, dev.N, dev.necp), unif=rng.random((dev.N, dev.W, 3)), seed=0)
    return outputs(dev, returned=en)


@case("water_batched_sweep", route("lw", "batched", "rows", "point_lw"))
def _():
    dev = water()[1]
    dev.set_ecp_batched([12, 6, 6], 4, 3)
    return sweeps(dev, tapes=False)  # (device draws: the sweep's ECP tapes have the semi-local integrator's layout)


@case("water_dmc", WATER_ENERGY, WATER_SWEEP)
def _():
    """Two DMC steps with T-moves on replayed tapes: the starting energy on the walker-major state, then evaluations behind the sweeps
    that also refresh the walker-major inverses for the next step's T-moves (aos_T_needed)."""
    from conditioning import host_dmc_tapes

    dev = water()[1]
    w = np.ones(dev.W)
    avg, acc = dev.dmc_steps(0.02, 2, w, 10.0, -17.0, -17.0, tapes=host_dmc_tapes(31, 2, dev.N, dev.necp, dev.W))
    return outputs(dev, averages=avg, statistics=acc, weights=w)


@case("water_correlated", WATER_ENERGY)
def _():
    wf, dev = water()
    rng = np.random.default_rng(23)
    a0, b0 = np.asarray(wf.parameters["wf2acoeff"]), np.asarray(wf.parameters["wf2bcoeff"])
    a = np.stack([a0 + 0.05 * rng.standard_normal(a0.shape) for _ in range(2)])
    b = np.stack([b0 + 0.05 * rng.standard_normal(b0.shape) for _ in range(2)])
    rot, unif = ecp_tapes(dev, 1)
    lp, en = dev.correlated(a, b, 10.0, rot=rot[0], unif=unif[0], seed=5)
    return dict(logpsi=lp, energies=en, walkers=dev.configs(), points=dev.last_ecp_points())


@case("water_correlated_md", route("coulomb x4", "lds", "rows", "accum x4"))
def _():
    import pyqmc_amd as pa

    mol = systems.water()
    mf = systems.random_mf(mol, nvirt=6)
    wf = helpers.gpu_wf(mol, mf, determinants=systems.random_determinants(mol, mf, 2))
    wf.recompute(pa.initial_guess(mol, 13, rng=np.random.default_rng(3)))
    dev = wf.fused_device()
    rng = np.random.default_rng(24)
    c0 = np.asarray(wf.parameters["wf1det_coeff"])
    cd = np.stack([c0 + 0.05 * rng.standard_normal(c0.shape) for _ in range(2)])
    rot, unif = ecp_tapes(dev, 1)
    lp, en = dev.correlated_md(cd, None, None, 10.0, rot=rot[0], unif=unif[0], seed=5)
    return dict(logpsi=lp, energies=en, walkers=dev.configs(), points=dev.last_ecp_points())


# ---------------------------------------------------------------- both sides of the 16 384-walker boundary
# quad-cooperative kinetic rows on both; at 16 384 the side stream, the one-block scan and k_energy_finish, above it none, scan_ints and
# k_energy_assemble + k_row_means
WATER_LARGE = route("lw quad", "lds", "column", "point_lw")


@case("water_16384", WATER_LARGE)
def _():
    return sweeps(water(16384)[1], nsteps=2, large=True)


@case("water_16388", WATER_LARGE)
def _():
    return sweeps(water(16388)[1], nsteps=2, large=True)


# ---------------------------------------------------------------- other handle kinds
@case("md50_j3_sweeps", route("coulomb x4", "lds", "rows", "accum x4"))
def _():
    import pyqmc_amd as pa

    mol = systems.water()
    mf = systems.random_mf(mol, nvirt=8)
    wf = helpers.gpu_wf3(mol, mf, systems.random_determinants(mol, mf, 50))
    wf.recompute(pa.initial_guess(mol, 64, rng=np.random.default_rng(9)))
    return sweeps(wf.fused_device(), nsteps=2)


def general():
    import pyqmc_amd as pa

    mol = systems.water_general()  # all-electron: no ECP
    wf = pa.generate_wf(mol, systems.random_mf(mol))
    wf.recompute(pa.initial_guess(mol, 13, rng=np.random.default_rng(3)))
    return wf.fused_device()


@case("general_sweep", route("lw", "none", "none", "none"))
def _():
    return sweeps(general())


@case("general_energy", route("coulomb x4", "none", "none", "none"))
def _():
    return energy(general())


def periodic(sup, wf):
    import pyqmc_amd as pa

    a, b = pbc_jastrow_coeffs(sup)
    wf.parameters["wf2acoeff"], wf.parameters["wf2bcoeff"] = a, b
    dev = wf.fused_device()
    dev.set_ewald(10, 1)
    wf.recompute(pa.initial_guess(sup, 13, rng=np.random.default_rng(3)))
    return dev


def diamond():
    import pyqmc_amd as pa

    sup, mf = helpers.pbc_slater_case("fcc2cubic")
    dev = periodic(sup, pa.generate_wf(sup, mf))
    assert dev.necp == 8
    return dev


@case("diamond_sweep", route("periodic lw", "lds nseg=8", "rows", "point_lw"))
def _():
    return sweeps(diamond())


@case("diamond_energy", route("coulomb x4", "lds nseg=8", "rows", "point walker-major"))
def _():
    return energy(diamond())


def twisted():
    import pyqmc_amd as pa

    sup, mf = helpers.twist_case("prim")
    dev = periodic(sup, pa.generate_wf(sup, mf))
    assert dev.cplx and dev.necp == 2
    return dev


def complex_outputs(out):
    return {k: np.stack([np.real(v), np.imag(v)]) if np.iscomplexobj(v) else v for k, v in out.items()}


@case("twist_sweep", route("periodic complex lw", "lds nseg=2", "rows", "complex point_lw"))
def _():
    return complex_outputs(sweeps(twisted()))


@case("twist_sweep_point_lw0", route("periodic complex lw", "lds nseg=2", "rows", "complex accum x4"), PQA_ECP_POINT_LW="0")
def _():
    return complex_outputs(sweeps(twisted()))


# ---------------------------------------------------------------- recording and the test
def record(path):
    """Run with PQA_LIB pointing at the parent commit's library (which prints no energy route: the outputs alone are recorded)."""
    out = {}
    for name, (_, run) in CASES.items():
        for k, v in run().items():
            out[f"{name}/{k}"] = v
    np.savez_compressed(path, **out)
    return out


@pytest.fixture(scope="module")
def parent():
    return helpers.golden("energy_routes_parent")


@pytest.mark.parametrize("name", list(CASES))
def test_route_and_parent_bits(name, parent, capfd):
    routes, run = CASES[name]
    capfd.readouterr()
    got = run()
    lines = [line[len(ROUTE):] for line in capfd.readouterr().err.splitlines() if line.startswith(ROUTE)]
    assert lines == routes
    keys = sorted(k.split("/", 1)[1] for k in parent.files if k.startswith(name + "/"))
    assert keys == sorted(got) and keys
    for k in keys:
        want = parent[f"{name}/{k}"]
        assert got[k].dtype == want.dtype and got[k].shape == want.shape, k
        assert got[k].tobytes() == want.tobytes(), k
    if name == "water_three_steps_defer0":  # the deferred evaluations and the ones that read their totals back: the same bits
        for k in keys:
            assert parent[f"water_three_steps/{k}"].tobytes() == got[k].tobytes(), k
