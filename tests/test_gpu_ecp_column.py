"""The ECP pass's Slater ratios from the inverse column (k_ecp_orbcol, csrc/pqa_ecp_orbcol.hpp) against the route it
replaces: orbital rows from k_orb<1> and the first-generation dot product (PQA_ECP_POINT_LW=0), on the same walkers, rotations and uniforms.

The route applies to the evaluation that follows a lane-per-walker sweep (it reads the resident planes), so every case runs one fused sweep
with replayed ECP tapes and compares the per-walker rows that evaluation leaves on the device (``energy_last``).  The sweep does not read the
energy: both routes see the same walkers, which every case asserts.  ``PQA_RES_DEBUG`` makes the handle name the route it took.

Tolerance.  The two routes add the same products in another order: the old one forms phi_k = sum_mu AO_mu C[mu][k] on the matrix pipe and then
sum_k phi_k T[k][e]; the new one V[mu] = sum_k C[mu][k] T[k][e] and then sum_mu AO_mu V[mu].  The scale of such differences was measured on the
parent build between ITS two float64 orders of these sums, the thread-per-point pass (first-generation dot) and the wave-per-walker accumulation
(PQA_ECP_WAVE=1), as max_w |ecp_w - ecp'_w| / max_w |ecp_w| (helpers.relerr) on the shapes below and on 300-walker samples of them:
    water, 13 walkers, threshold -1      2.9e-16        water, 300 walkers        2.9e-17
    (H2O)8, 9 walkers, threshold 10      3.2e-16        (H2O)8, 300 walkers       6.2e-16
The new route re-associates both the orbital sum and the column sum, so it may differ from the old one by four times the largest of these
figures: TOL = 4 x 6.23e-16.  Both figures go to the parity report (``note``)."""

import numpy as np
import pytest

import helpers
from helpers import relerr
from pyqmc_amd import systems
from pyqmc_amd.configs import OpenConfigs

pytestmark = pytest.mark.gpu

PARENT_ROUTE_DIFFERENCE = 6.23e-16  # the parent's point pass against its wave-per-walker accumulation (module docstring)
TOL = 4 * PARENT_ROUTE_DIFFERENCE
NEW, OLD = "k_ecp_orbcol", "k_orb rows + dot product"


def note(key, val):  # recorded with the other measured errors (the parity report test_gpu_parity's fixture writes)
    from tests.test_gpu_parity import REPORT  # (the module object pytest collected: its fixture writes this dictionary)

    REPORT["ecp_column_" + key] = float(val)
    print(f"[ecp_column] {key} = {float(val):.3e}", flush=True)
    return float(val)


def tapes(mol, W, seed):
    """One step's ECP rotations (N, necp, 3, 3) and mask uniforms (N, necp, W), as pqa_vmc_sweeps replays them."""
    rng = np.random.default_rng(seed)
    N = sum(mol.nelec)
    q = rng.standard_normal((N, mol.natm, 4))
    q /= np.linalg.norm(q, axis=-1, keepdims=True)
    w_, x, y, z = np.moveaxis(q, -1, 0)
    rot = np.stack([np.stack([1 - 2 * (y * y + z * z), 2 * (x * y - z * w_), 2 * (x * z + y * w_)], -1),
                    np.stack([2 * (x * y + z * w_), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w_)], -1),
                    np.stack([2 * (x * z - y * w_), 2 * (y * z + x * w_), 1 - 2 * (x * x + y * y)], -1)], -2)
    return rot[None], rng.random((1, N, mol.natm, W))


def evaluate(make_wf, mol, start, env, monkeypatch, capfd, threshold=10.0, tstep=0.3, seed=21):
    """One fused sweep + evaluation on a fresh handle under ``env``: (energy rows (6, W), walkers, ECP points, the routes the handle named)."""
    for k in ("PQA_ECP_POINT_LW", "PQA_ECP_WAVE", "PQA_RADTAB"):
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    monkeypatch.setenv("PQA_RES_DEBUG", "1")
    wf = make_wf()
    dev = wf.fused_device()
    wf.recompute(OpenConfigs(start.copy()))
    rot, unif = tapes(mol, len(start), seed)
    capfd.readouterr()
    dev.vmc_sweeps(tstep, 1, seed=seed, threshold=threshold, ecp_rot=rot, ecp_unif=unif, energy=True)
    rows = dev.energy_last()
    routes = [line.split(": ", 1)[1] for line in capfd.readouterr().err.splitlines() if line.startswith("[pqa] ecp route: ")]
    return rows, dev.configs(), dev.last_ecp_points(), routes


def compare(tag, make_wf, mol, start, monkeypatch, capfd, env=None, **kw):
    """The default route (which must be the new kernel) against PQA_ECP_POINT_LW=0 on the same walkers and draws."""
    new = evaluate(make_wf, mol, start, dict(env or {}), monkeypatch, capfd, **kw)
    old = evaluate(make_wf, mol, start, dict(env or {}, PQA_ECP_POINT_LW="0"), monkeypatch, capfd, **kw)
    assert new[3] == [NEW] and old[3] == [OLD]
    assert np.array_equal(new[1], old[1]) and new[2] == old[2] > 0
    for row in (0, 1, 2, 4):  # ke, ee, ei, grad2: the same kernels on the same state
        assert np.array_equal(new[0][row], old[0][row])
    note(tag + "_parent_route_difference", PARENT_ROUTE_DIFFERENCE)
    assert note(tag + "_ecp", relerr(new[0][3], old[0][3])) <= TOL
    return new, old


def test_runs_share_blocks_and_straddle_them(monkeypatch, capfd):
    """Water, 13 walkers, every point kept (threshold -1): 64-point blocks shared by many 6- and 12-point runs, runs cut by block boundaries,
    a partial last block."""
    import pyqmc_amd as pa

    mol = systems.water()
    mf = systems.random_mf(mol)
    start = pa.initial_guess(mol, 13, rng=np.random.default_rng(3)).configs
    new, _ = compare("water13", lambda: helpers.gpu_wf(mol, mf), mol, start, monkeypatch, capfd, threshold=-1.0)
    assert new[2] % 64 != 0 and new[2] > 3 * 64


def test_headline_shape(monkeypatch, capfd):
    """(H2O)8, 9 walkers, threshold 10 with replayed uniforms: 32 electrons per spin, 184 AOs, 12-point (oxygen) and 6-point (hydrogen) runs in
    one block."""
    import pyqmc_amd as pa

    mol = systems.water_cluster()
    mf = systems.random_mf(mol)
    start = pa.initial_guess(mol, 9, rng=np.random.default_rng(4)).configs
    compare("cluster9", lambda: helpers.gpu_wf(mol, mf), mol, start, monkeypatch, capfd, threshold=10.0)


def test_occupation_that_is_not_the_first_orbitals(monkeypatch, capfd):
    """One determinant out of 12 orbitals whose occupied lists are not 0 .. n-1: the det_occ path, nmo > n."""
    import pyqmc_amd as pa

    mol = systems.water()
    mf = systems.random_mf(mol, nvirt=8)
    dets = [(1.0, [[0, 2, 3, 9], [1, 2, 5, 11]])]
    start = pa.initial_guess(mol, 13, rng=np.random.default_rng(5)).configs
    compare("water13_occ", lambda: helpers.gpu_wf(mol, mf, determinants=dets), mol, start, monkeypatch, capfd, threshold=-1.0)


def test_unequal_spins_and_a_spin_without_points(monkeypatch, capfd):
    """Five up and three down electrons; then the same handle shape with every down electron beyond the range of every ECP atom (their
    terms end below 2.2 bohr; a step of 0.02 keeps them there): the down spin has no point, its launch is skipped, the up spin's result stands."""
    import pyqmc_amd as pa

    mol = systems.Mol(systems.water()._names, systems.water().atom_coords(), nelec=(5, 3))
    mf = systems.random_mf(mol)
    start = pa.initial_guess(mol, 13, rng=np.random.default_rng(6)).configs
    make = lambda: helpers.gpu_wf(mol, mf)
    compare("water13_5up3dn", make, mol, start, monkeypatch, capfd, threshold=-1.0)
    far = start.copy()
    far[:, 5:, :] = np.array([0.0, 0.0, -4.5]) + 0.3 * np.random.default_rng(7).standard_normal((13, 3, 3))
    new, old = compare("water13_no_down_points", make, mol, far, monkeypatch, capfd, threshold=-1.0, tstep=0.02)
    d = np.linalg.norm(new[1][:, 5:, None, :] - mol.atom_coords()[None, None], axis=-1)
    assert d.min() > 2.5  # no down electron in range of an ECP atom: every point of this evaluation is an up electron's
    up_only = evaluate(make, mol, far, {}, monkeypatch, capfd, threshold=-1.0, tstep=0.02)
    assert np.array_equal(up_only[0], new[0])


@pytest.mark.parametrize("radtab", ["0", "1"])
def test_radial_tables_off_and_on(radtab, monkeypatch, capfd):
    """The contracted shells' radial sums from their tables (default) and from the primitives (PQA_RADTAB=0), as in the old route."""
    import pyqmc_amd as pa

    mol = systems.water()
    mf = systems.random_mf(mol)
    start = pa.initial_guess(mol, 13, rng=np.random.default_rng(8)).configs
    compare("water13_radtab" + radtab, lambda: helpers.gpu_wf(mol, mf), mol, start, monkeypatch, capfd, env={"PQA_RADTAB": radtab}, threshold=-1.0)


def test_a_handle_the_route_refuses(monkeypatch, capfd):
    """50 determinants and a three-body factor: the handle names the old route, and the walker means of three steps' energies are, bit for
    bit, those the parent commit's library gave for this call (tests/golden/ecp_column_refused.npz)."""
    import pyqmc_amd as pa

    for k in ("PQA_ECP_POINT_LW", "PQA_ECP_WAVE", "PQA_RADTAB"):
        monkeypatch.delenv(k, raising=False)
    monkeypatch.setenv("PQA_RES_DEBUG", "1")
    mol = systems.water()
    mf = systems.random_mf(mol, nvirt=8)
    wf = helpers.gpu_wf3(mol, mf, systems.random_determinants(mol, mf, 50))
    dev = wf.fused_device()
    wf.recompute(pa.initial_guess(mol, 64, rng=np.random.default_rng(9)))
    capfd.readouterr()
    acc, en, _ = dev.vmc_sweeps(0.3, 3, seed=12, energy=True)
    routes = [line.split(": ", 1)[1] for line in capfd.readouterr().err.splitlines() if line.startswith("[pqa] ecp route: ")]
    assert routes == [OLD]
    g = helpers.golden("ecp_column_refused")
    assert np.array_equal(np.asarray(en), g["energy_means"]) and np.array_equal(acc, g["acceptance"])


def test_two_evaluations_give_the_same_bits(monkeypatch, capfd):
    import pyqmc_amd as pa

    mol = systems.water_cluster()
    mf = systems.random_mf(mol)
    start = pa.initial_guess(mol, 9, rng=np.random.default_rng(10)).configs
    a = evaluate(lambda: helpers.gpu_wf(mol, mf), mol, start, {}, monkeypatch, capfd)
    b = evaluate(lambda: helpers.gpu_wf(mol, mf), mol, start, {}, monkeypatch, capfd)
    assert a[3] == b[3] == [NEW]
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])
