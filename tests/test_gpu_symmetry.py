"""Symmetry-operator ratios on the device (pqa_symmetry / the fused route of SymmetryAccumulator and SymmetryAccumulatorPBC): the
reference's values (g41), the ratios against device recomputes at the transformed walkers, exact eigenfunctions per walker,
inverse consistency, agreement with the protocol route, no side effects on the handle, route selection and the drivers."""

import ast

import numpy as np
import pytest

from pyqmc_amd import systems
from pyqmc_amd.configs import OpenConfigs, PeriodicConfigs, enforce_pbc
from tests import helpers

pytestmark = pytest.mark.gpu


def _rotation(axis, angle):
    """Row-vector rotation matrix (x' = x @ R)."""
    k = np.asarray(axis, dtype=float)
    k /= np.linalg.norm(k)
    K = np.array([[0, -k[2], k[1]], [k[2], 0, -k[0]], [-k[1], k[0], 0]])
    return (np.eye(3) + np.sin(angle) * K + (1 - np.cos(angle)) * K @ K).T


SIGMA_X, SIGMA_Y, C2Z = np.diag([-1.0, 1.0, 1.0]), np.diag([1.0, -1.0, 1.0]), np.diag([-1.0, -1.0, 1.0])
GENERIC = _rotation([0.3, -0.5, 0.8], 0.7)


def _configs(mol, W, seed):
    import pyqmc_amd as pa

    return pa.initial_guess(mol, W, rng=np.random.default_rng(seed))


def _transform(x, S, o=None, lat=None):
    o = np.zeros(3) if o is None else np.asarray(o, dtype=float)
    y = np.einsum("ijk,kl->ijl", x - o, S) + o
    return enforce_pbc(lat, y)[0] if lat is not None else y


def _recomputed(wf, x, ops, origins=None, lat=None):
    """Psi(SR)/Psi(R) (nop, W) from device recomputes at the transformed walkers; the handle is left at x."""
    mk = (lambda c: PeriodicConfigs(c, lat)) if lat is not None else OpenConfigs
    s0, l0 = wf.recompute(mk(x.copy()))
    out = []
    for k, S in enumerate(ops):
        s, l = wf.recompute(mk(_transform(x, S, None if origins is None else origins[k], lat)))
        out.append(s / s0 * np.exp(l - l0))
    wf.recompute(mk(x.copy()))
    return np.array(out)


def _fused(wf, ops, origins=None):
    from pyqmc_amd.symmetry import device_symmetry

    return device_symmetry(wf.fused_device(), np.asarray(ops), origins)


def _relerr(f, d):
    return float(np.max(np.abs(f - d) / (np.abs(d) + 1e-12)))


# ---------------------------------------------------------------- the reference's values
@pytest.mark.parametrize("name", ["a", "b"])
def test_symmetry_golden(name):
    import pyqmc_amd as pa

    g = helpers.golden("g41_symmetry")
    mol = systems.water()
    dets = ast.literal_eval(str(g[f"{name}_det_json"]).replace("null", "None"))
    occ = np.zeros((2, g[f"{name}_mo"].shape[-1]))
    occ[:, :4] = 1
    wf = pa.generate_wf(mol, systems.MeanField(g[f"{name}_mo"], occ), determinants=dets)
    wf.parameters["wf2acoeff"], wf.parameters["wf2bcoeff"] = g[f"{name}_acoeff"], g[f"{name}_bcoeff"]
    configs = pa.OpenConfigs(g[f"{name}_configs"].copy())
    wf.recompute(configs)
    names = [str(n) for n in g[f"{name}_names"]]
    acc = pa.SymmetryAccumulator(dict(zip(names, g[f"{name}_ops"])))
    res = acc(configs, wf)
    assert acc.last_route == "fused" and list(res) == names
    for k, n in enumerate(names):
        ref = g[f"{name}_ratio"][k]
        assert res[n].shape == (32,)
        assert np.max(np.abs(res[n] - ref) / (1 + np.abs(ref))) < 1e-9, n


def test_symmetry_golden_periodic():
    import pyqmc_amd as pa

    g = helpers.golden("g41_symmetry")
    sup, wf = helpers.gpu_pbc_wf("gamma")
    wf.parameters["wf2acoeff"], wf.parameters["wf2bcoeff"] = g["p_acoeff"], g["p_bcoeff"]
    configs = PeriodicConfigs(g["p_configs"].copy(), sup.lattice_vectors(), wrap=g["p_wrap"].copy())
    wf.recompute(configs)
    names = [str(n) for n in g["p_names"]]
    acc = pa.SymmetryAccumulatorPBC(dict(zip(names, g["p_ops"])), dict(zip(names, g["p_origins"])))
    res = acc(configs, wf)
    assert acc.last_route == "fused"
    for k, n in enumerate(names):
        ref = g["p_ratio"][k]
        assert np.max(np.abs(res[n] - ref) / (1 + np.abs(ref))) < 1e-9, n


# ---------------------------------------------------------------- against device recomputes
def test_ratios_water_against_recompute():
    mol = systems.water()
    wf = helpers.gpu_wf(mol, systems.random_mf(mol))
    x = _configs(mol, 256, 1).configs
    ops = [SIGMA_X, SIGMA_Y, C2Z, GENERIC, np.eye(3)]
    direct = _recomputed(wf, x, ops)
    fused = _fused(wf, ops)
    assert _relerr(fused, direct) < 1e-9
    assert np.max(np.abs(fused[-1] - 1.0)) < 1e-12


def test_ratios_water_50_determinants_against_recompute():
    mol = systems.water()
    mf = systems.random_mf(mol, nvirt=6)
    wf = helpers.gpu_wf(mol, mf, systems.random_determinants(mol, mf, 50))
    x = _configs(mol, 128, 2).configs
    ops = [SIGMA_Y, GENERIC]
    direct = _recomputed(wf, x, ops)
    assert _relerr(_fused(wf, ops), direct) < 1e-9


def test_ratios_zero_leading_diagonal():
    """Up electron 1 at the mirror image of up electron 0: the reflection exchanges them and B's leading diagonal vanishes."""
    mol = systems.water()
    wf = helpers.gpu_wf(mol, systems.random_mf(mol))
    x = _configs(mol, 64, 3).configs.copy()
    x[:, 1] = x[:, 0] @ SIGMA_X
    direct = _recomputed(wf, x, [SIGMA_X])
    assert _relerr(_fused(wf, [SIGMA_X]), direct) < 1e-9


def test_ratios_diamond_222_against_recompute():
    sup, wf = helpers.gpu_pbc_wf("k222")
    lat = sup.lattice_vectors()
    x = np.random.default_rng(4).random((64, sum(sup.nelec), 3)) @ lat
    a = sup.atom_coords()
    ops = [-np.eye(3), _rotation([1.0, 1.0, 0.0], np.pi), GENERIC]
    origins = np.stack([0.5 * (a[0] + a[1]), a[1], np.array([0.7, -0.3, 1.9])])
    direct = _recomputed(wf, x, ops, origins, lat)
    assert _relerr(_fused(wf, ops, origins), direct) < 1e-9


def test_ratios_above_64_electrons_per_spin():
    """The g35 cluster, 72 electrons per spin: the LU runs on a 72 x 72 tile past one lane per column."""
    mol, mf, _, _ = helpers.case("g35_big")
    wf = helpers.gpu_wf(mol, mf)
    x = _configs(mol, 8, 5).configs
    ops = [_rotation([0.1, 0.2, 1.0], 0.02), SIGMA_X]
    direct = _recomputed(wf, x, ops)
    assert _relerr(_fused(wf, ops), direct) < 1e-9


# ---------------------------------------------------------------- exact eigenfunctions
def _ao_reflection(mol, S, seed=0):
    """T (nao, nao) with chi(r @ S) = chi(r) @ T: a signed permutation for a reflection that maps the molecule onto itself."""
    from oracle import gto

    table = gto.AOTable(mol)
    rng = np.random.default_rng(seed)
    atoms = np.asarray(mol.atom_coords())
    pts = (atoms[rng.integers(len(atoms), size=40 * len(atoms))] + rng.standard_normal((40 * len(atoms), 3))).reshape(-1, 3)
    A = gto.eval_ao(table, pts, 1)[0]
    B = gto.eval_ao(table, pts @ S, 1)[0]
    T = np.linalg.lstsq(A, B, rcond=None)[0]
    Tr = np.round(T)
    assert np.max(np.abs(T - Tr)) < 1e-8 and np.max(np.abs(A @ Tr - B)) < 1e-10 * max(1.0, np.abs(B).max())
    return Tr


def _adapted_orbitals(mol, irreps, seed):
    """MO coefficients (nao, len(irreps)): random vectors projected onto the (eps_x, eps_y) eigenspaces of x -> -x and y -> -y."""
    Tx, Ty = _ao_reflection(mol, SIGMA_X), _ao_reflection(mol, SIGMA_Y)
    nao = Tx.shape[0]
    rng = np.random.default_rng(seed)
    cols = []
    for ex, ey in irreps:
        c = rng.standard_normal(nao)
        c = 0.5 * (c + ex * (Tx @ c))
        c = 0.5 * (c + ey * (Ty @ c))
        cols.append(c / np.linalg.norm(c))
    C = np.stack(cols, axis=1)
    assert np.linalg.matrix_rank(C) == len(irreps)
    return C


def _element_jastrow(wf, mol, seed=11):
    """One-body coefficients shared by atoms of one element (the reflections map H onto H): Psi keeps the determinant's parity."""
    a, b = helpers.jastrow_params(mol, seed)
    sym = [mol.atom_symbol(i) for i in range(mol.natm)]
    first = {}
    for i, s in enumerate(sym):
        first.setdefault(s, i)
        a[i] = a[first[s]]
    wf.parameters["wf2acoeff"], wf.parameters["wf2bcoeff"] = a, b
    return wf


def _parity(irreps):
    px = np.prod([e[0] for e in irreps])
    py = np.prod([e[1] for e in irreps])
    return px, py


def _exact_case(mol, irreps_up, irreps_dn, W, seed):
    import pyqmc_amd as pa

    mo = np.stack([_adapted_orbitals(mol, irreps_up, seed), _adapted_orbitals(mol, irreps_dn, seed + 1)])
    wf = pa.generate_wf(mol, systems.MeanField(mo, np.ones((2, mo.shape[-1]))))
    _element_jastrow(wf, mol)
    # walkers drawn from |Psi|^2, as the drivers hand them to the accumulator: the ratio's round-off grows with the conditioning of
    # the Slater matrix, and the guess's walkers are not kept away from the nodes
    _, cfg = pa.vmc_worker(wf, _configs(mol, W, seed), 0.3, 30, {}, seed=seed)
    wf.recompute(cfg)
    ux, uy = _parity(irreps_up)
    dx, dy = _parity(irreps_dn)
    expect = np.array([ux * dx, uy * dy, ux * dx * uy * dy, 1.0])
    got = _fused(wf, [SIGMA_X, SIGMA_Y, C2Z, np.eye(3)])
    return got, expect


def _assert_exact(got, expect):
    err = np.abs(got - expect[:, None])
    bad = np.nonzero(np.any(err >= 1e-10, axis=0))[0]
    # (on failure: how many walkers, and the identity's deviation there, which measures the conditioning of their Slater matrices)
    assert len(bad) == 0, (len(bad), err.max(axis=1), err[-1, bad[:8]], err[:, bad[:8]].max(axis=0))


@pytest.mark.parametrize("case", ["even", "odd"])
def test_exact_eigenfunction_water(case):
    mol = systems.water()
    up = [(1, 1), (1, 1), (1, -1), (-1, 1)]
    dn = [(1, 1), (1, 1), (1, 1), (1, -1)] if case == "odd" else up
    got, expect = _exact_case(mol, up, dn, 512, 21)
    if case == "odd":
        assert set(expect) == {1.0, -1.0}
    _assert_exact(got, expect)


def test_exact_eigenfunction_cluster_65536():
    """(H2O)8 centred at the origin: both reflections map it onto itself (32 electrons per spin, 65 536 walkers)."""
    base = systems.water_cluster()
    xyz = np.asarray(base.atom_coords())
    sym = [base.atom_symbol(i) for i in range(base.natm)]
    mol = systems.Mol(list(sym), [tuple(r) for r in xyz - xyz.mean(axis=0)])
    rng = np.random.default_rng(3)
    choices = [(1, 1), (1, -1), (-1, 1), (-1, -1)]
    up = [choices[i] for i in rng.integers(4, size=32)]
    dn = [choices[i] for i in rng.integers(4, size=32)]
    got, expect = _exact_case(mol, up, dn, 65536, 31)
    assert -1.0 in expect and np.all(np.abs(expect) == 1)
    _assert_exact(got, expect)


# ---------------------------------------------------------------- consistency
@pytest.mark.parametrize("periodic", [False, True])
def test_inverse_consistency(periodic):
    """ratio_S(R) ratio_{S^-1}(SR) = 1 for an operator the wave function does not have (periodic: a lattice automorphism about a
    general origin, so that S^-1 undoes the fold)."""
    if periodic:
        sup, wf = helpers.gpu_pbc_wf("gamma")
        lat = sup.lattice_vectors()
        S = np.array([[0.0, 1.0, 0.0], [-1.0, 0.0, 0.0], [0.0, 0.0, 1.0]])  # C4 about z: maps the fcc lattice onto itself
        o = np.array([0.41, -0.73, 1.3])
        x = np.random.default_rng(6).random((128, sum(sup.nelec), 3)) @ lat
        mk = lambda c: PeriodicConfigs(c, lat)  # noqa: E731
    else:
        mol = systems.water()
        wf = helpers.gpu_wf(mol, systems.random_mf(mol))
        lat, S, o = None, GENERIC, np.zeros(3)
        x = _configs(mol, 256, 6).configs
        mk = OpenConfigs
    wf.recompute(mk(x.copy()))
    r1 = _fused(wf, [S], [o])[0]
    wf.recompute(mk(_transform(x, S, o, lat)))
    r2 = _fused(wf, [np.linalg.inv(S)], [o])[0]
    assert np.max(np.abs(r1 - 1.0)) > 1e-3  # not a symmetry
    assert np.max(np.abs(r1 * r2 - 1.0)) < 1e-9


@pytest.mark.parametrize("case", ["multidet", "periodic"])
def test_fused_matches_protocol(case):
    import pyqmc_amd as pa

    if case == "multidet":
        mol = systems.water()
        mf = systems.random_mf(mol, nvirt=6)
        wf = helpers.gpu_wf(mol, mf, systems.random_determinants(mol, mf, 10))
        configs = _configs(mol, 128, 9)
        acc = pa.SymmetryAccumulator({"sx": SIGMA_X, "g": GENERIC})
    else:
        sup, wf = helpers.gpu_pbc_wf("gamma")
        lat = sup.lattice_vectors()
        configs = PeriodicConfigs(np.random.default_rng(9).random((64, sum(sup.nelec), 3)) @ lat, lat)
        a = sup.atom_coords()
        acc = pa.SymmetryAccumulatorPBC({"i": -np.eye(3), "g": GENERIC}, {"i": 0.5 * (a[0] + a[1]), "g": np.array([0.7, -0.3, 1.9])})
    wf.recompute(configs)
    fused = acc(configs, wf)
    assert acc.last_route == "fused"
    prot = acc._protocol(configs, wf)
    for n in acc.keys():
        assert _relerr(fused[n], prot[n]) < 1e-9, n


# ---------------------------------------------------------------- no side effects
@pytest.mark.parametrize("periodic", [False, True])
def test_no_side_effects_on_handle(periodic):
    import pyqmc_amd as pa

    if periodic:
        sup, wf = helpers.gpu_pbc_wf("gamma")
        lat = sup.lattice_vectors()
        configs = PeriodicConfigs(np.random.default_rng(10).random((256, sum(sup.nelec), 3)) @ lat, lat)
        acc = pa.SymmetryAccumulatorPBC({"i": -np.eye(3), "g": GENERIC}, {"i": np.array([0.3, 0.2, 0.1]), "g": np.zeros(3)})
    else:
        mol = systems.water()
        mf = systems.random_mf(mol, nvirt=6)
        wf = helpers.gpu_wf(mol, mf, systems.random_determinants(mol, mf, 10))
        configs = _configs(mol, 256, 10)
        acc = pa.SymmetryAccumulator({"sx": SIGMA_X, "g": GENERIC})
    wf.recompute(configs)
    pa.vmc_worker(wf, configs, 0.3, 2, {}, seed=3, state_current=True)  # leaves the state in the sweep's layout
    sl, ja = wf.wf_factors
    dev = wf.fused_device()

    def state():
        return [sl._get_state(0), sl._get_state(1), ja._get_state(), wf.value(), [dev.wrap_delta()] if periodic else [],
                [dev.get_walkers(np.arange(dev.W))]]

    before = state()
    acc(configs, wf)
    assert acc.last_route == "fused"
    after = state()
    for b, a in zip(before, after):
        for u, v in zip(b, a):
            assert np.array_equal(u, v)


class _Nothing:
    def avg(self, configs, wf):
        return {}

    def __call__(self, configs, wf):
        return {}

    def keys(self):
        return {}.keys()

    def shapes(self):
        return {}


def test_vmc_and_dmc_bitwise_unchanged_by_symmetry():
    import pyqmc_amd as pa

    mol = systems.water()
    mf = systems.random_mf(mol)
    runs = []
    for other in (pa.SymmetryAccumulator({"sx": SIGMA_X, "g": GENERIC}), _Nothing()):
        wf = helpers.gpu_wf(mol, mf)
        np.random.seed(6)  # (the energy accumulator's ECP draws)
        df, cfg = pa.vmc(wf, _configs(mol, 256, 11), nblocks=3, nsteps_per_block=2, tstep=0.3,
                         accumulators={"energy": pa.EnergyAccumulator(mol), "symmetry": other}, seed=5)
        np.random.seed(7)
        ddf, dcfg, dw = pa.rundmc(wf, cfg, tstep=0.02, nblocks=2, nsteps_per_block=2, vmc_warmup=1,
                                  accumulators={"energy": pa.EnergyAccumulator(mol), "symmetry": other})
        runs.append((df["energytotal"], cfg.configs.copy(), ddf["energytotal"], dcfg.configs.copy(), dw.copy()))
    for u, v in zip(*runs):
        assert np.array_equal(u, v)


# ---------------------------------------------------------------- route selection and the drivers
def test_route_selection_three_body_complex_twisted():
    import pyqmc_amd as pa
    from pyqmc_amd._ffi import PqaError

    mol = systems.water()
    wf = helpers.gpu_wf3(mol, systems.random_mf(mol))
    x = _configs(mol, 16, 12).configs
    direct = _recomputed(wf, x, [GENERIC])
    configs = pa.OpenConfigs(x.copy())
    wf.recompute(configs)
    acc = pa.SymmetryAccumulator({"g": GENERIC})
    res = acc(configs, wf)
    assert acc.last_route == "protocol"
    assert _relerr(res["g"], direct[0]) < 1e-9
    with pytest.raises(PqaError, match="three-body"):
        _fused(wf, [GENERIC])

    for sup, kmf in (helpers.pbc_complex_case(), helpers.twist_case("prim")):
        cwf = pa.generate_wf(sup, kmf)
        lat = sup.lattice_vectors()
        cfg = PeriodicConfigs(np.random.default_rng(13).random((4, sum(sup.nelec), 3)) @ lat, lat)
        cwf.recompute(cfg)
        o = np.array([0.2, 0.1, -0.3])
        acc = pa.SymmetryAccumulatorPBC({"i": -np.eye(3)}, {"i": o})
        res = acc(cfg, cwf)
        assert acc.last_route == "protocol" and np.iscomplexobj(res["i"]) and res["i"].shape == (4,)
        with pytest.raises(PqaError, match="complex orbitals / twisted cell"):
            _fused(cwf, [-np.eye(3)], [o])


def test_vmc_and_dmc_columns():
    import pyqmc_amd as pa

    mol = systems.water()
    up = [(1, 1), (1, 1), (1, -1), (-1, 1)]
    dn = [(1, 1), (1, 1), (1, 1), (1, -1)]
    mo = np.stack([_adapted_orbitals(mol, up, 41), _adapted_orbitals(mol, dn, 42)])
    wf = _element_jastrow(pa.generate_wf(mol, systems.MeanField(mo, np.ones((2, 4)))), mol)
    ops = {"sx": SIGMA_X, "sy": SIGMA_Y, "g": GENERIC}
    df, cfg = pa.vmc(wf, _configs(mol, 256, 14), nblocks=3, nsteps_per_block=2, tstep=0.3,
                     accumulators={"symmetry": pa.SymmetryAccumulator(ops)}, seed=3)
    (ux, uy), (dx, dy) = _parity(up), _parity(dn)
    ex, ey = ux * dx, uy * dy  # -1, +1
    for n in ops:
        assert df["symmetry" + n].shape == (3,)
    assert np.max(np.abs(df["symmetrysx"] - ex)) < 1e-9 and np.max(np.abs(df["symmetrysy"] - ey)) < 1e-9
    np.random.seed(8)
    ddf, _, _ = pa.rundmc(wf, cfg, tstep=0.02, nblocks=2, nsteps_per_block=2, vmc_warmup=1,
                          accumulators={"energy": pa.EnergyAccumulator(mol), "symmetry": pa.SymmetryAccumulator(ops)})
    for n in ops:
        assert ddf["symmetry" + n].shape == (2,)
    assert np.max(np.abs(ddf["symmetrysx"] - ex)) < 1e-9 and np.max(np.abs(ddf["symmetrysy"] - ey)) < 1e-9
