"""Host side of the orbital-coefficient columns of the device route (pqa_sr_moments_orb): the B-matrix identity the kernel rests on,
stated in NumPy on the oracle's objects; the column description of a transform with orbital keys; the route decisions with their
reasons; the C ABI entry.  The numbers of the kernel are checked on the GPU (tests/test_gpu_sr_orbitals.py)."""

import numpy as np
import pytest

import helpers
from pyqmc_amd import _ffi, systems
from pyqmc_amd import wf as pwf
from pyqmc_amd.accumulators import (SR_ORBITAL_SOURCES, SR_SOURCES, LinearTransform, StochasticReconfiguration, sr_columns,
                                    sr_columns_orb, sr_route)
from pyqmc_amd.configs import OpenConfigs
from pyqmc_amd.energy import EnergyAccumulator

PARAMS = {"wf1det_coeff": np.array([0.9, 0.3, -0.2, 0.1]), "wf1mo_coeff_alpha": np.ones((5, 4)), "wf1mo_coeff_beta": np.ones((5, 3)),
          "wf2acoeff": np.zeros((3, 4, 2)), "wf2bcoeff": np.zeros((4, 3)), "wf3ccoeff": np.zeros((3, 2, 2, 2, 3))}


def _mol53():
    sym, xyz = zip(*systems._WATER)
    return systems.Mol(sym, xyz, nelec=(5, 3))


def _b_matrix_gradient(sl, s):
    """G = ao^T B with B[e][m] = sum_u wu[u] T_u[e][col_u(m)] on the oracle Slater's state: (W, nao, nmo_s)."""
    pg = sl.pgradient()
    W = pg["det_coeff"].shape[0]
    n, nmo = sl._nelec[s], sl.parameters["mo_coeff_alpha" if s == 0 else "mo_coeff_beta"].shape[1]
    D = len(sl._det_occup[s])
    wu = np.zeros((W, D))
    for di, c in enumerate(sl.parameters["det_coeff"]):
        wu[:, sl._det_map[s][di]] += c * pg["det_coeff"][:, di]
    B = np.zeros((W, n, nmo))
    for u in range(D):
        for col, m in enumerate(sl._det_occup[s][u]):  # T_u[e][col] = inverse[u][col][e]
            B[:, :, m] += wu[:, u, None] * sl._inverse[s][:, u, col, :]
    b = sl._nelec[0] * s
    ao, _ = sl._mo(sl._x_last[:, b : b + n].reshape(-1, 3), s, 1)
    return np.einsum("wea,wem->wam", ao[0].reshape(W, n, -1), B), B


@pytest.mark.parametrize("case", ["water-4det", "nelec-5-3"])
def test_b_matrix_identity(case):
    if case == "water-4det":
        mol = systems.water()
        mf = systems.random_mf(mol, nvirt=6)
        dets = systems.random_determinants(mol, mf, 4)
    else:
        mol = _mol53()
        mf, dets = systems.random_mf(mol), None
    wf = helpers.oracle_wf(mol, mf, dets)
    wf.recompute(OpenConfigs(systems.initial_guess(mol, 12, rng=np.random.default_rng(3)).configs.copy()))
    sl = wf.wf_factors[0]
    ref = sl.pgradient()
    for s, key in enumerate(("mo_coeff_alpha", "mo_coeff_beta")):
        G, B = _b_matrix_gradient(sl, s)
        err = helpers.relerr(G, ref[key])
        print(case, key, G.shape, err)
        assert G.shape == ref[key].shape and err < 1e-13, (key, err)
        # an orbital no determinant of the spin occupies: a zero column of B, hence an exactly zero derivative
        free = sorted(set(range(B.shape[2])) - set(np.unique(sl._det_occup[s]).tolist()))
        assert all(np.all(G[:, :, m] == 0.0) and np.all(ref[key][:, :, m] == 0.0) for m in free)


def test_columns_of_a_transform_with_orbital_keys():
    to_opt = {"wf2bcoeff": np.zeros((4, 3), dtype=bool), "wf1mo_coeff_beta": np.zeros((5, 3), dtype=bool),
              "wf1det_coeff": np.array([False, True, True, False]), "wf1mo_coeff_alpha": np.zeros((5, 4), dtype=bool)}
    to_opt["wf2bcoeff"][1:, 1] = True            # flat 4, 7, 10
    to_opt["wf1mo_coeff_beta"][[0, 4], [2, 1]] = True   # flat 2, 13
    to_opt["wf1mo_coeff_alpha"][3, :] = True     # flat 12 .. 15
    tr = LinearTransform(PARAMS, to_opt)
    src, pos = sr_columns_orb(tr)
    assert src.dtype == np.int32 and pos.dtype == np.int32
    assert src.tolist() == [2, 2, 2, 5, 5, 0, 0, 4, 4, 4, 4] and pos.tolist() == [4, 7, 10, 2, 13, 1, 2, 12, 13, 14, 15]
    rng = np.random.default_rng(0)
    pg = {k: rng.standard_normal((5,) + v.shape) for k, v in PARAMS.items()}
    flat = {0: pg["wf1det_coeff"], 1: pg["wf2acoeff"], 2: pg["wf2bcoeff"], 3: pg["wf3ccoeff"], 4: pg["wf1mo_coeff_alpha"],
            5: pg["wf1mo_coeff_beta"]}
    cols = np.stack([flat[s].reshape(5, -1)[:, p] for s, p in zip(src, pos)], axis=1)
    assert np.array_equal(cols, tr.serialize_gradients(pg))
    # today's keys: what sr_columns gives, and its table is as it was
    plain = LinearTransform(PARAMS, {k: v for k, v in to_opt.items() if k in SR_SOURCES})
    assert all(np.array_equal(a, b) for a, b in zip(sr_columns_orb(plain), sr_columns(plain)))
    assert SR_SOURCES == {"wf1det_coeff": 0, "wf2acoeff": 1, "wf2bcoeff": 2, "wf3ccoeff": 3}
    assert SR_ORBITAL_SOURCES == {"wf1mo_coeff_alpha": 4, "wf1mo_coeff_beta": 5}
    assert [len(a) for a in sr_columns_orb(LinearTransform(PARAMS, {"wf1mo_coeff_beta": np.zeros((5, 3), dtype=bool)}))] == [0, 0]


class _Handle:
    """What sr_route looks at on a device handle (no device is touched on the CPU)."""

    cplx = twisted = pbc = False
    nelec, nmo = (4, 4), (4, 3)

    def sr_moments(self, *a, **k):
        raise AssertionError("the route decision must not evaluate anything")

    sr_moments_orb = sr_moments


def _product(dev=None, fold=None, params=PARAMS):
    dev = dev or _Handle()
    factors = []
    for cls, prefix in ((pwf.Slater, "wf1"), (pwf.JastrowSpin, "wf2"), (pwf.ThreeBodyJastrow, "wf3")):
        f = object.__new__(cls)
        f._dev, f.dtype = dev, float
        f.parameters = {k[3:]: v.copy() for k, v in params.items() if k.startswith(prefix)}
        factors.append(f)
    factors[0]._fold = fold
    return pwf.MultiplyWF(*factors)


def _sr(wf, keys=("wf1det_coeff", "wf1mo_coeff_alpha", "wf1mo_coeff_beta", "wf2bcoeff"), params=PARAMS, **kw):
    to_opt = {k: np.ones(params[k].shape, dtype=bool) for k in keys}
    return StochasticReconfiguration(EnergyAccumulator(systems.water()), LinearTransform(wf.parameters, to_opt), **kw)


def test_route_decisions():
    wf = _product()
    # on request: device
    assert sr_route(wf, _sr(wf, route="device"))[0] == "device" and _sr(wf, route="device").resolve_route(wf) == "device"
    assert sr_route(wf, _sr(wf, keys=("wf1mo_coeff_beta",), route="device"))[0] == "device"
    # not asked for: protocol, the reason names the key and says what takes it
    for route in (None, "protocol"):
        r, why = sr_route(wf, _sr(wf, route=route))
        assert r == "protocol" and "wf1mo_coeff_alpha" in why and "route='device'" in why and "wf2bcoeff" not in why
    assert _sr(wf).resolve_route(wf) == "protocol"
    # the per-k layout of a periodic Slater factor
    folded = _product(fold={"kpts": np.zeros((1, 3)), "blocks": None, "nmo_k": [[4], [3]]})
    r, why = sr_route(folded, _sr(folded, route="device"))
    assert r == "protocol" and "unfold_mo_gradient" in why
    with pytest.raises(NotImplementedError, match="unfold_mo_gradient"):
        _sr(folded, route="device").resolve_route(folded)
    assert sr_route(folded, _sr(folded, keys=("wf1det_coeff", "wf2bcoeff"), route="device"))[0] == "device"  # (today's keys: as before)
    # a periodic handle, complex orbitals, more than 64 per spin
    cell = _Handle()
    cell.pbc = True
    r, why = sr_route(_product(cell), _sr(wf, route="device"))
    assert r == "protocol" and "periodic" in why
    cx = _Handle()
    cx.cplx = True
    assert sr_route(_product(cx), _sr(wf, route="device")) == ("protocol", "complex orbitals / twisted cell")
    big = _Handle()
    big.nelec, big.nmo = (65, 65), (65, 65)
    r, why = sr_route(_product(big), _sr(wf, route="device"))
    assert r == "protocol" and "more than 64" in why
    with pytest.raises(NotImplementedError, match="more than 64"):
        _sr(wf, route="device").resolve_route(_product(big))


def test_route_refuses_moments_beyond_the_limit():
    # (P + 2) P doubles beyond 256 MiB: P = 5800 -> 269 MB
    params = dict(PARAMS, wf1mo_coeff_alpha=np.ones((100, 58)))
    wide = _Handle()
    wide.nelec, wide.nmo = (58, 3), (58, 3)
    wf = _product(wide, params=params)
    sr = _sr(wf, keys=("wf1mo_coeff_alpha",), params=params, route="device")
    assert sr.transform.nparams == 5800
    r, why = sr_route(wf, sr)
    assert r == "protocol" and "5800 parameters" in why and "256 MiB" in why
    params = dict(PARAMS, wf1mo_coeff_alpha=np.ones((99, 58)))  # 5742: 263.8e6 bytes < 268.4e6
    wf = _product(wide, params=params)
    assert sr_route(wf, _sr(wf, keys=("wf1mo_coeff_alpha",), params=params, route="device"))[0] == "device"


def test_abi_entry():
    for name, nargs in (("pqa_sr_moments_orb", 15), ("pqa_sr_moments", 13)):
        assert name in _ffi._PROTOTYPES and name in _ffi.header_symbols()
        assert len(_ffi._PROTOTYPES[name][1]) == nargs
    import __graft_entry__ as ge

    ge.build()
    assert hasattr(_ffi.lib(), "pqa_sr_moments_orb") and hasattr(_ffi.lib(), "pqa_sr_moments") and "pqa_sr" in ge.UNITS
    # the header declares as many arguments as the prototype has
    import re

    text = re.sub(r"/\*.*?\*/", "", open(_ffi.HEADER_PATH).read(), flags=re.S)
    for name, nargs in (("pqa_sr_moments_orb", 15), ("pqa_sr_moments", 13)):
        assert re.search(r"\b" + name + r"\s*\(([^)]*)\)", text).group(1).count(",") == nargs - 1
