"""DMC mixed estimators, the parts that need no GPU: the identity behind the weighted one-body mean (pqa_obdm_sweeps_w) in NumPy on
the oracle's objects, the block combination the two accumulator routes of dmc_propagate share, the route decision on stub objects,
the argument checks of the Python wrappers, and the ABI of the four entries.

    value_mean = sum_s (w o B_s)^T T_s / (nsweeps sum_w w_w)   =   sum_w w_w value[w] / sum_w w_w      (and the norm likewise)
"""

import types

import numpy as np
import pytest

from oracle import dm as odm
from pyqmc_amd import systems
from pyqmc_amd.configs import OpenConfigs
from test_obdm_cpu import OracleOrbitals
from test_obdm_fused_cpu import NORB, NSWEEPS, TSTEP, WARMUP, W, _err, _wf, closed_form


@pytest.mark.parametrize("kw", [dict(), dict(electrons=np.array([5, 1, 6]), naux=10)], ids=["all", "mixed-naux"])
def test_weighted_identity_two_determinants(kw):
    import pyqmc_amd as pa

    mol = systems.water()
    mf, wf = _wf("twodet", mol)
    nao = np.asarray(mf.mo_coeff[0]).shape[0]
    ev = OracleOrbitals(mol, 0.4 * np.random.default_rng(2).standard_normal((nao, NORB)))
    configs = pa.initial_guess(mol, W, rng=np.random.default_rng(3))
    wf.recompute(OpenConfigs(configs.configs.copy()))
    acc = odm.OBDM(mol, ev, nsweeps=NSWEEPS, tstep=TSTEP, warmup=WARMUP, **kw)
    np.random.seed(11)
    ref = acc(configs, wf)
    wts = np.exp(np.random.default_rng(4).standard_normal(W))
    wts[2] = 0.0
    # the same draws again, by hand (oracle/dm.py: OBDM.__call__)
    es = acc._electrons
    np.random.seed(11)
    aux = odm.seed_walkers(mol, kw.get("naux", W), len(es))
    aux = odm.density_walk(aux, ev, 0, WARMUP, TSTEP)[1][-1]
    pick = np.random.randint(0, aux.configs.shape[0], size=(NSWEEPS, W))
    _, snaps, vals = odm.density_walk(aux, ev, 0, NSWEEPS, TSTEP)
    at_e = ev.mos(configs.configs[:, es].reshape(-1, 3), 0).reshape(W, len(es), NORB)
    value, norm = np.zeros((NORB, NORB)), np.zeros(NORB)
    for s in range(NSWEEPS):
        R = closed_form(wf, es, snaps[s].configs[pick[s], 0])
        phi = vals[s][pick[s]]
        F = np.sum(phi**2, axis=1, keepdims=True) / NORB
        B, T = phi / F, np.einsum("we,wej->wj", R, at_e)
        value += (wts[:, None] * B).T @ T
        norm += wts @ (phi**2 / F)
    value, norm = value / (NSWEEPS * wts.sum()), norm / (NSWEEPS * wts.sum())
    ev_, en_ = _err(value, np.einsum("w,wij->ij", wts, ref["value"]) / wts.sum()), _err(norm, wts @ ref["norm"] / wts.sum())
    print(f"weighted obdm identity {sorted(kw)}: value {ev_:.2e} norm {en_:.2e}")
    assert ev_ < 1e-12 and en_ < 1e-12
    assert np.max(np.abs(ref["value"])) > 1e-3
    # and the weights matter: the plain mean is another number
    assert _err(value, ref["value"].mean(axis=0)) > 1e-6


def test_combine_steps_is_the_reference_block_combination():
    from pyqmc_amd.dmc import combine_steps

    rng = np.random.default_rng(5)
    df = [{"energytotal": rng.standard_normal(), "energyecp": complex(rng.standard_normal(), rng.standard_normal()),
           "rdm1value": rng.standard_normal((3, 3)), "sqSq": rng.standard_normal(4), "weight": 0.5 + rng.random(),
           "acceptance": rng.random(), "tmove_acceptance": rng.random()} for _ in range(4)]
    # pyqmc/method/dmc.py:212-219, restated
    weight = np.asarray([d["weight"] for d in df])
    avg_weight = weight / np.mean(weight)
    ref = {k: np.mean([d[k] * w for d, w in zip(df, avg_weight)], axis=0) for k in df[0].keys()}
    ref["weight"] = np.mean(weight)
    got = combine_steps(df)
    assert set(got) == set(ref)
    for k in ref:
        assert np.array_equal(got[k], ref[k]), k
    assert got["rdm1value"].shape == (3, 3) and np.iscomplexobj(got["energyecp"])


class _InScope:
    def __init__(self, why=None):
        self.why = why

    def resident_scope(self, wf):
        return self.why

    def avg_resident(self, wf, weights=None):
        return {}


class _NoResident:
    def __call__(self, configs, wf):
        return {}


def test_route_on_stubs(monkeypatch):
    import pyqmc_amd as pa
    from pyqmc_amd import dmc, wf as pwf

    en, stub_wf = object(), types.SimpleNamespace()
    assert dmc.dmc_accumulator_route(stub_wf, {"energy": en}) == ("fused", "the energy is the only accumulator")
    route, why = dmc.dmc_accumulator_route(stub_wf, {"energy": en, "s2": _InScope()})  # (not a device wave function at all)
    assert route == "host" and "device handle" in why
    monkeypatch.setattr(pwf, "readonly_device", lambda wf: object())
    assert dmc.dmc_accumulator_route(stub_wf, {"energy": en, "a": _InScope(), "b": _InScope()})[0] == "resident"
    assert dmc.dmc_accumulator_route(stub_wf, {"en": en, "a": _InScope()}, ekey=("en", "total"))[0] == "resident"
    route, why = dmc.dmc_accumulator_route(stub_wf, {"energy": en, "a": _InScope(), "b": _InScope("complex evaluator")})
    assert (route, why) == ("host", "b: complex evaluator")
    route, why = dmc.dmc_accumulator_route(stub_wf, {"energy": en, "x": _NoResident()})
    assert route == "host" and "x: _NoResident" in why and "avg_resident" in why
    assert pa.dmc_accumulator_route is dmc.dmc_accumulator_route
    with pytest.raises(ValueError, match="accumulator_route"):
        dmc.dmc_propagate(stub_wf, None, None, 0.01, 10, 0, 0, accumulators={"energy": en}, accumulator_route="device")


def test_weights_are_checked_before_the_device():
    """Negative or non-finite weights and a wrong length are refused by the wrappers themselves (the stub handle has no ``call``)."""
    from pyqmc_amd import _ffi
    from pyqmc_amd.obdm import OrbitalEvaluator, device_obdm_sweeps_w
    from pyqmc_amd.sq import device_sq_w

    dev = types.SimpleNamespace(W=4)
    ev = types.SimpleNamespace(norb=2, dev=types.SimpleNamespace(_h=None))
    bad = {"negative": [1.0, -0.5, 1.0, 1.0], "nan": [1.0, np.nan, 1.0, 1.0], "inf": [1.0, np.inf, 1.0, 1.0], "length": [1.0, 1.0, 1.0],
           "zero sum": [0.0, 0.0, 0.0, 0.0], "shape": np.ones((4, 1))}
    for tag, w in bad.items():
        with pytest.raises(ValueError, match="weights"):
            _ffi.walker_weights(w, 4)
        with pytest.raises(ValueError, match="weights"):
            device_obdm_sweeps_w(dev, ev, [0, 1], 1, w, assign=np.zeros((1, 4), dtype=np.int32))
        with pytest.raises(ValueError, match="weights"):
            device_sq_w(dev, np.ones((2, 3)), w)
        with pytest.raises(ValueError, match="weights"):
            OrbitalEvaluator.fetch_w(ev, 0, 4, (2, 2), 1.0, w)
    good = _ffi.walker_weights([0.0, 2, 1, 0.5], 4)
    assert good.dtype == np.float64 and good.flags.c_contiguous and good.shape == (4,)


def test_accumulators_offer_the_resident_interface():
    import inspect

    import pyqmc_amd as pa

    for cls in (pa.OBDMAccumulator, pa.TBDMAccumulator, pa.S2Accumulator, pa.SymmetryAccumulator, pa.SymmetryAccumulatorPBC, pa.SqAccumulator):
        sig = inspect.signature(cls.avg_resident)
        assert list(sig.parameters) == ["self", "wf", "weights"] and sig.parameters["weights"].default is None, cls
        assert callable(cls.resident_scope)
    assert "accumulator_route" in inspect.signature(pa.dmc_propagate).parameters
    assert "accumulator_route" in inspect.signature(pa.rundmc).parameters


def test_abi():
    import __graft_entry__ as ge
    from pyqmc_amd import _ffi

    nargs = {"pqa_obdm_sweeps_w": 13, "pqa_dm_points_resident": 5, "pqa_dm_fetch_w": 6, "pqa_sq_w": 8}
    for name, n in nargs.items():
        assert name in _ffi._PROTOTYPES and name in _ffi.header_symbols()
        assert hasattr(_ffi.lib(), name) and len(_ffi._PROTOTYPES[name][1]) == n
    assert len(_ffi._PROTOTYPES["pqa_obdm_sweeps"][1]) == 15 and len(_ffi._PROTOTYPES["pqa_dm_fetch"][1]) == 6
    assert "pqa_obdm" in ge.UNITS and "pqa_sq" in ge.UNITS
