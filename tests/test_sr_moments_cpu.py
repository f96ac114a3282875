"""Host side of the device route of StochasticReconfiguration (pqa_sr_moments): the route decision with its reasons, the column
description built from a LinearTransform, the refusal of route="device" out of scope, and the C ABI entry.  The numbers are
checked on the GPU (tests/test_gpu_sr_moments.py)."""

import numpy as np
import pytest

import helpers
from pyqmc_amd import _ffi, accumulators, systems
from pyqmc_amd import wf as pwf
from pyqmc_amd.accumulators import LinearTransform, StochasticReconfiguration, sr_columns, sr_route
from pyqmc_amd.energy import EnergyAccumulator

PARAMS = {"wf1det_coeff": np.array([0.9, 0.3, -0.2, 0.1]), "wf1mo_coeff_alpha": np.ones((5, 4)), "wf1mo_coeff_beta": np.ones((5, 4)),
          "wf2acoeff": np.zeros((3, 4, 2)), "wf2bcoeff": np.zeros((4, 3)), "wf3ccoeff": np.zeros((3, 2, 2, 2, 3))}


class _Handle:
    """What sr_route looks at on a device handle (no device is touched on the CPU)."""

    cplx = twisted = False

    def sr_moments(self, *a, **k):
        raise AssertionError("the route decision must not evaluate anything")


def _product(dev=None, three=True, cplx=False):
    """A MultiplyWF of the product classes on one stand-in handle, parameters as PARAMS."""
    dev = dev or _Handle()
    dev.cplx = cplx
    factors = []
    for cls, prefix in ((pwf.Slater, "wf1"), (pwf.JastrowSpin, "wf2"), (pwf.ThreeBodyJastrow, "wf3"))[: 3 if three else 2]:
        f = object.__new__(cls)
        f._dev, f.dtype = dev, float
        f.parameters = {k[3:]: v.copy() for k, v in PARAMS.items() if k.startswith(prefix)}
        factors.append(f)
    return pwf.MultiplyWF(*factors)


def _to_opt(*keys):
    return {k: np.ones(PARAMS[k].shape, dtype=bool) for k in keys}


class _Recorded:
    def __call__(self, configs, wf):
        return {}

    def keys(self):
        return set()


def _sr(wf, keys=("wf1det_coeff", "wf2acoeff", "wf2bcoeff", "wf3ccoeff"), enacc=None, **kw):
    return StochasticReconfiguration(enacc or EnergyAccumulator(systems.water()), LinearTransform(wf.parameters, _to_opt(*keys)), **kw)


def test_route_decision_and_reasons():
    wf = _product()
    assert sr_route(wf, _sr(wf))[0] == "device"
    assert sr_route(_product(three=False), _sr(_product(three=False), keys=("wf2acoeff", "wf2bcoeff")))[0] == "device"
    # an oracle wave function has no device handle
    mol = systems.water()
    owf = helpers.oracle_wf(mol, systems.random_mf(mol))
    route, why = sr_route(owf, StochasticReconfiguration(EnergyAccumulator(mol), LinearTransform(owf.parameters, None)))
    assert route == "protocol" and "MultiplyWF" in why
    # a recorded energy object (the golden SR tests), also as a subclass
    route, why = sr_route(wf, _sr(wf, enacc=_Recorded()))
    assert route == "protocol" and "_Recorded" in why

    class Sub(EnergyAccumulator):
        pass

    assert sr_route(wf, _sr(wf, enacc=Sub(mol))) == ("protocol", "the energy object is a Sub, not a pyqmc_amd.EnergyAccumulator")
    # an injected product
    route, why = sr_route(wf, _sr(wf, gram=lambda a, b: a.T @ b))
    assert route == "protocol" and "gram" in why
    # orbital coefficients have no device source
    route, why = sr_route(wf, _sr(wf, keys=("wf1mo_coeff_alpha", "wf2bcoeff")))
    assert route == "protocol" and "wf1mo_coeff_alpha" in why and "wf2bcoeff" not in why
    # complex handles, nothing selected
    assert sr_route(_product(cplx=True), _sr(wf))[0] == "protocol"
    none = StochasticReconfiguration(EnergyAccumulator(mol), LinearTransform(wf.parameters, {"wf2bcoeff": np.zeros((4, 3), dtype=bool)}))
    assert sr_route(wf, none)[0] == "protocol"


def test_resolve_route():
    wf = _product()
    assert _sr(wf).resolve_route(wf) == "device" and _sr(wf, route="device").resolve_route(wf) == "device"
    assert _sr(wf, route="protocol").resolve_route(wf) == "protocol"
    assert _sr(wf, enacc=_Recorded()).resolve_route(wf) == "protocol"
    with pytest.raises(NotImplementedError, match="_Recorded"):
        _sr(wf, enacc=_Recorded(), route="device").resolve_route(wf)
    with pytest.raises(ValueError):
        _sr(wf, route="host")


def test_device_route_on_an_oracle_wf_raises():
    mol = systems.water()
    owf = helpers.oracle_wf(mol, systems.random_mf(mol))
    with pytest.raises(NotImplementedError, match="MultiplyWF"):
        accumulators.gradient_generator(mol, owf, route="device")
    sr = StochasticReconfiguration(EnergyAccumulator(mol), LinearTransform(owf.parameters, None), route="device")
    with pytest.raises(NotImplementedError, match="MultiplyWF"):
        sr.avg(None, owf)
    assert accumulators.gradient_generator(mol, owf).resolve_route(owf) == "protocol"  # (None: falls back, protocol stays reachable)
    assert accumulators.gradient_generator(mol, owf, route="protocol").route == "protocol"


def test_columns_of_a_transform():
    to_opt = {"wf2bcoeff": np.zeros((4, 3), dtype=bool), "wf1det_coeff": np.array([False, True, True, False]),
              "wf3ccoeff": np.zeros((3, 2, 2, 2, 3), dtype=bool), "wf2acoeff": np.zeros((3, 4, 2), dtype=bool)}
    to_opt["wf2bcoeff"][1:, 1] = True            # flat 4, 7, 10
    to_opt["wf3ccoeff"][2, 1, 0, 1, 2] = True    # flat ((((2 * 2 + 1) * 2 + 0) * 2 + 1) * 3 + 2 = 65
    tr = LinearTransform(PARAMS, to_opt)         # (acoeff: nothing selected, the key is dropped)
    src, pos = sr_columns(tr)
    assert src.dtype == np.int32 and pos.dtype == np.int32
    assert src.tolist() == [2, 2, 2, 0, 0, 3] and pos.tolist() == [4, 7, 10, 1, 2, 65]
    # the columns are those serialize_gradients gathers
    rng = np.random.default_rng(0)
    pg = {k: rng.standard_normal((5,) + v.shape) for k, v in PARAMS.items()}
    flat = {0: pg["wf1det_coeff"], 1: pg["wf2acoeff"], 2: pg["wf2bcoeff"], 3: pg["wf3ccoeff"]}
    cols = np.stack([flat[s].reshape(5, -1)[:, p] for s, p in zip(src, pos)], axis=1)
    assert np.array_equal(cols, tr.serialize_gradients(pg))
    assert [len(a) for a in sr_columns(LinearTransform(PARAMS, {"wf2bcoeff": np.zeros((4, 3), dtype=bool)}))] == [0, 0]


def test_abi_entry():
    assert "pqa_sr_moments" in _ffi._PROTOTYPES and "pqa_sr_moments" in _ffi.header_symbols()
    res, args = _ffi._PROTOTYPES["pqa_sr_moments"]
    assert len(args) == 13
    import __graft_entry__ as ge

    ge.build()
    assert hasattr(_ffi.lib(), "pqa_sr_moments") and "pqa_sr" in ge.UNITS
