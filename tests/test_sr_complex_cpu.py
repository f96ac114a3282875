"""Host side of the device route of StochasticReconfiguration for complex and twisted handles (pqa_sr_moments_c): the opt-in route
decision (complex_device) with its reasons, the column description with the imaginary-part tail, and the planar algebra the kernels
implement.  The numbers are checked on the GPU (tests/test_gpu_sr_complex.py)."""

import numpy as np
import pytest

from pyqmc_amd import _ffi, accumulators, systems
from pyqmc_amd import wf as pwf
from pyqmc_amd.accumulators import LinearTransform, StochasticReconfiguration, sr_columns, sr_columns_c, sr_route
from pyqmc_amd.energy import EnergyAccumulator

PARAMS = {"wf1det_coeff": np.array([0.9, 0.3, -0.2, 0.1]), "wf1mo_coeff_alpha": np.ones((5, 4)), "wf1mo_coeff_beta": np.ones((5, 4)),
          "wf2acoeff": np.zeros((3, 4, 2)), "wf2bcoeff": np.zeros((4, 3)), "wf3ccoeff": np.zeros((3, 2, 2, 2, 3))}


class _Handle:
    """What sr_route looks at on a device handle (no device is touched on the CPU)."""

    cplx = twisted = False

    def sr_moments(self, *a, **k):
        raise AssertionError("the route decision must not evaluate anything")


def _product(dev=None, three=True, cplx=False, twisted=False):
    """A MultiplyWF of the product classes on one stand-in handle, parameters as PARAMS."""
    dev = dev or _Handle()
    dev.cplx, dev.twisted = cplx, twisted
    factors = []
    for cls, prefix in ((pwf.Slater, "wf1"), (pwf.JastrowSpin, "wf2"), (pwf.ThreeBodyJastrow, "wf3"))[: 3 if three else 2]:
        f = object.__new__(cls)
        f._dev, f.dtype = dev, float
        f.parameters = {k[3:]: v.copy() for k, v in PARAMS.items() if k.startswith(prefix)}
        factors.append(f)
    return pwf.MultiplyWF(*factors)


def _to_opt(*keys):
    return {k: np.ones(PARAMS[k].shape, dtype=bool) for k in keys}


def _sr(wf, keys=("wf1det_coeff", "wf2acoeff", "wf2bcoeff", "wf3ccoeff"), **kw):
    return StochasticReconfiguration(EnergyAccumulator(systems.water()), LinearTransform(wf.parameters, _to_opt(*keys)), **kw)


@pytest.mark.parametrize("kind", [dict(cplx=True), dict(cplx=True, twisted=True), dict(twisted=True)])
def test_route_is_opt_in(kind):
    wf = _product(**kind)
    # the flag off: today's answers and messages
    route, why = sr_route(wf, _sr(wf))
    assert route == "protocol" and "complex" in why
    assert _sr(wf).resolve_route(wf) == "protocol" and _sr(wf).complex_device is False
    with pytest.raises(NotImplementedError, match="complex"):
        _sr(wf, route="device").resolve_route(wf)
    # the flag on
    route, why = sr_route(wf, _sr(wf, complex_device=True))
    assert route == "device" and "complex" in why
    assert _sr(wf, complex_device=True).resolve_route(wf) == "device"
    assert _sr(wf, complex_device=True, route="device").resolve_route(wf) == "device"
    assert _sr(wf, complex_device=True, route="protocol").resolve_route(wf) == "protocol"
    # orbital keys of such a handle stay on the protocol route
    orb = ("wf1mo_coeff_alpha", "wf2bcoeff")
    route, why = sr_route(wf, _sr(wf, keys=orb, complex_device=True))
    assert route == "protocol" and "wf1mo_coeff_alpha" in why and "complex" in why
    with pytest.raises(NotImplementedError, match="complex"):
        _sr(wf, keys=orb, complex_device=True, route="device").resolve_route(wf)
    # the other conditions are unchanged
    assert sr_route(wf, _sr(wf, complex_device=True, gram=lambda a, b: a.T @ b)) == ("protocol", "an injected gram")

    class Sub(EnergyAccumulator):
        pass

    sub = StochasticReconfiguration(Sub(systems.water()), LinearTransform(wf.parameters, _to_opt("wf2bcoeff")), complex_device=True)
    assert sr_route(wf, sub)[0] == "protocol" and "Sub" in sr_route(wf, sub)[1]


def test_flag_leaves_real_handles_alone():
    wf = _product()
    assert sr_route(wf, _sr(wf, complex_device=True)) == sr_route(wf, _sr(wf))
    assert sr_route(wf, _sr(wf))[0] == "device"


def test_gradient_generator_passes_the_flag():
    mol = systems.water()
    wf = _product(cplx=True)
    to_opt = _to_opt("wf2acoeff", "wf2bcoeff")
    assert accumulators.gradient_generator(mol, wf, to_opt).complex_device is False
    assert accumulators.gradient_generator(mol, wf, to_opt).resolve_route(wf) == "protocol"
    on = accumulators.gradient_generator(mol, wf, to_opt, complex_device=True, route="device")
    assert on.complex_device is True and on.resolve_route(wf) == "device"
    with pytest.raises(NotImplementedError, match="complex"):
        accumulators.gradient_generator(mol, wf, to_opt, route="device")


def _complex_transform():
    params = dict(PARAMS, wf1det_coeff=PARAMS["wf1det_coeff"].astype(complex))
    to_opt = {"wf2bcoeff": np.zeros((4, 3), dtype=bool), "wf1det_coeff": np.array([False, True, True, True]),
              "wf2acoeff": np.zeros((3, 4, 2), dtype=bool)}
    to_opt["wf2bcoeff"][1:, 1] = True
    to_opt["wf2acoeff"][0, :2, 1] = True
    return params, LinearTransform(params, to_opt)


def test_columns_with_tail():
    params, tr = _complex_transform()
    src, pos, tail = sr_columns_c(tr)
    assert tail.dtype == np.int32
    assert (src.tolist(), pos.tolist()) == tuple(a.tolist() for a in sr_columns(tr))
    assert src.tolist() == [2, 2, 2, 0, 0, 0, 1, 1] and tail.tolist() == [3, 4, 5]
    assert tail.tolist() == np.flatnonzero(tr.complex_inds).tolist()
    assert len(src) + len(tail) == len(tr.serialize_parameters(params))
    # a transform without complex keys has no tail
    _, _, none = sr_columns_c(LinearTransform(PARAMS, _to_opt("wf1det_coeff", "wf2bcoeff")))
    assert none.dtype == np.int32 and len(none) == 0


def test_planar_algebra_and_tail_rule():
    """What k_sr_gather_c / k_sr_syrk_c compute, in NumPy: the tail columns as (-Im, Re) of their twins, and the moments from the four
    real products of the planes."""
    params, tr = _complex_transform()
    rng = np.random.default_rng(3)
    W = 37
    pg = {k: rng.standard_normal((W,) + v.shape) + (1j * rng.standard_normal((W,) + v.shape) if k == "wf1det_coeff" else 0)
          for k, v in params.items()}
    src, pos, tail = sr_columns_c(tr)
    flat = {0: pg["wf1det_coeff"], 1: pg["wf2acoeff"], 2: pg["wf2bcoeff"], 3: pg["wf3ccoeff"]}
    prim = np.stack([flat[s].reshape(W, -1)[:, p] for s, p in zip(src, pos)], axis=1)
    re = np.concatenate((prim.real, -prim.imag[:, tail]), axis=1)
    im = np.concatenate((prim.imag, prim.real[:, tail]), axis=1)
    dp = tr.serialize_gradients(pg)
    assert np.array_equal(re, dp.real) and np.array_equal(im, dp.imag)
    Pt = dp.shape[1]
    E = rng.standard_normal(W) + 1j * rng.standard_normal(W)
    A = np.concatenate((dp, E[:, None], np.ones((W, 1))), axis=1)
    s = 0.1 + rng.random(W)
    Ar, Ai, sr_, si_ = A.real, A.imag, s[:, None] * A.real[:, :Pt], s[:, None] * A.imag[:, :Pt]
    M = (Ar.T @ sr_ - Ai.T @ si_) + 1j * (Ar.T @ si_ + Ai.T @ sr_)
    ref = A.T @ (s[:, None] * A[:, :Pt])
    assert np.abs(M - ref).max() < 1e-13 * np.abs(ref).max()
    assert np.abs(M[:Pt] - M[:Pt].T).max() < 1e-13 * np.abs(ref).max()  # complex symmetric, no conjugation


def test_abi_entry():
    assert "pqa_sr_moments_c" in _ffi._PROTOTYPES and "pqa_sr_moments_c" in _ffi.header_symbols()
    assert len(_ffi._PROTOTYPES["pqa_sr_moments_c"][1]) == 17
