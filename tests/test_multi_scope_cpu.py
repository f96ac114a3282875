"""The scope of the multi-handle device calls on stand-in objects (no device): sample_many.fused_scope and AddWF.scope share the loop
over their members (sample_many.component_devices) and keep every reason string they had before they shared it, letter for letter, and
neither reports a reason that belongs to the other."""

from types import SimpleNamespace

import numpy as np
import pytest

from pyqmc_amd import sample_many
from pyqmc_amd.addwf import AddWF


def dev(device=0, pbc=False, twisted=False, nelec=(4, 4)):
    return SimpleNamespace(device=device, pbc=pbc, twisted=twisted, nelec=nelec, N=sum(nelec))


def wf(d):
    """A product on the handle ``d`` (None: a product that is on no single handle)."""
    return SimpleNamespace(_product_device=lambda: d)


def add_scope(coeffs, comps):
    return AddWF.scope(SimpleNamespace(coeffs=coeffs, wf_components=comps))


HOST = SimpleNamespace()  # a wave function without a device route at all
OPEN = SimpleNamespace(configs=np.zeros((4, 8, 3)))

FUSED = [  # (wave functions, configs, the reason the parent gives)
    ([], None, "0 wave functions (the device calls take 1 to 8)"),
    ([wf(dev()) for _ in range(9)], None, "9 wave functions (the device calls take 1 to 8)"),
    ([wf(dev())], SimpleNamespace(configs=np.zeros((4, 8, 3)), wrap=np.zeros((4, 8, 3))), "periodic walkers"),
    ([wf(dev())], SimpleNamespace(configs=np.zeros((2, 4, 8, 3))), "periodic walkers"),
    ([wf(dev()), HOST], OPEN, "wave function 1 is not a real Slater x two-body Jastrow product on one device handle"),
    ([wf(None), wf(dev())], None, "wave function 0 is not a real Slater x two-body Jastrow product on one device handle"),
    ([wf(dev()), wf(dev()), wf(dev(pbc=True))], None, "wave function 2 is periodic"),
    ([wf(dev()), wf(dev(twisted=True))], None, "wave function 1 is periodic"),
    ([wf(dev(device=1)), wf(dev())], None, "the handles are on different devices"),
]

ADD = [  # (coefficients, components, the reason the parent gives)
    ([1.0] * 9, [wf(dev()) for _ in range(9)], "more than 8 components"),
    ([1.0, 0.5 + 0.1j], [wf(dev()), wf(dev())], "complex coeffs"),
    ([1.0, 0.5], [wf(dev()), HOST], "component 1 is not a real Slater x two-body Jastrow product on one device handle"),
    ([1.0, 0.5], [wf(None), wf(dev())], "component 0 is not a real Slater x two-body Jastrow product on one device handle"),
    ([1.0, 0.5, 0.2], [wf(dev()), wf(dev()), wf(dev(pbc=True))], "component 2 is periodic"),
    ([1.0, 0.5], [wf(dev()), wf(dev(twisted=True))], "component 1 is periodic"),
    ([1.0, 0.5], [wf(dev(device=1)), wf(dev())], "the components live on different devices"),
    ([1.0, 0.5], [wf(dev()), wf(dev(nelec=(5, 3)))], "the components have different electrons"),
    ([1.0, 0.5], [wf(dev()), wf(dev(nelec=(5, 4)))], "the components have different electrons"),
]


@pytest.mark.parametrize("wfs,configs,why", FUSED)
def test_fused_scope_reasons(wfs, configs, why):
    assert sample_many.fused_scope(wfs, configs) == (None, why)
    assert sample_many.fused_handles(wfs, configs) is None


def test_fused_scope_shared_handle():
    d = dev()
    assert sample_many.fused_scope([wf(dev()), wf(d), wf(d)]) == (None, "two wave functions share a device handle")
    # the order of the checks: a shared handle is named before a second device, a member before either
    assert sample_many.fused_scope([wf(d), wf(d), wf(dev(device=1))])[1] == "two wave functions share a device handle"
    assert sample_many.fused_scope([wf(d), wf(d), wf(dev(device=1)), HOST])[1].startswith("wave function 3 is not")
    assert sample_many.fused_scope([wf(dev())] * 9, SimpleNamespace(configs=np.zeros((4, 3))))[1].startswith("9 wave functions")


@pytest.mark.parametrize("coeffs,comps,why", ADD)
def test_addwf_scope_reasons(coeffs, comps, why):
    assert add_scope(coeffs, comps) == (None, why)


def test_in_scope_returns_the_handles():
    ds = [dev(), dev(), dev()]
    assert sample_many.fused_scope([wf(d) for d in ds], OPEN) == (ds, None)
    assert sample_many.fused_handles([wf(d) for d in ds]) == ds
    assert add_scope([0.5, -0.5, 1.0 + 0j], [wf(d) for d in ds]) == (ds, None)  # (a complex dtype with no imaginary part is real)


def test_neither_caller_reports_the_others_reasons():
    d = dev()
    # fused_scope does not look at the electrons or the coefficients; AddWF.scope does not look for a shared handle (its constructor
    # refuses that) or at walkers, and counts in its own words
    assert sample_many.fused_scope([wf(dev()), wf(dev(nelec=(5, 3)))])[1] is None
    assert add_scope([1.0, 0.5], [wf(d), wf(d)]) == ([d, d], None)
    assert add_scope([1.0, 0.5], [wf(d), wf(dev(nelec=(5, 3)))])[1] == "the components have different electrons"
    mine = {w for _, _, w in FUSED} | {"two wave functions share a device handle"}
    theirs = {w for _, _, w in ADD}
    assert not mine & theirs
    for wfs, configs, _ in FUSED:
        assert sample_many.fused_scope(wfs, configs)[1] not in theirs
    for coeffs, comps, _ in ADD:
        assert add_scope(coeffs, comps)[1] not in mine
    # the same members, each caller's own noun
    members = [wf(dev()), wf(dev(pbc=True))]
    assert sample_many.fused_scope(members)[1] == "wave function 1 is periodic" and add_scope([1.0, 1.0], members)[1] == "component 1 is periodic"
