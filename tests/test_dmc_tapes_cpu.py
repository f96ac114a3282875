"""The replay tapes of pqa_dmc_steps on the Python side after the two recorders became one and the shapes one function
(pyqmc_amd.dmc.tape_shapes): what _record_tapes draws from the DMC tests' replay generator equals, bit for bit, what the commit before
drew (tests/golden/dmc_tapes_parent.npz, recorded by tools/make_propagation_golden.py --tapes from that commit's tree), tape_shapes
names those arrays' shapes, and DeviceWF.philox_dmc_tapes allocates through it.  3 electrons, 2 ECP atoms, 5 walkers, 2 steps; the
semi-local integrator with and without T-moves, the batched one with and without a selection that drops points.  No GPU."""

import importlib.util
import os

import numpy as np
import pytest

from pyqmc_amd import _ffi, dmc
from pyqmc_amd.wf import DeviceWF
from tests import helpers

_spec = importlib.util.spec_from_file_location("make_propagation_golden", os.path.join(helpers.ROOT, "tools", "make_propagation_golden.py"))
recorder = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(recorder)
CASES, SHAPE = recorder.TAPE_CASES, recorder.TAPE_SHAPE


def _shapes(name):
    tmoves, batched = CASES[name]
    return dmc.tape_shapes(tmoves=tmoves, batched=batched, **SHAPE)


def test_case_list():
    parent = helpers.golden("dmc_tapes_parent")
    assert {k.rsplit("__", 1)[0] for k in parent.files} == set(CASES)
    assert {(t, b is None) for t, b in CASES.values()} == {(True, True), (False, True), (True, False)}
    names = {n: {k.rsplit("__", 1)[1] for k in parent.files if k.startswith(n + "__")} for n in CASES}
    assert "tm_rot" not in names["semilocal_notm"] and "ecp_unif" in names["batched_drop"] and "ecp_unif" not in names["batched_all"]


@pytest.mark.parametrize("name", list(CASES))
def test_record_tapes_bitwise_against_parent(name):
    parent = helpers.golden("dmc_tapes_parent")
    got = recorder.replay_tapes(name)
    assert got and set(got) == {k for k in parent.files if k.rsplit("__", 1)[0] == name}
    for k, v in got.items():
        assert parent[k].dtype == v.dtype and parent[k].shape == v.shape and np.all(np.isfinite(v)), k
        assert np.array_equal(parent[k], v), k


@pytest.mark.parametrize("name", list(CASES))
def test_tape_shapes_are_the_recorded_shapes(name):
    parent = helpers.golden("dmc_tapes_parent")
    assert {f"{name}__{k}": s for k, s in _shapes(name).items()} == {k: parent[k].shape for k in parent.files if k.startswith(name + "__")}


@pytest.mark.parametrize("name", list(CASES))
def test_philox_dmc_tapes_allocates_through_tape_shapes(name, monkeypatch):
    """A stub handle whose ``call`` records its arguments: the dictionary has tape_shapes' arrays, and the struct handed to
    pqa_philox_dmc_tapes points into exactly those."""
    tmoves, batched = CASES[name]
    asked, calls = [], []
    inner = dmc.tape_shapes
    monkeypatch.setattr(dmc, "tape_shapes", lambda *a, **k: (asked.append((a, k)), inner(*a, **k))[1])
    dev = DeviceWF.__new__(DeviceWF)
    dev.N, dev.necp, dev._ecpb = SHAPE["N"], SHAPE["necp"], batched
    fields = [f for f, _ in _ffi.DmcTapes._fields_]
    dev.call = lambda *a: calls.append(a[:4] + ({f: getattr(_ffi.DmcTapes.from_address(a[4]), f) for f in fields},))  # (the struct, read during the call)
    t = dev.philox_dmc_tapes(9, SHAPE["nsteps"], SHAPE["W"], tmoves=tmoves)
    assert len(asked) == 1 and {k: v.shape for k, v in t.items()} == _shapes(name)
    assert all(v.dtype == np.float64 and v.flags.c_contiguous for v in t.values())
    (entry, seed, nsteps, W, pointers), = calls
    assert (entry, seed, nsteps, W) == ("pqa_philox_dmc_tapes", 9, SHAPE["nsteps"], SHAPE["W"])
    assert pointers == {f: (t[f].ctypes.data if f in t else None) for f in fields}
