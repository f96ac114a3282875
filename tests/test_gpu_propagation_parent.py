"""The two propagation entries after they got one call prologue (StepCall), one MoveBuf builder (step_moves), one draws descriptor
(dmc_draws) and the T-move phase as functions (tmove_phase), and the per-step DMC loops of pyqmc_amd.dmc after they became one
(_propagate_stepwise): every output bit, and after each call the resident walkers, the value, the last energy rows and the wrap
increments, equals what the commit before produced (tests/golden/propagation_parent.npz, recorded by tools/make_propagation_golden.py
from that commit's tree; this file replays the recorder's calls).

Shapes: 7 walkers (less than one block, the odd tail of the four-walker T-move blocks) and 300 (a tail in 256-thread grids); 1 and 3
steps; the recorder's table names what each case guards.  Two cases record the text of a refusal."""

import importlib.util
import os

import numpy as np
import pytest

from tests import helpers

pytestmark = pytest.mark.gpu

_spec = importlib.util.spec_from_file_location("make_propagation_golden", os.path.join(helpers.ROOT, "tools", "make_propagation_golden.py"))
recorder = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(recorder)


@pytest.fixture(scope="module")
def parent():
    return helpers.golden("propagation_parent")


def test_case_list(parent):
    """The fixture holds exactly the recorder's cases; the table covers the three kinds, every sweep route with and without tapes, both
    walker counts and both step counts."""
    assert {k.rsplit("__", 1)[0] for k in parent.files} == set(recorder.CASES)
    cases = recorder.CASES.values()
    assert {c[0] for c in cases} == {"vmc", "dmc", "loop"}
    assert {(c[4]["route"], c[4]["tapes"]) for c in cases if c[0] == "vmc" and c[1] == "water"} == {(r, t) for r in recorder.ROUTES if r for t in (False, True)}
    assert {c[2] for c in cases} == {7, 300} and {c[3] for c in cases} == {1, 3}
    assert {c[4].get("batched") for c in cases if c[0] == "dmc"} == {None, *recorder.SELECTIONS}


@pytest.mark.parametrize("name", list(recorder.CASES))
def test_bitwise_against_parent(parent, name):
    got = recorder.replay(name)
    assert got and set(got) == {k for k in parent.files if k.rsplit("__", 1)[0] == name}
    for k, v in got.items():
        assert parent[k].dtype == v.dtype and parent[k].shape == v.shape and np.all(np.isfinite(v)), k
        assert np.array_equal(parent[k], v), (k, bytes(v) if k.endswith("__message") else int((parent[k] != v).sum()))
