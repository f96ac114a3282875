"""The six multi-handle entries after they got one call prologue (MultiCall), one per-handle loop (multi_each) and one sweep driver
(multi_sweeps, csrc/pqa_multi.hpp): every output bit, and after the two sweep entries every handle's walkers and value, equals what the
commit before produced (tests/golden/multi_parent.npz, recorded by tools/make_multi_golden.py from that commit's tree; this file
replays the recorder's calls).

Shapes: 7 walkers (less than one 256-thread block) and 300 (two blocks with a tail, four chunks of the estimators' products with
walker_chunk=80); K = 1, 2, 3 for every entry and 8 where the K-indexed tables are widest; 0, 1 and 3 sweeps; the recorder's table
names what each case guards.  The vanished-determinant cases (two up electrons of one walker at one point: the multi_update branch that
rebuilds the Slater state) are compared with NaNs counting as equal and need not be finite; the parent's two recordings of them agreed
bit for bit."""

import importlib.util
import os

import numpy as np
import pytest

from tests import helpers

pytestmark = pytest.mark.gpu

_spec = importlib.util.spec_from_file_location("make_multi_golden", os.path.join(helpers.ROOT, "tools", "make_multi_golden.py"))
recorder = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(recorder)


@pytest.fixture(scope="module")
def parent():
    return helpers.golden("multi_parent")


def test_case_list(parent):
    """The fixture holds exactly the recorder's cases, and the table covers every entry."""
    assert {k.rsplit("__", 1)[0] for k in parent.files} == set(recorder.CASES)
    assert {c[0] for c in recorder.CASES.values()} == {"overlap_sweeps", "add_sweeps", "add_weights", "add_energy", "mix_moments", "mix_wtdp"}
    assert len(recorder.NAN_CASES) == 2


@pytest.mark.parametrize("name", list(recorder.CASES))
def test_bitwise_against_parent(parent, name):
    got = recorder.replay(name)
    assert got and set(got) == {k for k in parent.files if k.rsplit("__", 1)[0] == name}
    nan_ok = name in recorder.NAN_CASES
    for k, v in got.items():
        assert parent[k].dtype == v.dtype and parent[k].shape == v.shape and (nan_ok or np.all(np.isfinite(v))), k
        assert np.array_equal(parent[k], v, equal_nan=nan_ok and v.dtype.kind == "f"), (k, np.abs(parent[k] - v).max())
