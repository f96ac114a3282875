"""The correlated entries after they got one host driver (correlated_run, csrc/pqa_correlated.hip), one argument struct and shared
contractions (jas_contract4 / jas_contract1, csrc/pqa_estim.hpp; j3_column), and pqa_variance, whose kernel contracts through the
same helper: every output bit equals what the commit before produced (tests/golden/correlated_parent.npz, recorded by
tools/make_correlated_golden.py from that commit's tree; this file replays the recorder's calls).

Shapes: seven walkers (three where a case has 70 sets) — more than one block of the wave-per-walker kernels, chunks of 3, 3, 1 with
walker_chunk=3 — and set counts at every tail of the 64-set column groups and 16-set tiles (the recorder's table names each)."""

import importlib.util
import os

import numpy as np
import pytest

from tests import helpers

pytestmark = pytest.mark.gpu

_spec = importlib.util.spec_from_file_location("make_correlated_golden", os.path.join(helpers.ROOT, "tools", "make_correlated_golden.py"))
recorder = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(recorder)


@pytest.fixture(scope="module")
def parent():
    return helpers.golden("correlated_parent")


def test_case_list(parent):
    """The fixture holds exactly the recorder's cases, each entry with every output."""
    outputs = {"correlated": {"logpsi", "en"}, "md": {"logpsi", "en"}, "j3": {"logpsi", "en"}, "variance": {"var", "ke"}}
    want = {f"{name}__{o}" for name in recorder.CASES for o in outputs[name.split("__")[0]]} | {"variance__water_k3_dvar__dvar"}
    assert set(parent.files) == want
    assert {recorder.CASES[n][0] for n in recorder.CASES} == {"correlated", "correlated_md", "correlated_j3", "variance"}


@pytest.mark.parametrize("name", list(recorder.CASES))
def test_bitwise_against_parent(parent, name):
    got = recorder.replay(name)
    assert got and all(k in parent.files for k in got)
    for k, v in got.items():
        assert parent[k].dtype == v.dtype and parent[k].shape == v.shape and np.all(np.isfinite(v)), k
        assert np.array_equal(parent[k], v), (k, np.abs(parent[k] - v).max())
