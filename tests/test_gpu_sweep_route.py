"""Which kernels a sweep runs (sweep_route, csrc/pqa_sweep.hip): the route every handle reports under PQA_RES_DEBUG is the one its
switches force, a system outside a resident sweep's scope falls back without an error, and a periodic handle never takes k_sweep_r8.

What the routes compute is compared pair by pair, bit for bit, elsewhere (test_gpu_conditioning.py, test_gpu_fullsize.py, test_gpu_parity.py);
here only the choice is under test.  2 VMC sweeps on device draws at 24 walkers: no multiple of the 8 walkers of a k_sweep_r8 block or
the 16 of a k_sweep_res block, so the last block of either is partly filled."""

import ast

import numpy as np
import pytest

import conditioning as cond
import helpers
import pyqmc_amd as pa
from pyqmc_amd import _ffi

pytestmark = pytest.mark.gpu

W, NS = 24, 2
SWITCHES = ("PQA_RES", "PQA_R8", "PQA_LW", "PQA_WW")
FORCED = [("k_sweep_r8", {"PQA_RES": "1", "PQA_R8": "1"}),
          ("k_sweep_res", {"PQA_RES": "1", "PQA_R8": "0"}),
          ("k_step_lw", {"PQA_RES": "0"}),
          ("k_sweep_ww", {"PQA_LW": "0", "PQA_WW": "1"}),
          ("k_propose/k_accept", {"PQA_LW": "0", "PQA_WW": "0"})]
assert [env for _, env in FORCED[:3]] == list(cond.PATHS.values())  # the three single-determinant paths of the conditioning tests


def _routes(make_wf, mol, env, monkeypatch, capfd):
    """The routes a fresh handle reports over NS sweeps under the switches ``env``; the call returned 0 (vmc_sweeps raises otherwise)
    and left no error text on the handle."""
    for k in SWITCHES:
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)  # read when the handle is created
    monkeypatch.setenv("PQA_RES_DEBUG", "1")
    wf = make_wf()
    dev = wf.fused_device()
    wf.recompute(pa.initial_guess(mol, W, rng=np.random.default_rng(11)))
    capfd.readouterr()
    acc, _, _ = dev.vmc_sweeps(cond.TSTEP, NS, seed=5)
    dev.sync()
    assert np.all((0.0 < np.asarray(acc)) & (np.asarray(acc) <= 1.0))
    assert _ffi.lib().pqa_last_error(dev._h) == b""
    out, err = capfd.readouterr()
    print(out, end="")
    return cond.reported_routes(err)


@pytest.mark.parametrize("kernel,env", FORCED, ids=[k for k, _ in FORCED])
def test_forced_route_is_the_reported_one(kernel, env, monkeypatch, capfd):
    """The water molecule of the conditioning tests (4 + 4 electrons) under each forcing setting: one route line, naming the forced kernel."""
    c = cond.case("water-1e-5")
    assert _routes(lambda: cond.gpu_wf(c.mol, c.mf), c.mol, env, monkeypatch, capfd) == [kernel]


def test_out_of_scope_is_a_silent_fallback(monkeypatch, capfd):
    """The same molecule with the first two determinants of the fixture g8's expansion, resident sweeps forced: no single-determinant
    sweep takes the handle, a wave-per-walker route is reported and nothing is left in pqa_last_error."""
    c = cond.case("multidet-all-1e-5")  # (its mean field carries the virtual orbitals the expansion excites into)
    dets = ast.literal_eval(str(helpers.golden("g8_protocol_h2o_multidet")["det_json"]))[:2]
    routes = _routes(lambda: helpers.gpu_wf(c.mol, c.mf, dets, jastrow_kws={"ion_cusp": False}), c.mol, {"PQA_RES": "1", "PQA_R8": "1"}, monkeypatch, capfd)
    assert len(routes) == 1 and routes[0] in ("k_sweep_ww", "k_propose/k_accept"), routes


@pytest.mark.parametrize("tag,kernel", [("fcc2cubic", "k_sweep_res"), ("gamma", "k_step_lw")])
def test_periodic_handles_never_take_r8(tag, kernel, monkeypatch, capfd):
    """Periodic handles with PQA_RES=1 PQA_R8=1.  The conventional diamond cell, the smallest cell of test_gpu_pbc.py that k_sweep_res
    takes: k_sweep_res and never k_sweep_r8.  The primitive cell, the smallest of all, has 249 lattice-sum candidates where res_setup
    admits 128 (test_gpu_conditioning.py::_pbc_params): out of both resident sweeps' scope, it takes the launch-per-move sweep, again
    without an error."""
    sup, mf = helpers.pbc_slater_case(tag)
    routes = _routes(lambda: helpers.gpu_pbc_wf(None, case=(sup, mf))[1], sup, {"PQA_RES": "1", "PQA_R8": "1"}, monkeypatch, capfd)
    assert routes == [kernel]
