"""The per-electron protocol entries after they got one staging path (csrc/pqa_stage.hpp) and one Python base class
(wf._ScalarFactor): every output bit equals what the commit before produced (tests/golden/protocol_parent.npz, recorded by
tools/make_protocol_golden.py from that commit's tree; this file replays the recorder's calls), an out-of-range walker index is
refused by every entry that takes one before anything is launched, a wrong updateinternals shape is refused by every factor, and
walker indices and points may live in device memory.

Shapes: water (8 electrons), 7 walkers — no multiple of any tile and more than one block of the wave-per-walker kernels (four
walkers a block in the GPS unit) — and 3 auxiliary points per walker."""

import ctypes as C
import importlib.util
import os

import numpy as np
import pytest

from pyqmc_amd import _ffi
from pyqmc_amd.configs import OpenElectron
from tests import helpers

pytestmark = pytest.mark.gpu

_spec = importlib.util.spec_from_file_location("make_protocol_golden", os.path.join(helpers.ROOT, "tools", "make_protocol_golden.py"))
recorder = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(recorder)

W = recorder.W
OPEN = ["slater", "jastrow", "j3", "gps", "geminal"]  # the five factors on water, each on a handle of its own


@pytest.fixture(scope="module")
def cases():
    """name -> (factor, system), each factor as the recorder builds it."""
    return {name: (wf, mol) for name, wf, mol in recorder.factors()}


@pytest.fixture(scope="module")
def replayed(cases):
    out = {}
    for name, (wf, mol) in cases.items():
        out.update(recorder.replay(name, wf, mol))
    return out


def test_bitwise_against_parent(replayed):
    g = helpers.golden("protocol_parent")
    assert sorted(g.files) == sorted(replayed), "the fixture's case list and the replayed one differ"
    assert {k.split("__")[0] for k in replayed} == set(OPEN) | {"product", "slater_complex"}
    bad = [k for k in g.files if not (g[k].dtype == replayed[k].dtype and np.array_equal(g[k], replayed[k]))]
    assert not bad, bad


def _widx_calls(cases):
    """(entry, call(widx pointer)) of every entry that takes walker indices, one row at the origin, after a recompute at W walkers."""
    import pyqmc_amd as pa

    pts, es, out = np.zeros((1, 3)), np.array([0, 5], dtype=np.int32), np.empty(16)
    dev = {name: getattr(cases[name][0], "_dev", None) for name in OPEN}
    dev["gps"], dev["geminal"] = cases["gps"][0]._gps, cases["geminal"][0]._gem
    for name in OPEN:
        wf, mol = cases[name]
        wf.recompute(pa.initial_guess(mol, W, rng=np.random.default_rng(3)))
    p = _ffi.ptr
    yield "pqa_slater_eval", "slater", lambda w: dev["slater"].call("pqa_slater_eval", 0, p(pts), 1, 1, w, 1, 0, p(out))
    yield "pqa_jastrow_eval", "jastrow", lambda w: dev["jastrow"].call("pqa_jastrow_eval", 0, p(pts), 1, 1, w, 0, p(out))
    yield "pqa_j3_eval", "j3", lambda w: dev["j3"].call("pqa_j3_eval", 0, p(pts), 1, 1, w, 0, p(out))
    yield "pqa_testvalue_many", "slater", lambda w: dev["slater"].call("pqa_testvalue_many", p(es), 2, p(pts), 1, w, 1, p(out))
    yield "pqa_gps_eval", "gps", lambda w: dev["gps"].call("pqa_gps_eval", 0, p(pts), 1, 1, w, 0, p(out))
    yield "pqa_geminal_eval", "geminal", lambda w: dev["geminal"].call("pqa_geminal_eval", 0, p(pts), 1, 1, w, 0, 0, p(out))
    yield "pqa_geminal_testvalue_many", "geminal", lambda w: dev["geminal"].call("pqa_geminal_testvalue_many", p(es), 2, p(pts), 1, w, p(out))


def test_walker_index_out_of_range_is_refused(cases):
    """The check runs on the host, on a copy of the indices, before the entry launches anything (stage_points)."""
    for entry, name, call in _widx_calls(cases):
        wf = cases[name][0]
        before = wf.value()
        for bad in (W, -1):
            with pytest.raises(_ffi.PqaError, match="walker index"):
                call(_ffi.ptr(np.array([bad], dtype=np.int32)))
        after = wf.value()
        assert all(np.array_equal(a, b) for a, b in zip(before, after)), entry


def test_updateinternals_wants_one_position_per_walker(cases):
    import pyqmc_amd as pa

    for name in OPEN:
        wf, mol = cases[name]
        configs = pa.initial_guess(mol, W, rng=np.random.default_rng(3))
        wf.recompute(configs)
        with pytest.raises(ValueError, match=rf"one position per walker \({W}, 3\)"):
            wf.updateinternals(0, OpenElectron(np.zeros((W - 1, 3))), configs)


def _device_pointer_worker(q):
    """In a process of its own, where torch initialises the GPU before the library does (as in the distributed tests)."""
    try:
        import torch

        torch.cuda.set_device(0)
        import pyqmc_amd as pa

        rng = np.random.default_rng(5)
        widx = np.array([1, 4, 6], dtype=np.int32)
        pts = rng.standard_normal((3, 1, 3))
        tp, tw = torch.from_numpy(pts).to("cuda:0"), torch.from_numpy(widx).to("cuda:0")
        torch.cuda.synchronize()  # the library reads them on its own stream
        res = {}
        for name, wf, mol in recorder.factors():
            if name in ("jastrow", "gps"):
                wf.recompute(pa.initial_guess(mol, W, rng=np.random.default_rng(3)))
                dev, entry = (wf._dev, "pqa_jastrow_eval") if name == "jastrow" else (wf._gps, "pqa_gps_eval")
                host, got = np.empty((4, 3)), np.empty((4, 3))
                dev.call(entry, 2, _ffi.ptr(pts), 3, 1, _ffi.ptr(widx), 1, _ffi.ptr(host))
                dev.call(entry, 2, C.c_void_p(tp.data_ptr()), 3, 1, C.c_void_p(tw.data_ptr()), 1, _ffi.ptr(got))
                res[name] = (host, got)
            if name == "gps":
                break
        q.put(res)
    except BaseException as exc:  # (the parent must not wait for a result that will not come)
        q.put(repr(exc))
        raise


def test_device_pointers_for_points_and_walker_indices():
    """pts and widx of 3 of the 7 walkers in device memory (torch tensors, data_ptr() as dist.py hands buffers over) give the bits
    of the host-pointer call."""
    import torch.multiprocessing as mp

    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    p = ctx.Process(target=_device_pointer_worker, args=(q,))
    p.start()
    res = q.get(timeout=300)
    p.join(timeout=60)
    assert p.exitcode == 0 and sorted(res) == ["gps", "jastrow"], res
    for name, (host, got) in res.items():
        assert np.all(np.isfinite(host)) and np.any(host != 0) and np.array_equal(got, host), name
