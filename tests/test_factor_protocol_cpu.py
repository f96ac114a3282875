"""wf._ScalarFactor / wf._OwnHandle, the Python side of the per-electron protocol of the four scalar factors, over a fake handle that
records ``call(name, *args)``: which entries each factor calls and with how many arguments, the output shapes of the three modes, no
call for an empty mask, the saved-values slots, the (W, 3) check of updateinternals, and what a pickle of a factor on a handle of
its own does on the other side."""

import ctypes as C
import pickle

import numpy as np
import pytest

from pyqmc_amd import wf as wfmod
from pyqmc_amd.configs import OpenConfigs, OpenElectron
from pyqmc_amd.geminal import GeminalJastrow
from pyqmc_amd.gps import GPSJastrow

W, N = 5, 2
RESIDENT = np.arange(W * N * 3, dtype=float).reshape(W, N, 3)


class FakeHandle:
    """Stands in for DeviceWF: records the calls; a recompute's walkers are kept as an array."""

    twisted = False
    N = N

    def __init__(self):
        self.W, self.calls, self.walkers = 0, [], None

    def call(self, name, *args):
        self.calls.append((name, args))
        if name.endswith("_recompute"):
            self.walkers = np.ctypeslib.as_array(C.cast(args[0], C.POINTER(C.c_double)), shape=(args[1], N, 3)).copy()

    def set_param(self, key, value):
        self.calls.append(("set_param", (key,)))

    def names(self):
        return [c[0] for c in self.calls]

    def __getstate__(self):  # (recorded pointers do not travel)
        return {"W": self.W}

    def __setstate__(self, d):
        self.__init__()
        self.W = d["W"]


class _Gps(GPSJastrow):
    def _get_state(self):
        return None, RESIDENT


class _Gem(GeminalJastrow):
    def _get_state(self):
        return None, RESIDENT


def _factor(prefix):
    h = FakeHandle()
    if prefix in ("pqa_jastrow", "pqa_j3"):
        f = object.__new__(wfmod.JastrowSpin if prefix == "pqa_jastrow" else wfmod.ThreeBodyJastrow)
        f._dev = h
        f._bind_parameters({"coeff": np.zeros(2)})
    elif prefix == "pqa_gps":
        f = object.__new__(_Gps)
        f._gps, f._W, f.n_support = h, 0, 1
        f._bind_parameters({"Xsupport": np.zeros((1, 2, 3)), "alpha": np.zeros(1), "f": np.ones(1)})
    else:
        f = object.__new__(_Gem)
        f._gem, f._W, f._saved, f.nao = h, 0, None, 2
        f._bind_parameters({"gcoeff": np.zeros(3)})
    return f, h


PREFIXES = ["pqa_jastrow", "pqa_j3", "pqa_gps", "pqa_geminal"]
OWN = {"pqa_gps": "pqa_gps_set", "pqa_geminal": "pqa_geminal_set"}


def _recomputed(prefix):
    f, h = _factor(prefix)
    sign, u = f.recompute(OpenConfigs(RESIDENT.copy()))
    assert np.array_equal(sign, np.ones(W)) and u.shape == (W,)
    return f, h


@pytest.mark.parametrize("prefix", PREFIXES)
def test_recompute_pushes_and_records_the_walker_count(prefix):
    f, h = _recomputed(prefix)
    push = [OWN[prefix]] if prefix in OWN else ["set_param"]  # the parameters together, or one by one through the shared DeviceWF
    assert h.names() == push + [prefix + "_recompute"]
    assert np.array_equal(h.walkers, RESIDENT)
    assert (f._W, h.W) == (W, 0) if prefix in OWN else h.W == W  # the factor's own count, or the shared DeviceWF's
    h.calls.clear()
    sign, u = f.value()
    assert h.names() == [prefix + "_value"] and sign.shape == u.shape == (W,)


@pytest.mark.parametrize("prefix", PREFIXES)
def test_entries_argument_counts_and_shapes(prefix):
    f, h = _recomputed(prefix)
    extra = 1 if prefix == "pqa_geminal" else 0
    one, aux = OpenElectron(np.zeros((W, 3))), OpenElectron(np.zeros((W, 4, 3)))
    mask = np.array([1, 0, 1, 1, 0], dtype=bool)
    h.calls.clear()
    assert f.testvalue(1, one)[0].shape == (W,)
    assert f.testvalue(1, aux)[0].shape == (W, 4)
    assert f.testvalue(1, one, mask)[0].shape == (3,)
    assert f.testvalue(1, aux, mask)[0].shape == (3, 4)
    g, v = f.gradient_value(1, one)[:2]
    assert g.shape == (3, W) and v.shape == (W,)
    assert f.gradient(1, one).shape == (3, W)
    g, lap = f.gradient_laplacian(1, one)
    assert g.shape == (3, W) and lap.shape == (W,)
    assert h.names() == [prefix + "_eval"] * 7
    assert all(len(a) == 7 + extra for _, a in h.calls)
    # (e, pts, nrow, npt, widx, mode[, keep_saved], out)
    assert [(a[0], a[2], a[3], a[4] is None, a[5]) for _, a in h.calls] == [
        (1, W, 1, True, 0), (1, W, 4, True, 0), (1, 3, 1, False, 0), (1, 3, 4, False, 0), (1, W, 1, True, 1), (1, W, 1, True, 1), (1, W, 1, True, 2)]
    h.calls.clear()
    f.updateinternals(1, one, None, mask=mask)
    f.updateinternals(1, one, None)
    assert h.names() == [prefix + "_update"] * 2 and all(len(a) == 3 + extra for _, a in h.calls)
    assert h.calls[0][1][2] is not None and h.calls[1][1][2] is None  # the byte mask, or NULL


@pytest.mark.parametrize("prefix", PREFIXES)
def test_empty_mask_makes_no_call(prefix):
    f, h = _recomputed(prefix)
    h.calls.clear()
    none = np.zeros(W, dtype=bool)
    assert f.testvalue(0, OpenElectron(np.zeros((W, 3))), none)[0].shape == (0,)
    assert f.testvalue(0, OpenElectron(np.zeros((W, 4, 3))), none)[0].shape == (0, 4)
    assert h.calls == []
    with pytest.raises(ValueError, match="one entry per walker"):
        f.testvalue(0, OpenElectron(np.zeros((W, 3))), np.zeros(W + 1, dtype=bool))


@pytest.mark.parametrize("prefix", PREFIXES)
def test_updateinternals_checks_the_shape_before_the_call(prefix):
    f, h = _recomputed(prefix)
    h.calls.clear()
    for bad in (np.zeros((W - 1, 3)), np.zeros((W, 2, 3)), np.zeros((W, 2))):
        with pytest.raises(ValueError, match=rf"one position per walker \({W}, 3\)"):
            f.updateinternals(0, OpenElectron(bad), None)
    assert h.calls == []


def test_saved_values_slots():
    one = OpenElectron(np.zeros((W, 3)))
    for prefix in ("pqa_jastrow", "pqa_j3"):
        f, _ = _recomputed(prefix)
        assert f.testvalue(0, one)[1] is None and f.gradient_value(0, one)[2] is None
    f, _ = _recomputed("pqa_gps")
    assert np.array_equal(f.testvalue(0, one)[1], np.array([1])) and np.array_equal(f.gradient_value(0, one)[2], np.array([1]))
    f, h = _recomputed("pqa_geminal")
    h.calls.clear()
    assert f.testvalue(0, one)[1] is None
    token = f.gradient_value(1, one)[2]
    assert token[:2] == ("pqa-geminal-saved", 1) and f._saved is token
    assert [a[6] for _, a in h.calls] == [0, 1]  # keep_saved: gradient_value alone
    f.updateinternals(1, one, None, saved_values=token)
    assert h.calls[-1][0] == "pqa_geminal_update" and h.calls[-1][1][3] == 1 and f._saved is None
    f.updateinternals(1, one, None, saved_values=token)  # the row was used: a stale token
    assert h.calls[-1][1][3] == 0
    token = f.gradient_value(1, one)[2]
    f.updateinternals(0, one, None, saved_values=token)  # another electron
    assert h.calls[-1][1][3] == 0
    for evaluate in (lambda: f.gradient(1, one), lambda: f.testvalue(1, one), lambda: f.gradient_laplacian(1, one),
                     lambda: f.testvalue_many([0, 1], one), lambda: f.recompute(OpenConfigs(RESIDENT.copy()))):
        token = f.gradient_value(1, one)[2]
        evaluate()  # every evaluation invalidates the kept row
        assert f._saved is None
        f.updateinternals(1, one, None, saved_values=token)
        assert h.calls[-1][1][3] == 0


@pytest.mark.parametrize("prefix", list(OWN))
def test_pickle_pushes_then_recomputes_from_the_resident_walkers(prefix):
    f, h = _recomputed(prefix)
    if prefix == "pqa_geminal":
        f.gradient_value(0, OpenElectron(np.zeros((W, 3))))
    twin = pickle.loads(pickle.dumps(f))
    th = twin._handle
    assert th is not h and th.names() == [OWN[prefix], prefix + "_recompute"]
    assert np.array_equal(th.walkers, RESIDENT) and twin._W == W and getattr(twin, "_saved", None) is None
    assert all(np.array_equal(twin.parameters[k], v) for k, v in f.parameters.items())
    h.calls.clear()
    twin.parameters[next(iter(twin.parameters))] = twin.parameters[next(iter(twin.parameters))]  # an assignment travels through _Push
    assert th.names()[-1] == OWN[prefix] and h.calls == []
    fresh, fh = _factor(prefix)  # never recomputed: nothing resident, nothing to recompute
    assert pickle.loads(pickle.dumps(fresh))._handle.names() == [OWN[prefix]]
