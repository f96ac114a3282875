"""Gaussian-process Jastrow factor with the protocol of ``pyqmc/wf/gps2.py`` (``GPSJastrow``), computed by the device unit
``csrc/pqa_gps.hip`` behind ``pqa_gps_*``.

    log Psi = sum_s alpha_s sum_{i != j} exp(-f |r_i - X[s, 0]|^2) exp(-f |r_j - X[s, 1]|^2)

The factor lives on a handle of its own, created without a Slater and without a Jastrow part (it carries the electron counts and
the cell), and keeps it under ``_gps`` — not ``_dev``: ``MultiplyWF.fused_device()``, ``vmc.device_of`` and ``readonly_device``
return None for a product that contains it, so such a product takes the per-factor protocol route and the fused estimators leave it
alone.  Walkers, the Gaussians ``e_cs`` and their sums over the electrons stay on the device between calls.

As in the reference, ``e_cs`` is rebuilt by ``recompute`` only: assigning ``Xsupport`` or ``f`` changes the NEW Gaussians of
``testvalue`` / ``gradient*`` / ``updateinternals`` and the distances of ``pgradient`` at once, the stored ones at the next
``recompute``.  A copy (``copy.copy``, pickle) is an independent object on a handle of its own with the same parameters, recomputed
from the resident walkers.
"""

import numpy as np

from . import _ffi
from .wf import DeviceWF, _DeviceFactor, _DeviceParams, _mask_args, _points, _xyz


class _Push:
    """What ``_DeviceParams`` sends an assignment to: the three parameters travel together (``pqa_gps_set``)."""

    def __init__(self, owner):
        self._owner = owner

    def set_param(self, key, value):
        self._owner._push()


class GPSJastrow(_DeviceFactor):
    """``GPSJastrow(mol, X_support, f=100)`` of gps2.py:4-19 on device ``device``.  ``X_support``: (nsupport, 2, 3)."""

    def __init__(self, mol, X_support, f=100, device=0):
        X_support = np.array(X_support, dtype=float)
        if X_support.ndim != 3 or X_support.shape[1:] != (2, 3) or X_support.shape[0] < 1:
            raise ValueError(f"X_support must have shape (nsupport, 2, 3) with nsupport >= 1, got {X_support.shape}")
        self.n_support = X_support.shape[0]
        self.dtype = float
        self._gps = DeviceWF(mol, device=device)
        self._W = 0
        self._bind_parameters({"Xsupport": X_support, "alpha": np.zeros(self.n_support), "f": np.array([f], dtype=float)})
        self._push()

    # ---- parameters / copies
    def _bind_parameters(self, items):
        self.parameters = _DeviceParams(_Push(self), items)

    def _push(self):
        p = self.parameters
        X, a = _ffi.f64(p["Xsupport"]), _ffi.f64(p["alpha"])
        self._gps.call("pqa_gps_set", self.n_support, _ffi.ptr(X), _ffi.ptr(a), float(np.asarray(p["f"]).ravel()[0]))

    def __getstate__(self):
        d = super().__getstate__()
        d["_resident"] = self._get_state()[1] if self._W else None
        return d

    def __setstate__(self, d):
        x = d.pop("_resident")
        super().__setstate__(d)
        self._W = 0
        self._push()
        if x is not None:
            self._recompute(x)

    # ---- protocol
    def _recompute(self, x):
        x = _ffi.f64(x)
        W = x.shape[0]
        u = np.empty(W)
        self._gps.call("pqa_gps_recompute", _ffi.ptr(x), W, _ffi.ptr(u))
        self._W = W
        return np.ones(W), u

    def recompute(self, configs):
        self._push()
        return self._recompute(_xyz(self._gps, configs))

    def value(self):
        u = np.empty(self._W)
        self._gps.call("pqa_gps_value", _ffi.ptr(u))
        return np.ones(self._W), u

    def _eval(self, e, epos, mask, mode):
        m, _ = _mask_args(mask, self._W)
        pts, widx, aux = _points(epos, m, self._gps)
        nrow, npt = pts.shape[0], pts.shape[1]
        out = np.empty(nrow * npt) if mode == 0 else np.empty((4, nrow))
        if nrow:
            self._gps.call("pqa_gps_eval", int(e), _ffi.ptr(pts), nrow, npt, _ffi.ptr(widx), mode, _ffi.ptr(out))
        return out, nrow, npt, aux

    def testvalue(self, e, epos, mask=None):
        r, nrow, npt, aux = self._eval(e, epos, mask, 0)
        return (r.reshape(nrow, npt) if aux else r), np.array([1])

    def gradient_value(self, e, epos):
        r, *_ = self._eval(e, epos, None, 1)
        return r[:3], r[3], np.array([1])

    def gradient(self, e, epos):
        return self._eval(e, epos, None, 1)[0][:3]

    def gradient_laplacian(self, e, epos):
        r, *_ = self._eval(e, epos, None, 2)
        return r[:3], r[3]

    def updateinternals(self, e, epos, configs, mask=None, saved_values=None):
        _, m8 = _mask_args(mask, self._W)
        x = _ffi.f64(_xyz(self._gps, epos))
        if x.shape != (self._W, 3):
            raise ValueError(f"updateinternals takes one position per walker ({self._W}, 3), got {x.shape}")
        self._gps.call("pqa_gps_update", int(e), _ffi.ptr(x), _ffi.ptr(m8))

    def pgradient(self):
        W, ns = self._W, self.n_support
        a, X, f = np.empty((W, ns)), np.empty((W, ns, 2, 3)), np.empty((W, 1))
        self._gps.call("pqa_gps_pgradient", _ffi.ptr(a), _ffi.ptr(X), _ffi.ptr(f))
        return {"alpha": a, "Xsupport": X, "f": f}

    def _get_state(self):
        """(e_cs (W, nsupport, nelec, 2), walkers (W, nelec, 3)) as the device holds them."""
        e, x = np.empty((self._W, self.n_support, self._gps.N, 2)), np.empty((self._W, self._gps.N, 3))
        self._gps.call("pqa_gps_get_state", _ffi.ptr(e), _ffi.ptr(x))
        return e, x
