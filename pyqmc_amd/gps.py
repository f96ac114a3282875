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
from .wf import DeviceWF, _OwnHandle, _ScalarFactor


class GPSJastrow(_OwnHandle, _ScalarFactor):
    """``GPSJastrow(mol, X_support, f=100)`` of gps2.py:4-19 on device ``device``.  ``X_support``: (nsupport, 2, 3)."""

    _entry, _handle_attr = "pqa_gps", "_gps"

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

    def _push(self):
        p = self.parameters
        X, a = _ffi.f64(p["Xsupport"]), _ffi.f64(p["alpha"])
        self._gps.call("pqa_gps_set", self.n_support, _ffi.ptr(X), _ffi.ptr(a), float(np.asarray(p["f"]).ravel()[0]))

    def _saved_values(self):
        return np.array([1])

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
