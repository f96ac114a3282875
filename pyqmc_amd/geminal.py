"""AO-pair (geminal) Jastrow factor with the protocol of ``pyqmc/wf/geminaljastrow.py`` (``GeminalJastrow``), computed by the device
unit ``csrc/pqa_geminal.hip`` behind ``pqa_geminal_*``.

    log Psi = sum_{i>j} sum_{mn} G_mn chi_m(r_i) chi_n(r_j),        G = triu(gcoeff) + triu(gcoeff)^T

The factor lives on a handle of its own.  The handle needs the basis tables, which ``DeviceWF`` uploads with a Slater part only, so it
is created with the first columns of the identity as orbitals; the unit ignores the Slater state.  The handle sits under ``_gem`` —
not ``_dev``: ``MultiplyWF.fused_device()``, ``vmc.device_of`` and ``readonly_device`` return None for a product that contains the
factor, so such a product takes the per-factor protocol route and the fused estimators leave it alone.  Walkers, their AO values and
the sums over the electrons stay on the device between calls.

As in the reference, the AO values are rebuilt by ``recompute`` only; an assignment to ``gcoeff`` is pushed at once and takes effect
in the next call.  A copy (``copy.copy``, pickle) is an independent object on a handle of its own with the same parameters,
recomputed from the resident walkers.

Scope: open systems, and periodic cells with real Gamma-point AOs of the cell handed in (the AO kernel folds the point into it, as
the reference's ``get_supercell(mol, eye(3))`` evaluator does).  Twisted and complex handles raise ``NotImplementedError``.
"""

import itertools

import numpy as np

from . import _ffi, tables
from .wf import DeviceWF, _DeviceFactor, _DeviceParams, _mask_args, _points, _xyz

_serial = itertools.count()


class _Push:
    """What ``_DeviceParams`` sends an assignment to (``pqa_geminal_set``)."""

    def __init__(self, owner):
        self._owner = owner

    def set_param(self, key, value):
        self._owner._push()


class GeminalJastrow(_DeviceFactor):
    """``GeminalJastrow(mol)`` of geminaljastrow.py:49-68 on device ``device``; ``parameters["gcoeff"]``: nao (nao + 1) / 2 zeros."""

    def __init__(self, mol, device=0, _gem=None):
        if _gem is None:
            if hasattr(mol, "a") and not hasattr(mol, "original_cell"):
                from . import pbc as _pbc

                mol = _pbc.get_supercell(mol, np.eye(3))
            eye = np.eye(tables.basis_tables(mol)["nao"])
            _gem = DeviceWF(mol, mo_coeff=[eye[:, : int(mol.nelec[0])], eye[:, : int(mol.nelec[1])]], device=device)
        if _gem.twisted or _gem.cplx:
            raise NotImplementedError("GeminalJastrow: twisted and complex handles are not supported (real AOs only)")
        self._gem = _gem
        self.nao = int(_gem.nao)
        self.dtype = float
        self._W = 0
        self._saved = None
        self._bind_parameters({"gcoeff": np.zeros(self.nao * (self.nao + 1) // 2)})
        self._push()

    # ---- parameters / copies
    def _bind_parameters(self, items):
        self.parameters = _DeviceParams(_Push(self), items)

    def _push(self):
        p = _ffi.f64(self.parameters["gcoeff"]).ravel()
        self._gem.call("pqa_geminal_set", _ffi.ptr(p), p.size)

    def __getstate__(self):
        d = super().__getstate__()
        d["_resident"] = self._get_state()[1] if self._W else None
        d["_saved"] = None
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
        self._gem.call("pqa_geminal_recompute", _ffi.ptr(x), W, _ffi.ptr(u))
        self._W = W
        self._saved = None
        return np.ones(W), u

    def recompute(self, configs):
        self._push()
        return self._recompute(_xyz(self._gem, configs))

    def value(self):
        u = np.empty(self._W)
        self._gem.call("pqa_geminal_value", _ffi.ptr(u))
        return np.ones(self._W), u

    def _eval(self, e, epos, mask, mode, keep=False):
        m, _ = _mask_args(mask, self._W)
        pts, widx, aux = _points(epos, m, self._gem)
        nrow, npt = pts.shape[0], pts.shape[1]
        out = np.empty(nrow * npt) if mode == 0 else np.empty((4, nrow))
        self._saved = None
        if nrow:
            self._gem.call("pqa_geminal_eval", int(e), _ffi.ptr(pts), nrow, npt, _ffi.ptr(widx), mode, int(keep), _ffi.ptr(out))
        return out, nrow, npt, aux

    def testvalue(self, e, epos, mask=None):
        r, nrow, npt, aux = self._eval(e, epos, mask, 0)
        return (r.reshape(nrow, npt) if aux else r), None

    def testvalue_many(self, e, epos, mask=None):
        """geminaljastrow.py:238-256: ratios for moving each electron of ``e`` to ``epos`` -> (nconf[mask], len(e))."""
        es = np.ascontiguousarray(np.atleast_1d(e), dtype=np.int32)
        x = _xyz(self._gem, epos)
        if x.ndim != 2:
            raise ValueError("testvalue_many takes one position per walker: epos.configs (nconf, 3)")
        m, _ = _mask_args(mask, self._W)
        widx = None
        if m is not None:
            widx = np.ascontiguousarray(np.nonzero(m)[0], dtype=np.int32)
            x = x[m]
        pts = _ffi.f64(x)
        out = np.empty((len(pts), len(es)))
        self._saved = None
        if len(pts) and len(es):
            self._gem.call("pqa_geminal_testvalue_many", _ffi.ptr(es), len(es), _ffi.ptr(pts), len(pts), _ffi.ptr(widx), _ffi.ptr(out))
        return out

    def gradient_value(self, e, epos):
        r, *_ = self._eval(e, epos, None, 1, keep=True)
        self._saved = ("pqa-geminal-saved", int(e), next(_serial))  # names the AO row the device kept
        return r[:3], r[3], self._saved

    def gradient(self, e, epos):
        return self._eval(e, epos, None, 1)[0][:3]

    def gradient_laplacian(self, e, epos):
        r, *_ = self._eval(e, epos, None, 2)
        return r[:3], r[3]

    def updateinternals(self, e, epos, configs, mask=None, saved_values=None):
        _, m8 = _mask_args(mask, self._W)
        x = _ffi.f64(_xyz(self._gem, epos))
        if x.shape != (self._W, 3):
            raise ValueError(f"updateinternals takes one position per walker ({self._W}, 3), got {x.shape}")
        use_saved = saved_values is not None and saved_values is self._saved and saved_values[1] == int(e)
        self._gem.call("pqa_geminal_update", int(e), _ffi.ptr(x), _ffi.ptr(m8), int(use_saved))
        self._saved = None

    def pgradient(self):
        out = np.empty((self._W, self.nao * (self.nao + 1) // 2))
        self._gem.call("pqa_geminal_pgradient", _ffi.ptr(out))
        return {"gcoeff": out}

    def _get_state(self):
        """(ao_val (W, nelec, nao), walkers (W, nelec, 3)) as the device holds them."""
        a, x = np.empty((self._W, self._gem.N, self.nao)), np.empty((self._W, self._gem.N, 3))
        self._gem.call("pqa_geminal_get_state", _ffi.ptr(a), _ffi.ptr(x))
        return a, x
