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
from .wf import DeviceWF, _OwnHandle, _ScalarFactor, _mask_args, _xyz

_serial = itertools.count()


class GeminalJastrow(_OwnHandle, _ScalarFactor):
    """``GeminalJastrow(mol)`` of geminaljastrow.py:49-68 on device ``device``; ``parameters["gcoeff"]``: nao (nao + 1) / 2 zeros."""

    _entry, _handle_attr = "pqa_geminal", "_gem"

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

    def _push(self):
        p = _ffi.f64(self.parameters["gcoeff"]).ravel()
        self._gem.call("pqa_geminal_set", _ffi.ptr(p), p.size)

    def __getstate__(self):
        d = super().__getstate__()
        d["_saved"] = None
        return d

    # ---- protocol: the base class's, with the saved AO row (invalidated by every evaluation) threaded through
    def _recompute(self, x):
        self._saved = None
        return super()._recompute(x)

    def _eval(self, e, epos, mask, mode, keep=False):
        self._saved = None
        return super()._eval(e, epos, mask, mode, int(keep))

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

    def _update_extra(self, e, saved_values):
        use_saved = saved_values is not None and saved_values is self._saved and saved_values[1] == int(e)
        self._saved = None  # (the update consumes the kept row)
        return (int(use_saved),)

    def pgradient(self):
        out = np.empty((self._W, self.nao * (self.nao + 1) // 2))
        self._gem.call("pqa_geminal_pgradient", _ffi.ptr(out))
        return {"gcoeff": out}

    def _get_state(self):
        """(ao_val (W, nelec, nao), walkers (W, nelec, 3)) as the device holds them."""
        a, x = np.empty((self._W, self._gem.N, self.nao)), np.empty((self._W, self._gem.N, 3))
        self._gem.call("pqa_geminal_get_state", _ffi.ptr(a), _ffi.ptr(x))
        return a, x
