"""Superposition wave functions — ``AddWF`` with the protocol of ``pyqmc/wf/addwf.py``.

``AddWF(coeffs, wf_components)`` is Psi = sum_k c_k Psi_k over any protocol objects: device factors, ``MultiplyWF`` products on one
handle each, or the CPU oracle's wave functions.  Every method follows from the weights w_k(R) = c_k Psi_k(R) / Psi(R), sum_k w_k = 1:

    testvalue(e, r)         Psi(R') / Psi(R) = sum_k w_k tv_k                 (tv_k: the component's testvalue; R': e moved to r)
    testvalue_many          sum_k w_k tvm_k
    ratio(e, r)             rho_k = w_k tv_k / sum_j w_j tv_j                 (the weights at R')
    gradient                sum_k rho_k g_k
    gradient_laplacian      (sum_k rho_k g_k, sum_k rho_k l_k)
    gradient_value          (sum_k rho_k g_k, sum_k w_k val_k, the components' saved values)
    pgradient               each component's entries times w_k ("wf{k}..." keys; none for ``coeffs``)

Each device component lives on a handle of its own; two components on one handle are refused.  Copy and pickle rebuild every
component's handle (as ``MultiplyWF``) and re-bind the ``wf{k}`` parameter view.

Two routes.  ``"protocol"`` is NumPy over the components' outputs and takes anything, complex ``coeffs`` and components included.
``"fused"`` is for real Slater x two-body Jastrow products on distinct handles of one device, open boundaries, at most 8 components and
real ``coeffs`` (the scope of ``pqa_overlap_sweeps``): ``value``, ``ratio_current_config`` and ``pgradient`` then take their weights from
``pqa_add_weights``, ``pyqmc_amd.vmc_worker`` moves the walkers with ``pqa_add_sweeps`` and ``EnergyAccumulator`` evaluates
``pqa_add_energy`` (the energy has no protocol route: an in-scope ``AddWF`` is evaluated there whatever its ``route``).  The entry
points read the handles as they are: parameters reach a handle when they are assigned, walkers and inverses with ``recompute`` /
``updateinternals``, exactly as on the protocol route.  ``route=None`` (default) takes the fused route when in scope; ``route="fused"`` raises a ``ValueError`` naming the
reason when not.  ``last_route`` records what the last call ran.

Deliberate differences from the reference:

* the reference value of the log-sum-exp is each walker's own maximum over the components; the reference takes one maximum over all
  walkers (addwf.py:42, :67, :116) and underflows to 0 / 0 when walkers differ by hundreds in log|Psi|;
* ``updateinternals(saved_values=None)`` works; the reference reads a missing ``self.wf_factors`` (addwf.py:55).
"""

import numpy as np

from . import _ffi
from .sample_many import component_devices, finish, handle_array
from .wf import Parameters

MAX_FUSED = 8


def _handles(wf):
    """ids of the device handles a component lives on (empty for host wave functions)."""
    parts = getattr(wf, "wf_factors", None) or getattr(wf, "wf_components", None)
    if parts:
        return set().union(*[_handles(f) for f in parts])
    d = getattr(wf, "_dev", None)
    return set() if d is None else {id(d)}


def add_weights(devs, coeffs, sign=True, logabs=True, w=True):
    """``pqa_add_weights`` -> (sign (W), log|Psi| (W), w (K, W)); None where not asked for."""
    K, W = len(devs), devs[0].W
    c = _ffi.f64(coeffs)
    s = np.empty(W) if sign else None
    l = np.empty(W) if logabs else None
    wk = np.empty((K, W)) if w else None
    finish(devs, _ffi.lib().pqa_add_weights(handle_array(devs), K, _ffi.ptr(c), _ffi.ptr(s), _ffi.ptr(l), _ffi.ptr(wk)))
    return s, l, wk


def add_sweeps(devs, coeffs, tstep, gauss, unif):
    """``pqa_add_sweeps`` with the tapes gauss (nsteps*N, W, 3), scaled by sqrt(tstep), and unif (nsteps*N, W) -> acceptance (nsteps)."""
    K, N = len(devs), devs[0].N
    nsteps = gauss.shape[0] // N
    c, gauss, unif = _ffi.f64(coeffs), _ffi.f64(gauss), _ffi.f64(unif)
    acc = np.empty(nsteps)
    rc = _ffi.lib().pqa_add_sweeps(handle_array(devs), K, _ffi.ptr(c), float(tstep), int(nsteps), _ffi.ptr(gauss), _ffi.ptr(unif), _ffi.ptr(acc))
    finish(devs, rc, moved=True)
    return acc


def add_energy(devs, coeffs, threshold=10.0, rot=None, unif=None, seed=0):
    """``pqa_add_energy`` -> (6, W): ke, ee, ei, ecp, grad2, total of the superposition; every handle with the same ECP draws."""
    K, W = len(devs), devs[0].W
    c = _ffi.f64(coeffs)
    rot = None if rot is None else _ffi.f64(rot)
    unif = None if unif is None else _ffi.f64(unif)
    out = np.empty((6, W))
    rc = _ffi.lib().pqa_add_energy(handle_array(devs), K, _ffi.ptr(c), float(threshold), _ffi.ptr(rot), _ffi.ptr(unif), int(seed), _ffi.ptr(out))
    finish(devs, rc, moved=True)
    return out


class AddWF:
    """Psi = sum_k coeffs[k] wf_components[k] (see the module docstring)."""

    def __init__(self, coeffs, wf_components, route=None):
        if route not in (None, "fused", "protocol"):
            raise ValueError(f"route must be None, 'fused' or 'protocol', not {route!r}")
        if len(coeffs) != len(wf_components) or len(wf_components) < 1:
            raise ValueError("one coefficient per component, and at least one component")
        self.coeffs = coeffs
        self.wf_components = list(wf_components)
        seen = set()
        for k, wf in enumerate(self.wf_components):
            mine = _handles(wf)
            if mine & seen:
                raise ValueError(f"component {k} shares a device handle with an earlier component: every device component of an AddWF "
                                 "needs a handle of its own (copy.deepcopy gives one)")
            seen |= mine
        self.parameters = Parameters([wf.parameters for wf in self.wf_components])
        cplx = any(wf.dtype == complex for wf in self.wf_components) or any(np.iscomplexobj(c) for c in coeffs)
        self.dtype = complex if cplx else float
        self.route = route
        self.last_route = None
        if route == "fused":
            self.fused_devices()

    # ---- copy / pickle: as MultiplyWF, every component is rebuilt on a handle of its own ----------------------------------
    def __getstate__(self):
        return {"coeffs": self.coeffs, "wf_components": self.wf_components, "route": self.route}

    def __setstate__(self, d):  # the "wf{k}key" view must point at the components' re-bound parameter views
        self.__init__(d["coeffs"], d["wf_components"], route=d["route"])

    def __copy__(self):
        import copy

        return copy.deepcopy(self)

    # ---- routes ----------------------------------------------------------------------------------------------------------
    def scope(self):
        """(device handles, None) when the fused entry points can take this wave function, else (None, the reason)."""
        if len(self.wf_components) > MAX_FUSED:
            return None, f"more than {MAX_FUSED} components"
        if any(np.iscomplexobj(c) and np.imag(c) != 0 for c in self.coeffs):
            return None, "complex coeffs"
        devs, why = component_devices(self.wf_components, "component")
        if devs is None:
            return None, why
        if len({d.device for d in devs}) != 1:
            return None, "the components live on different devices"
        if len({(d.nelec, d.N) for d in devs}) != 1:
            return None, "the components have different electrons"
        return devs, None

    def fused_devices(self):
        """The components' handles when the fused route runs (``route`` None or "fused", in scope), else None; ``route="fused"``
        out of scope is a ValueError."""
        if self.route == "protocol":
            return None
        devs, why = self.scope()
        if devs is None and self.route == "fused":
            raise ValueError(f"route='fused' is out of scope: {why}")
        return devs

    def _real_coeffs(self):
        return np.real(np.asarray(self.coeffs)).astype(float)

    def _resident(self, devs):
        return devs is not None and devs[0].W > 0 and len({d.W for d in devs}) == 1

    # ---- values and weights ----------------------------------------------------------------------------------------------
    def _combine(self, vals):
        """Components' (sign, log) -> (sign, log|Psi|, w (K, W)) with each walker's own maximum as the reference value."""
        ph, lv = np.array([v[0] for v in vals]), np.array([v[1] for v in vals])
        ref = np.max(np.real(lv), axis=0)
        t = np.asarray(self.coeffs)[:, None] * ph * np.exp(lv - ref)
        s = np.sum(t, axis=0)
        with np.errstate(divide="ignore", invalid="ignore"):
            return s / np.abs(s), np.log(np.abs(s)) + ref, t / s

    def _state(self, sign=True, logabs=True, w=True):
        devs = self.fused_devices()
        if self._resident(devs):
            self.last_route = "fused"
            return add_weights(devs, self._real_coeffs(), sign, logabs, w)
        self.last_route = "protocol"
        return self._combine([wf.value() for wf in self.wf_components])

    def recompute(self, configs):
        vals = [wf.recompute(configs) for wf in self.wf_components]
        devs = self.fused_devices()
        if self._resident(devs):
            self.last_route = "fused"
            return add_weights(devs, self._real_coeffs(), w=False)[:2]
        self.last_route = "protocol"
        return self._combine(vals)[:2]

    def value(self):
        return self._state(w=False)[:2]

    def ratio_current_config(self, mask=None):
        """c_k Psi_k(R) / Psi(R) -> (K, nconf[mask])."""
        return self._weights(mask)

    def updateinternals(self, e, epos, configs, mask=None, saved_values=None):
        if saved_values is None:
            saved_values = [None] * len(self.wf_components)
        for wf, saved in zip(self.wf_components, saved_values):
            wf.updateinternals(e, epos, configs, mask=mask, saved_values=saved)

    # ---- one-electron quantities -----------------------------------------------------------------------------------------
    @staticmethod
    def _over(w, tv):
        """w (K, n) against tv (K, n) or (K, n, naux)."""
        return w if tv.ndim == 2 else w[:, :, None]

    def _weights(self, mask=None):
        w = self._state(sign=False, logabs=False)[2]
        return w if mask is None else w[:, np.asarray(mask, dtype=bool)]

    def _ratio(self, w, e, epos, mask=None):
        """rho_k from the current weights w (K, nconf[mask]), formed once per protocol call."""
        tv = np.array([wf.testvalue(e, epos, mask=mask)[0] for wf in self.wf_components])
        num = self._over(w, tv) * tv
        with np.errstate(divide="ignore", invalid="ignore"):
            return num / np.sum(num, axis=0)

    def testvalue(self, e, epos, mask=None):
        tv, saved = zip(*[wf.testvalue(e, epos, mask=mask) for wf in self.wf_components])
        tv = np.array(tv)
        return np.sum(self._over(self._weights(mask), tv) * tv, axis=0), saved

    def testvalue_many(self, e, epos, mask=None):
        tvm = np.array([wf.testvalue_many(e, epos, mask=mask) for wf in self.wf_components])
        return np.sum(self._weights(mask)[:, :, None] * tvm, axis=0)

    def ratio(self, e, epos, mask=None):
        """c_k Psi_k(R') / Psi(R') with electron e at epos -> (K, nconf[mask]) (one more axis for auxiliary positions)."""
        return self._ratio(self._weights(mask), e, epos, mask)

    def gradient(self, e, epos):
        rho = self._ratio(self._weights(), e, epos)
        g = np.array([wf.gradient(e, epos) for wf in self.wf_components])
        return np.sum(rho[:, None, :] * g, axis=0)

    def gradient_value(self, e, epos):
        w = self._weights()
        rho = self._ratio(w, e, epos)  # (first: the components keep the rows of their gradient_value call for the update)
        g, vals, saved = zip(*[wf.gradient_value(e, epos) for wf in self.wf_components])
        return np.sum(rho[:, None, :] * np.array(g), axis=0), np.sum(w * np.array(vals), axis=0), saved

    def gradient_laplacian(self, e, epos):
        rho = self._ratio(self._weights(), e, epos)
        g, lap = zip(*[wf.gradient_laplacian(e, epos) for wf in self.wf_components])
        return np.sum(rho[:, None, :] * np.array(g), axis=0), np.sum(rho * np.array(lap), axis=0)

    def pgradient(self):
        w = self.ratio_current_config()
        out = []
        for k, wf in enumerate(self.wf_components):
            pg = wf.pgradient()
            out.append({key: np.asarray(pg[key]) * w[k].reshape((-1,) + (1,) * (np.ndim(pg[key]) - 1)) for key in pg.keys()})
        return Parameters(out)
