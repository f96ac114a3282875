"""Parameter-gradient accumulators — SURVEY.md §8(f2).

Public names, argument meaning and returned keys are those of the reference's ``LinearTransform``
(``pyqmc/observables/accumulators.py:98-185``) and ``StochasticReconfiguration`` / ``PGradTransform``
(``pyqmc/observables/stochastic_reconfiguration.py:22-176``); the implementation is this package's own:

* ``LinearTransform`` keeps, per optimised key, the flat positions of the selected entries; (de)serialisation is fancy
  indexing with those positions.
* ``StochasticReconfiguration.avg`` gets all three moments from ONE product on the fp64 matrix cores (``pqa_gram`` ->
  ``k_gram_mfma``): with ``A = [dp | E | 1]`` (nconf, p+2) and ``B = w f dp`` (nconf, p),
  ``A^T B = [[dpidpj], [dpH], [dppsi]]``.  The per-walker derivatives come from ``wf.pgradient()`` (``k_pgrad_det``,
  ``k_pgrad_mo``, ``k_j3_pgrad``).
* On the device route (``sr_route``) ``avg`` takes energy means and moments from ONE call on the resident state (``pqa_sr_moments``):
  neither the walkers nor the derivative arrays come to the host.  With ``route="device"`` the orbital coefficients of an open
  system are columns too (``pqa_sr_moments_orb``: ``k_sr_orb`` writes them straight into the gathered matrix).  With
  ``complex_device=True`` complex and twisted handles take the route as well (``pqa_sr_moments_c``: complex columns, complex energy).
"""

import numpy as np

from . import _ffi


class LinearTransform:
    """Optimised subset of a parameter dictionary as one real vector.

    ``to_opt[k]``: boolean array shaped like ``parameters[k]``; keys without any selected entry are ignored.  Layout of
    the vector (as the reference, ``accumulators.py:134-150``): selected entries key after key in C order (real parts),
    followed by the imaginary parts of the selected entries of the complex keys."""

    def __init__(self, parameters, to_opt=None):
        if to_opt is None:
            to_opt = {k: np.ones(np.shape(v), dtype=bool) for k, v in parameters.items()}
        self.to_opt, self.shapes, self.dtypes, self._pos = {}, {}, {}, {}
        for k, m in to_opt.items():
            m = np.asarray(m, dtype=bool)
            if not m.any():
                continue
            v = np.asarray(parameters[k])
            self.to_opt[k], self.shapes[k], self.dtypes[k] = m, v.shape, v.dtype
            self._pos[k] = np.flatnonzero(m.ravel())
        self.slices = {k: int(np.prod(s)) for k, s in self.shapes.items()}
        self.complex = {k: np.issubdtype(d, np.complexfloating) for k, d in self.dtypes.items()}
        self.nimag = {k: (len(self._pos[k]) if self.complex[k] else 0) for k in self._pos}
        self.nparams = int(sum(len(p) for p in self._pos.values()))
        flags = [np.full(len(self._pos[k]), self.complex[k]) for k in self._pos]
        self.complex_inds = np.concatenate(flags) if any(self.nimag.values()) else np.zeros(0, dtype=bool)

    def _gather(self, arrays, lead):
        cols = [np.asarray(arrays[k]).reshape(lead + (-1,))[..., p] for k, p in self._pos.items()]
        return np.concatenate(cols, axis=-1) if cols else np.zeros(lead + (0,))

    def serialize_parameters(self, parameters):
        x = self._gather(parameters, ())
        return np.concatenate((x.real, x[self.complex_inds].imag)) if len(self.complex_inds) else np.real(x)

    def serialize_gradients(self, pgrad):
        """(nconf, nparams [+ imaginary tail]) matrix of d log Psi / d p; the tail columns are i times their real twins."""
        if not self._pos:
            return np.zeros(0)
        nconf = np.shape(next(iter(pgrad.values())))[0]
        g = self._gather(pgrad, (nconf,))
        return np.concatenate((g, 1j * g[:, self.complex_inds]), axis=1) if len(self.complex_inds) else g

    def deserialize(self, wf, parameters):
        """Vector -> {key: array}: selected entries from the vector, the rest from ``wf.parameters``."""
        out, re0, im0 = {}, 0, self.nparams
        for k, p in self._pos.items():
            flat = np.array(wf.parameters[k], dtype=self.dtypes[k]).ravel()
            new = np.asarray(parameters[re0 : re0 + len(p)]).real.astype(self.dtypes[k])
            if self.complex[k]:
                new = new + 1j * np.asarray(parameters[im0 : im0 + len(p)])
                im0 += len(p)
            flat[p] = new
            re0 += len(p)
            out[k] = flat.reshape(self.shapes[k])
        return out


def nodal_regularization(grad2, nodal_cutoff=1e-3):
    """Pathak-Wagner weight (``stochastic_reconfiguration.py:22-46``): with the node-distance estimate ``r = 1/grad2`` and
    ``x = r / cutoff^2``, walkers with ``x < 1`` are weighted ``x (9 - 15 x + 7 x^2)``, the others 1.  Returns (mask, f)."""
    x = 1.0 / (np.asarray(grad2, dtype=float) * nodal_cutoff**2)
    near = x < 1.0
    return near, np.where(near, x * (9.0 + x * (-15.0 + 7.0 * x)), 1.0)


def device_gram(wf):
    """``(A, B) -> A^T B`` on the device that holds ``wf`` (``pqa_gram``).  Raises when ``wf`` has no device handle: the
    moment matrices of the product path are never formed on the host."""
    dev = next((d for d in (getattr(w, "_dev", None) for w in [wf, *getattr(wf, "wf_factors", ())]) if hasattr(d, "call")), None)
    if dev is None:
        raise RuntimeError("StochasticReconfiguration needs a wave function resident on the HIP device (pqa_gram)")

    def real_gram(a, b):
        a, b = _ffi.f64(a), _ffi.f64(b)
        c = np.empty((a.shape[1], b.shape[1]))
        dev.call("pqa_gram", a.shape[0], a.shape[1], b.shape[1], _ffi.ptr(a), _ffi.ptr(b), _ffi.ptr(c))
        return c

    def gram(a, b):
        if not (np.iscomplexobj(a) or np.iscomplexobj(b)):
            return real_gram(a, b)
        ar, ai, br, bi = np.real(a), np.imag(a), np.real(b), np.imag(b)  # (ar + i ai)^T (br + i bi), no conjugation
        return real_gram(ar, br) - real_gram(ai, bi) + 1j * (real_gram(ar, bi) + real_gram(ai, br))

    return gram


SR_SOURCES = {"wf1det_coeff": 0, "wf2acoeff": 1, "wf2bcoeff": 2, "wf3ccoeff": 3}  # parameter -> source code of pqa_sr_moments


def sr_columns(transform):
    """``(src, pos)`` of ``pqa_sr_moments`` for a ``LinearTransform`` whose keys are all in ``SR_SOURCES``: column i of the serialised
    derivative matrix is flat entry ``pos[i]`` of the parameter ``src[i]`` names (key after key, selected entries in C order)."""
    src = [np.full(len(p), SR_SOURCES[k], dtype=np.int32) for k, p in transform._pos.items()]
    pos = [np.asarray(p, dtype=np.int32) for p in transform._pos.values()]
    return (np.concatenate(src), np.concatenate(pos)) if src else (np.zeros(0, dtype=np.int32), np.zeros(0, dtype=np.int32))


SR_ORBITAL_SOURCES = {"wf1mo_coeff_alpha": 4, "wf1mo_coeff_beta": 5}  # the further source codes of pqa_sr_moments_orb
SR_MOMENT_BYTES = 256 << 20  # most bytes of the (P + 2, P) moments the device calls take


def sr_columns_orb(transform):
    """``sr_columns`` for a transform whose keys may include the orbital coefficients: ``(src, pos)`` of ``pqa_sr_moments_orb``,
    ``pos`` of an orbital column the flat C-order index into its (nao, nmo_s) matrix."""
    codes = {**SR_SOURCES, **SR_ORBITAL_SOURCES}
    src = [np.full(len(p), codes[k], dtype=np.int32) for k, p in transform._pos.items()]
    pos = [np.asarray(p, dtype=np.int32) for p in transform._pos.values()]
    return (np.concatenate(src), np.concatenate(pos)) if src else (np.zeros(0, dtype=np.int32), np.zeros(0, dtype=np.int32))


def sr_columns_c(transform):
    """``(src, pos, tail)`` of ``pqa_sr_moments_c``: ``sr_columns`` and the primary indices of the entries of complex-dtype keys, whose
    ``1j *`` twins form the tail of the serialised derivative matrix (``LinearTransform.serialize_gradients``)."""
    src, pos = sr_columns(transform)
    return src, pos, np.flatnonzero(transform.complex_inds).astype(np.int32)


def _sr_device(wf, complex_device=False):
    """(device handle, None) when ``wf`` is ``generate_wf``'s product on one real handle - with ``complex_device`` also on a complex or
    twisted one (``pqa_sr_moments_c``) -, else (None, reason)."""
    from . import wf as pwf

    if not isinstance(wf, pwf.MultiplyWF):
        return None, f"{type(wf).__name__} is not a pyqmc_amd.MultiplyWF on one device handle"
    kinds = [type(f) for f in wf.wf_factors]
    if kinds not in ([pwf.Slater, pwf.JastrowSpin], [pwf.Slater, pwf.JastrowSpin, pwf.ThreeBodyJastrow]):
        return None, "factors other than Slater x JastrowSpin [x ThreeBodyJastrow]: " + ", ".join(k.__name__ for k in kinds)
    dev = wf.fused_device()
    if dev is None or not hasattr(dev, "sr_moments"):
        return None, "the factors do not share one device handle"
    if (dev.cplx or dev.twisted) and not complex_device:
        return None, "complex orbitals / twisted cell"
    return dev, None


def sr_route(wf, sr):
    """``("device", reason)`` when ``sr.avg`` can take its moments from the resident state (``pqa_sr_moments``), else
    ``("protocol", reason)``.  The device route needs: ``wf`` on one real device handle (``generate_wf``'s Slater x two-body Jastrow,
    with or without the three-body factor); ``sr.enacc`` a ``pyqmc_amd.EnergyAccumulator`` itself (not a subclass or a stand-in);
    ``sr.transform`` a ``LinearTransform`` whose optimised keys are all among ``SR_SOURCES``; no injected ``gram``.  The orbital
    coefficients (``SR_ORBITAL_SOURCES``) are in the scope only when ``sr.route == "device"`` asks for them, and then for an open
    system (no ``_fold``, no cell) with at most 64 electrons and orbitals of a spin and moments within ``SR_MOMENT_BYTES``; with
    ``route=None`` they keep the protocol route.  A complex or twisted handle is in the scope only for an ``sr`` built with
    ``complex_device=True`` (``pqa_sr_moments_c``), and never with orbital coefficients."""
    from .energy import EnergyAccumulator

    dev, why = _sr_device(wf, getattr(sr, "complex_device", False))
    if dev is None:
        return "protocol", why
    if type(sr.enacc) is not EnergyAccumulator:
        return "protocol", f"the energy object is a {type(sr.enacc).__name__}, not a pyqmc_amd.EnergyAccumulator"
    if sr._gram is not None:
        return "protocol", "an injected gram"
    if type(sr.transform) is not LinearTransform:
        return "protocol", f"the transform is a {type(sr.transform).__name__}, not a pyqmc_amd.LinearTransform"
    other = [k for k in sr.transform.to_opt if k not in SR_SOURCES]
    orbital = [k for k in other if k in SR_ORBITAL_SOURCES]
    if len(orbital) < len(other):
        return "protocol", "parameters without a device source: " + ", ".join(k for k in other if k not in orbital)
    if orbital and (dev.cplx or dev.twisted):
        return "protocol", "orbital coefficients (" + ", ".join(orbital) + ") of complex orbitals / a twisted cell"
    if orbital:
        if sr.route != "device":
            return "protocol", "orbital coefficients (" + ", ".join(orbital) + ") are device columns only on request: route='device' takes them"
        from .wf import orbital_sr_scope

        why = orbital_sr_scope(dev)
        if why is None and getattr(wf.wf_factors[0], "_fold", None) is not None:
            why = "orbital coefficients in the per-k parameter layout (the chain rule of pbc.unfold_mo_gradient)"
        p = sr.transform.nparams
        if why is None and (p + 2) * p * 8 > SR_MOMENT_BYTES:
            why = f"the moments of {p} parameters exceed the {SR_MOMENT_BYTES >> 20} MiB the device call takes"
        if why:
            return "protocol", why
    if sr.transform.nparams == 0:
        return "protocol", "no parameter is optimised"
    if dev.cplx or dev.twisted:
        pt = sr.transform.nparams + int(np.count_nonzero(sr.transform.complex_inds))
        if (pt + 2) * pt * 16 > SR_MOMENT_BYTES:
            return "protocol", f"the complex moments of {pt} columns exceed the {SR_MOMENT_BYTES >> 20} MiB the device call takes"
        return "device", "one complex device handle (complex_device), device energy, every parameter has a device source"
    return "device", "one real device handle, device energy, every parameter has a device source"


class StochasticReconfiguration:
    """Energy plus the moments ``dpH = <E f dp>``, ``dppsi = <f dp>``, ``dpidpj = <dp (f dp)^T>`` of the logarithmic
    parameter derivatives (``stochastic_reconfiguration.py:49-118``) and the SR step from their averages (:120-176).

    ``gram``: callable ``(A, B) -> A^T B``; default: the device product of the wave function's own handle (tests of the
    host logic inject a NumPy one).

    ``route``: where ``avg`` forms its averages.  ``"protocol"``: derivatives through ``wf.pgradient()``, energies through the energy
    object, one product (``pqa_gram``).  ``"device"``: one ``pqa_sr_moments`` call on the resident state; ``NotImplementedError`` with
    the reason when ``sr_route`` says the case is out of its scope.  None (default): the device route when in scope, else the protocol
    route.  ``last_route`` records what the last evaluation took.

    ``complex_device``: with True a complex or twisted handle is in the device scope too (``pqa_sr_moments_c``: complex columns and
    the imaginary-part tail of complex-dtype keys); False (default) keeps those on the protocol route."""

    def __init__(self, enacc, transform, nodal_cutoff=1e-3, eps=1e-1, inverse_strategy="pseudo_inverse", verbose=False, gram=None,
                 route=None, complex_device=False):
        if route not in (None, "device", "protocol"):
            raise ValueError(f"route must be None, 'device' or 'protocol', got {route!r}")
        self.enacc, self.transform = enacc, transform
        self.nodal_cutoff, self.eps, self.inverse_strategy, self.verbose = nodal_cutoff, eps, inverse_strategy, verbose
        self._gram = gram
        self.route, self.last_route = route, None
        self.complex_device = bool(complex_device)

    def resolve_route(self, wf):
        """The route ``avg`` takes for ``wf``: ``"device"`` or ``"protocol"`` (see ``route``)."""
        if self.route == "protocol":
            return "protocol"
        r, why = sr_route(wf, self)
        if self.route == "device" and r != "device":
            raise NotImplementedError(f"StochasticReconfiguration(route='device'): {why}")
        return r

    def _derivatives(self, configs, wf, cutoff):
        dp = self.transform.serialize_gradients(wf.pgradient())
        en = self.enacc(configs, wf)
        return dp, en, dp * nodal_regularization(en["grad2"], cutoff)[1][:, None]

    def __call__(self, configs, wf):
        self.last_route = "protocol"
        dp, d, fdp = self._derivatives(configs, wf, self.nodal_cutoff)
        d["dpH"] = d["total"][:, None] * fdp
        d["dppsi"] = fdp
        d["dpidpj"] = dp[:, :, None] * fdp[:, None, :]
        return d

    def avg_resident(self, wf, weights=None):
        """``avg`` on the device route for the walkers resident behind ``wf``, without comparing them with a host container: binds
        the energy object, advances its call count and derives the key of the energy draws as ``EnergyAccumulator.__call__`` does,
        then one ``pqa_sr_moments`` call (``pqa_sr_moments_orb`` when orbital coefficients are optimised; ``pqa_sr_moments_c`` on a
        complex or twisted handle, whose ``ecp`` and ``total`` means are complex as ``EnergyAccumulator``'s are)."""
        from .energy import KEYS

        dev, why = _sr_device(wf, self.complex_device)
        if dev is None:
            raise NotImplementedError(f"StochasticReconfiguration.avg_resident: {why}")
        enacc = self.enacc
        enacc.bind(dev)
        enacc._calls += 1
        key = int(np.random.randint(0, 2**31 - 1)) if enacc.seed is None else enacc.seed + enacc._calls
        if dev.cplx or dev.twisted:
            src, pos, tail = sr_columns_c(self.transform)
            en, m = dev.sr_moments_c(src, pos, tail, 1e-3, weights=weights, threshold=enacc.threshold, seed=key)
            self.last_route = "device"
            d = {k: (en[i] if k in ("ecp", "total") else en[i].real) for i, k in enumerate(KEYS)}
            d["dpidpj"], d["dpH"], d["dppsi"] = m[:-2], m[-2], m[-1]
            return d
        orbital = any(k in SR_ORBITAL_SOURCES for k in self.transform.to_opt)
        src, pos = (sr_columns_orb if orbital else sr_columns)(self.transform)
        # the reference regularises with the default cut-off in avg (:105)
        en, m = (dev.sr_moments_orb if orbital else dev.sr_moments)(src, pos, 1e-3, weights=weights, threshold=enacc.threshold, seed=key)
        self.last_route = "device"
        d = {k: en[i] for i, k in enumerate(KEYS)}
        d["dpidpj"], d["dpH"], d["dppsi"] = m[:-2], m[-2], m[-1]
        return d

    @staticmethod
    def _same_walkers(dev, configs):
        if dev.twisted:  # twisted handles hold unfolded coordinates (the comparison of EnergyAccumulator.__call__)
            return np.allclose(dev.configs(), configs.configs + configs.wrap @ configs.lvecs, rtol=0, atol=1e-9)
        return np.array_equal(dev.configs(), configs.configs)

    def avg(self, configs, wf, weights=None):
        if self.resolve_route(wf) == "device":
            dev = _sr_device(wf, self.complex_device)[0]
            if self.enacc.check_configs and not (dev.W == len(configs.configs) and self._same_walkers(dev, configs)):
                raise ValueError("walkers on the device differ from `configs`: call wf.recompute(configs) "
                                 "(or keep wf.updateinternals in step with configs.move) first")
            return self.avg_resident(wf, weights)
        self.last_route = "protocol"
        dp, en, fdp = self._derivatives(configs, wf, 1e-3)  # the reference regularises with the default cut-off here (:105)
        nconf = configs.configs.shape[0]
        w = np.full(nconf, 1.0 / nconf) if weights is None else np.asarray(weights, dtype=float) / np.sum(weights)
        d = {k: np.tensordot(w, v, axes=(0, 0)) for k, v in en.items()}
        p = self.transform.nparams
        if p > 0:
            gram = self._gram or device_gram(wf)
            lhs = np.concatenate((dp, en["total"][:, None], np.ones((nconf, 1))), axis=1)
            m = gram(lhs, w[:, None] * fdp)
            d["dpidpj"], d["dpH"], d["dppsi"] = m[:-2], m[-2], m[-1]
        return d

    def keys(self):
        return self.enacc.keys().union(["dpH", "dppsi", "dpidpj"])

    def shapes(self):
        p = self.transform.nparams
        return {**self.enacc.shapes(), "dpH": (p,), "dppsi": (p,), "dpidpj": (p, p)}

    def delta_p(self, steps, data, verbose=False):
        """``[-step S^-1 g for step in steps]`` with ``g = 2 Re(<E dp> - <E><dp>)`` and the covariance
        ``S = Re(<dp dp^T> - <dp><dp>^T)`` of averaged ``data``; ``S^-1`` by truncated pseudo-inverse (``rcond = eps``)
        or as ``(S + eps 1)^-1``."""
        mean_dp = np.asarray(data["dppsi"])
        g = 2.0 * np.real(np.asarray(data["dpH"]) - data["total"] * mean_dp)
        S = np.real(np.asarray(data["dpidpj"]) - np.outer(mean_dp, mean_dp))
        if self.inverse_strategy == "pseudo_inverse":
            v = np.linalg.pinv(S, rcond=self.eps) @ g
        elif self.inverse_strategy == "regularized_inverse":
            v = np.linalg.solve(S + self.eps * np.identity(len(g)), g)
        else:
            raise ValueError("Invalid inverse strategy. Valid options are pseudo_inverse and regularized_inverse.")
        gn, vn = np.linalg.norm(g), np.linalg.norm(v)
        report = {"pgrad": gn, "SRdot": float(g @ v) / (vn * gn)}
        if verbose or self.verbose:
            print("Gradient norm: ", report["pgrad"], " SR dot: ", report["SRdot"])
        return [-s * v for s in steps], report


PGradTransform = StochasticReconfiguration


def gradient_generator(mol, wf, to_opt=None, nodal_cutoff=1e-3, eps=1e-3, inverse_strategy="regularized_inverse", route=None,
                       complex_device=False, **ewald_kwargs):
    """The gradient object of line minimisation (``observables/accumulators.py:27-42``): an ``EnergyAccumulator`` and the
    ``LinearTransform`` of ``to_opt`` in a ``StochasticReconfiguration``.  ``route`` / ``complex_device``: see
    ``StochasticReconfiguration``; ``"device"`` is checked against ``wf`` here already."""
    from .energy import EnergyAccumulator

    sr = StochasticReconfiguration(EnergyAccumulator(mol, **ewald_kwargs), LinearTransform(wf.parameters, to_opt),
                                   nodal_cutoff=nodal_cutoff, eps=eps, inverse_strategy=inverse_strategy, route=route,
                                   complex_device=complex_device)
    sr.resolve_route(wf)  # (route="device" out of scope: NotImplementedError now, not at the first block)
    return sr
