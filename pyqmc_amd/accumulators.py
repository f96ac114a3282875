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
SR_ORBITAL_SOURCES = {"wf1mo_coeff_alpha": 4, "wf1mo_coeff_beta": 5}  # the further source codes of pqa_sr_moments_orb
SR_MOMENT_BYTES = 256 << 20  # most bytes of the (P + 2, P) moments the device calls take


def _sr_columns(transform, codes):
    src = [np.full(len(p), codes[k], dtype=np.int32) for k, p in transform._pos.items()]
    pos = [np.asarray(p, dtype=np.int32) for p in transform._pos.values()]
    return (np.concatenate(src), np.concatenate(pos)) if src else (np.zeros(0, dtype=np.int32), np.zeros(0, dtype=np.int32))


def sr_columns(transform):
    """``(src, pos)`` of ``pqa_sr_moments`` for a ``LinearTransform`` whose keys are all in ``SR_SOURCES``: column i of the serialised
    derivative matrix is flat entry ``pos[i]`` of the parameter ``src[i]`` names (key after key, selected entries in C order)."""
    return _sr_columns(transform, SR_SOURCES)


def sr_columns_orb(transform):
    """``sr_columns`` for a transform whose keys may include the orbital coefficients: ``(src, pos)`` of ``pqa_sr_moments_orb``,
    ``pos`` of an orbital column the flat C-order index into its (nao, nmo_s) matrix."""
    return _sr_columns(transform, {**SR_SOURCES, **SR_ORBITAL_SOURCES})


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
        cx = dev.cplx or dev.twisted
        if cx:
            moments, cols = dev.sr_moments_c, sr_columns_c
        elif any(k in SR_ORBITAL_SOURCES for k in self.transform.to_opt):
            moments, cols = dev.sr_moments_orb, sr_columns_orb
        else:
            moments, cols = dev.sr_moments, sr_columns
        # the reference regularises with the default cut-off in avg (:105)
        en, m = moments(*cols(self.transform), 1e-3, weights=weights, threshold=enacc.threshold, seed=key)
        self.last_route = "device"
        d = {k: (en[i] if not cx or k in ("ecp", "total") else en[i].real) for i, k in enumerate(KEYS)}
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

MIX_SOURCES = {k: v for k, v in SR_SOURCES.items() if v <= 2}  # the parameters pqa_mix_moments / pqa_mix_wtdp have columns for


def mix_route(wfs, acc):
    """``("device", reason)`` when a multi-state accumulator ``acc`` can take its averages from the walkers resident behind ``wfs``
    (``pqa_mix_moments`` / ``pqa_mix_wtdp``), else ``("protocol", reason)``.  The device route needs: ``sample_many.fused_scope(wfs)``
    (real Slater x two-body Jastrow products on distinct handles of one device, open boundaries, at most 8 states); ``acc.enacc`` a
    ``pyqmc_amd.EnergyAccumulator`` itself; every transform of ``acc`` (``acc.transforms``, or ``acc.transform``; an accumulator
    without either has none) a ``LinearTransform`` whose optimised keys are all among ``MIX_SOURCES``, with moments within
    ``SR_MOMENT_BYTES``."""
    from .energy import EnergyAccumulator
    from .sample_many import fused_scope

    devs, why = fused_scope(wfs)
    if devs is None:
        return "protocol", why
    if type(acc.enacc) is not EnergyAccumulator:
        return "protocol", f"the energy object is a {type(acc.enacc).__name__}, not a pyqmc_amd.EnergyAccumulator"
    transforms = getattr(acc, "transforms", None)
    if transforms is None:
        transforms = [acc.transform] if hasattr(acc, "transform") else []
    K = len(wfs)
    for i, t in enumerate(transforms):
        if type(t) is not LinearTransform:
            return "protocol", f"transform {i} is a {type(t).__name__}, not a pyqmc_amd.LinearTransform"
        other = [k for k in t.to_opt if k not in MIX_SOURCES]
        if other:
            return "protocol", "parameters without a device source: " + ", ".join(other)
        if (t.nparams + 2 * K) * t.nparams * 8 > SR_MOMENT_BYTES:
            return "protocol", f"the moments of {t.nparams} parameters exceed the {SR_MOMENT_BYTES >> 20} MiB the device call takes"
    return "device", "real open-boundary handles of one device, device energy, every parameter has a device source"


def resolve_mix_route(acc, wfs, route, name):
    """The route a multi-state accumulator ``acc`` (class ``name``) takes for ``wfs`` when it was asked for ``route``: "protocol" as
    it is, "device" or ``NotImplementedError`` with ``mix_route``'s reason, None: what ``mix_route`` says."""
    if route == "protocol":
        return "protocol"
    r, why = mix_route(wfs, acc)
    if route == "device" and r != "device":
        raise NotImplementedError(f"{name}(route='device'): {why}")
    return r


def mix_energy_keys(enacc, devs):
    """Per state, in state order, what ``EnergyAccumulator.__call__`` does before its energy pass: bind the handle, advance the call
    count, derive the key of the draws (one ``np.random.randint`` each without a seed) -> keys (K) of ``pqa_mix_moments``."""
    keys = []
    for dev in devs:
        enacc.bind(dev)
        enacc._calls += 1
        keys.append(int(np.random.randint(0, 2**31 - 1)) if enacc.seed is None else enacc.seed + enacc._calls)
    return keys


class StochasticReconfigurationMultipleWF:
    """Energies, overlap derivatives and SR moments of ALL states from one sample of their mixture
    (``stochastic_reconfiguration.py:179-369``): ``avg(configs, wfs, weights)`` returns ``{energy key: (K, K)}`` and, for every state
    ``i`` with optimised parameters, ``("dp", i)`` (P_i, K), ``("dpipj", i)`` (P_i, P_i) and ``("dpH", i)`` (P_i, K);
    ``block_average``, ``_collect_terms`` and ``delta_p`` turn blocks of those into one step per state.  ``eps`` regularises
    ``(S + eps 1)^-1``; the mixture has no nodal divergence, so there is no nodal cut-off.

    ``route``: where ``avg`` forms its averages.  ``"protocol"``: the reference's host formula on ``wf.pgradient()``, the energy
    object's per-walker rows and the (K, K, W) weights.  ``"device"``: one ``pqa_mix_moments`` call on the resident state (``weights``
    are then recomputed there from the same values); ``NotImplementedError`` with the reason when ``mix_route`` says the case is out
    of scope.  None (default): the device route when in scope, else the protocol route.  ``last_route`` records what the last
    evaluation took.  On the device route ``avg_resident(wfs)`` is ``avg`` without a host container, and
    ``sample_many.sample_overlap_worker`` calls it without fetching walkers or weights.

    Three deliberate differences from the reference: ``shapes()`` raises there (it reads ``self.transform``, which does not exist);
    here it returns the shapes ``avg`` returns, with K = ``len(transforms)``.  ``avg(weights=None)`` fails there on ``None.shape``;
    here it raises a ``ValueError`` that says so.  ``delta_p`` fails there on an unbound ``report`` when no state has parameters;
    here the report is then ``{}``."""

    multiple_wf = True

    def __init__(self, enacc, transforms, eps=1e-1, route=None):
        if route not in (None, "device", "protocol"):
            raise ValueError(f"route must be None, 'device' or 'protocol', got {route!r}")
        self.enacc, self.transforms, self.eps = enacc, transforms, eps
        self.route, self.last_route = route, None

    def resolve_route(self, wfs):
        """The route ``avg`` takes for ``wfs``: ``"device"`` or ``"protocol"`` (see ``route``)."""
        return resolve_mix_route(self, wfs, self.route, "StochasticReconfigurationMultipleWF")

    def avg_resident(self, wfs):
        """``avg`` on the device route for the walkers resident behind ``wfs``: the energy object bound and keyed per state as the
        protocol route does (``mix_energy_keys``), then one ``pqa_mix_moments`` call."""
        from .energy import KEYS
        from .sample_many import fused_scope, mix_moments

        devs, why = fused_scope(wfs)
        if devs is None:
            raise NotImplementedError(f"StochasticReconfigurationMultipleWF.avg_resident: {why}")
        keys = mix_energy_keys(self.enacc, devs)
        for wf in wfs:
            wf.wf_factors[0]._saved = None  # (the saved rows of a gradient_value call are overwritten)
        _, en, mom = mix_moments(devs, [sr_columns(t) for t in self.transforms], threshold=self.enacc.threshold, seeds=keys)
        self.last_route = "device"
        K = len(wfs)
        d = {k: en[i] for i, k in enumerate(KEYS)}
        for i, m in enumerate(mom):
            if m is None:
                continue
            p = m.shape[1]
            d[("dp", i)], d[("dpipj", i)], d[("dpH", i)] = m[p:p + K].T.copy(), m[:p].copy(), m[p + K:].T.copy()
        return d

    def avg(self, configs, wfs, weights=None):
        if weights is None:
            raise ValueError("StochasticReconfigurationMultipleWF.avg needs the (K, K, nconf) mixture weights (sample_many.compute_weights)")
        if self.resolve_route(wfs) == "device":
            dev = wfs[0].fused_device()
            if self.enacc.check_configs and not (dev.W == len(configs.configs) and np.array_equal(dev.configs(), configs.configs)):
                raise ValueError("walkers on the device differ from `configs`: call wf.recompute(configs) "
                                 "(or keep wf.updateinternals in step with configs.move) first")
            return self.avg_resident(wfs)
        from .sample_many import invert_list_of_dicts

        self.last_route = "protocol"
        energies = invert_list_of_dicts([self.enacc(configs, wf) for wf in wfs])
        dppsi = [transform.serialize_gradients(wf.pgradient()) for transform, wf in zip(self.transforms, wfs)]
        nconfig = weights.shape[-1]
        d = {}
        for k, en in energies.items():
            d[k] = np.einsum("jc,ijc->ij", np.asarray(en), weights / nconfig)
        for wfi, dp in enumerate(dppsi):
            if self.transforms[wfi].nparams == 0:
                continue
            d[("dp", wfi)] = np.einsum("cp,jc->pj", dp, weights[wfi, :, :], optimize=True) / nconfig
            d[("dpipj", wfi)] = np.einsum("cp,cq,c->pq", dp, dp, weights[wfi, wfi, :], optimize=True) / nconfig
            d[("dpH", wfi)] = np.einsum("jc,cp,jc->pj", energies["total"], dp, weights[wfi, :, :]) / nconfig
        return d

    def keys(self):
        return self.enacc.keys().union(["dpH", "dppsi", "dpidpj"])

    def shapes(self):
        K = len(self.transforms)
        d = {k: (K, K) for k in self.enacc.shapes()}
        for i, t in enumerate(self.transforms):
            if t.nparams:
                d[("dp", i)], d[("dpipj", i)], d[("dpH", i)] = (t.nparams, K), (t.nparams, t.nparams), (t.nparams, K)
        return d

    def update_state(self, hdf_file):
        """Nothing to restore: the accumulator keeps no state."""
        pass

    def block_average(self, data, weights):
        """Averages and errors over blocks: ``weights`` (block, K, K) the overlap blocks, ``data`` the blocks of ``avg``; energies
        divided by sqrt(N_i N_j), state i's ``dp`` / ``dpH`` by its row of that and ``dpipj`` by N_i."""
        import scipy.stats

        weight_avg = np.mean(weights, axis=0)
        N = np.abs(weight_avg.diagonal())
        Nij = np.sqrt(np.outer(N, N))
        avg, error = {}, {}
        avg["total"] = np.mean(data["total"], axis=0) / Nij
        error["total"] = scipy.stats.sem(data["total"], axis=0) / Nij
        nwf = weights.shape[1]
        for k in ["dp", "dpH"]:
            for w in range(nwf):
                if self.transforms[w].nparams == 0:
                    continue
                it = data[(k, w)]
                avg[(k, w)] = np.mean(it, axis=0) / Nij[w]
                error[(k, w)] = scipy.stats.sem(it, axis=0) / Nij[w]
        for w in range(nwf):
            if self.transforms[w].nparams == 0:
                continue
            it = data[("dpipj", w)]
            avg[("dpipj", w)] = np.mean(it, axis=0) / Nij[w, w]
            error[("dpipj", w)] = scipy.stats.sem(it, axis=0) / Nij[w, w]
        avg["overlap"] = weight_avg
        return avg, error

    def _collect_terms(self, avg, error):
        ret = {}
        nwf = avg["total"].shape[0]
        N = np.abs(avg["overlap"].diagonal())
        Nij = np.sqrt(np.outer(N, N))
        ret["norm"] = N
        ret["overlap"] = avg["overlap"] / Nij
        fac = np.ones((nwf, nwf)) + np.identity(nwf)
        for wfi in range(nwf):
            if self.transforms[wfi].nparams == 0:
                continue
            ret[("dp_energy", wfi)] = fac[wfi] * np.real(avg[("dpH", wfi)] - avg["total"][wfi] * avg[("dp", wfi)])
            ret[("dp_norm", wfi)] = 2.0 * np.real(avg[("dp", wfi)][:, wfi])
            norm_part = np.einsum("i,p->pi", avg["overlap"][wfi, :], ret[("dp_norm", wfi)]) / N[wfi]
            ret[("dp_overlap", wfi)] = fac[wfi] * (avg[("dp", wfi)] - 0.5 * norm_part) / Nij[wfi]
            ret[("dpipj", wfi)] = np.real(avg[("dpipj", wfi)] - np.einsum("i,j->ij", avg[("dp", wfi)][:, wfi], avg[("dp", wfi)][:, wfi]))
        ret["energy"] = avg["total"]
        return ret

    def delta_p(self, steps, data, overlap_penalty, verbose=False):
        """Per state ``[-step (S + eps 1)^-1 g for step in steps]`` (empty vectors for a state without parameters) with g the energy
        gradient plus the penalised overlap gradient against the states before it; returns (steps per state, report of the last state
        that has parameters)."""
        data = self._collect_terms(data, None)
        nwf = data["energy"].shape[0]
        dp_all = []
        report = {}
        for wf in range(nwf):
            overlap_cost = 0.0
            for i in range(wf):
                overlap_cost += overlap_penalty[wf, i] * data["overlap"][wf, i]
            if verbose:
                print("wave function", wf)
                print("Overlap cost", overlap_cost)
            if self.transforms[wf].nparams == 0:
                dp_all.append([np.zeros((0)) for step in steps])
                continue
            Sij = np.real(data[("dpipj", wf)])
            ovlp = 0.0
            for i in range(wf):
                ovlp += 2.0 * data[("dp_overlap", wf)][:, i] * overlap_penalty[wf, i] * data["overlap"][wf, i]
            pgrad = data[("dp_energy", wf)][:, wf] + ovlp
            invSij = np.linalg.inv(Sij + self.eps * np.eye(Sij.shape[0]))
            v = np.einsum("ij,j->i", invSij, pgrad)
            dp_all.append([-step * v for step in steps])
            report = {"pgrad": np.linalg.norm(pgrad), "SRdot": np.dot(pgrad, v) / (np.linalg.norm(v) * np.linalg.norm(pgrad))}
            if verbose:
                print("overlap gradient norm", np.linalg.norm(ovlp))
                print("Gradient norm: ", np.linalg.norm(pgrad))
                print("Dot product between gradient and SR step: ", report["SRdot"])
        return dp_all, report


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
