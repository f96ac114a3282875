"""One-body density matrix accumulator — SURVEY.md §8(f3); public interface of ``pyqmc/observables/obdm.py``.

``rho[i][j] = <c+_i c_j>`` in the orbital basis ``orb_coeff`` is sampled by moving one electron of Psi to an auxiliary
position r' distributed as ``f(r) = sum_i |phi_i(r)|^2`` (obdm.py:26-49).  The work is done by the HIP library on a
device handle that holds ``orb_coeff`` as its orbitals (``OrbitalEvaluator``):

* ``pqa_dm_walk``: the Metropolis walk of the auxiliary walkers (obdm.py:215-250), resident on the device — one orbital
  launch (``k_orb``) and one accept kernel per sample; the last ``nsweeps`` samples stay on the device;
* ``pqa_dm_points``: the basis orbitals at the configurations' electrons;
* ``pqa_obdm_accumulate``: per sweep, the estimator's contraction (obdm.py:170-190) with the ratios Psi(R')/Psi(R) of
  ``wf.testvalue_many`` (``k_testvalue_many`` on the wave function's own handle);
* ``pqa_dm_fetch``: the per-configuration result, or its mean over configurations reduced on the device (``avg``).

The host only draws random numbers — from ``numpy.random`` in the reference's order, so that a seeded run reproduces the
reference draw for draw — and moves the small per-sweep arrays (positions, assignments, ratios).

Two routes give the ratios (``route``, as in ``TBDMAccumulator``):

* **protocol**: the four steps above, sweep by sweep through ``wf.testvalue_many`` — every wave function.
* **fused** (``pqa_obdm_sweeps``, ``csrc/pqa_obdm.hip``): real wave functions living on one device handle whose resident walkers are
  the configurations — Slater (one or more determinants), optionally times JastrowSpin, open or periodic at Gamma — with a real
  evaluator on the same device.  The electrons' coordinates are read from the resident walkers, the ratios of all sweeps come in
  closed form from the resident state, and the estimator is contracted on the device in the same call: per configuration
  (``__call__``) or, for ``avg`` / ``avg_resident``, as the walker mean ``B^T T / W`` on the fp64 matrix cores without a
  per-configuration matrix.  With ``rng="numpy"`` the draws are those of the protocol route; ``rng="device"`` draws the walk and the
  assignments from the device's Philox streams, keyed by one ``numpy.random`` integer per evaluation.

With ``complex_device=True`` (opt-in) complex and twisted handles and complex evaluators take the fused route as well
(``pqa_obdm_sweeps_c``): the complex ratios come in closed form from the resident complex inverse, the per-configuration mode hands
them to the same contraction kernel the protocol route uses, and ``avg`` / ``avg_resident`` form ``B^T T / W`` from planar real and
imaginary panels (Re = Br^T Tr - Bi^T Ti, Im = Br^T Ti + Bi^T Tr).  ``value`` is complex and ``norm`` real, as on the protocol route.
A twisted evaluator needs a twisted wave-function handle (an untwisted periodic handle holds folded walkers, which have lost the wrap
phase of the orbitals at the electrons): that pair stays on the protocol route.

With ``three_body_device=True`` (opt-in) real wave functions with a three-body Jastrow factor take the fused route as well
(``pqa_obdm_sweeps_j3``): U3 is a sum over electron pairs and every listed electron of a walker goes to the same point, so one table
G_s(r')[j] = t(r', s; r_j, s_j) per moving spin gives A3_e = sum_j G[j] - G[e] - P_e for all of them (``k_j3_moves``,
``csrc/pqa_j3dm.hpp``), added to the two-body difference in the exponent.  Complex or twisted three-body handles stay on the protocol
route.

``avg_resident(wf, weights=w)`` is the weighted walker mean sum_w w_w res_w / sum_w w_w of DMC's mixed estimator
(``pqa_obdm_sweeps_w``: the same product with the weight applied to B as it is loaded; unit weights give the bits of ``avg``).

``last_route`` names the route of the last evaluation.
"""

import numpy as np

from . import _ffi
from . import pbc as _pbc
from .configs import OpenConfigs, PeriodicConfigs
from .systems import initial_guess
from .wf import DeviceWF, readonly_device

ROUTES = (None, "fused", "protocol")


class _OneElectronView:
    """``mol`` with one electron per spin: lets a device handle carry ``norb`` orbitals without a determinant to fill."""

    def __init__(self, mol):
        object.__setattr__(self, "_mol", mol)
        object.__setattr__(self, "nelec", (1, 1))

    def __getattr__(self, name):
        return getattr(object.__getattribute__(self, "_mol"), name)


class OrbitalEvaluator:
    """``orb_coeff`` as an orbital evaluator on the device: the role ``MoleculeOrbitalEvaluator(mol, [C_up, C_dn])`` /
    ``PBCOrbitalEvaluatorKpoints(mol, [C_up, C_dn], kpts)`` play in obdm.py:79-91 and tbdm.py:87-104.  ``orb_coeff`` is
    one (nao, norb) matrix used for both spins or a pair of them.  Periodic: per spin a list ``[k]`` of (nao_prim, norb_k)
    blocks at the k-points ``kpts`` that fold onto the supercell; the orbitals are concatenated over k."""

    def __init__(self, mol, orb_coeff, kpts=None, eval_gto_precision=None, device=0):
        twist = None
        if kpts is None:
            if hasattr(mol, "a"):
                raise ValueError("kpts is required if the system is periodic")
            single = isinstance(orb_coeff, np.ndarray) and orb_coeff.ndim == 2
            pair = [np.asarray(orb_coeff)] * 2 if single else [np.asarray(orb_coeff[0]), np.asarray(orb_coeff[1])]
        else:
            if not hasattr(mol, "original_cell"):
                mol = _pbc.get_supercell(mol, np.eye(3))
            kpts = np.asarray(kpts, dtype=float).reshape(-1, 3)
            single = isinstance(orb_coeff[0], np.ndarray) and orb_coeff[0].ndim == 2  # [k] blocks shared by both spins
            per_spin = [list(orb_coeff), list(orb_coeff)] if single else [list(orb_coeff[0]), list(orb_coeff[1])]
            pair = _pbc.fold_mo_coeff(mol, kpts, per_spin)
            twist = _pbc.common_twist(mol, kpts)
        self._nmo = [int(c.shape[-1]) for c in pair]
        self.norb = self._nmo[0]
        self.mol = mol
        dets = [(1.0, [[self._nmo[0] - 1], [self._nmo[1] - 1]])]  # nmo_s = highest occupied index + 1
        kw = {} if eval_gto_precision is None else {"eval_gto_precision": eval_gto_precision}
        self.dev = DeviceWF(_OneElectronView(mol), mo_coeff=pair, determinants=dets, device=device, twist_k=twist, **kw)
        self.mo_dtype = complex if self.dev.cplx else float
        self.lattice = np.asarray(mol.lattice_vectors(), dtype=float) if hasattr(mol, "a") else None

    def nmo(self):
        return list(self._nmo)

    def true_positions(self, obj):
        """Coordinates the device is handed: a container's positions plus, for a periodic one, ``wrap @ lattice`` — the
        orbital kernel folds every point itself and derives a twisted cell's wrap phase exp(i k . wrap . L)
        (orbitals.py:201-213) from the fold, so electrons that left the cell carry the right Bloch phase."""
        x = np.asarray(obj.configs, dtype=float)
        if self.lattice is not None and getattr(obj, "wrap", None) is not None:
            x = x + np.asarray(obj.wrap, dtype=float) @ self.lattice
        return x

    def container(self, x):
        """One-electron configurations (n,1,3) for true positions ``x`` (n,3): folded into the cell, with wrap counters."""
        x = np.asarray(x, dtype=float).reshape(-1, 1, 3)
        return OpenConfigs(x.copy()) if self.lattice is None else PeriodicConfigs(x, self.lattice)

    def mos(self, points, spin=0):
        """(npts, norb_spin) orbital values at ``points`` (npts, 3) (any position: periodic handles fold internally)."""
        return self.dev.eval_mo(int(spin), np.asarray(points, dtype=float).reshape(-1, 3), 1)[0]

    # ---- device-resident pieces of the estimators --------------------------------------------------------------
    def walk(self, slot, spin, x, gauss, unif, tstep, nkeep):
        """``pqa_dm_walk`` with replay tapes: advances the true positions ``x`` (n,3) in place; returns the decisions
        (nsamples,n) and the positions of the last ``nkeep`` samples (nkeep,n,3)."""
        nsamples, n = unif.shape
        keep, acc = np.empty((nkeep, n, 3)), np.empty((nsamples, n))
        self.dev.call("pqa_dm_walk", int(slot), int(spin), n, nsamples, float(tstep), _ffi.ptr(x), _ffi.ptr(gauss), _ffi.ptr(unif), 0,
                      int(nkeep), _ffi.ptr(keep), _ffi.ptr(acc))
        return acc, keep

    def walk_device(self, slot, spin, x, nsamples, seed, tstep, nkeep):
        """``pqa_dm_walk`` on the device's own Philox streams keyed by ``seed`` (no tapes): as ``walk`` without the decisions."""
        n = len(x)
        keep = np.empty((nkeep, n, 3))
        self.dev.call("pqa_dm_walk", int(slot), int(spin), n, int(nsamples), float(tstep), _ffi.ptr(x), None, None, int(seed), int(nkeep),
                      _ffi.ptr(keep), None)
        return None, keep

    def points(self, slot, spin, x):
        x = _ffi.f64(x).reshape(-1, 3)
        self.dev.call("pqa_dm_points", int(slot), int(spin), _ffi.ptr(x), len(x))

    def fetch(self, which, nconf, shape, scale, mean, cplx=False):
        """``pqa_dm_fetch``: accumulator ``which`` (0 value, 1 / 2 norms) times ``scale``, per configuration
        (nconf, *shape) or averaged over the configurations on the device (*shape)."""
        ncol = int(np.prod(shape)) * (2 if cplx else 1)
        out = np.empty(((1 if mean else nconf), ncol))
        self.dev.call("pqa_dm_fetch", int(which), ncol, float(scale), int(mean), _ffi.ptr(out))
        out = out.view(complex) if cplx else out
        return out.reshape(shape) if mean else out.reshape((nconf,) + tuple(shape))

    def points_resident(self, slot, dev, electrons, cplx=False, j3=False):
        """``pqa_dm_points_resident``: what ``points`` leaves in ``slot``, for the listed ``electrons`` of the walkers resident
        behind the wave-function handle ``dev``, gathered device to device (the slot's walk names the spin).  ``cplx``:
        ``pqa_dm_points_resident_c``, which admits complex and twisted handles and complex evaluators; ``j3``:
        ``pqa_dm_points_resident_j3``, which admits real handles with a three-body Jastrow factor."""
        es = np.ascontiguousarray(np.asarray(electrons).ravel(), dtype=np.int32)
        entry = "pqa_dm_points_resident_j3" if j3 else "pqa_dm_points_resident_c" if cplx else "pqa_dm_points_resident"
        dev.call(entry, self.dev._h, int(slot), _ffi.ptr(es), len(es))

    def fetch_w(self, which, nconf, shape, scale, weights, cplx=False):
        """``pqa_dm_fetch_w``: the walker mean of accumulator ``which`` with the walker ``weights`` (nconf,), times ``scale``."""
        w = _ffi.walker_weights(weights, nconf)
        ncol = int(np.prod(shape)) * (2 if cplx else 1)
        out = np.empty(ncol)
        self.dev.call("pqa_dm_fetch_w", int(which), ncol, float(scale), _ffi.ptr(w), _ffi.ptr(out))
        return (out.view(complex) if cplx else out).reshape(shape)


def draw_walk_tapes(n, nsamples):
    """Standard normals (nsamples,n,3) and uniforms (nsamples,n) in the order the reference's walk consumes
    ``numpy.random`` (per sample: the displacements of all walkers, then their acceptance numbers; obdm.py:232-240)."""
    gauss, unif = np.empty((nsamples, n, 3)), np.empty((nsamples, n))
    for s in range(nsamples):
        gauss[s] = np.random.randn(n, 3)
        unif[s] = np.random.rand(n)
    return gauss, unif


class AuxiliaryWalkers:
    """``n`` one-electron walkers distributed as the orbital density of one spin, resident in a slot of the evaluator's
    device handle.  ``start`` places them like the reference (``initial_guess`` electrons re-read one by one,
    obdm.py:121-124); ``advance`` runs the walk and keeps the last ``keep`` samples on the device."""

    tape_bytes = 256 << 20  # most host memory the tapes of one ``pqa_dm_walk`` call take

    def __init__(self, orbitals, slot):
        self.orbitals, self.slot, self.x = orbitals, slot, None

    def start(self, naux, electrons_per_config):
        seed = initial_guess(self.orbitals.mol, int(naux / electrons_per_config) + 1, rng=np.random)
        self.x = np.ascontiguousarray(self.orbitals.true_positions(seed).reshape(-1, 3)[:naux])

    def advance(self, spin, nsamples, tstep, keep=0, seed=None):
        """``nsamples`` steps of the walk; returns (decisions (nsamples, n), positions of the last ``keep`` samples).  The tapes are
        drawn and walked in groups of samples that stay within ``tape_bytes`` (the last group holds the kept samples): the draw
        order and the positions are those of one call, since a call starts from the positions its predecessor returned.
        ``seed``: the device's Philox streams instead of tapes (no decisions are returned)."""
        if seed is not None:
            return self.orbitals.walk_device(self.slot, spin, self.x, nsamples, seed, tstep, keep)
        n = len(self.x)
        group = max(1, int(self.tape_bytes // (32 * n)))  # a sample's tapes: 3 normals and 1 uniform per walker
        sizes, left = [], nsamples
        while left > max(group, keep):
            take = min(group, left - keep) if keep else group
            sizes.append(take)
            left -= take
        sizes.append(left)
        acc, kept = [], None
        for i, ns in enumerate(sizes):
            gauss, unif = draw_walk_tapes(n, ns)
            a, kept = self.orbitals.walk(self.slot, spin, self.x, gauss, unif, tstep, keep if i == len(sizes) - 1 else 0)
            acc.append(a)
        return (acc[0] if len(acc) == 1 else np.concatenate(acc)), kept

    @property
    def configs(self):
        return self.orbitals.container(self.x)


def sample_onebody(configs, orbitals, nsamples=1, tstep=0.5, spin=0):
    """The reference's free function (obdm.py:215-250) on the device walk: advances the one-electron ``configs`` (n,1,3)
    and returns (decisions (nsamples,n), list of configurations, list of orbital values (n,norb)) per sample."""
    w = AuxiliaryWalkers(orbitals, 0)
    w.x = np.ascontiguousarray(orbitals.true_positions(configs).reshape(-1, 3))
    acc, kept = w.advance(spin, nsamples, tstep, keep=nsamples)
    snaps = [orbitals.container(k) for k in kept]
    if nsamples:
        last = snaps[-1]
        configs.configs[...] = last.configs
        if getattr(configs, "wrap", None) is not None:
            configs.wrap[...] = last.wrap
    return acc, snaps, [orbitals.mos(k, spin) for k in kept]


def _sweeps(entry, dev, ev, electrons, nsweeps, assign, seed, mean, first, walker_chunk, with_ratios, weights):
    """One call of the library entry ``entry`` (``pqa_obdm_sweeps``, ``_w``, ``_c`` or ``_j3``) behind the ``device_obdm_sweeps*``
    helpers: the electron list, the checked weights and assignments and the outputs (complex for ``_c``) are prepared once, and the
    argument list is the named entry's (``_c`` and ``_j3`` share one; ``_w`` is the mean mode alone and has no ratio output)."""
    es = np.ascontiguousarray(np.asarray(electrons).ravel(), dtype=np.int32)
    W, norb = dev.W, ev.norb
    dtype = complex if entry == "pqa_obdm_sweeps_c" else float
    if weights is not None or entry == "pqa_obdm_sweeps_w":  # (the weighted entry refuses None)
        if not mean:
            raise ValueError("walker weights need the mean mode")
        weights = _ffi.walker_weights(weights, W)
    out = {}
    if assign is not None:
        assign = np.ascontiguousarray(assign, dtype=np.int32)
        if assign.shape != (nsweeps, W):
            raise ValueError(f"assignments ({nsweeps}, {W}) expected, got {assign.shape}")
        out["assign"] = assign
    else:
        out["assign"] = np.empty((nsweeps, W), dtype=np.int32)
    if with_ratios and entry != "pqa_obdm_sweeps_w":
        out["ratio"] = np.empty((nsweeps, W, len(es)), dtype=dtype)
    if mean:
        out["value"], out["norm"] = np.empty((norb, norb), dtype=dtype), np.empty(norb)
    head = (ev.dev._h, 0, _ffi.ptr(es), len(es), int(nsweeps), _ffi.ptr(assign), int(seed))
    tail = (None if assign is not None else _ffi.ptr(out["assign"]), _ffi.ptr(out.get("value")), _ffi.ptr(out.get("norm")))
    if entry == "pqa_obdm_sweeps":
        args = head + (int(mean), int(first), int(walker_chunk), _ffi.ptr(out.get("ratio"))) + tail
    elif entry == "pqa_obdm_sweeps_w":
        args = head + (int(walker_chunk), _ffi.ptr(weights)) + tail
    else:
        args = head + (int(mean), int(first), int(walker_chunk), _ffi.ptr(weights), _ffi.ptr(out.get("ratio"))) + tail
    dev.call(entry, *args)
    return out


def device_obdm_sweeps(dev, ev, electrons, nsweeps, assign=None, seed=0, mean=False, first=True, walker_chunk=0, with_ratios=False):
    """``pqa_obdm_sweeps``: the one-body estimator of wave-function handle ``dev`` over the first ``nsweeps`` kept samples of slot 0
    of the evaluator ``ev`` (an ``OrbitalEvaluator``) for the listed ``electrons``.  ``assign`` (nsweeps, W): the auxiliary walker of
    every configuration, or None: drawn on the device from ``seed``.  Returns a dict: ``assign`` (the assignments used), ``ratio``
    (nsweeps, W, nelec) with ``with_ratios``, and with ``mean`` the walker means ``value`` (norb, norb) and ``norm`` (norb,) already
    divided by ``nsweeps``; without ``mean`` the evaluator's per-configuration accumulators hold the sums (``ev.fetch``)."""
    return _sweeps("pqa_obdm_sweeps", dev, ev, electrons, nsweeps, assign, seed, mean, first, walker_chunk, with_ratios, None)


def device_obdm_sweeps_w(dev, ev, electrons, nsweeps, weights, assign=None, seed=0, walker_chunk=0):
    """``pqa_obdm_sweeps_w``: the mean mode of ``device_obdm_sweeps`` with the walker ``weights`` (W,): ``value`` and ``norm`` are
    sum_s sum_w w_w (...) / (nsweeps sum_w w_w).  Returns a dict with ``assign``, ``value`` and ``norm``."""
    return _sweeps("pqa_obdm_sweeps_w", dev, ev, electrons, nsweeps, assign, seed, True, True, walker_chunk, False, weights)


def device_obdm_sweeps_c(dev, ev, electrons, nsweeps, assign=None, seed=0, mean=False, first=True, walker_chunk=0, with_ratios=False,
                         weights=None):
    """``pqa_obdm_sweeps_c``: ``device_obdm_sweeps`` for complex and twisted handles ``dev`` and complex evaluators ``ev`` (real ones are
    taken too).  The same dict, with complex ``ratio`` (nsweeps, W, nelec) and ``value`` (norb, norb) and a real ``norm``; ``weights``
    (W,): the weighted mean of ``device_obdm_sweeps_w`` (``mean`` only).  Without ``mean`` the evaluator's per-configuration accumulators
    hold complex sums (``ev.fetch(..., cplx=True)``)."""
    return _sweeps("pqa_obdm_sweeps_c", dev, ev, electrons, nsweeps, assign, seed, mean, first, walker_chunk, with_ratios, weights)


def device_obdm_sweeps_j3(dev, ev, electrons, nsweeps, assign=None, seed=0, mean=False, first=True, walker_chunk=0, with_ratios=False,
                          weights=None):
    """``pqa_obdm_sweeps_j3``: ``device_obdm_sweeps`` for real handles ``dev`` with a three-body Jastrow factor (handles without one are
    taken too and give the bits of ``device_obdm_sweeps`` / ``device_obdm_sweeps_w``).  The same dict, real; ``weights`` (W,): the
    weighted mean of ``device_obdm_sweeps_w`` (``mean`` only)."""
    return _sweeps("pqa_obdm_sweeps_j3", dev, ev, electrons, nsweeps, assign, seed, mean, first, walker_chunk, with_ratios, weights)


class _FusedScope:
    """What ``OBDMAccumulator`` and ``TBDMAccumulator`` share of the fused route's scope: the two opt-in flags, the handle lookup, the
    choice of the library entry and the common part of the reason ladder.  A subclass names its three entries in ``ENTRIES`` (real,
    complex, three-body), holds ``orbitals`` and ``_mol``, and adds the estimator's own tail to ``_common_scope``."""

    ENTRIES = (None, None, None)

    @staticmethod
    def _flag(name, value):
        """The opt-in flag ``name`` (``complex_device`` / ``three_body_device``) as a bool; anything but True or False is refused."""
        if not isinstance(value, (bool, np.bool_)):
            raise ValueError(f"{name} must be True or False")
        return bool(value)

    def _device(self, wf):
        """The handle the fused route reads ``wf`` from, or None."""
        return readonly_device(wf, complex_ok=self.complex_device, three_body_ok=self.three_body_device)

    def _j3_entry(self, dev):
        """Whether the evaluation of the handle ``dev`` goes through the three-body entry."""
        return self.three_body_device and bool(dev.has_j3)

    def _complex_entry(self, dev):
        """Whether the evaluation of the handle ``dev`` goes through the complex entry."""
        ev = self.orbitals.dev
        return self.complex_device and bool(dev.cplx or dev.twisted or ev.cplx or ev.twisted)

    def _entry(self, dev):
        """The library entry that evaluates the handle ``dev``: the three-body one before the complex one before the real one."""
        return self.ENTRIES[2 if self._j3_entry(dev) else 1 if self._complex_entry(dev) else 0]

    def _common_scope(self, wf):
        """(handle, reason): why the fused route cannot take ``wf`` as far as both estimators agree — wave-function kind, evaluator
        kind, devices, electron numbers — or None; the handle is None when the wave function has none in scope."""
        dev, ev = self._device(wf), self.orbitals.dev
        if dev is None:
            if self.three_body_device:
                d3 = getattr(wf, "fused_device", lambda: None)()
                if d3 is not None and getattr(d3, "has_j3", False) and (d3.cplx or d3.twisted):
                    return None, f"the three-body wave function is complex or twisted ({self.ENTRIES[2]} takes real handles)"
                if self.complex_device:
                    return None, "the wave function is not a Slater (x two-body x three-body Jastrow) product on one device handle"
                return None, "the wave function is not a real Slater (x two-body x three-body Jastrow) product on one device handle"
            if self.complex_device:
                return None, "the wave function is not a Slater (x two-body Jastrow) product on one device handle"
            return None, "the wave function is not a real Slater (x two-body Jastrow) product on one device handle"
        if self._j3_entry(dev) and (ev.cplx or ev.twisted):
            return dev, "the orbital evaluator is complex (a three-body wave function needs a real one)"
        if self.complex_device:
            if ev.twisted and not dev.twisted:
                return dev, "the orbital evaluator is twisted and the wave function's handle is not (its folded walkers have lost the wrap phase)"
        elif ev.cplx or ev.twisted:
            return dev, "the orbital evaluator is complex"
        if ev.device != dev.device:
            return dev, "the wave function and the evaluator are on different devices"
        if tuple(dev.nelec) != tuple(self._mol.nelec):
            return dev, "the wave function has other electron numbers than the accumulator's system"
        return dev, None


class OBDMAccumulator(_FusedScope):
    """Keys ``value`` (norb,norb), ``norm`` (norb,) per configuration (obdm.py:26-213).

    ``spin`` 0/1 restricts the moved electrons to the up/down ones, ``electrons`` to an explicit list; ``naux`` auxiliary
    walkers (default: one per configuration), ``nsweeps`` auxiliary samples per evaluation, ``warmup`` samples before the
    first.

    ``route``: None takes the fused route whenever the wave function and the evaluator are in its scope and the protocol route
    otherwise; "fused" raises outside the scope; "protocol" always goes through ``wf.testvalue_many``.  ``rng``: "numpy" draws the
    walk and the assignments from ``numpy.random`` in the reference's order on both routes; "device" (fused route only) draws one
    ``numpy.random`` integer per evaluation and leaves the rest to the device's Philox streams.  ``walker_chunk``: walkers per
    scratch chunk of the fused route (0: the library's bound).  ``last_route`` names the route of the last evaluation.
    ``complex_device``: with True complex and twisted handles and complex evaluators are in the fused scope too
    (``pqa_obdm_sweeps_c``), except a twisted evaluator with an untwisted handle; with False (the default) they take the protocol
    route and ``route="fused"`` raises for them.  ``three_body_device``: with True real wave functions with a three-body Jastrow
    factor are in the fused scope too (``pqa_obdm_sweeps_j3``, a real evaluator); complex or twisted three-body handles stay on the
    protocol route.  With False (the default) three-body wave functions take the protocol route."""

    ENTRIES = ("pqa_obdm_sweeps", "pqa_obdm_sweeps_c", "pqa_obdm_sweeps_j3")

    def __init__(self, mol, orb_coeff, nsweeps=5, tstep=0.50, warmup=10000, naux=None, spin=None, electrons=None, kpts=None,
                 eval_gto_precision=None, device=0, route=None, rng="numpy", walker_chunk=0, complex_device=False,
                 three_body_device=False):
        if route not in ROUTES:
            raise ValueError(f"route must be one of {ROUTES}")
        if rng not in ("numpy", "device"):
            raise ValueError("rng must be 'numpy' or 'device'")
        if rng == "device" and route == "protocol":
            raise ValueError("rng='device' draws inside pqa_obdm_sweeps: it needs the fused route")
        self.complex_device = self._flag("complex_device", complex_device)
        self._route, self._rng, self._walker_chunk, self.last_route = route, rng, int(walker_chunk), None
        self.three_body_device = self._flag("three_body_device", three_body_device)
        self.last_assign = None  # (nsweeps, nconf) assignments of the last fused evaluation
        nup, ntot = mol.nelec[0], int(np.sum(mol.nelec))
        if spin is not None:
            if spin not in (0, 1):
                raise ValueError("Spin not equal to 0 or 1")
            self._electrons = np.arange(0, nup) if spin == 0 else np.arange(nup, ntot)
        else:
            self._electrons = np.arange(ntot) if electrons is None else np.asarray(electrons)
        self.orbitals = OrbitalEvaluator(mol, orb_coeff, kpts=kpts, eval_gto_precision=eval_gto_precision, device=device)
        self._mol, self.dtype, self.norb = self.orbitals.mol, self.orbitals.mo_dtype, self.orbitals.norb
        self.nelec = len(self._electrons)
        self._tstep, self._nsweeps, self._warmup, self._naux = tstep, nsweeps, warmup, naux
        self._walkers = None

    @property
    def _extra_config(self):
        return None if self._walkers is None else self._walkers.configs

    def _out_of_scope(self, wf, nconf=None):
        """Why the fused route cannot take ``wf`` (and ``nconf`` configurations), or None when it can."""
        dev, why = self._common_scope(wf)
        if why is not None:
            return why
        es = np.asarray(self._electrons).ravel()
        if len(es) < 1:
            return "no electron is listed"
        if es.min() < 0 or es.max() >= dev.N or len(np.unique(es)) != len(es):
            return "the electron list repeats an electron or names one the wave function does not have"
        if nconf is not None and dev.W != nconf:
            return "the wave function's resident walkers are not the configurations"
        return None

    def resolve_route(self, wf, nconf=None):
        """The route an evaluation takes for ``wf``: "fused" or "protocol" (see ``route``)."""
        if self._route == "protocol":
            return "protocol"
        why = self._out_of_scope(wf, nconf)
        if why is not None and (self._route == "fused" or self._rng == "device"):
            raise ValueError(f"OBDMAccumulator(route='fused'): {why} (outside the fused scope: use the protocol route)")
        return "protocol" if why is not None else "fused"

    def _start(self, nconf, seed=None):
        if self._walkers is None:
            self._walkers = AuxiliaryWalkers(self.orbitals, 0)
            self._walkers.start(nconf if self._naux is None else self._naux, self.nelec)
            self._walkers.advance(0, self._warmup, self._tstep, seed=None if seed is None else seed + 1)

    def _sample(self, configs, wf):
        """Runs one evaluation on the device, protocol route; returns whether the accumulated value is complex."""
        ev, nconf = self.orbitals, configs.configs.shape[0]
        self._start(nconf)
        naux = len(self._walkers.x)
        pick = np.random.randint(0, naux, size=(self._nsweeps, nconf)).astype(np.int32)  # drawn before the walk (obdm.py:150)
        _, kept = self._walkers.advance(0, self._nsweeps, self._tstep, keep=self._nsweeps)
        ev.points(0, 0, ev.true_positions(configs)[:, self._electrons])
        cplx = False
        for s in range(self._nsweeps):
            there = ev.container(kept[s][pick[s]]).electron(0)
            ratio = np.ascontiguousarray(wf.testvalue_many(self._electrons, there))
            rc = np.iscomplexobj(ratio)
            cplx = rc or ev.dev.cplx
            ev.dev.call("pqa_obdm_accumulate", 0, s, nconf, self.nelec, _ffi.ptr(pick[s]), _ffi.ptr(ratio), int(rc), int(s == 0))
        # the reference resamples its last sample in place and walks on from THAT set (one walker per configuration,
        # obdm.py:160-163); kept so that a seeded run stays draw-for-draw comparable
        self._walkers.x = np.ascontiguousarray(kept[-1][pick[-1]])
        return cplx

    def _sample_fused(self, dev, mean, with_ratios=False, weights=None):
        """One evaluation on the fused route: the walk, then ONE ``pqa_obdm_sweeps`` call on the walkers resident behind ``dev``
        (``weights``: ``pqa_obdm_sweeps_w``, the weighted mean).  Returns (value_mean, norm_mean) of the mean mode (else None, the
        evaluator's accumulators hold the result) and the ratios (nsweeps, W, nelec) when asked for."""
        ev, nconf, nsw = self.orbitals, dev.W, self._nsweeps
        if weights is not None:  # (refused before numpy.random is touched)
            weights = _ffi.walker_weights(weights, nconf)
        seed = int(np.random.randint(0, 2**31 - 1)) if self._rng == "device" else None
        self._start(nconf, seed)
        naux = len(self._walkers.x)
        pick = None
        if seed is None:
            pick = np.random.randint(0, naux, size=(nsw, nconf)).astype(np.int32)  # drawn before the walk (obdm.py:150)
        _, kept = self._walkers.advance(0, nsw, self._tstep, keep=nsw, seed=seed)
        entry = self._entry(dev)
        if entry == "pqa_obdm_sweeps" and weights is not None:  # (the real entry's weighted mean is an entry of its own)
            entry = "pqa_obdm_sweeps_w"
        out = _sweeps(entry, dev, ev, self._electrons, nsw, pick, 0 if seed is None else seed, mean, True, self._walker_chunk, with_ratios,
                      weights)
        vm, nm, ratio, used = out.get("value"), out.get("norm"), out.get("ratio"), out["assign"]
        self.last_assign = used
        self._walkers.x = np.ascontiguousarray(kept[-1][self.last_assign[-1]])  # the reference's resampling step, as in _sample
        return (vm, nm), ratio

    def _result(self, configs, wf, mean):
        nconf, scale = configs.configs.shape[0], 1.0 / self._nsweeps
        self.last_route = self.resolve_route(wf, nconf)
        if self.last_route == "fused":
            dev = self._device(wf)
            (vm, nm), _ = self._sample_fused(dev, mean)
            if mean:
                return {"value": vm, "norm": nm}
            cplx = self._complex_entry(dev)
        else:
            cplx = self._sample(configs, wf)
        return {"value": self.orbitals.fetch(0, nconf, (self.norb, self.norb), scale, mean, cplx),
                "norm": self.orbitals.fetch(1, nconf, (self.norb,), scale, mean)}

    def __call__(self, configs, wf):
        return self._result(configs, wf, False)

    def avg(self, configs, wf):
        """Mean over the configurations, reduced on the device (obdm.py:195-197)."""
        return self._result(configs, wf, True)

    def resident_scope(self, wf):
        """None when ``avg_resident`` can run for ``wf``, else the reason (the fused route's rules)."""
        if self._route == "protocol":
            return "the accumulator is bound to route='protocol'"
        return self._out_of_scope(wf)

    def avg_resident(self, wf, weights=None):
        """``avg`` on the fused route for the walkers resident behind ``wf``, without a host container.  ``weights`` (W,): the
        weighted walker mean sum_w w_w res_w / sum_w w_w (DMC's mixed estimator) instead of the plain one."""
        if self.resolve_route(wf) != "fused":
            raise ValueError("OBDMAccumulator.avg_resident needs the fused route")
        self.last_route = "fused"
        (vm, nm), _ = self._sample_fused(self._device(wf), True, weights=weights)
        return {"value": vm, "norm": nm}

    def evaluate_orbitals(self, configs):
        return self.orbitals.mos(self.orbitals.true_positions(configs))

    def keys(self):
        return {"value", "norm"}

    def shapes(self):
        return {"value": (self.norb, self.norb), "norm": (self.norb,)}


def normalize_obdm(obdm, norm):
    """rho_ij / sqrt(norm_i norm_j) (obdm.py:252-253)."""
    return obdm / np.sqrt(np.outer(norm, norm))
