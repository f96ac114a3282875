"""Two-body density matrix accumulator — SURVEY.md §8(f3); public interface of ``pyqmc/observables/tbdm.py``.

One spin sector ``tbdm[s1,s2][i,j,k,l] = <c+_{s1,i} c+_{s2,k} c_{s2,l} c_{s1,j}>`` (PySCF's index convention), sampled
by moving an electron pair (a, b) to auxiliary positions (r1', r2') drawn from the orbital densities (Eq. 10 of
DOI:10.1063/1.4793531; tbdm.py:188-283).  On the device handle of an ``obdm.OrbitalEvaluator``:

* two resident auxiliary walks (``pqa_dm_walk``, slots 0 and 1) and the basis orbitals at the electrons of both groups
  (``pqa_dm_points``);
* the estimator in factorised form (``pqa_tbdm_accumulate`` -> ``k_tbdm_acc``): with the pair ratios
  ``R[a][b] = Psi(r_a -> r1', r_b -> r2') / Psi`` the sum over electron pairs is ``M = Phi_a^T R Phi_b`` — two small
  matrix products per configuration — and ``value[(i,j,k,l)] = M[i][k] conj(phi_j(r1')) conj(phi_l(r2')) / (f1 f2)``.
  The reference builds a (configurations x pairs x index tuples) tensor instead.

Two routes give the pair ratios:

* **fused** (``pqa_tbdm_sweep``): real wave functions living on one device handle whose resident walkers are the configurations —
  Slater (one or more determinants), optionally times JastrowSpin, open or periodic at Gamma — with a real evaluator on the same
  device.  The ratios come in closed form from the resident state (pqa_tbdm.hip), which is not modified, for a walker chunk at a
  time, and ``k_tbdm_acc`` consumes them on the device: only the two assignments cross the bus.
  With ``complex_device=True`` (opt-in) complex and twisted handles and complex evaluators take this route as well
  (``pqa_tbdm_sweep_c``): the complex pair ratios come in closed form from the resident complex inverse (complex determinant
  weights, a complex quotient, the real Jastrow difference) and ``k_tbdm_acc`` reads them as it reads the protocol route's.  The
  entry is chosen per pair: anything complex or twisted on either side goes through ``pqa_tbdm_sweep_c``, two real handles through
  ``pqa_tbdm_sweep`` bit for bit as before, and a twisted evaluator with an untwisted handle (whose folded walkers have lost the
  wrap phase of the orbitals at the electrons) stays on the protocol route.  ``value`` is complex and the norms real, as on the
  protocol route.
  With ``three_body_device=True`` (opt-in) real wave functions with a three-body Jastrow factor take it too (``pqa_tbdm_sweep_j3``):
  both electrons of every pair go to the same two points, so two tables G_s(q)[j] = t(q, s; r_j, s_j), the listed electrons' P_e, the
  cross term t(r1, r2) and the old pair terms give dU3_ab for all pairs of a walker (``k_j3_moves``, ``csrc/pqa_j3dm.hpp``).
  Complex or twisted three-body handles stay on the protocol route.
* **protocol**: every other wave function.  ``testvalue`` + ``updateinternals`` move electron a to r1' (Sherman-Morrison on the
  device), ``testvalue_many`` gives the ratios of all partners b at once (``k_testvalue_many``), and a second ``updateinternals``
  moves a back.

``last_route`` names the route of the last evaluation.  ``numpy.random`` is consumed in the reference's order on both routes (the
ratios draw nothing).
"""

import numpy as np

from . import _ffi
from .obdm import AuxiliaryWalkers, OrbitalEvaluator, _FusedScope

ROUTES = (None, "fused", "protocol")


def _sweep(entry, dtype, dev, ev, k, spins, assign_a, assign_b, ijkl, first, walker_chunk, with_ratios):
    a, b = (np.ascontiguousarray(x, dtype=np.int32) for x in (assign_a, assign_b))
    if a.shape != (dev.W,) or b.shape != (dev.W,):
        raise ValueError(f"assignments ({dev.W},) expected, got {a.shape} and {b.shape}")
    R = np.empty((dev.W, dev.nelec[spins[0]], dev.nelec[spins[1]]), dtype=dtype) if with_ratios else None
    if ijkl is not None:
        ijkl = np.ascontiguousarray(ijkl, dtype=np.int32)
    dev.call(entry, ev.dev._h, int(k), int(spins[0]), int(spins[1]), _ffi.ptr(a), _ffi.ptr(b), _ffi.ptr(ijkl),
             0 if ijkl is None else ijkl.shape[1], int(first), int(walker_chunk), _ffi.ptr(R))
    return R


def device_tbdm_sweep(dev, ev, k, spins, assign_a, assign_b, ijkl=None, first=True, walker_chunk=0, with_ratios=False):
    """``pqa_tbdm_sweep``: the pair ratios of wave-function handle ``dev`` at kept sample ``k`` of the two resident walks of the
    evaluator ``ev`` (an ``OrbitalEvaluator``), contracted into ``ev``'s accumulators for the index tuples ``ijkl`` (4, M) (None:
    ratios only).  Returns the ratios (W, nea, neb) with ``with_ratios``, else None."""
    return _sweep("pqa_tbdm_sweep", float, dev, ev, k, spins, assign_a, assign_b, ijkl, first, walker_chunk, with_ratios)


def device_pair_ratios(dev, ev, k, spins, assign_a, assign_b, walker_chunk=0):
    """R (W, nea, neb) = Psi(r_a -> r1', r_b -> r2') / Psi of ``dev``'s resident walkers, r1' / r2' the auxiliary walkers
    ``assign_a`` / ``assign_b`` of kept sample ``k`` in slots 0 / 1 of the evaluator ``ev``; nothing is accumulated."""
    return device_tbdm_sweep(dev, ev, k, spins, assign_a, assign_b, walker_chunk=walker_chunk, with_ratios=True)


def device_tbdm_sweep_c(dev, ev, k, spins, assign_a, assign_b, ijkl=None, first=True, walker_chunk=0, with_ratios=False):
    """``pqa_tbdm_sweep_c``: ``device_tbdm_sweep`` for complex and twisted handles ``dev`` and complex evaluators ``ev`` (real ones are
    taken too): complex ratios (W, nea, neb), and ``ev``'s value accumulator is complex (``ev.fetch(..., cplx=True)``)."""
    return _sweep("pqa_tbdm_sweep_c", complex, dev, ev, k, spins, assign_a, assign_b, ijkl, first, walker_chunk, with_ratios)


def device_pair_ratios_c(dev, ev, k, spins, assign_a, assign_b, walker_chunk=0):
    """``device_pair_ratios`` through ``pqa_tbdm_sweep_c``: complex R (W, nea, neb); nothing is accumulated."""
    return device_tbdm_sweep_c(dev, ev, k, spins, assign_a, assign_b, walker_chunk=walker_chunk, with_ratios=True)


def device_tbdm_sweep_j3(dev, ev, k, spins, assign_a, assign_b, ijkl=None, first=True, walker_chunk=0, with_ratios=False):
    """``pqa_tbdm_sweep_j3``: ``device_tbdm_sweep`` for real handles ``dev`` with a three-body Jastrow factor (handles without one are
    taken too and give ``device_tbdm_sweep``'s bits)."""
    return _sweep("pqa_tbdm_sweep_j3", float, dev, ev, k, spins, assign_a, assign_b, ijkl, first, walker_chunk, with_ratios)


def device_pair_ratios_j3(dev, ev, k, spins, assign_a, assign_b, walker_chunk=0):
    """``device_pair_ratios`` through ``pqa_tbdm_sweep_j3``: R (W, nea, neb); nothing is accumulated."""
    return device_tbdm_sweep_j3(dev, ev, k, spins, assign_a, assign_b, walker_chunk=walker_chunk, with_ratios=True)


class TBDMAccumulator(_FusedScope):
    """Keys ``value`` (M,), ``norm_a`` (norb_a,), ``norm_b`` (norb_b,) per configuration for the M index tuples ``ijkl``
    (default: the whole sector).  ``orb_coeff`` (2, nao, norb): orbital basis per spin; ``spin`` = (s1, s2).

    ``route``: None takes the fused route whenever the wave function and the evaluator are in its scope and the protocol route
    otherwise; "fused" raises outside the scope; "protocol" always moves the electrons.  ``walker_chunk``: walkers per scratch chunk
    of the fused route (0: the library's bound).  ``complex_device``: with True complex and twisted handles and complex evaluators
    are in the fused scope too (``pqa_tbdm_sweep_c``), except a twisted evaluator with an untwisted handle; with False (the default)
    they take the protocol route and ``route="fused"`` raises for them.  ``three_body_device``: with True real wave functions with a
    three-body Jastrow factor are in the fused scope too (``pqa_tbdm_sweep_j3``, a real evaluator); complex or twisted three-body
    handles stay on the protocol route.  With False (the default) three-body wave functions take the protocol route."""

    ENTRIES = ("pqa_tbdm_sweep", "pqa_tbdm_sweep_c", "pqa_tbdm_sweep_j3")

    def __init__(self, mol, orb_coeff, spin, nsweeps=4, tstep=0.50, warmup=200, naux=None, ijkl=None, kpts=None,
                 eval_gto_precision=None, device=0, route=None, walker_chunk=0, complex_device=False, three_body_device=False):
        if route not in ROUTES:
            raise ValueError(f"route must be one of {ROUTES}")
        self.complex_device = self._flag("complex_device", complex_device)
        self.three_body_device = self._flag("three_body_device", three_body_device)
        self._route, self._walker_chunk, self.last_route = route, int(walker_chunk), None
        self.orbitals = OrbitalEvaluator(mol, orb_coeff, kpts=kpts, eval_gto_precision=eval_gto_precision, device=device)
        self._mol, self.dtype = self.orbitals.mol, self.orbitals.mo_dtype
        self._tstep, self._nsweeps, self._warmup, self._naux, self._spin_sector = tstep, nsweeps, warmup, naux, tuple(spin)
        nup, ndn = self._mol.nelec
        self._electrons = [np.arange(s * nup, nup + s * ndn) for s in spin]
        na, nb = self.orbitals.nmo()
        if ijkl is None:
            ijkl = np.stack(np.meshgrid(np.arange(na), np.arange(na), np.arange(nb), np.arange(nb), indexing="ij"), -1).reshape(-1, 4)
        self._ijkl = np.ascontiguousarray(np.asarray(ijkl).T, dtype=np.int32)  # (4, M)
        self._walkers = None

    @property
    def _aux_configs(self):
        return None if self._walkers is None else [w.configs for w in self._walkers]

    def _pair_ratios(self, configs, wf, there_a, there_b):
        """R (nconf, nea, neb): electron a at ``there_a`` and electron b at ``there_b``; 0 where a and b are one electron."""
        ea, eb = self._electrons
        R = np.zeros((configs.configs.shape[0], len(ea), len(eb)), dtype=wf.dtype)
        for ia, a in enumerate(ea):
            partners = eb != a
            first, saved = wf.testvalue(a, there_a)
            wf.updateinternals(a, there_a, configs, saved_values=saved)
            R[:, ia, partners] = first[:, None] * wf.testvalue_many(eb[partners], there_b)
            wf.updateinternals(a, configs.electron(a), configs)  # and back: the state ends where it started
        return R

    def _scope(self, wf):
        """(handle, reason): the handle the fused route reads ``wf`` from, and why it cannot take it, or None when it can."""
        dev, why = self._common_scope(wf)
        if why is None and min(len(e) for e in self._electrons) < 1:
            why = "a spin block of the sector is empty"
        return dev, why

    def _fused_device(self, configs, wf):
        """The handle the fused route evaluates ``wf`` on, or None: a read-only-scope wave function whose resident walkers are the
        configurations, whole non-empty spin blocks, an evaluator in scope (real; with ``complex_device`` also complex, and twisted
        when the handle is) on the same device."""
        if self._route == "protocol":
            return None
        dev, why = self._scope(wf)
        ok = why is None and dev.W == configs.configs.shape[0]
        if not ok and self._route == "fused":
            if self.three_body_device:
                raise ValueError("route='fused' needs a Slater (x two-body x three-body Jastrow) wave function on one device handle whose "
                                 "resident walkers are the configurations, and an orbital evaluator in scope on the same device: "
                                 + (why or "the handle holds other walkers than the configurations"))
            if self.complex_device:
                raise ValueError("route='fused' needs a Slater (x two-body Jastrow) wave function on one device handle whose resident "
                                 "walkers are the configurations, and an orbital evaluator on the same device that is twisted only if "
                                 "the handle is: " + (why or "the handle holds other walkers than the configurations"))
            raise ValueError("route='fused' needs a real Slater (x two-body Jastrow) wave function on one device handle whose resident "
                             "walkers are the configurations, and a real orbital evaluator on the same device")
        return dev if ok else None

    def resident_scope(self, wf):
        """None when ``avg_resident`` can run for ``wf``, else the reason (the fused route's rules)."""
        if self._route == "protocol":
            return "the accumulator is bound to route='protocol'"
        return self._scope(wf)[1]

    def avg_resident(self, wf, weights=None):
        """The walker mean for the walkers resident behind ``wf``, without a host container: the electrons' coordinates are gathered
        on the device (``pqa_dm_points_resident``), the sweeps are those of the fused route, and with ``weights`` (W,) the three
        means are the weighted ones sum_w w_w res_w / sum_w w_w (``pqa_dm_fetch_w``).  ``numpy.random`` is consumed as by
        ``__call__``."""
        why = self.resident_scope(wf)
        if why is not None:
            raise ValueError(f"TBDMAccumulator.avg_resident: {why}")
        dev = self._device(wf)
        nconf, scale = dev.W, 1.0 / self._nsweeps
        if weights is not None:
            weights = _ffi.walker_weights(weights, nconf)
        cplx = self._sample(None, wf, resident=dev)
        if cplx and weights is None:  # (the complex entry's plain mean is the unit-weight instance of the weighted reduction: same bits)
            weights = np.ones(nconf)
        na, nb = self.orbitals.nmo()
        shapes = ((self._ijkl.shape[1],), (na,), (nb,))
        if weights is None:
            out = [self.orbitals.fetch(i, nconf, sh, scale, True, cplx and i == 0) for i, sh in enumerate(shapes)]
        else:
            out = [self.orbitals.fetch_w(i, nconf, sh, scale, weights, cplx and i == 0) for i, sh in enumerate(shapes)]
        return dict(zip(("value", "norm_a", "norm_b"), out))

    def _sample(self, configs, wf, resident=None):
        """One evaluation into the evaluator's accumulators.  ``resident``: the wave function's handle, whose resident walkers are
        the configurations (no host container: fused route, coordinates gathered on the device)."""
        ev = self.orbitals
        nconf = configs.configs.shape[0] if resident is None else resident.W
        dev = self._fused_device(configs, wf) if resident is None else resident
        self.last_route = "protocol" if dev is None else "fused"
        if self._walkers is None:
            naux = nconf if self._naux is None else self._naux
            self._walkers = [AuxiliaryWalkers(ev, 0), AuxiliaryWalkers(ev, 1)]
            for w in self._walkers:  # the reference warms both walks up on the spin-0 orbitals with the default step (tbdm.py:133-135)
                w.start(naux, int(np.sum(self._mol.nelec)))
                w.advance(0, self._warmup, 0.5)
        kept, pick = [], []
        for s, w in enumerate(self._walkers):
            kept.append(w.advance(s, self._nsweeps, self._tstep, keep=self._nsweeps)[1])
            pick.append(np.random.randint(0, len(w.x), size=(self._nsweeps, nconf)).astype(np.int32))  # after the walk (tbdm.py:156-161)
        if resident is None:
            x = ev.true_positions(configs)
            for s in (0, 1):
                ev.points(s, s, x[:, self._electrons[s]])
        else:
            for s in (0, 1):
                ev.points_resident(s, dev, self._electrons[s], cplx=self._complex_entry(dev), j3=self._j3_entry(dev))
        j3 = dev is not None and self._j3_entry(dev)
        cplx = dev is not None and not j3 and self._complex_entry(dev)
        sweep = device_tbdm_sweep_j3 if j3 else device_tbdm_sweep_c if cplx else device_tbdm_sweep
        for sw in range(self._nsweeps if dev is not None else 0):  # the ratios stay on the device
            sweep(dev, ev, sw, self._spin_sector, pick[0][sw], pick[1][sw], self._ijkl, sw == 0, self._walker_chunk)
        for sw in range(self._nsweeps if dev is None else 0):
            there = [ev.container(kept[s][sw][pick[s][sw]]).electron(0) for s in (0, 1)]
            R = np.ascontiguousarray(self._pair_ratios(configs, wf, *there))
            rc = np.iscomplexobj(R)
            cplx = rc or ev.dev.cplx
            ev.dev.call("pqa_tbdm_accumulate", sw, nconf, R.shape[1], R.shape[2], _ffi.ptr(pick[0][sw]), _ffi.ptr(pick[1][sw]), _ffi.ptr(R),
                        int(rc), _ffi.ptr(self._ijkl), self._ijkl.shape[1], int(sw == 0))
        return cplx

    def _result(self, configs, wf, mean):
        cplx, nconf, scale = self._sample(configs, wf), configs.configs.shape[0], 1.0 / self._nsweeps
        na, nb = self.orbitals.nmo()
        return {"value": self.orbitals.fetch(0, nconf, (self._ijkl.shape[1],), scale, mean, cplx),
                "norm_a": self.orbitals.fetch(1, nconf, (na,), scale, mean), "norm_b": self.orbitals.fetch(2, nconf, (nb,), scale, mean)}

    def __call__(self, configs, wf):
        return self._result(configs, wf, False)

    def avg(self, configs, wf):
        """Mean over the configurations, reduced on the device."""
        return self._result(configs, wf, True)

    def keys(self):
        return {"value", "norm_a", "norm_b"}

    def shapes(self):
        nmo = self.orbitals.nmo()
        return {"value": (self._ijkl.shape[1],), "norm_a": (nmo[self._spin_sector[0]],), "norm_b": (nmo[self._spin_sector[1]],)}


def normalize_tbdm(tbdm, norm_a, norm_b):
    """tbdm_ijkl / sqrt(norm_a_i norm_a_j norm_b_k norm_b_l): ratio of averages of Eq. (10), PySCF index convention
    (tbdm.py:286-290)."""
    ra, rb = np.sqrt(norm_a), np.sqrt(norm_b)
    return tbdm / (ra[:, None, None, None] * ra[None, :, None, None] * rb[None, None, :, None] * rb[None, None, None, :])
