"""Structure factor — public interface of ``pyqmc/observables/accumulators.py`` (``SqAccumulator``).

Per walker and wave vector q

    Sq(q)     = |sum_j       exp(i q.r_j)|^2 / N
    spinSq(q) = |sum_j s_j * exp(i q.r_j)|^2 / N        (s_j = +1 for the n_up first electrons, -1 for the others)

on the q vectors of ``qlist``, or, when none is given, on the half-space grid ``generate_positive_gpoints(nq, recvec)`` of the
cell's reciprocal lattice.  Two routes compute it:

* **fused** (``pqa_sq``): every wave function whose device handle holds ``configs`` as its resident walkers, whatever its kind
  (one or many determinants, three-body, complex, twisted): S(q) reads only the coordinates, which the kernel takes in place
  (pqa_sq.hip), periodic points folded into the cell.  Grid points go through a power recurrence of the three base phases,
  an explicit ``qlist`` through one sincos per (q, electron).
* **host**: every other case (the CPU oracle's objects, no wave function, walkers that are not the handle's).  NumPy over walker
  chunks, so that the (walkers, N, Q) phase temporary stays within ``host_chunk_bytes``.

``last_route`` names the route of the last evaluation ("fused" or "host").
"""

import numpy as np

from . import _ffi
from .ewald import generate_positive_gpoints


def device_handle(wf):
    """The device handle ``wf`` lives on (the shared one of a MultiplyWF, or a bare factor's own), or None."""
    dev = wf.fused_device() if hasattr(wf, "fused_device") else getattr(wf, "_dev", None)
    return dev if hasattr(dev, "vmc_sweeps") else None


def device_sq(dev, qlist, qn=None, recip=None, mean=False):
    """``pqa_sq`` on a device handle: (Sq, spinSq) of the resident walkers, each (W, Q), or (Q,) walker means with ``mean``.
    ``qn`` (Q, 3) integer coordinates of the q vectors in the basis of the rows of ``recip`` (3, 3) select the recurrence path."""
    q = _ffi.f64(np.reshape(qlist, (-1, 3)))
    nq = q.shape[0]
    qi = None if qn is None else np.ascontiguousarray(np.reshape(qn, (nq, 3)), dtype=np.int32)
    rc = None if qi is None else _ffi.f64(np.reshape(recip, (3, 3)))
    shape = (nq,) if mean else (dev.W, nq)
    sq, sp = np.empty(shape), np.empty(shape)
    dev.call("pqa_sq", int(nq), _ffi.ptr(q), _ffi.ptr(qi), _ffi.ptr(rc), int(bool(mean)), _ffi.ptr(sq), _ffi.ptr(sp))
    return sq, sp


def device_sq_w(dev, qlist, weights, qn=None, recip=None):
    """``pqa_sq_w`` on a device handle: the weighted walker means (Sq, spinSq), each (Q,), of the resident walkers with the walker
    ``weights`` (W,); ``qn`` / ``recip`` as in ``device_sq``."""
    w = _ffi.walker_weights(weights, dev.W)
    q = _ffi.f64(np.reshape(qlist, (-1, 3)))
    nq = q.shape[0]
    qi = None if qn is None else np.ascontiguousarray(np.reshape(qn, (nq, 3)), dtype=np.int32)
    rc = None if qi is None else _ffi.f64(np.reshape(recip, (3, 3)))
    sq, sp = np.empty(nq), np.empty(nq)
    dev.call("pqa_sq_w", int(nq), _ffi.ptr(q), _ffi.ptr(qi), _ffi.ptr(rc), _ffi.ptr(w), _ffi.ptr(sq), _ffi.ptr(sp))
    return sq, sp


class SqAccumulator:
    """Charge and spin structure factors (accumulators.py:191-234): ``__call__`` -> {"Sq": (nconf, Q), "spinSq": (nconf, Q)},
    ``avg`` -> the walker means (Q,).

    cell: provides ``nelec`` and, without ``qlist``, ``lattice_vectors()``; nq: half-width of the q grid; qlist: (Q, 3) Cartesian
    q vectors (``nq`` is then ignored and ``cell`` may be a molecule)."""

    host_chunk_bytes = 64 << 20  # bound of the host route's complex phase temporary

    def __init__(self, cell, nq=4, qlist=None):
        if qlist is not None:
            self.qlist = np.asarray(qlist, dtype=float).reshape(-1, 3)
            self.qn = self.recip = None
        else:
            recvec = np.linalg.inv(cell.lattice_vectors()).T
            self.qlist, self.qn = generate_positive_gpoints(nq, recvec)
            self.recip = recvec * 2 * np.pi  # the rows the integer coordinates refer to: qlist == qn @ recip
        self.nup = int(cell.nelec[0])
        self.nelec = int(sum(cell.nelec))
        self.last_route = None

    def _fused(self, configs, wf):
        dev = device_handle(wf)
        if dev is None or tuple(dev.nelec) != (self.nup, self.nelec - self.nup):
            return None
        if configs is not None and dev.W != configs.configs.shape[0]:  # (configs = None: the resident walkers themselves)
            return None
        # the handle's resident walkers are `configs` (the drivers fetch them from the device before any host accumulator)
        return dev

    def _host(self, x, mean):
        W, N = x.shape[0], x.shape[1]
        Q = self.qlist.shape[0]
        step = max(1, int(self.host_chunk_bytes // max(16 * N * Q, 1)))
        sq, sp = np.empty((W, Q)), np.empty((W, Q))
        for w0 in range(0, W, step):
            ph = np.exp(1j * (x[w0 : w0 + step] @ self.qlist.T))  # (chunk, N, Q)
            up, dn = ph[:, : self.nup].sum(axis=1), ph[:, self.nup :].sum(axis=1)
            tot, spin = up + dn, up - dn
            sq[w0 : w0 + step] = (tot.real**2 + tot.imag**2) / self.nelec
            sp[w0 : w0 + step] = (spin.real**2 + spin.imag**2) / self.nelec
        return (sq.mean(axis=0), sp.mean(axis=0)) if mean else (sq, sp)

    def _eval(self, configs, wf, mean):
        dev = self._fused(configs, wf)
        if dev is not None:
            self.last_route = "fused"
            sq, sp = device_sq(dev, self.qlist, self.qn, self.recip, mean=mean)
        else:
            self.last_route = "host"
            sq, sp = self._host(np.asarray(configs.configs, dtype=float), mean)
        return {"Sq": sq, "spinSq": sp}

    def __call__(self, configs, wf):
        return self._eval(configs, wf, False)

    def avg(self, configs, wf):
        return self._eval(configs, wf, True)

    def resident_scope(self, wf):
        """None when ``avg_resident`` can run for ``wf``, else the reason (the fused route's rules)."""
        dev = device_handle(wf)
        if dev is None:
            return "the wave function does not live on one device handle"
        if tuple(dev.nelec) != (self.nup, self.nelec - self.nup):
            return "the wave function has other electron numbers than the accumulator's system"
        if self._fused(None, wf) is None:  # (the route predicate of __call__ / avg decides here too)
            return "the accumulator's fused route does not take this wave function"
        return None

    def avg_resident(self, wf, weights=None):
        """The walker means for the walkers resident behind ``wf``, without a host container; with ``weights`` (W,) the weighted
        means sum_w w_w res_w / sum_w w_w, reduced on the device (``pqa_sq_w``)."""
        why = self.resident_scope(wf)
        if why is not None:
            raise ValueError(f"SqAccumulator.avg_resident: {why}")
        dev = self._fused(None, wf)
        self.last_route = "fused"
        if weights is None:
            sq, sp = device_sq(dev, self.qlist, self.qn, self.recip, mean=True)
        else:
            sq, sp = device_sq_w(dev, self.qlist, weights, self.qn, self.recip)
        return {"Sq": sq, "spinSq": sp}

    def keys(self):
        return set(["Sq", "spinSq"])

    def shapes(self):
        return {"Sq": (len(self.qlist),), "spinSq": (len(self.qlist),)}
