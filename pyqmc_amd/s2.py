"""Total-spin estimator — public interface of ``pyqmc/observables/s2_accumulator.py`` (``S2Accumulator``).

For fixed electron counts Sz = (N_up - N_dn)/2 is sharp and S^2 = Sz(Sz+1) + S_- S_+, whose local value is

    S^2_loc(R) = Sz(Sz+1) + N_dn - sum_{i up, j dn} Psi(R^{i<->j}) / Psi(R),

R^{i<->j} putting up electron i at r_j and down electron j at r_i.  Two routes compute the swap ratios:

* **fused** (``pqa_s2``): real wave functions living on one device handle — Slater (one or more determinants), optionally times
  JastrowSpin, open or periodic at Gamma.  The ratios come in closed form from the resident state (pqa_s2.hip) and the state is
  not modified.
* **protocol**: every other wave function (complex orbitals, twisted cells, a three-body Jastrow factor, the CPU oracle's
  objects, ...).  Per pair: up electron i is moved to r_j (``testvalue`` + ``configs.move`` + ``updateinternals``), the ratio of
  moving down electron j to r_i is read with ``testvalue``, and i is moved back; ``wf.recompute(configs)`` at the end leaves the
  wave function describing ``configs`` without the round-off of the unwinding moves.

``last_route`` names the route of the last evaluation ("fused" or "protocol").
"""

import numpy as np

from . import _ffi
from .wf import readonly_device as fused_handle  # (the fused-route predicate, kept under its name here)


def device_s2(dev, with_ratios=False):
    """``pqa_s2`` on a device handle: S^2 (W) of the resident walkers and, with ``with_ratios``, the swap ratios (W, N_up, N_dn)."""
    nu, nd = dev.nelec
    s2 = np.empty(dev.W)
    rat = np.empty((dev.W, nu, nd)) if with_ratios else None
    dev.call("pqa_s2", _ffi.ptr(s2), None if rat is None else _ffi.ptr(rat))
    return (s2, rat) if with_ratios else s2


class S2Accumulator:
    """Local estimator of <S^2> (s2_accumulator.py): ``__call__`` -> {"S2": (nconf,)}, ``avg`` -> {"S2": mean}.

    nelec: (n_up, n_dn); electrons 0 .. n_up-1 are spin up, the rest spin down (the Slater convention)."""

    def __init__(self, nelec):
        self.nelec = tuple(int(n) for n in nelec)
        nu, nd = self.nelec
        self.sz = 0.5 * (nu - nd)
        self.last_route = None

    def __call__(self, configs, wf):
        dev = fused_handle(wf)
        if dev is not None and tuple(dev.nelec) == self.nelec and dev.W == configs.configs.shape[0]:
            # the handle's resident walkers are `configs` (the drivers fetch them from the device before any host accumulator)
            self.last_route = "fused"
            return {"S2": device_s2(dev)}
        self.last_route = "protocol"
        return {"S2": self._protocol(configs, wf)}

    def _protocol(self, configs, wf):
        nu, nd = self.nelec
        nconf = configs.configs.shape[0]
        accept = np.ones(nconf, dtype=bool)
        orig = configs.configs.copy()
        swap = np.zeros(nconf, dtype=wf.dtype)
        for i in range(nu):
            for j in range(nu, nu + nd):
                new_i = configs.make_irreducible(i, orig[:, j].copy())
                r1, saved = wf.testvalue(i, new_i)
                configs.move(i, new_i, accept)
                wf.updateinternals(i, new_i, configs, mask=accept, saved_values=saved)
                r2, _ = wf.testvalue(j, configs.make_irreducible(j, orig[:, i].copy()))
                swap += r1 * r2
                back = configs.make_irreducible(i, orig[:, i].copy())
                _, saved = wf.testvalue(i, back)
                configs.move(i, back, accept)
                wf.updateinternals(i, back, configs, mask=accept, saved_values=saved)
        configs.configs[...] = orig
        if nu and nd:
            wf.recompute(configs)
        return self.sz * (self.sz + 1) + nd - swap

    def avg(self, configs, wf):
        return {k: np.mean(v, axis=0) for k, v in self(configs, wf).items()}

    def resident_scope(self, wf):
        """None when ``avg_resident`` can run for ``wf``, else the reason (the fused route's rules)."""
        dev = fused_handle(wf)
        if dev is None:
            return "the wave function is not a real Slater (x two-body Jastrow) product on one device handle"
        if tuple(dev.nelec) != self.nelec:
            return "the wave function has other electron numbers than the accumulator"
        return None

    def avg_resident(self, wf, weights=None):
        """The walker mean of S^2 for the walkers resident behind ``wf``, without a host container; with ``weights`` (W,) the
        weighted mean sum_w w_w S2_w / sum_w w_w (W doubles come back, the weighting is done on the host)."""
        why = self.resident_scope(wf)
        if why is not None:
            raise ValueError(f"S2Accumulator.avg_resident: {why}")
        dev = fused_handle(wf)
        if weights is not None:
            weights = _ffi.walker_weights(weights, dev.W)
        self.last_route = "fused"
        s2 = device_s2(dev)
        return {"S2": np.mean(s2) if weights is None else np.dot(weights, s2) / weights.sum()}

    def keys(self):
        return self.shapes().keys()

    def shapes(self):
        return {"S2": ()}
