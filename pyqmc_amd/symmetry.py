"""Symmetry-operator estimators — public interface of ``pyqmc/observables/accumulators.py`` (``SymmetryAccumulator``,
``SymmetryAccumulatorPBC``).

For every named 3x3 operator S the local value is the ratio Psi(SR)/Psi(R), SR moving every electron to

    x' = (x - o) @ S + o        (row vectors, the reference's ``einsum("ijk,kl->ijl", x, S)``),

with o = 0 for ``SymmetryAccumulator`` and ``origins[name]`` for ``SymmetryAccumulatorPBC``, which also folds the transformed
points back into the cell (``enforce_pbc``).  Its average over walkers sampled from |Psi|^2 is <Psi|S|Psi>/<Psi|Psi>: +1 or -1
on every walker when Psi is even or odd under S.  Two routes compute it:

* **fused** (``pqa_symmetry``): real wave functions living on one device handle — Slater (one or more determinants), optionally
  times JastrowSpin, open or periodic at Gamma.  Every ratio is assembled on the device from the resident state
  (pqa_symmetry.hip), which is not modified.
* **protocol**: every other wave function (complex orbitals, twisted cells, a three-body Jastrow factor, the CPU oracle's
  objects, ...).  The reference's loop: per operator a copy of ``configs`` is transformed and recomputed, and
  ``wf.recompute(configs)`` at the end leaves the wave function describing ``configs`` again.

``last_route`` names the route of the last evaluation ("fused" or "protocol").
"""

import copy

import numpy as np

from . import _ffi
from .configs import enforce_pbc
from .wf import readonly_device


def device_symmetry(dev, ops, origins=None):
    """``pqa_symmetry`` on a device handle: ratios (nop, W) of the resident walkers under the operators ``ops`` (nop, 3, 3), each
    about its origin (``origins`` (nop, 3), or None for 0); periodic points are folded into the cell."""
    ops = _ffi.f64(np.reshape(ops, (-1, 3, 3)))
    nop = ops.shape[0]
    org = None if origins is None else _ffi.f64(np.reshape(origins, (nop, 3)))
    out = np.empty((nop, dev.W))
    dev.call("pqa_symmetry", nop, _ffi.ptr(ops), _ffi.ptr(org), _ffi.ptr(out))
    return out


class SymmetryAccumulator:
    """Psi(SR)/Psi(R) for every operator of ``symmetry_operators`` ({name: 3x3 matrix}, accumulators.py:237-283):
    ``__call__`` -> {name: (nconf,)}, ``avg`` -> {name: mean}."""

    def __init__(self, symmetry_operators):
        self.symmetry_operators = symmetry_operators
        self.last_route = None

    def _origins(self):
        return None

    def _fused(self, dev):
        """{name: (W,)} of the walkers resident behind the handle ``dev``."""
        names = list(self.symmetry_operators)
        self.last_route = "fused"
        if not names:
            return {}
        org = self._origins()
        ops = np.stack([np.asarray(self.symmetry_operators[k], dtype=float) for k in names])
        out = device_symmetry(dev, ops, None if org is None else np.stack([np.asarray(org[k], dtype=float) for k in names]))
        return dict(zip(names, out))

    def __call__(self, configs, wf):
        dev = readonly_device(wf)
        if dev is not None and dev.W == configs.configs.shape[0]:
            # the handle's resident walkers are `configs` (the drivers fetch them from the device before any host accumulator)
            return self._fused(dev)
        self.last_route = "protocol"
        return self._protocol(configs, wf)

    def resident_scope(self, wf):
        """None when ``avg_resident`` can run for ``wf``, else the reason (the fused route's rules)."""
        if readonly_device(wf) is None:
            return "the wave function is not a real Slater (x two-body Jastrow) product on one device handle"
        return None

    def avg_resident(self, wf, weights=None):
        """The walker means for the walkers resident behind ``wf``, without a host container; with ``weights`` (W,) the weighted
        means sum_w w_w ratio_w / sum_w w_w (nop W doubles come back, the weighting is done on the host)."""
        why = self.resident_scope(wf)
        if why is not None:
            raise ValueError(f"{type(self).__name__}.avg_resident: {why}")
        dev = readonly_device(wf)
        if weights is not None:
            weights = _ffi.walker_weights(weights, dev.W)
        return {k: np.mean(v) if weights is None else np.dot(weights, v) / weights.sum() for k, v in self._fused(dev).items()}

    def _protocol(self, configs, wf):
        symmetry_observables = {}
        original_wf_value = wf.value()
        configs_copy = copy.deepcopy(configs)
        for S_name, S_matrix in self.symmetry_operators.items():
            configs_copy.configs = np.einsum("ijk,kl->ijl", configs.configs, S_matrix)
            transformed_wf_value = wf.recompute(configs_copy)
            symmetry_observables[S_name] = (transformed_wf_value[0] / original_wf_value[0]) * np.exp(
                transformed_wf_value[1] - original_wf_value[1])
        wf.recompute(configs)
        return symmetry_observables

    def avg(self, configs, wf):
        return {k: np.mean(it, axis=0) for k, it in self(configs, wf).items()}

    def keys(self):
        return self.shapes().keys()

    def shapes(self):
        return {S: () for S in self.symmetry_operators.keys()}


class SymmetryAccumulatorPBC(SymmetryAccumulator):
    """Psi(SR)/Psi(R) with every operator applied about its own origin and the transformed points folded into the cell
    (accumulators.py:286-341): ``origins`` {name: (3,)} with the keys of ``symmetry_operators``."""

    def __init__(self, symmetry_operators, origins):
        super().__init__(symmetry_operators)
        self.origins = origins

    def _origins(self):
        return self.origins

    def _protocol(self, configs, wf):
        symmetry_observables = {}
        original_wf_value = wf.value()
        for S_name, S_matrix in self.symmetry_operators.items():
            configs_copy = copy.deepcopy(configs)
            configs_copy.configs -= self.origins[S_name][np.newaxis, np.newaxis, :]
            configs_copy.configs = np.einsum("ijk,kl->ijl", configs_copy.configs, S_matrix)
            configs_copy.configs += self.origins[S_name][np.newaxis, np.newaxis, :]
            if hasattr(configs, "wrap") and hasattr(configs, "lvecs"):
                configs_copy.configs, configs_copy.wrap = enforce_pbc(configs_copy.lvecs, configs_copy.configs)
            transformed_wf_value = wf.recompute(configs_copy)
            symmetry_observables[S_name] = (transformed_wf_value[0] / original_wf_value[0]) * np.exp(
                transformed_wf_value[1] - original_wf_value[1])
        wf.recompute(configs)
        return symmetry_observables
