"""Accumulators over several wave functions — ``pyqmc/observables/accumulators_multiwf.py``.

``avg(configs, wfs, weights)`` evaluates a single-wave-function accumulator on every wave function of ``wfs`` at the mixture's walkers
and forms ``sum_c q_j(c) weights[i, j, c] / nconfig`` for every pair ``(i, j)``; ``weights`` is ``psi_i^* psi_j / rho`` per walker
(``sample_many.compute_weights``).  ``sample_many.sample_overlap`` accepts exactly the accumulators that carry the
``multiple_wf`` marker; a plain single-wave-function accumulator is refused there up front.
"""

import numpy as np


def invert_list_of_dicts(A, asarray=True):
    """``[{'A': 1, 'B': 2}, {'A': 3, 'B': 5}]`` -> ``{'A': [1, 3], 'B': [2, 5]}``."""
    if asarray:
        return {k: np.asarray([a[k] for a in A]) for k in A[0].keys()}
    return {k: [a[k] for a in A] for k in A[0].keys()}


class EnergyAccumulatorMultipleWF:
    """Weighted energies ``{key: (nwf, nwf)}`` of an ``EnergyAccumulator`` (accumulators_multiwf.py:29-60): the energies of each
    wave function minus ``offset``, weighted by ``weights[i, j, c]`` and averaged over the walkers; ``offset`` is returned as well.

    One deliberate difference: ``offset`` is returned as a NumPy array.  The reference returns it as given, and with its default
    ``offset=0`` (a Python int) ``sample_overlap_worker``'s ``rolling_average`` fails on it (``it.shape``).

    ``route``: None (default) or "protocol": the host formula on the energy object's per-walker rows.  "device": the energies from
    one ``pqa_mix_moments`` call on the resident state (no state has columns), ``NotImplementedError`` with ``mix_route``'s reason
    when out of its scope; ``avg_resident(wfs)`` is ``avg`` without a host container then.  ``last_route`` records what the last
    evaluation took."""

    multiple_wf = True

    def __init__(self, enacc, offset=0, route=None):
        if route not in (None, "device", "protocol"):
            raise ValueError(f"route must be None, 'device' or 'protocol', got {route!r}")
        self.enacc = enacc
        self._offset = offset
        self.route, self.last_route = route, None

    def resolve_route(self, wfs):
        """The route ``avg`` takes for ``wfs``: "device" only when asked for (see ``route``)."""
        from .accumulators import resolve_mix_route

        return resolve_mix_route(self, wfs, self.route or "protocol", "EnergyAccumulatorMultipleWF")

    def avg_resident(self, wfs):
        """``avg`` on the device route for the walkers resident behind ``wfs``: the energy object bound and keyed per state as the
        protocol route does, then one ``pqa_mix_moments`` call without columns."""
        from .accumulators import mix_energy_keys
        from .energy import KEYS
        from .sample_many import fused_scope, mix_moments

        devs, why = fused_scope(wfs)
        if devs is None:
            raise NotImplementedError(f"EnergyAccumulatorMultipleWF.avg_resident: {why}")
        keys = mix_energy_keys(self.enacc, devs)
        for wf in wfs:
            wf.wf_factors[0]._saved = None  # (the saved rows of a gradient_value call are overwritten)
        empty = (np.zeros(0, dtype=np.int32), np.zeros(0, dtype=np.int32))
        _, en, _ = mix_moments(devs, [empty] * len(devs), offset=self._offset, threshold=self.enacc.threshold, seeds=keys)
        self.last_route = "device"
        weighted_dat = {k: en[i] for i, k in enumerate(KEYS)}
        weighted_dat["offset"] = np.asarray(self._offset) + 0.0
        return weighted_dat

    def avg(self, configs, wfs, weights):
        """weights (nwf, nwf, nconfig); returns {key: (nwf, nwf)} and ``offset``."""
        if self.resolve_route(wfs) == "device":
            dev = wfs[0].fused_device()
            if self.enacc.check_configs and not (dev.W == len(configs.configs) and np.array_equal(dev.configs(), configs.configs)):
                raise ValueError("walkers on the device differ from `configs`: call wf.recompute(configs) "
                                 "(or keep wf.updateinternals in step with configs.move) first")
            return self.avg_resident(wfs)
        self.last_route = "protocol"
        energies = invert_list_of_dicts([self.enacc(configs, wf) for wf in wfs])
        weighted_dat = {}
        nconfig = configs.configs.shape[0]
        for k, en in energies.items():
            weighted_dat[k] = np.einsum("jc,ijc->ij", en - self._offset, weights) / nconfig
        weighted_dat["offset"] = np.asarray(self._offset) + 0.0
        return weighted_dat

    def keys(self):
        return self.enacc.keys()

    def shapes(self):
        """The shapes of the single-wave-function accumulator (without the wave-function axes)."""
        return self.enacc.shapes()


class AdaptSingleAccumulator:
    """Any single-wave-function accumulator weighted the same way (accumulators_multiwf.py:63-91), without an offset.

    One deliberate difference: the reference's ``keys`` and ``shapes`` read ``self.enacc``, an attribute this class never sets (they
    raise there); here they read ``self.acc``."""

    multiple_wf = True

    def __init__(self, acc):
        self.acc = acc

    def avg(self, configs, wfs, weights):
        quantities = invert_list_of_dicts([self.acc(configs, wf) for wf in wfs])
        weighted_dat = {}
        nconfig = configs.configs.shape[0]
        for k, en in quantities.items():
            weighted_dat[k] = np.einsum("jc,ijc->ij", en, weights) / nconfig
        return weighted_dat

    def keys(self):
        return self.acc.keys()

    def shapes(self):
        return self.acc.shapes()
