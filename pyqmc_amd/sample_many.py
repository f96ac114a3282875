"""Sampling the mixture of several wave functions — ``pyqmc/method/sample_many.py``.

``sample_overlap_worker`` moves the walkers by Metropolis with the distribution proportional to ``sum_i |Psi_i|^2`` over the
wave functions ``wfs`` (deep copies of one device wave function, each on a handle of its own), through the protocol entry points
(``gradient``, ``gradient_value``, ``updateinternals`` with ``saved_values``).  Its draws are ``np.random.normal`` and
``np.random.rand`` in the reference's order, so a test can replay them.  Line minimisation (``pyqmc_amd.linemin``) calls it with
``energy=None``, the only value in scope here: the weighted energies need the reference's ``EnergyAccumulatorMultipleWF``, which
this package does not have.
"""

import numpy as np


def limdrift(g, cutoff=1):
    """``mc.limdrift`` (mc.py:76-89): each row of ``g`` (nconf, 3) shortened to at most ``cutoff``."""
    tot = np.linalg.norm(g, axis=1)
    mask = tot > cutoff
    g[mask, :] = cutoff * g[mask, :] / tot[mask, np.newaxis]
    return g


def _no_energy(energy):
    if energy is not None:
        raise NotImplementedError("sample_overlap with an energy accumulator needs EnergyAccumulatorMultipleWF, which pyqmc_amd does not "
                                  "provide: pass energy=None")


def compute_weights(wfs):
    """``psi_i^* psi_j / rho`` for every pair of wave functions and every walker -> weights[i, j, walker]."""
    phase, log_vals = [np.nan_to_num(np.array(x)) for x in zip(*[wf.value() for wf in wfs])]
    ref = np.max(log_vals, axis=0)  # for numerical stability
    rho = np.mean(np.nan_to_num(np.exp(2 * (log_vals - ref))), axis=0)
    psi = phase * np.nan_to_num(np.exp(log_vals - ref))
    return np.einsum("ic,jc->ijc", psi.conj(), psi / rho)


def invert_list_of_dicts(A, asarray=True):
    """``[{'A': 1, 'B': 2}, {'A': 3, 'B': 5}]`` -> ``{'A': [1, 3], 'B': [2, 5]}``."""
    if asarray:
        return {k: np.asarray([a[k] for a in A]) for k in A[0].keys()}
    return {k: [a[k] for a in A] for k in A[0].keys()}


def rolling_average(block, data, nsteps):
    for k, it in data.items():
        if k not in block:
            block[k] = np.zeros((*it.shape,), dtype=it.dtype)
        block[k] += it / nsteps


def sample_overlap_worker(wfs, configs, tstep, nsteps, energy):
    r"""``nsteps`` Metropolis sweeps with the distribution :math:`\propto \sum_i |\Psi_i|^2` (sample_many.py:137-195).
    Returns (weighted block, unweighted block, configs)."""
    _no_energy(energy)
    for wf in wfs:
        wf.recompute(configs)
    weighted_block = {}
    unweighted_block = {"acceptance": 0.0}
    nconf, nelec = configs.configs.shape[:2]
    for n in range(nsteps):
        for e in range(nelec):
            grads = [np.real(wf.gradient(e, configs.electron(e)).T) for wf in wfs]
            grad = limdrift(np.mean(grads, axis=0))
            gauss = np.random.normal(scale=np.sqrt(tstep), size=(nconf, 3))
            newcoorde = configs.configs[:, e, :] + gauss + grad * tstep
            newcoorde = configs.make_irreducible(e, newcoorde)
            grads, vals, saved_values = list(zip(*[wf.gradient_value(e, newcoorde) for wf in wfs]))
            grads = [np.real(g.T) for g in grads]
            new_grad = limdrift(np.mean(grads, axis=0))
            forward = np.sum(gauss**2, axis=1)
            backward = np.sum((gauss + tstep * (grad + new_grad)) ** 2, axis=1)
            t_prob = np.exp(1 / (2 * tstep) * (forward - backward))
            wf_ratios = np.abs(vals) ** 2
            log_values = np.real(np.array([wf.value()[1] for wf in wfs]))
            weights = np.exp(2 * (log_values - log_values[0]))
            ratio = t_prob * np.sum(wf_ratios * weights, axis=0) / weights.sum(axis=0)
            accept = ratio > np.random.rand(nconf)
            configs.move(e, newcoorde, accept)
            for wf, saved in zip(wfs, saved_values):
                wf.updateinternals(e, newcoorde, configs, mask=accept, saved_values=saved)
        weights = compute_weights(wfs)
        rolling_average(unweighted_block, {"overlap": np.mean(weights, axis=-1)}, nsteps)
    return weighted_block, unweighted_block, configs


def sample_overlap(wfs, configs, energy, nsteps=10, nblocks=10, tstep=0.5, hdf_file=None, client=None, npartitions=None):
    """``nblocks`` blocks of ``sample_overlap_worker`` (sample_many.py:80-105, :205-223) -> (weighted, unweighted, configs), the
    block dictionaries inverted to ``{quantity: array over blocks}``.  No block file and no parallel client here."""
    _no_energy(energy)
    if client is not None or npartitions is not None:
        raise NotImplementedError("pyqmc_amd.sample_overlap runs on one device: client / npartitions must be None")
    if hdf_file is not None:
        raise NotImplementedError("pyqmc_amd.sample_overlap writes no block file: hdf_file must be None")
    weighted, unweighted = [], []
    for _ in range(nblocks):
        w, u, configs = sample_overlap_worker(wfs, configs, tstep, nsteps, energy)
        weighted.append(w)
        unweighted.append(u)
    return invert_list_of_dicts(weighted), invert_list_of_dicts(unweighted), configs
