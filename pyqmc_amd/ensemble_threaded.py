"""Excited states by penalised ensemble optimisation, all states at once — ``pyqmc/method/ensemble_optimization_threaded.py``.

Where ``ensemble.optimize_ensemble`` optimises the states one after the other (Gauss-Seidel: state ``i`` sees the updated states before
it), this driver takes every state's gradient from the SAME parameters and applies all updates afterwards (Jacobi).  One iteration:
one mixture sampling of all states for the normalisation, then per (state, sub-iteration) a VMC run of the state with the single-state
SR accumulator (``transform.onewf()``) and a mixture sampling of the states ``0 .. wfi`` with ``transform.allwfs()``, each on a walker
set of its own that is carried from iteration to iteration, then the steps.  Names, arguments, defaults, data flow and the records are
the reference's; the optimisation file goes through ``BlockFile`` as in ``ensemble`` (parameters ``wf/<i>/<key>``, one record per
(state, sub-iteration) with ``energy{i}``, ``energy_error{i}``, ``overlap{i}``, ``iteration``, ``wavefunction``, ``sub_iteration``).

The reference submits the runs to a thread pool, each with a share of a parallel client's workers.  Here there is one device: the runs
follow one another in the reference's submission order (all VMC runs, then all mixture samplings), and ``client``, ``npartitions`` and
``overlap_thread_weight`` must be None.  This module is host code only; the device work is what the updaters' routes give it
(``StochasticReconfigurationWfbyWf(..., route=..., mixture_route=...)``).
"""

import copy

import numpy as np

from .ensemble import StochasticReconfigurationWfbyWf, _sample_overlap, _vmc, hdf_save, renormalize, set_wf_params  # noqa: F401


def round_to_fixed_sum(x, target_sum):
    """Integers close to ``x * target_sum / sum(x)`` that sum to ``target_sum`` before every entry below 1 is raised to 1
    (ensemble_optimization_threaded.py:33-70): floors, then one more for the largest fractional parts.  ``ValueError`` when no
    rounding reaches the sum (a total that is zero or not finite)."""
    x = np.asarray(x)
    with np.errstate(divide="ignore", invalid="ignore"):
        x = x * target_sum / np.sum(x)
    if not np.all(np.isfinite(x)):
        raise ValueError("Target sum is not achievable with integer rounding.")
    y = np.floor(x).astype(int)
    diff = target_sum - np.sum(y)
    if diff < 0 or diff > len(x):
        raise ValueError("Target sum is not achievable with integer rounding.")
    frac = x - y
    idx = np.argsort(frac)[::-1]
    y[idx[:diff]] += 1
    y[y < 1] = 1
    return y


def _one_device(client, npartitions, overlap_thread_weight, name):
    if client is not None or npartitions is not None or overlap_thread_weight is not None:
        raise NotImplementedError(f"pyqmc_amd.ensemble_threaded.{name} runs on one device: client / npartitions / overlap_thread_weight "
                                  "must be None")


def evaluate_gradients_threaded(wfs, configs_ensemble, updater, client=None, npartitions=None, vmc_kwargs=None, overlap_kwargs=None,
                                verbose=True, overlap_thread_weight=None):
    """The Monte Carlo runs every state's gradient needs (ensemble_optimization_threaded.py:73-234), one after another in the
    reference's submission order.  ``configs_ensemble[wfi][sub_iteration]`` is the pair of walker sets of the VMC run and of the
    mixture sampling; ``updater[wfi][sub_iteration]`` a ``StochasticReconfigurationWfbyWf``.  Returns (VMC blocks, weighted mixture
    blocks, unweighted mixture blocks, configs_ensemble), the first three indexed ``[wfi][sub_iteration]``.  (The reference's default
    ``npartitions=1`` belongs to its client; here None.)"""
    _one_device(client, npartitions, overlap_thread_weight, "evaluate_gradients_threaded")
    vmc_kwargs = {} if vmc_kwargs is None else vmc_kwargs
    overlap_kwargs = {} if overlap_kwargs is None else overlap_kwargs
    nwf = len(wfs)
    data_sample1_ensemble = [[0 for _ in range(len(updater[wfi]))] for wfi in range(nwf)]
    data_weighted_ensemble = [[0 for _ in range(len(updater[wfi]))] for wfi in range(nwf)]
    data_unweighted_ensemble = [[0 for _ in range(len(updater[wfi]))] for wfi in range(nwf)]
    for wfi, wf in enumerate(wfs):
        for sub_iteration, transform in enumerate(updater[wfi]):
            data_sample1_ensemble[wfi][sub_iteration], configs_ensemble[wfi][sub_iteration][0] = _vmc(
                wf, configs_ensemble[wfi][sub_iteration][0], accumulators={"": transform.onewf()}, **vmc_kwargs)
    for wfi in range(nwf):
        for sub_iteration, transform in enumerate(updater[wfi]):
            (data_weighted_ensemble[wfi][sub_iteration], data_unweighted_ensemble[wfi][sub_iteration],
             configs_ensemble[wfi][sub_iteration][1]) = _sample_overlap(
                wfs[0 : wfi + 1], configs_ensemble[wfi][sub_iteration][1], transform.allwfs(), **overlap_kwargs)
    return data_sample1_ensemble, data_weighted_ensemble, data_unweighted_ensemble, configs_ensemble


def optimize_ensemble(wfs, configs, updater, hdf_file, client=None, tau=1, max_iterations=100, overlap_penalty=None, npartitions=None,
                      verbose=True, overlap_thread_weight=None, warmup_kwargs=None, vmc_kwargs=None, overlap_kwargs=None):
    """Optimise the states ``wfs`` together (ensemble_optimization_threaded.py:237-370).  ``updater[wfi]`` is the list of
    ``StochasticReconfigurationWfbyWf`` objects of state ``wfi``'s sub-iterations.  Empty or missing keyword dictionaries take the
    reference's defaults (warm-up: 1 block of 100 steps; VMC: 10 blocks of 10 steps; mixture: 10 blocks of 10 steps).  An existing
    ``hdf_file`` restarts: parameters and walkers from the file, from iteration max(iteration) + 1, without the warm-up.  Returns
    ``wfs``."""
    _one_device(client, npartitions, overlap_thread_weight, "optimize_ensemble")
    if warmup_kwargs is None or len(warmup_kwargs) == 0:
        warmup_kwargs = dict(nblocks=1, nsteps_per_block=100)
    if vmc_kwargs is None or len(vmc_kwargs) == 0:
        vmc_kwargs = dict(nblocks=10, nsteps_per_block=10)
    if overlap_kwargs is None or len(overlap_kwargs) == 0:
        overlap_kwargs = dict(nblocks=10, nsteps=10)
    nwf = len(wfs)
    if overlap_penalty is None:
        overlap_penalty = np.ones((nwf, nwf)) * 0.5
    iteration_offset = 0
    store = None
    if hdf_file is not None:
        from .blockfile import BlockFile

        store = BlockFile(hdf_file)
    if store is not None and store.exists():  # restarting -- read in data
        params = store.load_parameters()
        for wfi, wf in enumerate(wfs):
            pre = f"{wfi}/"
            for k, v in params.items():
                if k.startswith(pre):
                    wf.parameters[k[len(pre):]] = np.asarray(v)
        ds = store.datasets()
        if "iteration" in ds:
            iteration_offset = np.max(ds["iteration"][...]) + 1
        store.load_walkers(configs)
    else:
        _, configs = _vmc(wfs[0], configs, **warmup_kwargs)

    configs_ensemble = [[[copy.deepcopy(configs) for _ in range(2)] for _ in range(len(updater[wfi]))] for wfi in range(nwf)]
    for i in range(iteration_offset, max_iterations):
        _, data_unweighted, configs = _sample_overlap(wfs, configs_ensemble[0][0][0], None, **overlap_kwargs)
        norm = np.mean(data_unweighted["overlap"], axis=0)
        if verbose:
            print("Normalization step", norm.diagonal())
        renormalize(wfs, norm.diagonal(), pivot=0)
        data_sample1_ensemble, data_weighted_ensemble, data_unweighted_ensemble, configs_ensemble = evaluate_gradients_threaded(
            wfs, configs_ensemble, updater, vmc_kwargs=vmc_kwargs, overlap_kwargs=overlap_kwargs, verbose=verbose)
        for wfi, wf in enumerate(wfs):
            for sub_iteration, transform in enumerate(updater[wfi]):
                avg, error = transform.block_average(data_sample1_ensemble[wfi][sub_iteration], data_weighted_ensemble[wfi][sub_iteration],
                                                     data_unweighted_ensemble[wfi][sub_iteration]["overlap"])
                if verbose:
                    print("Iteration", i, "wf ", wfi, " sub iteration ", sub_iteration, "Energy", avg["total"], "Overlap",
                          avg["overlap"][wfi, :])
                dp, report = transform.delta_p([tau], avg, overlap_penalty, verbose=verbose)
                x = transform.transform.serialize_parameters(wf.parameters)
                x = x + dp[0]
                set_wf_params(wf, x, transform)
                save_data = {
                    f"energy{wfi}": avg["total"],
                    f"energy_error{wfi}": error["total"],
                    f"overlap{wfi}": avg["overlap"],
                    "iteration": i,
                    "wavefunction": wfi,
                    "sub_iteration": sub_iteration,
                }
                hdf_save(hdf_file, save_data, {"tau": tau}, wfs, configs_ensemble[wfi][sub_iteration][0])
    return wfs
