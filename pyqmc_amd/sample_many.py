"""Sampling the mixture of several wave functions — ``pyqmc/method/sample_many.py``.

``sample_overlap_worker`` moves the walkers by Metropolis with the distribution proportional to ``sum_i |Psi_i|^2`` over the
wave functions ``wfs`` (deep copies of one device wave function, each on a handle of its own).  Two routes give the same walk:

* ``"fused"``: ``pqa_overlap_sweeps`` runs the sweeps of all K handles on the device (real Slater x two-body Jastrow handles, any
  number of determinants, open boundaries, one device, distinct handles, K <= 8);
* ``"protocol"``: the reference's loop over the protocol entry points (``gradient``, ``gradient_value``, ``value``,
  ``updateinternals`` with ``saved_values``) for everything else.

Both draw ``np.random.normal`` and ``np.random.rand`` in the reference's order, so seeded runs agree and a test can replay the draws.
``energy`` is a multiple-wave-function accumulator (``avg(configs, wfs, weights)``, e.g. ``EnergyAccumulatorMultipleWF``) or None;
the route the last worker call took is in ``last_route``.

A multi-state accumulator on its device route (``resolve_route(wfs) == "device"``: ``StochasticReconfigurationMultipleWF``, and on
request ``StochasticReconfigurationWfbyWf`` and ``EnergyAccumulatorMultipleWF``) is evaluated on the resident walkers through its
``avg_resident(wfs)`` (``mix_moments`` / ``mix_wtdp`` below: ``pqa_mix_moments`` / ``pqa_mix_wtdp``): the fused worker then fetches
neither the walkers nor the weights between sweeps.
"""

import ctypes as C

import numpy as np

from . import _ffi

last_route = None  # "fused" or "protocol": the route of the last sample_overlap_worker call


def limdrift(g, cutoff=1):
    """``mc.limdrift`` (mc.py:76-89): each row of ``g`` (nconf, 3) shortened to at most ``cutoff``."""
    tot = np.linalg.norm(g, axis=1)
    mask = tot > cutoff
    g[mask, :] = cutoff * g[mask, :] / tot[mask, np.newaxis]
    return g


def _check_energy(energy):
    if energy is not None and not getattr(energy, "multiple_wf", False):
        raise NotImplementedError("sample_overlap needs an accumulator over several wave functions (avg(configs, wfs, weights)): wrap "
                                  "a single-wave-function accumulator in EnergyAccumulatorMultipleWF or AdaptSingleAccumulator")


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


def component_devices(wfs, noun):
    """``(handles, None)``, or ``(None, reason)`` at the first member of ``wfs`` that is not a real Slater x two-body Jastrow product on
    one handle with open boundaries; ``noun`` is the caller's word for a member ("wave function", ``AddWF.scope``: "component")."""
    devs = []
    for i, wf in enumerate(wfs):
        d = wf._product_device() if hasattr(wf, "_product_device") else None
        if d is None:
            return None, f"{noun} {i} is not a real Slater x two-body Jastrow product on one device handle"
        if d.pbc or getattr(d, "twisted", False):
            return None, f"{noun} {i} is periodic"
        devs.append(d)
    return devs, None


def handle_array(devs):
    return (C.c_void_p * len(devs))(*[d._h.value for d in devs])


def finish(devs, rc, moved=False):
    """The tail of a multi-handle wrapper; ``moved``: the call moved walkers or ran the handles' energy passes."""
    for d in devs if moved else ():
        d._zero = [None, None]  # (the determinants changed)
    _ffi.check(devs[0]._h, rc)


def fused_scope(wfs, configs=None):
    """``(handles, None)`` when the multi-handle device calls (``pqa_overlap_sweeps``, ``pqa_mix_moments``) can take ``wfs``, else
    ``(None, reason)``; see the module docstring.  ``configs`` None: the walkers are the resident ones, only the handles are looked at."""
    if len(wfs) < 1 or len(wfs) > 8:
        return None, f"{len(wfs)} wave functions (the device calls take 1 to 8)"
    if configs is not None and (hasattr(configs, "wrap") or np.ndim(configs.configs) != 3):
        return None, "periodic walkers"
    devs, why = component_devices(wfs, "wave function")
    if devs is None:
        return None, why
    if len({id(d) for d in devs}) != len(devs):
        return None, "two wave functions share a device handle"
    if len({d.device for d in devs}) != 1:
        return None, "the handles are on different devices"
    return devs, None


def fused_handles(wfs, configs=None):
    """The device handles of ``wfs`` when the fused route can take them, else None (``fused_scope`` without the reason)."""
    return fused_scope(wfs, configs)[0]


def _route(wfs, configs, route):
    if route not in (None, "fused", "protocol"):
        raise ValueError(f"route must be None, 'fused' or 'protocol', not {route!r}")
    devs = None if route == "protocol" else fused_handles(wfs, configs)
    if route == "fused" and devs is None:
        raise ValueError("route='fused' needs real Slater x two-body Jastrow wave functions on distinct handles of one device, open "
                         "boundaries and at most 8 wave functions")
    return devs


def overlap_sweeps(devs, tstep, gauss, unif, weights=False):
    """``pqa_overlap_sweeps`` on the handles ``devs`` with the tapes gauss (nsteps*N, W, 3) and unif (nsteps*N, W) -> (overlap
    (nsteps, K, K), weights (K, K, W) of the last sweep or None, acceptance)."""
    K, W, N = len(devs), devs[0].W, devs[0].N
    nsteps = gauss.shape[0] // N
    gauss, unif = _ffi.f64(gauss), _ffi.f64(unif)
    ovl = np.empty((nsteps, K, K))
    wts = np.empty((K, K, W)) if weights else None
    acc = C.c_double()
    rc = _ffi.lib().pqa_overlap_sweeps(handle_array(devs), K, float(tstep), int(nsteps), _ffi.ptr(gauss), _ffi.ptr(unif), _ffi.ptr(ovl),
                                       None if wts is None else _ffi.ptr(wts), C.byref(acc))
    finish(devs, rc, moved=True)
    return ovl, wts, acc.value


def mix_moments(devs, columns, offset=0.0, threshold=10.0, rot=None, unif=None, seeds=None, walker_chunk=0, per_walker=False):
    """``pqa_mix_moments`` on the handles ``devs`` (which hold the same walkers).  ``columns``: per state ``(src, pos)`` as
    ``accumulators.sr_columns`` gives them (empty: the state has no columns).  ``seeds`` (K) keys each handle's energy draws, or
    ``rot`` / ``unif`` (K sets as ``DeviceWF.energy`` takes them) replay them.  Returns (overlap (K, K), en (6, K, K), moments: per
    state None or (P_i + 2K, P_i) with the rows dpipj (P_i), dp[:, j] (K), dpH[:, j] (K)[, u (K, W), en_walker (K, W, 6) with
    ``per_walker``])."""
    K, W = len(devs), devs[0].W
    if len(columns) != K:
        raise ValueError(f"{K} column descriptions expected, got {len(columns)}")
    cols = [(np.ascontiguousarray(s, dtype=np.int32).ravel(), np.ascontiguousarray(p, dtype=np.int32).ravel()) for s, p in columns]
    if any(len(s) != len(p) for s, p in cols):
        raise ValueError("src and pos of a state must be equally long")
    P = np.array([len(s) for s, _ in cols], dtype=np.int32)
    src, pos = np.concatenate([s for s, _ in cols]), np.concatenate([p for _, p in cols])
    rot = None if rot is None else _ffi.f64(rot)
    unif = None if unif is None else _ffi.f64(unif)
    seeds = np.zeros(K, dtype=np.uint64) if seeds is None else np.ascontiguousarray(seeds, dtype=np.uint64)
    if seeds.shape != (K,):
        raise ValueError(f"seeds ({K},) expected, got {seeds.shape}")
    overlap, en = np.empty((K, K)), np.empty((6, K, K))
    sizes = [(int(p) + 2 * K) * int(p) for p in P]
    moments = np.empty(max(sum(sizes), 1))
    u = np.empty((K, W)) if per_walker else None
    enw = np.empty((K, W, 6)) if per_walker else None
    rc = _ffi.lib().pqa_mix_moments(handle_array(devs), K, _ffi.ptr(P), _ffi.ptr(src), _ffi.ptr(pos), float(offset), float(threshold),
                                    _ffi.ptr(rot), _ffi.ptr(unif), _ffi.ptr(seeds), int(walker_chunk), _ffi.ptr(overlap), _ffi.ptr(en),
                                    _ffi.ptr(moments), _ffi.ptr(u), _ffi.ptr(enw))
    finish(devs, rc)
    offs = np.concatenate(([0], np.cumsum(sizes)))
    mom = [moments[offs[i]:offs[i + 1]].reshape(int(P[i]) + 2 * K, int(P[i])) if P[i] else None for i in range(K)]
    return (overlap, en, mom, u, enw) if per_walker else (overlap, en, mom)


def mix_wtdp(devs, src, pos, walker_chunk=0):
    """``pqa_mix_wtdp`` on the handles ``devs``: (overlap (K, K), wtdp (K, K, P)) with the derivative columns ``(src, pos)`` of the LAST
    state; ``wtdp[j, k]`` and ``wtdp[k, j]`` are equal bits."""
    K = len(devs)
    src, pos = np.ascontiguousarray(src, dtype=np.int32).ravel(), np.ascontiguousarray(pos, dtype=np.int32).ravel()
    if len(src) != len(pos):
        raise ValueError("src and pos must be equally long")
    overlap, wtdp = np.empty((K, K)), np.empty((K, K, len(src)))
    rc = _ffi.lib().pqa_mix_wtdp(handle_array(devs), K, len(src), _ffi.ptr(src), _ffi.ptr(pos), int(walker_chunk), _ffi.ptr(overlap),
                                 _ffi.ptr(wtdp))
    finish(devs, rc)
    return overlap, wtdp


def _resident(energy, wfs):
    """True when ``energy`` takes its averages from the walkers resident behind ``wfs`` (``avg_resident``) for this call."""
    return hasattr(energy, "avg_resident") and energy.resolve_route(wfs) == "device"


def _worker_fused(devs, wfs, configs, tstep, nsteps, energy):
    for wf in wfs:
        wf.recompute(configs)
        wf.wf_factors[0]._saved = None
    weighted_block = {}
    unweighted_block = {"acceptance": 0.0}
    nconf, nelec = configs.configs.shape[:2]
    per_call = 1 if energy is not None else nsteps  # an accumulator may draw from np.random between sweeps: tapes per sweep then
    for n0 in range(0, nsteps, max(per_call, 1)):
        m = min(per_call, nsteps - n0)
        gauss, unif = np.empty((m * nelec, nconf, 3)), np.empty((m * nelec, nconf))
        for i in range(m * nelec):
            gauss[i] = np.random.normal(scale=np.sqrt(tstep), size=(nconf, 3))
            unif[i] = np.random.rand(nconf)
        resident = energy is not None and _resident(energy, wfs)  # (the walkers and the weights stay on the device then)
        overlap, weights, _ = overlap_sweeps(devs, tstep, gauss, unif, weights=energy is not None and not resident)
        if energy is not None and not resident:
            configs.configs[...] = devs[0].configs()
        for j in range(m):
            rolling_average(unweighted_block, {"overlap": overlap[j]}, nsteps)
            if resident:
                rolling_average(weighted_block, energy.avg_resident(wfs), nsteps)
            elif energy is not None:
                rolling_average(weighted_block, energy.avg(configs, wfs, weights), nsteps)
    configs.configs[...] = devs[0].configs()
    return weighted_block, unweighted_block, configs


def _worker_protocol(wfs, configs, tstep, nsteps, energy):
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
        if energy is not None:
            rolling_average(weighted_block, energy.avg(configs, wfs, weights), nsteps)
    return weighted_block, unweighted_block, configs


def sample_overlap_worker(wfs, configs, tstep, nsteps, energy, route=None):
    r"""``nsteps`` Metropolis sweeps with the distribution :math:`\propto \sum_i |\Psi_i|^2` (sample_many.py:130-186).
    Returns (weighted block, unweighted block, configs).  ``route``: None (fused when every handle is eligible), "fused" (an error
    if one is not) or "protocol"."""
    global last_route
    _check_energy(energy)
    devs = _route(wfs, configs, route)
    last_route = "protocol" if devs is None else "fused"
    if devs is None:
        return _worker_protocol(wfs, configs, tstep, nsteps, energy)
    return _worker_fused(devs, wfs, configs, tstep, nsteps, energy)


def hdf_save(hdf_file, weighted, unweighted, attr, configs):
    """sample_many.py:27-39 through ``BlockFile``: one record per block, its datasets in the groups ``weighted`` and ``unweighted``
    (``weighted/total``, ``unweighted/overlap``, ...), the walkers overwritten."""
    if hdf_file is not None:
        from .blockfile import BlockFile

        rec = {f"{label}/{k}": v for label, data in (("weighted", weighted), ("unweighted", unweighted)) for k, v in data.items()}
        BlockFile(hdf_file).append(rec, attr, configs)


def sample_overlap(wfs, configs, energy, nsteps=10, nblocks=10, tstep=0.5, hdf_file=None, client=None, npartitions=None, route=None):
    """``nblocks`` blocks of ``sample_overlap_worker`` (sample_many.py:63-88, :189-213) -> (weighted, unweighted, configs), the
    block dictionaries inverted to ``{quantity: array over blocks}``.  ``hdf_file``: every block appended through ``BlockFile``; an
    existing file gives the starting walkers (the reference's restart).  No parallel client here."""
    _check_energy(energy)
    if client is not None or npartitions is not None:
        raise NotImplementedError("pyqmc_amd.sample_overlap runs on one device: client / npartitions must be None")
    if hdf_file is not None:
        from .blockfile import BlockFile

        store = BlockFile(hdf_file)
        if store.exists():
            store.load_walkers(configs)
    weighted, unweighted = [], []
    for _ in range(nblocks):
        w, u, configs = sample_overlap_worker(wfs, configs, tstep, nsteps, energy, route=route)
        weighted.append(w)
        unweighted.append(u)
        hdf_save(hdf_file, w, u, dict(tstep=tstep), configs)
    return invert_list_of_dicts(weighted), invert_list_of_dicts(unweighted), configs


def normalize(weighted, unweighted):
    """Averages and standard errors over blocks (sample_many.py:216-235): the unweighted quantities as they are, the weighted ones
    divided by sqrt(N_i N_j) with N the diagonal of the mean overlap."""
    import scipy.stats

    avg, error = {}, {}
    for k, it in unweighted.items():
        avg[k] = np.mean(it, axis=0)
        error[k] = scipy.stats.sem(it, axis=0)
    N = np.abs(avg["overlap"].diagonal())
    Nij = np.sqrt(np.outer(N, N))
    for k, it in weighted.items():
        avg[k] = np.mean(it, axis=0) / Nij
        error[k] = scipy.stats.sem(it, axis=0) / Nij
    return avg, error
