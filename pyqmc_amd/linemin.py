"""Wave-function optimisation by line minimisation — ``pyqmc/method/linemin.py`` on this package's drivers.

Names, arguments, defaults and the returned ``(wf, df)`` are the reference's.  Each (sub-)iteration runs a gradient VMC
(``pyqmc_amd.vmc`` with ``{"pgrad": pgrad}``), takes the stochastic-reconfiguration direction (``pgrad.delta_p``) and picks the
step along it by correlated sampling: the walkers are drawn from the mixture of two wave functions on the line
(``sample_many.sample_overlap``) and every one of ``npts`` parameter sets is evaluated on them (``correlated_compute_worker``).

``correlated_compute_worker`` takes one of two routes and reports which in ``data["route"]``:

* ``"fused"`` — a real single-determinant Slater x two-body-Jastrow wave function on one device handle, whose optimised
  parameters are Jastrow coefficients only (``wf2acoeff`` / ``wf2bcoeff``), with the semi-local ECP integrator: ONE C call,
  ``pqa_correlated``, evaluates all sets on the resident walkers: the Slater part once, then per set only the contraction of
  basis-resolved Jastrow rows with its coefficients (csrc/pqa_correlated.hip);
  with ``evaluation_route="fused"`` also several determinants and ``wf1det_coeff`` among the parameters (real, untwisted, no
  three-body factor): ONE C call, ``pqa_correlated_md``, which adds the determinant sums of all sets as one matrix-core product
  per walker (``data["entry"]`` names the call that ran);
  with ``three_body_device=True`` (opt-in) also a real, untwisted Slater x two-body x three-body Jastrow wave function with any
  number of determinants and ``wf3ccoeff`` among the parameters: ONE C call, ``pqa_correlated_j3``, which builds the
  coefficient-independent three-body tables once per electron and ECP point and contracts them with every set's ``ccoeff``;
* ``"protocol"`` — anything else: per set, the parameters are set, the wave function recomputed and the energy accumulator
  run, as the reference does.  It is the default for several determinants; ``evaluation_route`` (``line_minimization``,
  ``correlated_sampling_minimum``, ``correlated_compute``, ``correlated_compute_worker``) selects a route by name.

One deliberate difference from the reference: both routes leave ``wf`` at its original parameters (the reference leaves it at
the last point of the line).  ``line_minimization`` sets the chosen parameters afterwards either way.

The optimisation file (``opt_hdf``) goes through ``pyqmc_amd.blockfile``: an HDF5 file where h5py exists, else the
``.npz`` pair, with the reference's layout — per-step datasets, the attributes, the walkers, and the ``wf/<key>`` parameters
overwritten every step.  A file that exists restarts the run (linemin.py:164-174).
"""

import copy
import logging

import numpy as np

from . import sample_many as sm
from .energy import EnergyAccumulator
from .wf import ThreeBodyJastrow, linear_det_jastrow_device, linear_j3_device, linear_jastrow_device


def opt_hdf(hdf_file, data, attr, configs, parameters):
    """Append one optimisation step to ``hdf_file`` (linemin.py:23-38)."""
    if hdf_file is None:
        return
    from .blockfile import BlockFile

    BlockFile(hdf_file).append(data, attr, configs, parameters={k: np.asarray(v) for k, v in parameters.items()})


def polyfit_relative(xfit, yfit, degree):
    p = np.polyfit(xfit, yfit, degree)
    ypred = np.polyval(p, xfit)
    resid = (ypred - yfit) ** 2
    relative_error = np.var(resid) / np.var(yfit)
    return p, relative_error


def stable_fit(xfit, yfit, tolerance=1e-2):
    """Minimum of a linear or quadratic fit of ``yfit`` over ``xfit`` (linemin.py:49-91): the lower end point when a line fits
    about as well, the vertex of a good convex quadratic, else the lowest sample; never above the lowest sample."""
    steprange = np.max(xfit)
    minstep = np.min(xfit)
    a = np.argmin(yfit)
    pq, relative_errq = polyfit_relative(xfit, yfit, 2)
    pl, relative_errl = polyfit_relative(xfit, yfit, 1)
    if relative_errl / relative_errq < 2:  # a linear fit is about as good
        est_min = steprange if pl[0] < 0 else minstep
        out_y = np.polyval(pl, est_min)
    elif relative_errq < tolerance and pq[0] > 0:  # the quadratic fit is good
        est_min = -pq[1] / (2 * pq[0])
        if est_min > steprange:
            est_min = steprange
        if est_min < minstep:
            est_min = minstep
        out_y = np.polyval(pq, est_min)
    else:
        est_min = xfit[a]
        out_y = yfit[a]
    if out_y > yfit[a]:
        est_min = xfit[a]
    return est_min


def find_minimum(xfit, yfit):
    """The ``xfit`` of the lowest ``yfit`` (linemin.py:94-100)."""
    return xfit[np.argmin(yfit)]


def _vmc(wf, coords, accumulators, options):
    from .vmc import vmc

    return vmc(wf, coords, accumulators=accumulators, **options)


def _no_client(client, npartitions):
    if client is not None or npartitions is not None:
        raise NotImplementedError("pyqmc_amd line minimisation runs on one device: client / npartitions must be None")


def line_minimization(wf, coords, pgrad_acc, steprange=0.2, max_iterations=30, warmup_options=None, correlated_reference_wfs=None,
                      stderr_weight=3.0, vmcoptions=None, lmoptions=None, correlatedoptions=None, update_kws=None, verbose=False, npts=40,
                      hdf_file=None, client=None, npartitions=None, correlated_sampling=True, evaluation_route=None,
                      three_body_device=False):
    """Optimise the energy by stochastic-reconfiguration directions and correlated-sampling line searches (linemin.py:103-260).
    ``pgrad_acc``: a ``StochasticReconfiguration`` (e.g. ``accumulators.gradient_generator``) or a list of them (sub-iterations).
    ``evaluation_route``: the route of the line points' evaluation (``correlated_route``; None: the default choice).
    ``three_body_device``: with True wave functions with a three-body Jastrow factor take the fused route (``correlated_route``).
    Returns (wf, list of per-step dictionaries)."""
    _no_client(client, npartitions)
    three_body_device = _flag("three_body_device", three_body_device)
    from .blockfile import BlockFile

    vmcoptions = {} if vmcoptions is None else vmcoptions
    vmcoptions.update({"verbose": verbose})
    if correlatedoptions is None:
        correlatedoptions = dict(nsteps=3, nblocks=1)
    if warmup_options is None:
        warmup_options = dict(nblocks=1, nsteps_per_block=100)
    if "tstep" not in warmup_options and "tstep" in vmcoptions:
        warmup_options["tstep"] = vmcoptions["tstep"]
    assert npts >= 3, f"linemin npts={npts}; need npts >= 3 for correlated sampling"
    if correlated_reference_wfs is None:
        correlated_reference_wfs = [0, 1]

    iteration_offset = 0
    sub_iteration_offset = 0
    store = None if hdf_file is None else BlockFile(hdf_file)
    if store is not None and store.exists():  # restarting (linemin.py:164-174)
        for k, v in store.load_parameters().items():
            wf.parameters[k] = v
        ds = store.datasets()
        if "iteration" in ds:
            iteration_offset = int(np.max(ds["iteration"]))
        if "sub_iteration" in ds:
            sub_iteration_offset = int(ds["sub_iteration"][-1]) + 1
        store.load_walkers(coords)
    else:
        if verbose:
            print("starting warmup")
        _, coords = _vmc(wf, coords, {}, warmup_options)
        if verbose:
            print("finished warmup", flush=True)
    if iteration_offset >= max_iterations:
        logging.warning(f"iteration_offset {iteration_offset} >= max_iterations {max_iterations}; no steps will be run.")

    attr = dict(max_iterations=max_iterations, npts=npts, steprange=steprange, correlated_reference_wfs=correlated_reference_wfs)
    try:
        sub_iterations = len(pgrad_acc)
    except TypeError:
        if verbose:
            print("Was passed a single PGradAccumulator; using 1 sub_iteration. This is deprecated behavior.")
        sub_iterations = 1
        pgrad_acc = [pgrad_acc]

    df = []
    for it in range(iteration_offset, max_iterations):
        for sub_it in range(sub_iteration_offset, sub_iterations):
            if verbose:
                print("#############################\nStarting iteration", it, "sub iteration", sub_it)
            pgrad = pgrad_acc[sub_it]
            x0 = pgrad.transform.serialize_parameters(wf.parameters)
            df_vmc, coords = _vmc(wf, coords, {"pgrad": pgrad}, vmcoptions)
            data = {k: np.mean(df_vmc["pgrad" + k], axis=0) for k in pgrad.keys()}
            data["total_err"] = np.std(df_vmc["pgradtotal"], axis=0) / np.sqrt(df_vmc["pgradtotal"].shape[0])
            if np.isnan(df_vmc["pgradtotal"]).any():
                raise ValueError("NaN in optimization. Try reducing the step size or increasing stabilization.")
            if verbose:
                print("Current energy", data["total"], data["total_err"])
            step_data = {"energy": data["total"].real, "energy_error": data["total_err"].real, "iteration": it, "sub_iteration": sub_it,
                         "nconfig": coords.configs.shape[0]}
            if correlated_sampling:
                x0, min_data = correlated_sampling_minimum(steprange, npts, stderr_weight, correlated_reference_wfs, pgrad, wf, data, x0,
                                                           coords, client, npartitions, evaluation_route=evaluation_route,
                                                           three_body_device=three_body_device, **correlatedoptions)
                step_data.update(min_data)
                if verbose:
                    print("Moved", step_data["est_min"])
            else:
                x0, min_data = sr_step(steprange, pgrad, data, x0)
                step_data.update(min_data)
            set_wf_params(wf, x0, pgrad)
            opt_hdf(hdf_file, step_data, attr, coords, wf.parameters)
            df.append(step_data)
        sub_iteration_offset = 0
    return wf, df


def sr_step(steprange, pgrad, data, x0):
    """One stochastic-reconfiguration step of length ``steprange`` (linemin.py:263-276)."""
    xs, update_report = pgrad.delta_p([steprange], data, verbose=False)
    return xs[0] + x0, update_report


def correlated_sampling_minimum(steprange, npts, stderr_weight, correlated_reference_wfs, pgrad, wf, data, x0, coords, client, npartitions,
                                evaluation_route=None, three_body_device=False, **correlatedoptions):
    """Step along the SR direction that minimises ``mean energy + stderr_weight * spread`` over ``npts`` points of
    ``np.linspace(-steprange / (npts - 2), steprange, npts)`` (linemin.py:280-328).  ``correlatedoptions``: ``nsteps`` / ``nblocks``
    / ``tstep`` of the mixture sampling (the reference accepts them and drops them, sampling 10 blocks x 10 sweeps);
    ``evaluation_route`` and ``three_body_device`` go to ``correlated_compute_worker``, not into the sampling's options."""
    three_body_device = _flag("three_body_device", three_body_device)
    steps = np.linspace(-steprange / (npts - 2), steprange, npts)
    dps, update_report = pgrad.delta_p(steps, data, verbose=False)
    params = [x0 + dp for dp in dps]
    correlated_data = correlated_compute(wf, coords, params, pgrad, client=client, npartitions=npartitions, ref_wfs=correlated_reference_wfs,
                                         evaluation_route=evaluation_route, three_body_device=three_body_device, **correlatedoptions)
    w = correlated_data["weight"].copy()
    w = w / np.mean(w, axis=1, keepdims=True)
    en = np.real(np.mean(correlated_data["total"] * w, axis=1))
    en_std = np.std(correlated_data["total"], axis=1)
    yfit = en + stderr_weight * en_std
    est_min = find_minimum(steps, yfit)
    x0 = pgrad.delta_p([est_min], data, verbose=False)[0][0] + x0
    update_report["tau"] = steps
    update_report["yfit"] = yfit
    update_report["est_min"] = est_min
    update_report["correlated_energy"] = en
    update_report["correlated_energy_std"] = en_std
    return x0, update_report


def correlated_compute(wf, configs, params, pgrad_acc, client=None, npartitions=None, ref_wfs=None, evaluation_route=None,
                       three_body_device=False, **kws):
    """Walkers drawn from the mixture of the ``ref_wfs`` parameter sets (deep copies of ``wf``), then every set of ``params``
    evaluated on them (linemin.py:331-375).  ``kws``: ``nsteps`` / ``nblocks`` / ``tstep`` of ``sample_many.sample_overlap``."""
    _no_client(client, npartitions)
    three_body_device = _flag("three_body_device", three_body_device)
    if ref_wfs is None:
        ref_wfs = [0, 1]
    wfs = [copy.deepcopy(wf) for i in ref_wfs]
    for i in ref_wfs:
        set_wf_params(wfs[i], params[i], pgrad_acc)
    _, _, configs = sm.sample_overlap(wfs, configs, None, **kws)
    del wfs  # (their device handles)
    return correlated_compute_worker(wf, configs, params, pgrad_acc, ref_wfs, evaluation_route=evaluation_route,
                                     three_body_device=three_body_device)


def _flag(name, value):
    """The opt-in flag ``name`` as a bool; anything but True or False is refused (as the density-matrix accumulators' flags)."""
    if not isinstance(value, (bool, np.bool_)):
        raise ValueError(f"{name} must be True or False")
    return bool(value)


def _has_three_body(wf):
    dev = wf.fused_device() if hasattr(wf, "fused_device") else None
    return any(type(f) is ThreeBodyJastrow for f in getattr(wf, "wf_factors", ())) or bool(getattr(dev, "has_j3", False))


def correlated_route(wf, pgrad_acc, route=None, three_body_device=False):
    """The route ``correlated_compute_worker`` takes.  ``route=None``: ``"fused"`` when ``pqa_correlated`` covers this wave function,
    accumulator and parameter selection, else ``"protocol"``.  ``route="fused"``: ``"fused"`` also where only ``pqa_correlated_md``
    covers them (several determinants, ``wf1det_coeff`` among the parameters); ``NotImplementedError`` with the reason where neither
    does.  ``route="protocol"``: ``"protocol"``.  ``three_body_device=True`` (opt-in) changes the outcome for wave functions with
    a three-body Jastrow factor alone: where ``pqa_correlated_j3`` covers them (``wf.linear_j3_device``, a plain
    ``EnergyAccumulator`` with the semi-local ECP integrator) ``"fused"`` for ``route=None`` and ``route="fused"``, whatever the
    determinant count; elsewhere ``"protocol"`` for ``route=None`` and ``NotImplementedError`` with the reason for ``"fused"``."""
    if route not in (None, "fused", "protocol"):
        raise ValueError(f"evaluation route {route!r}: None, 'fused' or 'protocol' expected")
    three_body_device = _flag("three_body_device", three_body_device)
    if route == "protocol":
        return "protocol"
    enacc = getattr(pgrad_acc, "enacc", None)
    plain = type(enacc) is EnergyAccumulator and enacc.use_old_ecp
    # the entry asked of, and the parameters it has to cover (the default route asks pqa_correlated about every parameter listed)
    if three_body_device and _has_three_body(wf):
        device, keys = linear_j3_device, _opt_keys
    elif route is None:
        device, keys = (lambda wf, keys, why: linear_jastrow_device(wf, keys)), (lambda pgrad_acc: pgrad_acc.transform.to_opt)
    else:
        device, keys = linear_det_jastrow_device, _opt_keys
    why = []
    if not plain:
        why.append("the energy accumulator is not an EnergyAccumulator with the semi-local ECP integrator (use_old_ecp=True)")
    elif device(wf, keys(pgrad_acc), why) is not None:
        return "fused"
    if route is None:
        return "protocol"
    raise NotImplementedError(f"evaluation_route='fused': {why[0]}; use the set-recompute-energy route (evaluation_route='protocol')")


def _opt_keys(pgrad_acc):
    """The parameters with at least one optimised entry."""
    return {k for k, v in pgrad_acc.transform.to_opt.items() if np.any(v)}


def _weights(psi, ref_wfs):
    ref = np.amax(psi, axis=0)
    psirel = np.exp(2 * (psi - ref))
    rho = np.mean([psirel[i] for i in ref_wfs], axis=0)
    return psirel / rho


def correlated_compute_worker(wf, configs, params, pgrad_acc, ref_wfs, evaluation_route=None, three_body_device=False):
    """Energies and log values of ``wf`` at every parameter set of ``params`` on the same walkers, with the same random draws for
    every set (linemin.py:378-409).  Returns ``{energy key: (nsets, nconf)}``, ``weight`` (nsets, nconf) relative to the mixture
    of the ``ref_wfs`` sets, ``route`` and, on the fused route, ``entry`` (the C call).  ``wf`` keeps its parameters; its device
    state is that of ``configs``.  ``evaluation_route``, ``three_body_device``: see ``correlated_route``."""
    route = correlated_route(wf, pgrad_acc, evaluation_route, three_body_device)
    if route == "fused":
        return _correlated_fused(wf, configs, params, pgrad_acc, ref_wfs)
    x_orig = pgrad_acc.transform.serialize_parameters(wf.parameters)
    data = []
    current_state = np.random.get_state()
    calls = getattr(pgrad_acc.enacc, "_calls", None)  # (an EnergyAccumulator with an explicit seed keys its draws by its call count)
    psi = np.zeros((len(params), len(configs.configs)))
    for i, p in enumerate(params):
        np.random.set_state(current_state)
        if calls is not None:
            pgrad_acc.enacc._calls = calls
        set_wf_params(wf, p, pgrad_acc)
        psi[i] = wf.recompute(configs)[1]
        data.append(pgrad_acc.enacc(configs, wf))
    state_after = np.random.get_state()
    set_wf_params(wf, x_orig, pgrad_acc)
    wf.recompute(configs)
    np.random.set_state(state_after)
    data_ret = sm.invert_list_of_dicts(data)
    data_ret["weight"] = _weights(psi, ref_wfs)
    data_ret["route"] = "protocol"
    return data_ret


# The coefficient arrays of the fused entries: (parameter key, factor index, parameter name, argument name of DeviceWF.correlated*).
# pqa_correlated takes the two-body rows, pqa_correlated_md those and det_coeff, pqa_correlated_j3 all four.
_CORRELATED_SETS = (("wf1det_coeff", 0, "det_coeff", "det_coeff"), ("wf2acoeff", 1, "acoeff", "acoeff"), ("wf2bcoeff", 1, "bcoeff", "bcoeff"),
                    ("wf3ccoeff", 2, "ccoeff", "ccoeff"))


def _correlated_fused(wf, configs, params, pgrad_acc, ref_wfs):
    from .energy import KEYS

    tr, enacc = pgrad_acc.transform, pgrad_acc.enacc
    dev = wf.fused_device()
    wf.recompute(configs)  # (at the current parameters: the state every set shares)
    sets = [tr.deserialize(wf, p) for p in params]
    enacc.bind(dev)
    enacc._calls += 1
    # the draws one accumulator call makes (EnergyAccumulator.__call__), shared by every set as the reference's reset gives them
    key = int(np.random.randint(0, 2**31 - 1)) if enacc.seed is None else enacc.seed + enacc._calls
    if dev.has_j3:  # (correlated_route admits a three-body handle with three_body_device=True alone)
        entry, rows = "pqa_correlated_j3", _CORRELATED_SETS
    elif dev.ndet > 1 or "wf1det_coeff" in _opt_keys(pgrad_acc):
        entry, rows = "pqa_correlated_md", _CORRELATED_SETS[:3]
    else:
        entry, rows = "pqa_correlated", _CORRELATED_SETS[1:3]
    arrays = {arg: np.stack([s.get(pkey, wf.wf_factors[i].parameters[name]) for s in sets]) for pkey, i, name, arg in rows}
    psi, en = getattr(dev, entry[len("pqa_"):])(**arrays, threshold=enacc.threshold, seed=key)
    data_ret = {k: en[:, i, :] for i, k in enumerate(KEYS)}
    data_ret["weight"] = _weights(psi, ref_wfs)
    data_ret["route"] = "fused"
    data_ret["entry"] = entry
    return data_ret


def set_wf_params(wf, params, pgrad_acc):
    """Serialised parameters -> ``wf.parameters`` (linemin.py:412-415)."""
    newparms = pgrad_acc.transform.deserialize(wf, params)
    for k in newparms:
        wf.parameters[k] = newparms[k]
