"""Excited states by penalised ensemble optimisation — ``pyqmc/method/ensemble_optimization_wfbywf.py``.

The wave functions are optimised one after the other.  For state ``wfi`` a sub-iteration samples the mixture of all states
(``sample_many.sample_overlap``: the fused device route when the handles allow it), renormalises the states to state 0, runs VMC on
state ``wfi`` with the single-state SR accumulator (``transform.onewf()``), samples the mixture of states ``0 .. wfi`` again with
``transform.allwfs()`` (the overlap derivatives), and takes one SR step on energy + ``overlap_penalty`` x overlap.  Names, arguments,
defaults and the arithmetic are the reference's.  The optimisation file goes through ``BlockFile``: parameters ``wf/<i>/<key>``,
overwritten every step, and one record per step (``energy{i}``, ``energy_error{i}``, ``overlap{i}``, ``iteration``, ``wavefunction``,
``sub_iteration``).  ``client`` / ``npartitions`` are refused (one device); the reference's threaded variant is ``ensemble_threaded``.
"""

import numpy as np
import scipy.stats

from . import sample_many
from .accumulators import StochasticReconfiguration, resolve_mix_route, sr_columns


def _nparams(transform):
    n = transform.nparams
    return n() if callable(n) else n


class StochasticReconfigurationWfbyWf:
    """An accumulator over the mixture with a method that turns the block averages into a parameter step
    (ensemble_optimization_wfbywf.py:25-170).

    ``onewf()`` is the reference's ``StochasticReconfiguration(enacc, transform, eps)``: the third positional argument there is
    ``nodal_cutoff``, so ``eps`` sets the nodal cut-off of the single-state accumulator (and its regularisation keeps its default).
    This is restated as it is.

    ``mixture_route``: where ``allwfs().avg`` forms ``wtdp``.  None (default) or "protocol": the host ``einsum`` over
    ``wf.pgradient()`` of the last state and the (K, K, W) weights.  "device": ``pqa_mix_wtdp`` on the resident state,
    ``NotImplementedError`` with ``mix_route``'s reason when out of its scope; ``avg_resident(wfs)`` is ``avg`` without a host
    container then.  ``last_route`` records what the last mixture evaluation took."""

    multiple_wf = True

    def __init__(self, enacc, transform, eps=1e-3, route=None, mixture_route=None):
        if mixture_route not in (None, "device", "protocol"):
            raise ValueError(f"mixture_route must be None, 'device' or 'protocol', got {mixture_route!r}")
        self.enacc = enacc
        self.transform = transform
        self.eps = eps
        self._onewf = StochasticReconfiguration(enacc, transform, eps, route=route)  # route: of the single-state accumulator's avg
        self.mixture_route, self.last_route = mixture_route, None

    def onewf(self):
        return self._onewf

    def allwfs(self):
        return self

    def resolve_route(self, wfs):
        """The route ``avg`` takes for ``wfs``: "device" only when asked for (see ``mixture_route``)."""
        return resolve_mix_route(self, wfs, self.mixture_route or "protocol", "StochasticReconfigurationWfbyWf")

    def avg_resident(self, wfs):
        """``avg`` on the device route for the walkers resident behind ``wfs``: one ``pqa_mix_wtdp`` call."""
        devs, why = sample_many.fused_scope(wfs)
        if devs is None:
            raise NotImplementedError(f"StochasticReconfigurationWfbyWf.avg_resident: {why}")
        _, wtdp = sample_many.mix_wtdp(devs, *sr_columns(self.transform))
        self.last_route = "device"
        return {"wtdp": np.ascontiguousarray(np.moveaxis(wtdp, -1, 0))}

    def avg(self, configs, wfs, weights=None):
        """``wtdp[p, j, k] = sum_c dp_p(c) weights[j, k, c] / nconfig`` with the parameter derivatives of the LAST wave function."""
        if self.resolve_route(wfs) == "device":
            return self.avg_resident(wfs)
        self.last_route = "protocol"
        wfi = len(wfs) - 1
        dp = self.transform.serialize_gradients(wfs[wfi].pgradient())
        nconfig = weights.shape[-1]
        d = {}
        d["wtdp"] = np.einsum("cp,jkc->pjk", dp, weights, optimize=True) / nconfig
        return d

    def keys(self):
        return self.enacc.keys().union(["dpH", "dppsi", "dpidpj"])

    def shapes(self):
        d = {"dppsi": (_nparams(self.transform),)}
        d.update(self.enacc.shapes())
        return d

    def update_state(self, hdf_file):
        """Nothing to restore: the accumulator keeps no state."""
        pass

    def block_average(self, data_sample1, data, weights):
        """Averages and errors over blocks: ``wtdp`` (mixture blocks) divided by sqrt(N_i N_j) of the last state's row, the
        mean overlap, and the single-state SR moments (``data_sample1``)."""
        weight_avg = np.mean(weights, axis=0)
        N = np.abs(weight_avg.diagonal())
        Nij = np.sqrt(np.outer(N, N))
        avg = {}
        error = {}
        wfi = Nij.shape[0] - 1
        for k in ["wtdp"]:
            it = data[k]
            avg[k] = np.mean(it, axis=0) / Nij[wfi]
            error[k] = scipy.stats.sem(it, axis=0) / Nij[wfi]
        avg["overlap"] = weight_avg
        for k in ["total", "dppsi", "dpH", "dpidpj"]:
            it = data_sample1[k]
            avg[k] = np.mean(it, axis=0)
            error[k] = scipy.stats.sem(it, axis=0)
        return avg, error

    def _collect_terms(self, avg, error):
        ret = {}
        nwf = avg["overlap"].shape[0]
        N = np.abs(avg["overlap"].diagonal())
        Nij = np.sqrt(np.outer(N, N))
        ret["dp_energy"] = np.real(avg["dpH"] - avg["total"] * avg["dppsi"])
        ret["dpidpj"] = np.real(avg["dpidpj"] - np.einsum("i,j->ij", avg["dppsi"], avg["dppsi"]))
        fac = np.ones((nwf, nwf)) + np.identity(nwf)
        wfi = nwf - 1
        ret["norm"] = N
        ret["overlap"] = avg["overlap"] / Nij
        ret["dp_norm"] = 2.0 * np.real(avg["wtdp"][:, wfi, wfi])
        norm_part = np.einsum("i,p->pi", avg["overlap"][wfi, :], ret["dp_norm"]) / N
        ret["dp_overlap"] = fac[wfi] * (avg["wtdp"][:, wfi, :] - 0.5 * norm_part) / Nij[wfi]
        ret["energy"] = avg["total"]
        return ret

    def delta_p(self, steps, data, overlap_penalty, verbose=False):
        """``[-step (S + eps 1)^-1 g for step in steps]`` with g the energy gradient plus the penalised overlap gradient against the
        states before the last one; returns (steps, report)."""
        data = self._collect_terms(data, None)
        nwf = data["overlap"].shape[0]
        wfi = nwf - 1
        overlap_cost = 0.0
        for i in range(wfi):
            overlap_cost += overlap_penalty[wfi, i] * data["overlap"][wfi, i]
        if verbose:
            print("Overlap cost", overlap_cost)
        Sij = np.real(data["dpidpj"])
        invSij = np.linalg.inv(Sij + self.eps * np.eye(Sij.shape[0]))
        ovlp = 0.0
        for i in range(wfi):
            ovlp += 2.0 * data["dp_overlap"][:, i] * overlap_penalty[wfi, i] * data["overlap"][wfi, i]
        pgrad = data["dp_energy"] + ovlp
        v = np.einsum("ij,j->i", invSij, pgrad)
        dp = [-step * v for step in steps]
        report = {"pgrad": np.linalg.norm(pgrad), "SRdot": np.dot(pgrad, v) / (np.linalg.norm(v) * np.linalg.norm(pgrad))}
        if verbose:
            print("overlap gradient norm", np.linalg.norm(ovlp))
            print("Gradient norm: ", np.linalg.norm(pgrad))
            print("Dot product between gradient and SR step: ", report["SRdot"])
        return dp, report


def hdf_save(hdf_file, data, attr, wfs, configs):
    """One record of the optimisation file with every state's parameters (``wf/<i>/<key>``) and the walkers."""
    if hdf_file is not None:
        from .blockfile import BlockFile

        params = {f"{wfi}/{k}": np.array(it) for wfi, wf in enumerate(wfs) for k, it in wf.parameters.items()}
        BlockFile(hdf_file).append(data, attr, configs, parameters=params)


def set_wf_params(wf, params, updater):
    newparms = updater.transform.deserialize(wf, params)
    for k in newparms.keys():
        wf.parameters[k] = newparms[k]


def renormalize(wfs, norms, pivot=0, N=1):
    """Scale the determinant coefficients of every state but ``pivot`` by sqrt(norms[pivot] / norms[i] N), so that all states
    have the pivot's normalisation (``wf1det_coeff``, else ``det_coeff``, looked up on the last wave function as the reference does)."""
    for i, wf in enumerate(wfs):
        if i == pivot:
            continue
        renorm = np.sqrt(norms[pivot] / norms[i] * N)
        if "wf1det_coeff" in wfs[-1].parameters.keys():
            wf.parameters["wf1det_coeff"] = wf.parameters["wf1det_coeff"] * renorm
        elif "det_coeff" in wfs[-1].parameters.keys():
            wf.parameters["det_coeff"] = wf.parameters["det_coeff"] * renorm
        else:
            raise NotImplementedError("need wf1det_coeff or det_coeff in parameters")


def _vmc(wf, configs, accumulators=None, **kws):
    """The reference's ``mc.vmc(wf, configs, accumulators=..., **vmc_kwargs)`` on this package's ``vmc``: its deprecated ``nsteps``
    means ``nblocks = nsteps`` blocks of one step (mc.py:215-217); arguments only ``sample_overlap`` takes are dropped."""
    from .vmc import vmc

    kws = dict(kws)
    nsteps = kws.pop("nsteps", None)
    if nsteps is not None:
        kws["nblocks"], kws["nsteps_per_block"] = nsteps, 1
    kws = {k: v for k, v in kws.items() if k in ("nblocks", "nsteps_per_block", "tstep", "verbose", "seed")}
    return vmc(wf, configs, accumulators=accumulators, **kws)


def _sample_overlap(wfs, configs, energy, **kws):
    return sample_many.sample_overlap(wfs, configs, energy, **kws)


def optimize_ensemble(wfs, configs, updater, hdf_file, tau=1, max_iterations=100, overlap_penalty=None, npartitions=None, client=None,
                      verbose=False, vmc_kwargs={}):
    """Optimise the states ``wfs`` one after the other (ensemble_optimization_wfbywf.py:211-323).  ``updater[wfi]`` is the list of
    ``StochasticReconfigurationWfbyWf`` objects of state ``wfi``'s sub-iterations.  An existing ``hdf_file`` restarts: parameters and
    walkers from the file, from iteration max(iteration), state wavefunction[-1], sub-iteration sub_iteration[-1] + 1, without the
    initial VMC.  Returns ``wfs``."""
    if client is not None or npartitions is not None:
        raise NotImplementedError("pyqmc_amd.optimize_ensemble runs on one device: client / npartitions must be None")
    nwf = len(wfs)
    if overlap_penalty is None:
        overlap_penalty = np.ones((nwf, nwf)) * 0.5
    iteration_offset = 0
    wf_start = 0
    sub_iteration_offset = 0
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
            iteration_offset = np.max(ds["iteration"][...])
        if "sub_iteration" in ds:
            sub_iteration_offset = ds["sub_iteration"][-1] + 1
        if "wavefunction" in ds:
            wf_start = ds["wavefunction"][-1]
        store.load_walkers(configs)
    else:
        _, configs = _vmc(wfs[0], configs, **vmc_kwargs)

    for i in range(iteration_offset, max_iterations):
        for wfi in range(wf_start, nwf):
            wf = wfs[wfi]
            transform_list = updater[wfi]
            for sub_iteration in range(sub_iteration_offset, len(transform_list)):
                transform = transform_list[sub_iteration]
                data_weighted, data_unweighted, configs = _sample_overlap(wfs, configs, None, **vmc_kwargs)
                norm = np.mean(data_unweighted["overlap"], axis=0)
                if verbose:
                    print("Normalization step", norm.diagonal())
                renormalize(wfs, norm.diagonal(), pivot=0)
                data_sample1, configs = _vmc(wf, configs, accumulators={"": transform.onewf()}, **vmc_kwargs)
                data_weighted, data_unweighted, configs = _sample_overlap(wfs[0 : wfi + 1], configs, transform.allwfs(), **vmc_kwargs)
                avg, error = transform.block_average(data_sample1, data_weighted, data_unweighted["overlap"])
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
                hdf_save(hdf_file, save_data, {"tau": tau}, wfs, configs)
            sub_iteration_offset = 0
        wf_start = 0
    return wfs
