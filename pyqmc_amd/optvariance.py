"""Variance minimisation on fixed walkers — ``pyqmc/method/optvariance.py`` on this package's wave functions.

``optvariance(energy, wf, coords, params=None, **kwargs)`` takes the reference's arguments and returns ``(res.fun, wf)``.  The local
energy is evaluated once, ``Enref = energy(coords, wf)``; ``Enref["total"] - Enref["ke"]`` (ECP included) stays fixed and each cost
evaluation recomputes only the kinetic energy, the cost being the population variance of the local energy over the walkers.
``scipy.optimize.minimize(cost, x0, callback=..., **kwargs)`` runs on the parameters of ``params`` flattened in that order, with the
reference's printing callback.

Each cost evaluation takes one of two routes (``optvariance_route``):

* ``"fused"`` — a real single-determinant Slater x two-body-Jastrow wave function on one device handle, optimised over Jastrow
  coefficients only (``wf2acoeff`` / ``wf2bcoeff``): ONE C call, ``pqa_variance`` with K = 1, and no parameter upload
  (csrc/pqa_variance.hip).  Opt-in: ``jac=True`` makes the cost return ``(variance, gradient)`` from that same call (the kinetic
  energy is an exact quadratic in the coefficients, so the gradient is exact); without it the optimiser sees what the reference's
  does, within rounding;
* ``"protocol"`` — anything else (``params=None`` on ``generate_wf``'s wave function includes the orbital coefficients): the
  parameters are set, the wave function recomputed and ``ke`` taken from ``energy``, as the reference does.  ``jac=True`` is refused.

Deliberate differences from the reference: on return ``wf.parameters`` hold the optimum and the wave function is recomputed at
``coords`` with them (the reference leaves the state of its last evaluation).  Three fixes: the cost adds the kinetic energy (the
reference adds the pair (ke, grad2) that ``observables.energy.kinetic`` returns, which takes the variance over 2W numbers); the
shapes are kept in a list (the reference's ``np.array`` of them fails for keys of different rank, such as ``wf2acoeff`` with
``wf2bcoeff``); the flat vector is split at the cumulative sizes of the keys (the reference splits at the sizes themselves, which
agrees for one or two keys).
"""

import numpy as np

from .wf import linear_jastrow_device


def _keys(wf, params):
    return list(wf.parameters.keys()) if params is None else list(params)


def optvariance_route(wf, params=None):
    """``"fused"`` when ``pqa_variance`` covers this wave function and parameter selection, else ``"protocol"``."""
    keys = _keys(wf, params)
    return "fused" if keys and linear_jastrow_device(wf, keys) is not None else "protocol"


def flatten(wf, params):
    """(x0, shapes): the parameters of ``params`` flattened and concatenated in that order, and their shapes."""
    shapes = [np.shape(wf.parameters[k]) for k in params]
    return np.concatenate([np.ravel(wf.parameters[k]) for k in params]), shapes


def split(x, shapes):
    """Inverse of ``flatten``: the flat vector -> one array per key."""
    sizes = [int(np.prod(s)) for s in shapes]
    return [v.reshape(s) for v, s in zip(np.split(np.asarray(x), np.cumsum(sizes)[:-1]), shapes)]


def _protocol_cost(energy, wf, coords, params, shapes, eoff):
    def cost(x):
        for k, v in zip(params, split(x, shapes)):
            wf.parameters[k] = v
        wf.recompute(coords)
        ke = energy(coords, wf)["ke"]
        return np.std(eoff + ke) ** 2

    return cost


def _fused_cost(wf, params, shapes, eoff):
    dev = wf.fused_device()
    ja = wf.wf_factors[1].parameters
    a0, b0 = np.array(ja["acoeff"]), np.array(ja["bcoeff"])
    eoff = np.ascontiguousarray(np.real(eoff), dtype=float)
    Pa = a0.size

    def sets(x):
        p = dict(zip(params, split(x, shapes)))
        return p.get("wf2acoeff", a0)[None], p.get("wf2bcoeff", b0)[None]

    def cost(x):
        return float(dev.variance(*sets(x), eoff)[0][0])

    def cost_jac(x):
        var, dvar, _ = dev.variance(*sets(x), eoff, grad=True)
        g = {"wf2acoeff": dvar[0, :Pa], "wf2bcoeff": dvar[0, Pa:]}
        return float(var[0]), np.concatenate([g[k] for k in params])

    return cost, cost_jac


def optvariance(energy, wf, coords, params=None, **kwargs):
    """Minimise the variance of the local energy over ``coords`` against the parameters ``params`` (optvariance.py:20-70).

    ``energy``: an accumulator returning the total energy in ``"total"`` and the kinetic energy in ``"ke"``; ``params``: keys of
    ``wf.parameters`` (None: all); ``kwargs``: options of ``scipy.optimize.minimize`` (``jac=True`` on the fused route only).
    Returns (optimised variance, wf) with ``wf.parameters`` at the optimum and ``wf`` recomputed at ``coords``."""
    import scipy.optimize

    params = _keys(wf, params)
    route = optvariance_route(wf, params)
    if kwargs.get("jac") is True and route != "fused":
        raise ValueError("optvariance: jac=True needs the fused route (a real single-determinant Slater x two-body Jastrow wave function "
                         "on one device handle, params within wf2acoeff / wf2bcoeff); this call takes the protocol route")
    x0, shapes = flatten(wf, params)
    if route == "fused":
        wf.recompute(coords)  # (pqa_variance reads the walkers resident on the handle)
    Enref = energy(coords, wf)
    eoff = Enref["total"] - Enref["ke"]
    if route == "fused":
        cost, cost_jac = _fused_cost(wf, params, shapes, eoff)
        fun = cost_jac if kwargs.get("jac") is True else cost
    else:
        cost = fun = _protocol_cost(energy, wf, coords, params, shapes, eoff)

    def callback(xk):
        print(xk, cost(xk))
        return False

    res = scipy.optimize.minimize(fun, x0=x0, callback=callback, **kwargs)
    for k, v in zip(params, split(res.x, shapes)):
        wf.parameters[k] = v
    wf.recompute(coords)
    return res.fun, wf
