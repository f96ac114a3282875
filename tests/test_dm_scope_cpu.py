"""The fused-scope ladder of ``OBDMAccumulator`` and ``TBDMAccumulator`` on stub handles and evaluators, without a device.

Both accumulators decide their fused scope in ``obdm._FusedScope`` (the common part: wave-function kind, evaluator kind, devices,
electron numbers) plus a tail of their own.  The table below pins, for the full product of the two opt-in flags, six handle kinds and
three evaluator kinds, the exact reason (or None) with an in-scope and a failing tail per estimator, and the library entry every
in-scope combination is evaluated through.  Its literals were transcribed from what ``OBDMAccumulator._out_of_scope`` and
``TBDMAccumulator.resident_scope`` returned on these same stubs BEFORE the ladder was moved into one place (instances made with
``__new__``, the handle lookup overridden as here), and the entries from the ``_j3_entry`` / ``_complex_entry`` branches of that code.
"""

import itertools
import types

import numpy as np
import pytest

from pyqmc_amd.obdm import OBDMAccumulator
from pyqmc_amd.tbdm import TBDMAccumulator

NELEC = (2, 2)

HANDLES = {  # kind -> (cplx, twisted, has_j3); "none": the wave function lives on no single handle
    "real": (False, False, False), "complex": (True, False, False), "twisted": (True, True, False), "real+j3": (False, False, True),
    "complex+j3": (True, False, True), "none": None}
EVALUATORS = {"real": (False, False), "complex": (True, False), "twisted": (True, True)}  # kind -> (cplx, twisted)


def _handle(kind, device=0, nelec=NELEC):
    if HANDLES[kind] is None:
        return None
    cplx, twisted, j3 = HANDLES[kind]
    return types.SimpleNamespace(cplx=cplx, twisted=twisted, has_j3=j3, has_jastrow=True, has_slater=True, device=device, nelec=nelec,
                                 N=sum(nelec), W=8)


def _evaluator(kind, device=0):
    cplx, twisted = EVALUATORS[kind]
    return types.SimpleNamespace(cplx=cplx, twisted=twisted, has_j3=False, has_jastrow=False, has_slater=True, device=device, nelec=(1, 1),
                                 N=2, W=0)


def _admitted(kind, complex_device, three_body_device):
    """What the handle lookup (``wf.readonly_device`` with the accumulator's flags) does with a handle of this kind."""
    return {"real": True, "complex": complex_device, "twisted": complex_device, "real+j3": three_body_device, "complex+j3": False,
            "none": False}[kind]


def _accumulator(cls, complex_device, three_body_device, handle_kind, ev, electrons, dev):
    acc = cls.__new__(cls)
    acc.complex_device, acc.three_body_device, acc._route = complex_device, three_body_device, None
    acc.orbitals, acc._mol, acc._electrons = types.SimpleNamespace(dev=ev), types.SimpleNamespace(nelec=NELEC), electrons
    acc._device = lambda wf: dev if _admitted(handle_kind, complex_device, three_body_device) else None
    return acc


TAILS = {  # estimator -> (class, scope method, in-scope electrons, failing electrons)
    "obdm": (OBDMAccumulator, "_out_of_scope", np.array([0, 1, 2]), np.array([0, 1, 1])),
    "tbdm": (TBDMAccumulator, "resident_scope", [np.arange(0, 2), np.arange(2, 4)], [np.arange(0, 0), np.arange(0, 2)])}


def scope_and_entry(estimator, complex_device, three_body_device, handle_kind, ev_kind, failing_tail, entry_of, **handle_kw):
    """(reason, entry): the reason the accumulator gives for the stubs, and for an in-scope case ``entry_of(acc, handle)``."""
    cls, method, good, bad = TAILS[estimator]
    dev, ev = _handle(handle_kind, **handle_kw), _evaluator(ev_kind)
    acc = _accumulator(cls, complex_device, three_body_device, handle_kind, ev, bad if failing_tail else good, dev)
    why = getattr(acc, method)(types.SimpleNamespace(fused_device=lambda: dev))
    return why, (entry_of(acc, dev) if why is None else None)


NOT_REAL = "the wave function is not a real Slater (x two-body Jastrow) product on one device handle"
NOT_ANY = "the wave function is not a Slater (x two-body Jastrow) product on one device handle"
NOT_REAL3 = "the wave function is not a real Slater (x two-body x three-body Jastrow) product on one device handle"
NOT_ANY3 = "the wave function is not a Slater (x two-body x three-body Jastrow) product on one device handle"
CPLX3_O = "the three-body wave function is complex or twisted (pqa_obdm_sweeps_j3 takes real handles)"
CPLX3_T = "the three-body wave function is complex or twisted (pqa_tbdm_sweep_j3 takes real handles)"
EV_J3 = "the orbital evaluator is complex (a three-body wave function needs a real one)"
EV_TWIST = "the orbital evaluator is twisted and the wave function's handle is not (its folded walkers have lost the wrap phase)"
EV_CPLX = "the orbital evaluator is complex"
DEVICES = "the wave function and the evaluator are on different devices"
NELECS = "the wave function has other electron numbers than the accumulator's system"
REPEAT = "the electron list repeats an electron or names one the wave function does not have"
EMPTY = "a spin block of the sector is empty"
O, O_C, O_J3 = "pqa_obdm_sweeps", "pqa_obdm_sweeps_c", "pqa_obdm_sweeps_j3"
T, T_C, T_J3 = "pqa_tbdm_sweep", "pqa_tbdm_sweep_c", "pqa_tbdm_sweep_j3"

# (complex_device, three_body_device, handle, evaluator) -> (obdm, obdm with a repeated electron, tbdm, tbdm with an empty spin block):
# a reason, or for an in-scope combination (reason None) the entry it is evaluated through
TABLE = {
    (False, False, 'real', 'real'): (O, REPEAT, T, EMPTY),
    (False, False, 'real', 'complex'): (EV_CPLX, EV_CPLX, EV_CPLX, EV_CPLX),
    (False, False, 'real', 'twisted'): (EV_CPLX, EV_CPLX, EV_CPLX, EV_CPLX),
    (False, False, 'complex', 'real'): (NOT_REAL, NOT_REAL, NOT_REAL, NOT_REAL),
    (False, False, 'complex', 'complex'): (NOT_REAL, NOT_REAL, NOT_REAL, NOT_REAL),
    (False, False, 'complex', 'twisted'): (NOT_REAL, NOT_REAL, NOT_REAL, NOT_REAL),
    (False, False, 'twisted', 'real'): (NOT_REAL, NOT_REAL, NOT_REAL, NOT_REAL),
    (False, False, 'twisted', 'complex'): (NOT_REAL, NOT_REAL, NOT_REAL, NOT_REAL),
    (False, False, 'twisted', 'twisted'): (NOT_REAL, NOT_REAL, NOT_REAL, NOT_REAL),
    (False, False, 'real+j3', 'real'): (NOT_REAL, NOT_REAL, NOT_REAL, NOT_REAL),
    (False, False, 'real+j3', 'complex'): (NOT_REAL, NOT_REAL, NOT_REAL, NOT_REAL),
    (False, False, 'real+j3', 'twisted'): (NOT_REAL, NOT_REAL, NOT_REAL, NOT_REAL),
    (False, False, 'complex+j3', 'real'): (NOT_REAL, NOT_REAL, NOT_REAL, NOT_REAL),
    (False, False, 'complex+j3', 'complex'): (NOT_REAL, NOT_REAL, NOT_REAL, NOT_REAL),
    (False, False, 'complex+j3', 'twisted'): (NOT_REAL, NOT_REAL, NOT_REAL, NOT_REAL),
    (False, False, 'none', 'real'): (NOT_REAL, NOT_REAL, NOT_REAL, NOT_REAL),
    (False, False, 'none', 'complex'): (NOT_REAL, NOT_REAL, NOT_REAL, NOT_REAL),
    (False, False, 'none', 'twisted'): (NOT_REAL, NOT_REAL, NOT_REAL, NOT_REAL),
    (False, True, 'real', 'real'): (O, REPEAT, T, EMPTY),
    (False, True, 'real', 'complex'): (EV_CPLX, EV_CPLX, EV_CPLX, EV_CPLX),
    (False, True, 'real', 'twisted'): (EV_CPLX, EV_CPLX, EV_CPLX, EV_CPLX),
    (False, True, 'complex', 'real'): (NOT_REAL3, NOT_REAL3, NOT_REAL3, NOT_REAL3),
    (False, True, 'complex', 'complex'): (NOT_REAL3, NOT_REAL3, NOT_REAL3, NOT_REAL3),
    (False, True, 'complex', 'twisted'): (NOT_REAL3, NOT_REAL3, NOT_REAL3, NOT_REAL3),
    (False, True, 'twisted', 'real'): (NOT_REAL3, NOT_REAL3, NOT_REAL3, NOT_REAL3),
    (False, True, 'twisted', 'complex'): (NOT_REAL3, NOT_REAL3, NOT_REAL3, NOT_REAL3),
    (False, True, 'twisted', 'twisted'): (NOT_REAL3, NOT_REAL3, NOT_REAL3, NOT_REAL3),
    (False, True, 'real+j3', 'real'): (O_J3, REPEAT, T_J3, EMPTY),
    (False, True, 'real+j3', 'complex'): (EV_J3, EV_J3, EV_J3, EV_J3),
    (False, True, 'real+j3', 'twisted'): (EV_J3, EV_J3, EV_J3, EV_J3),
    (False, True, 'complex+j3', 'real'): (CPLX3_O, CPLX3_O, CPLX3_T, CPLX3_T),
    (False, True, 'complex+j3', 'complex'): (CPLX3_O, CPLX3_O, CPLX3_T, CPLX3_T),
    (False, True, 'complex+j3', 'twisted'): (CPLX3_O, CPLX3_O, CPLX3_T, CPLX3_T),
    (False, True, 'none', 'real'): (NOT_REAL3, NOT_REAL3, NOT_REAL3, NOT_REAL3),
    (False, True, 'none', 'complex'): (NOT_REAL3, NOT_REAL3, NOT_REAL3, NOT_REAL3),
    (False, True, 'none', 'twisted'): (NOT_REAL3, NOT_REAL3, NOT_REAL3, NOT_REAL3),
    (True, False, 'real', 'real'): (O, REPEAT, T, EMPTY),
    (True, False, 'real', 'complex'): (O_C, REPEAT, T_C, EMPTY),
    (True, False, 'real', 'twisted'): (EV_TWIST, EV_TWIST, EV_TWIST, EV_TWIST),
    (True, False, 'complex', 'real'): (O_C, REPEAT, T_C, EMPTY),
    (True, False, 'complex', 'complex'): (O_C, REPEAT, T_C, EMPTY),
    (True, False, 'complex', 'twisted'): (EV_TWIST, EV_TWIST, EV_TWIST, EV_TWIST),
    (True, False, 'twisted', 'real'): (O_C, REPEAT, T_C, EMPTY),
    (True, False, 'twisted', 'complex'): (O_C, REPEAT, T_C, EMPTY),
    (True, False, 'twisted', 'twisted'): (O_C, REPEAT, T_C, EMPTY),
    (True, False, 'real+j3', 'real'): (NOT_ANY, NOT_ANY, NOT_ANY, NOT_ANY),
    (True, False, 'real+j3', 'complex'): (NOT_ANY, NOT_ANY, NOT_ANY, NOT_ANY),
    (True, False, 'real+j3', 'twisted'): (NOT_ANY, NOT_ANY, NOT_ANY, NOT_ANY),
    (True, False, 'complex+j3', 'real'): (NOT_ANY, NOT_ANY, NOT_ANY, NOT_ANY),
    (True, False, 'complex+j3', 'complex'): (NOT_ANY, NOT_ANY, NOT_ANY, NOT_ANY),
    (True, False, 'complex+j3', 'twisted'): (NOT_ANY, NOT_ANY, NOT_ANY, NOT_ANY),
    (True, False, 'none', 'real'): (NOT_ANY, NOT_ANY, NOT_ANY, NOT_ANY),
    (True, False, 'none', 'complex'): (NOT_ANY, NOT_ANY, NOT_ANY, NOT_ANY),
    (True, False, 'none', 'twisted'): (NOT_ANY, NOT_ANY, NOT_ANY, NOT_ANY),
    (True, True, 'real', 'real'): (O, REPEAT, T, EMPTY),
    (True, True, 'real', 'complex'): (O_C, REPEAT, T_C, EMPTY),
    (True, True, 'real', 'twisted'): (EV_TWIST, EV_TWIST, EV_TWIST, EV_TWIST),
    (True, True, 'complex', 'real'): (O_C, REPEAT, T_C, EMPTY),
    (True, True, 'complex', 'complex'): (O_C, REPEAT, T_C, EMPTY),
    (True, True, 'complex', 'twisted'): (EV_TWIST, EV_TWIST, EV_TWIST, EV_TWIST),
    (True, True, 'twisted', 'real'): (O_C, REPEAT, T_C, EMPTY),
    (True, True, 'twisted', 'complex'): (O_C, REPEAT, T_C, EMPTY),
    (True, True, 'twisted', 'twisted'): (O_C, REPEAT, T_C, EMPTY),
    (True, True, 'real+j3', 'real'): (O_J3, REPEAT, T_J3, EMPTY),
    (True, True, 'real+j3', 'complex'): (EV_J3, EV_J3, EV_J3, EV_J3),
    (True, True, 'real+j3', 'twisted'): (EV_J3, EV_J3, EV_J3, EV_J3),
    (True, True, 'complex+j3', 'real'): (CPLX3_O, CPLX3_O, CPLX3_T, CPLX3_T),
    (True, True, 'complex+j3', 'complex'): (CPLX3_O, CPLX3_O, CPLX3_T, CPLX3_T),
    (True, True, 'complex+j3', 'twisted'): (CPLX3_O, CPLX3_O, CPLX3_T, CPLX3_T),
    (True, True, 'none', 'real'): (NOT_ANY3, NOT_ANY3, NOT_ANY3, NOT_ANY3),
    (True, True, 'none', 'complex'): (NOT_ANY3, NOT_ANY3, NOT_ANY3, NOT_ANY3),
    (True, True, 'none', 'twisted'): (NOT_ANY3, NOT_ANY3, NOT_ANY3, NOT_ANY3),
}

# beyond the product: the two rungs of the common ladder the product never reaches, (handle keywords) -> reason for both estimators
EXTRA = {("device", 1): DEVICES, ("nelec", (3, 1)): NELECS}


def test_the_table_is_the_full_product():
    keys = set(itertools.product((False, True), (False, True), HANDLES, EVALUATORS))
    assert set(TABLE) == keys and len(keys) == 72
    assert all(len(row) == 4 for row in TABLE.values())


@pytest.mark.parametrize("estimator", ["obdm", "tbdm"])
def test_scope_ladder_reasons_and_entries(estimator):
    col = 0 if estimator == "obdm" else 2
    for key, row in TABLE.items():
        for failing_tail in (False, True):
            want = row[col + failing_tail]
            why, entry = scope_and_entry(estimator, *key, failing_tail, lambda acc, dev: acc._entry(dev))
            if want.startswith("pqa_"):
                assert why is None and entry == want, (estimator, key, failing_tail, why, entry)
            else:
                assert why == want and entry is None, (estimator, key, failing_tail, why)


@pytest.mark.parametrize("estimator", ["obdm", "tbdm"])
def test_devices_and_electron_numbers(estimator):
    for (name, value), want in EXTRA.items():
        for flags in itertools.product((False, True), repeat=2):
            why, _ = scope_and_entry(estimator, *flags, "real", "real", True, None, **{name: value})
            assert why == want, (estimator, name, flags, why)


def test_tbdm_fused_device_is_the_reason_and_the_walker_count():
    """``_fused_device`` hands out the handle exactly when the reason is None and the resident walkers are the configurations."""
    cls, _, good, _ = TAILS["tbdm"]
    dev, ev = _handle("real"), _evaluator("real")
    acc = _accumulator(cls, False, False, "real", ev, good, dev)
    wf = types.SimpleNamespace(fused_device=lambda: dev)
    configs = lambda n: types.SimpleNamespace(configs=np.zeros((n, 4, 3)))  # noqa: E731
    assert acc._fused_device(configs(8), wf) is dev and acc._fused_device(configs(7), wf) is None
    acc.orbitals = types.SimpleNamespace(dev=_evaluator("complex"))
    assert acc.resident_scope(wf) == EV_CPLX and acc._fused_device(configs(8), wf) is None
    acc._route = "fused"
    with pytest.raises(ValueError, match="needs a real Slater"):
        acc._fused_device(configs(8), wf)
    acc._route = "protocol"
    assert acc._fused_device(configs(8), wf) is None and acc.resident_scope(wf) == "the accumulator is bound to route='protocol'"
