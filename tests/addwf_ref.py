"""The superposition (AddWF) cases of the golden file g49_addwf.npz, shared by its generator and the tests.

Every component is a Slater x two-body Jastrow product over one mean field; ``components(name, make)`` builds them with any of the
three builders of that signature: make_golden.make_wf (the reference), helpers.oracle_wf (the CPU oracle), helpers.gpu_wf (the device).
"""

import contextlib

import numpy as np

from pyqmc_amd import systems

GOLDEN = "g49_addwf"
NAUX = 5
TSTEP, NSWEEPS = 0.3, 2  # the trajectory of case a

# name -> walkers, the two electrons of the protocol calls (one of each spin), the electrons of testvalue_many, coeffs,
#         Jastrow seeds (helpers.jastrow_params) per component, det_coeff per component (None: one determinant)
CASES = {
    "a": dict(W=70, electrons=(1, 5), many=(0, 3, 6), coeffs=[0.8, 0.5], jseeds=(11, 12), det_coeff=None),
    "b": dict(W=24, electrons=(2, 6), many=(1, 4, 7), coeffs=[0.6, 0.5, 0.4], jseeds=(11, 11, 11),
              det_coeff=[[1.0, 0.2, -0.1, 0.05], [1.0, -0.3, 0.2, -0.2], [1.0, 0.4, 0.1, 0.3]]),
    "c": dict(W=8, electrons=(0, 7), many=(2, 5), coeffs=[0.8, 0.3 + 0.4j], jseeds=(11, 12), det_coeff=None),
}


def case_system(name):
    """(mol, mf, determinants or None)"""
    mol = systems.water()
    if CASES[name]["det_coeff"] is None:
        return mol, systems.random_mf(mol), None
    mf = systems.random_mf(mol, nvirt=4)
    return mol, mf, systems.random_determinants(mol, mf, len(CASES[name]["det_coeff"][0]))


def components(name, make):
    c = CASES[name]
    mol, mf, dets = case_system(name)
    wfs = []
    for k, seed in enumerate(c["jseeds"]):
        wf = make(mol, mf, determinants=dets, seed=seed)
        if c["det_coeff"] is not None:
            sl = wf.wf_factors[0]
            sl.parameters["det_coeff"] = np.array(c["det_coeff"][k], dtype=float)
            if isinstance(wf.parameters, dict):  # (a product whose parameters are a flat dictionary of the factors' arrays)
                wf.parameters["wf1det_coeff"] = sl.parameters["det_coeff"]
        wfs.append(wf)
    return mol, wfs


@contextlib.contextmanager
def replay(gauss_unit, unif):
    """np.random.normal / np.random.rand serve the recorded draws in order (gauss_unit: unit normals, scaled by the caller's scale)."""
    g, u = iter(gauss_unit), iter(unif)
    saved = (np.random.normal, np.random.rand)
    np.random.normal = lambda loc=0.0, scale=1.0, size=None: loc + scale * next(g)
    np.random.rand = lambda *shape: next(u)
    try:
        yield
    finally:
        np.random.normal, np.random.rand = saved


def protocol_entries(wf, configs, g, p, out):
    """Run the protocol calls of one case on ``wf`` in the generator's order; ``out[key]`` receives each result under the golden's
    key.  ``g`` holds the inputs (newpos, aux, mask, accept per electron)."""
    c = CASES[p[0]]
    s, l = wf.recompute(configs)
    out[p + "value_sign"], out[p + "value_log"] = s, l
    for e in c["electrons"]:
        q = p + f"e{e}_"
        ep = configs.make_irreducible(e, g[q + "newpos"])
        ea = configs.make_irreducible(e, g[q + "aux"])
        mask, accept = g[q + "mask"], g[q + "accept"]
        gr, v, _ = wf.gradient_value(e, ep)
        out[q + "gv_grad"], out[q + "gv_val"] = gr, v
        out[q + "grad"] = wf.gradient(e, ep)
        gr, lap = wf.gradient_laplacian(e, ep)
        out[q + "gl_grad"], out[q + "gl_lap"] = gr, lap
        out[q + "testvalue"] = wf.testvalue(e, ep)[0]
        out[q + "testvalue_mask"] = wf.testvalue(e, ep, mask)[0]
        out[q + "testvalue_aux"] = wf.testvalue(e, ea)[0]
        out[q + "testvalue_aux_mask"] = wf.testvalue(e, ea, mask)[0]
        out[q + "testvalue_many"] = wf.testvalue_many(np.asarray(c["many"]), configs.make_irreducible(e, g[q + "manypos"]))
        out[q + "ratio"] = wf.ratio(e, ep)
        out[q + "rcc"] = wf.ratio_current_config()
        out[q + "rcc_mask"] = wf.ratio_current_config(mask)
        _, _, saved = wf.gradient_value(e, ep)
        configs.move(e, ep, accept)
        wf.updateinternals(e, ep, configs, mask=accept, saved_values=saved)
        s, l = wf.value()
        out[q + "post_sign"], out[q + "post_log"] = s, l
    pg = wf.pgradient()
    out[p + "pgrad_keys"] = np.asarray(list(pg.keys()))
    out[p + "param_keys"] = np.asarray(list(wf.parameters.keys()))
    for k in pg.keys():
        out[p + "pgrad_" + k] = np.asarray(pg[k])
    out[p + "final_rcc"] = wf.ratio_current_config()
