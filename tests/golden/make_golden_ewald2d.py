"""Golden vectors of the reference's slab Ewald sum (pyqmc/observables/ewald2d.py, class Ewald) -> g46_ewald2d.npz.

    python tests/golden/make_golden_ewald2d.py

Uses make_golden's stubs (numba as an identity decorator, pyscf / h5py mocked) and runs the real reference class.  Per case every
input (symbols, atoms, charges, nelec, lattice, nlatvec, folded configurations) and the reference's alpha, gpoints, gweight,
ewald_ion_ion, ee and ei.
  a1  the reference's monolayer known answer (tests/unit/test_ewald.py:68-88): one +1 ion, one electron, Madelung energy -1.6155
  a2  its three-layer slab (:90-116): three +1 ions, three electrons, -5.1122
  b   oblique 7 x 6 cell, Lz = 30, six atoms of charge 2, six electrons, 16 walkers with heights of sigma 2.5: the full energy()
  c   the same lattice, five atoms of charges (4, 2, 2, 1, 1), ten electrons, 16 walkers.  ee and ii from the reference's
      ewald_elec_elec / set_ewald_ion_ion; ei assembled here from the reference's own ewald.real_cij, ewald_recip_weight and
      ewald_recip_weight_charge with the ATOM axis contracted in all three terms: the reference's arithmetic with the contraction of
      ewald2d.py:188 corrected (as written it applies the charges along the electron axis, which raises for natoms != nelec and is
      only right for equal charges)
  d   case b with nlatvec = 2
  e   one atom and one electron in the oblique cell, 8 walkers (the special-case branches :124-126 and :225-226)
In a1, a2, b, d and e natoms == nelec and the charges are equal, so the reference's ei is right as it stands; the generator checks
that the corrected assembly reproduces it there.  Every reference output is asserted finite, and k_max |z|_max (far below the
709 at which the reference's weight overflows) is printed per case.
"""

import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import make_golden as mg  # noqa: E402  (installs the stubs, puts the reference on the path)

import numpy as np  # noqa: E402
import pyqmc.observables.ewald as refewald  # noqa: E402
from pyqmc.configurations.coord import PeriodicConfigs  # noqa: E402
from pyqmc.observables.ewald2d import Ewald  # noqa: E402

from pyqmc_amd import systems  # noqa: E402

OBLIQUE = np.array([[7.0, 0.0, 0.0], [2.0, 6.0, 0.0], [0.0, 0.0, 30.0]])
SQUARE = np.array([[1.0, 1.0, 0.0], [-1.0, 1.0, 0.0], [0.0, 0.0, 30.0]])


def _slab_points(rng, n, lattice, sigma):
    """n points uniform in the plane, heights normal around the middle of the cell."""
    frac = np.concatenate([rng.uniform(0, 1, n + (2,)), np.full(n + (1,), 0.5)], axis=-1)
    x = frac @ lattice
    x[..., 2] += sigma * rng.standard_normal(n)
    return x


def cases():
    """(name, symbols, atoms, charges, nelec, lattice, nlatvec, configs)."""
    rng = np.random.default_rng(460)
    out = [("a1", ["H"], np.zeros((1, 3)), [1.0], (1, 0), SQUARE, 1, np.array([[[1.0, 0.0, 0.0]]])),
           ("a2", ["H"] * 3, np.array([[0.0, 0, 0], [1, 0, 1], [1, 0, -1]]), [1.0] * 3, (2, 1), SQUARE, 1,
            np.array([[[1.0, 0, 0], [1, 1, 1], [1, 1, -1]]]))]
    atoms_b = _slab_points(rng, (6,), OBLIQUE, 1.5)
    x_b = _slab_points(rng, (16, 6), OBLIQUE, 2.5)
    out.append(("b", ["He"] * 6, atoms_b, [2.0] * 6, (3, 3), OBLIQUE, 1, x_b))
    out.append(("c", ["C", "He", "He", "H", "H"], _slab_points(rng, (5,), OBLIQUE, 1.5), [4.0, 2.0, 2.0, 1.0, 1.0], (5, 5), OBLIQUE, 1,
                _slab_points(rng, (16, 10), OBLIQUE, 2.5)))
    out.append(("d", ["He"] * 6, atoms_b, [2.0] * 6, (3, 3), OBLIQUE, 2, x_b))
    out.append(("e", ["H"], _slab_points(rng, (1,), OBLIQUE, 1.5), [1.0], (1, 0), OBLIQUE, 1, _slab_points(rng, (8, 1), OBLIQUE, 2.5)))
    return out


def elec_ion_atom_axis(ew, configs):
    """ewald_elec_ion (ewald2d.py:162-203) with the atom axis contracted in the real-space term as well."""
    d = configs.dist.pairwise(ew.atom_coords, configs.configs)  # (nconf, natoms, nelec, 3)
    q = np.asarray(ew.atom_charges)
    real = np.einsum("i,cij->c", -q, refewald.real_cij(d, ew.lattice_displacements, ew.alpha))
    g_dot_r = np.einsum("kd,cijd->cijk", ew.gpoints, d)
    recip = -2 * np.einsum("i,cijk,cijk->c", q, np.cos(g_dot_r), ew.ewald_recip_weight(d))
    charge = -2 * np.einsum("i,cij->c", q, ew.ewald_recip_weight_charge(d))
    return real + recip + charge, float(np.abs(d[..., 2]).max())


def main():
    out = {}
    for name, symbols, atoms, charges, nelec, lattice, nlatvec, x in cases():
        cell = systems.Cell(symbols, atoms, lattice, nelec=nelec, charges=charges, dimension=2)
        ew = Ewald(cell, nlatvec=nlatvec)
        configs = PeriodicConfigs(np.asarray(x, dtype=float), cell.lattice_vectors())
        ee = np.broadcast_to(np.asarray(ew.ewald_elec_elec(configs), dtype=float), (len(x),)).copy()
        ei, zmax = elec_ion_atom_axis(ew, configs)
        if name != "c":  # natoms == nelec, equal charges: the reference's own contraction is right
            ei_ref = np.asarray(ew.ewald_elec_ion(configs), dtype=float)
            assert np.max(np.abs(ei_ref - ei)) <= 1e-13 * np.max(np.abs(ei)), (name, ei_ref, ei)
            ei = ei_ref
        ii = float(np.ravel(ew.ewald_ion_ion)[0])
        if sum(nelec) > 1:
            zmax = max(zmax, float(np.abs(configs.dist.dist_matrix(configs.configs)[0][..., 2]).max()))
        assert np.all(np.isfinite(ee)) and np.all(np.isfinite(ei)) and np.isfinite(ii), name
        out[f"{name}_symbols"] = np.asarray(symbols)
        out[f"{name}_atoms"] = np.asarray(atoms, dtype=float)
        out[f"{name}_charges"] = np.asarray(charges, dtype=float)
        out[f"{name}_nelec"] = np.asarray(nelec)
        out[f"{name}_lattice"] = np.asarray(lattice)
        out[f"{name}_nlatvec"] = np.asarray(nlatvec)
        out[f"{name}_configs"] = np.asarray(configs.configs)
        out[f"{name}_alpha"] = np.asarray(float(ew.alpha))
        out[f"{name}_gpoints"] = np.asarray(ew.gpoints, dtype=float)
        out[f"{name}_gweight"] = np.asarray(ew.gweight, dtype=float)
        out[f"{name}_ii"] = np.asarray(ii)
        out[f"{name}_ee"] = ee
        out[f"{name}_ei"] = ei
        print(name, nelec, "nk", len(ew.gweight), "k_max |z|_max", float(np.max(ew.gnorm)) * zmax, "ee", float(ee.mean()), "ei",
              float(ei.mean()), "ii", ii, "total", float((ee + ei).mean()) + ii, file=sys.stderr)
    mg.save("g46_ewald2d", **out)


if __name__ == "__main__":
    main()
