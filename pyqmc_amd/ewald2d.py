"""Slab (2D) Ewald energy — public interface of ``pyqmc/observables/ewald2d.py`` (``Ewald``), plus ``SlabEnergyAccumulator``.

The Coulomb energy of a cell that is periodic along its first two lattice vectors and open along the third (Yeh and Berkowitz,
J. Chem. Phys. 111, 3155).  Per pair of particles with minimal-image displacement d = (dx, dy, z) the reference sums

    real    sum_L erfc(alpha |d + L|) / |d + L|                      over the in-plane displacements L
    recip   2 sum_k cos(k.d) W(k, z),  W = (pi / (A k)) [e^{kz} erfc(k / 2 alpha + alpha z) + e^{-kz} erfc(k / 2 alpha - alpha z)]
    charge  -(2 pi / A) [z erf(alpha z) + exp(-alpha^2 z^2) / (alpha sqrt(pi))]

and ee = sum_{i<j} + N self, ei = -sum_{i,I} q_I (...), ii = sum_{I<J} q_I q_J (...) + self sum_I q_I^2.  Both routes evaluate W
in the scaled form W = (pi / (A k)) exp(-a^2 - s^2) [erfcx(a + s) + erfcx(a - s)], a = k / 2 alpha, s = alpha |z|, with
erfcx(t) = 2 exp(t^2) - erfcx(-t) for t < 0 (whose first part times the prefactor is exactly 2 exp(-k |z|)): the reference's
product exp(k z) erfc(.) is inf * 0 = NaN once k |z| exceeds about 709, this form cannot overflow.

The electron-ion sums contract the atom axis in all three terms.  The reference's real-space term (ewald2d.py:188) applies the
charges along the electron axis: it raises for natoms != nelec and is only right when all charges are equal.

Two routes compute ``Ewald.energy``; ``last_route`` names the one taken:

* **fused** (``pqa_ewald2d``): ``wf`` lives on a periodic device handle whose resident walkers are ``configs``.
* **host**: everything else (no ``wf``, the CPU oracle's objects).  NumPy / ``scipy.special.erfcx`` over walker chunks bounded by
  ``host_chunk_bytes``.
"""

import ctypes as C

import numpy as np
from scipy.special import erf, erfc, erfcx

from . import _ffi
from .configs import MinimalImageDistance
from .energy import KEYS, EnergyAccumulator
from .sq import device_handle


def slab_gpoints(gmax, recvec, latvec, alpha, cell_area, tol=1e-10):
    """k vectors (rows), norms, weights ``2 pi erfc(k / 2 alpha) / (A k) > tol`` and integer coordinates (nk, 2), in the order
    ``generate_positive_gpoints`` + ``set_gpoints`` produce them (ewald2d.py:74-104).  Only the index box that can hold surviving
    weights is enumerated (the reference filters a (gmax, 2 gmax + 1) grid; the survivors and their order are the same)."""
    f = lambda k: 2 * np.pi * erfc(k / (2 * alpha)) / (cell_area * k)
    lo, hi = 1e-8, 1e8  # bisect k where the weight crosses tol (monotone decreasing)
    for _ in range(200):
        mid = np.sqrt(lo * hi)
        lo, hi = (mid, hi) if f(mid) > tol else (lo, mid)
    kmax = hi * (1 + 1e-9)
    # k = n0 b0 + n1 b1 and b_a . a_b = 2 pi delta_ab: |n_a| = |k . a_a| / 2 pi <= |k| |a_a| / 2 pi
    n = np.minimum(np.floor(kmax * np.linalg.norm(latvec[:2], axis=1) / (2 * np.pi)).astype(int) + 1, gmax)
    blocks = [np.mgrid[1 : n[0] + 1, -n[1] : n[1] + 1, 0:1].reshape(3, -1), np.mgrid[0:1, 1 : n[1] + 1, 0:1].reshape(3, -1)]
    gpts = np.concatenate(blocks, axis=1)
    gpoints = np.einsum("ji,jk->ik", gpts, recvec * 2 * np.pi)
    gnorm = np.linalg.norm(gpoints, axis=-1)
    gweight = np.pi * erfc(gnorm / (2 * alpha)) * 2
    gweight /= cell_area * gnorm
    big = gweight > tol
    return gpoints[big], gnorm[big], gweight[big], np.ascontiguousarray(gpts.T[big][:, :2], dtype=np.int32)


def recip_weight(z, gnorm, alpha, cell_area):
    """W(k, z) of ewald2d.py:264-284 in the scaled form: z (...,) -> (..., nk).  Finite for every z."""
    s = alpha * np.abs(z)[..., np.newaxis]
    a = gnorm / (2 * alpha)
    scale = np.exp(-(a**2) - s**2)
    tm = a - s
    neg = tm < 0
    far = np.where(neg, 2 * np.exp(-gnorm * np.abs(z)[..., np.newaxis]), 0.0)
    w = scale * erfcx(a + s) + np.where(neg, -scale * erfcx(np.abs(tm)), scale * erfcx(np.abs(tm))) + far
    return np.pi / (cell_area * gnorm) * w


def charge_weight(z, alpha, cell_area):
    """The k = 0 weight of ewald2d.py:286-304: z (...,) -> (...,)."""
    return -np.pi / cell_area * (z * erf(alpha * z) + np.exp(-(alpha**2) * z**2) / (alpha * np.sqrt(np.pi)))


def real_cij(d, lattice_displacements, alpha):
    """ewald.real_cij (ewald.py:391-398): sum over the displacements of erfc(alpha r) / r; d (..., 3) -> (...,)."""
    cij = np.zeros(d.shape[:-1])
    for ld in lattice_displacements:
        r = np.linalg.norm(d + ld, axis=-1)
        cij += erfc(alpha * r) / r
    return cij


def ewald2d_tables(cell, gmax=200, nlatvec=1, alpha_scaling=5.0, gidx=None):
    """Everything position independent (ewald2d.py:32-160): ``set_alpha``, ``set_lattice_displacements``, ``set_gpoints``,
    ``ewald_self`` and ``set_ewald_ion_ion``, plus what ``pqa_ewald2d`` takes (``gidx``, ``recip``, ``kpref``).  ``gidx`` (nk, 2):
    explicit integer coordinates of the k vectors in the basis of the two in-plane reciprocal rows, instead of the selection by
    weight (one of each +-k pair, none zero)."""
    latvec = np.asarray(cell.lattice_vectors(), dtype=float)
    coords = np.asarray(cell.atom_coords(), dtype=float)
    charges = np.asarray(cell.atom_charges(), dtype=float)
    cell_area = np.linalg.det(latvec[:2, :2])
    recvec = np.linalg.inv(latvec).T
    alpha = alpha_scaling / np.amin(1 / np.linalg.norm(recvec[:2, :2], axis=1))
    space = [np.arange(-nlatvec, nlatvec + 1)] * 2
    xy = np.stack(np.meshgrid(*space, indexing="ij"), axis=-1).reshape((-1, 2))
    disp = np.concatenate([xy, np.zeros((xy.shape[0], 1))], axis=1) @ latvec
    if gidx is None:
        gpoints, gnorm, gweight, gidx = slab_gpoints(gmax, recvec, latvec, alpha, cell_area)
    else:
        gidx = np.ascontiguousarray(np.reshape(gidx, (-1, 2)), dtype=np.int32)
        gpoints = gidx @ (recvec[:2] * 2 * np.pi)
        gnorm = np.linalg.norm(gpoints, axis=-1)
        gweight = 2 * np.pi * erfc(gnorm / (2 * alpha)) / (cell_area * gnorm)
    sum_gweight = np.sum(gweight)
    self_const = -alpha / np.sqrt(np.pi) + sum_gweight - np.sqrt(np.pi) / (cell_area * alpha)
    tab = {
        "alpha": float(alpha), "cell_area": float(cell_area), "latvec": latvec, "lattice_displacements": np.ascontiguousarray(disp),
        "gpoints": np.ascontiguousarray(gpoints), "gnorm": np.ascontiguousarray(gnorm), "gweight": np.ascontiguousarray(gweight),
        "gidx": gidx, "recip": np.ascontiguousarray(recvec[:2] * 2 * np.pi),  # gpoints == gidx @ recip
        "kpref": np.ascontiguousarray(np.pi / (cell_area * gnorm) * np.exp(-((gnorm / (2 * alpha)) ** 2))),
        "sum_gweight": float(sum_gweight), "self_const": float(self_const),
        "atom_coords": np.ascontiguousarray(coords), "atom_charges": np.ascontiguousarray(charges),
    }
    ii = self_const * np.sum(charges**2)
    if len(charges) > 1:  # (one atom: only the self term, ewald2d.py:124-126)
        d, ij = MinimalImageDistance(latvec).dist_matrix(coords[np.newaxis])
        qq = np.prod(charges[np.asarray(ij)], axis=1)
        ii = ii + float(qq @ pair_sum(tab, d[0]))
    tab["ii"] = float(ii)
    return tab


def pair_sum(tab, d):
    """real + 2 sum_k cos(k.d) W(k, z) + 2 W_0(z) of the displacements d (..., 3) -> (...,)."""
    alpha, area = tab["alpha"], tab["cell_area"]
    z = d[..., 2]
    rec = (np.cos(d @ tab["gpoints"].T) * recip_weight(z, tab["gnorm"], alpha, area)).sum(axis=-1)
    return real_cij(d, tab["lattice_displacements"], alpha) + 2 * rec + 2 * charge_weight(z, alpha, area)


def device_ewald2d(dev, tab, mean=False, walker_chunk=0):
    """``pqa_ewald2d`` on a device handle: (ee, ei) of the resident walkers, each (W,), or the two walker means with ``mean``."""
    kn = np.ascontiguousarray(tab["gidx"], dtype=np.int32).reshape(-1, 2)
    knorm, kpref = _ffi.f64(tab["gnorm"]), _ffi.f64(tab["kpref"])
    lat = _ffi.f64(tab["lattice_displacements"]).reshape(-1, 3)
    xyz, q = _ffi.f64(tab["atom_coords"]).reshape(-1, 3), _ffi.f64(tab["atom_charges"])
    t = _ffi.Ewald2dTab(alpha=tab["alpha"], area=tab["cell_area"], self_const=tab["self_const"], nk=kn.shape[0], kn=_ffi.ptr(kn),
                        knorm=_ffi.ptr(knorm), kpref=_ffi.ptr(kpref), recip=(C.c_double * 6)(*np.ravel(tab["recip"])),
                        nlat=lat.shape[0], lat=_ffi.ptr(lat), nion=xyz.shape[0], ion_xyz=_ffi.ptr(xyz), ion_charge=_ffi.ptr(q),
                        walker_chunk=int(walker_chunk))
    shape = (1,) if mean else (dev.W,)
    ee, ei = np.empty(shape), np.empty(shape)
    dev.call("pqa_ewald2d", C.byref(t), int(bool(mean)), _ffi.ptr(ee), _ffi.ptr(ei))
    return (float(ee[0]), float(ei[0])) if mean else (ee, ei)


class Ewald:
    """``pyqmc.observables.ewald2d.Ewald``: ``energy(configs, wf=None) -> (ee, ei, ii)``, ee and ei per walker.

    cell: provides ``lattice_vectors()``, ``atom_coords()``, ``atom_charges()``; the first two lattice vectors span the periodic
    plane.  gmax, nlatvec, alpha_scaling: as the reference's; gidx: see ``ewald2d_tables``."""

    host_chunk_bytes = 64 << 20  # bound of the host route's (walkers, pairs, nk) temporaries

    def __init__(self, cell, gmax=200, nlatvec=1, alpha_scaling=5.0, gidx=None):
        self.tab = t = ewald2d_tables(cell, gmax=gmax, nlatvec=nlatvec, alpha_scaling=alpha_scaling, gidx=gidx)
        self.latvec, self.atom_coords, self.atom_charges = t["latvec"], t["atom_coords"][np.newaxis], t["atom_charges"]
        self.dist = MinimalImageDistance(self.latvec)
        self.cell_area, self.alpha = t["cell_area"], t["alpha"]
        self.lattice_displacements = t["lattice_displacements"]
        self.gpoints, self.gweight, self.gnorm, self.sum_gweight = t["gpoints"], t["gweight"], t["gnorm"], t["sum_gweight"]
        self.ewald_ion_ion = t["ii"]
        self.last_route = None

    def ewald_self(self, sum_charge_squared):
        return self.tab["self_const"] * sum_charge_squared

    def _fused(self, configs, wf):
        dev = None if wf is None else device_handle(wf)
        x = configs.configs
        if dev is None or not dev.pbc or sum(dev.nelec) != x.shape[1] or dev.W != x.shape[0]:
            return None
        # the handle's resident walkers are `configs` (the drivers fetch them from the device before any host accumulator)
        return dev

    def _host(self, x):
        W, N = x.shape[:2]
        natom = self.atom_coords.shape[1]
        per_walker = 8 * 6 * (N * (N - 1) // 2 + N * natom) * max(len(self.gnorm), 1)
        step = max(1, int(self.host_chunk_bytes // max(per_walker, 1)))
        ee, ei = np.empty(W), np.empty(W)
        for w0 in range(0, W, step):
            c = x[w0 : w0 + step]
            ee[w0 : w0 + step] = self.ewald_self(N)
            if N > 1:  # (one electron: only the self term, ewald2d.py:225-226)
                d, _ = self.dist.dist_matrix(c)
                ee[w0 : w0 + step] += pair_sum(self.tab, d).sum(axis=-1)
            d = self.dist.pairwise(self.atom_coords, c)  # (chunk, natoms, nelec, 3)
            ei[w0 : w0 + step] = -(pair_sum(self.tab, d).sum(axis=-1) * self.atom_charges).sum(axis=-1)
        return ee, ei

    def energy(self, configs, wf=None, mean=False):
        """(ee, ei, ii); ``mean``: the walker means of ee and ei instead of the per-walker arrays."""
        dev = self._fused(configs, wf)
        if dev is not None:
            self.last_route = "fused"
            ee, ei = device_ewald2d(dev, self.tab, mean=mean)
        else:
            self.last_route = "host"
            ee, ei = self._host(np.asarray(configs.configs, dtype=float))
            if mean:
                ee, ei = float(ee.mean()), float(ei.mean())
        return ee, ei, self.ewald_ion_ion


class SlabEnergyAccumulator:
    """Local energy of a slab: ``ke``, ``ecp`` and ``grad2`` of an ``EnergyAccumulator``, ``ee`` and ``ei`` from the slab Ewald sum,
    ``total = ke + ecp + ee + ei + ii``.  It holds the ``EnergyAccumulator`` by composition and is deliberately no subclass: the
    drivers select their fused energy pass (with the 3D sums) by ``isinstance(., EnergyAccumulator)``, so here ``pyqmc_amd.vmc``
    runs it as a host-called accumulator after each device sweep, and ``pyqmc_amd.rundmc`` refuses it.

    kwargs: ``gmax``, ``nlatvec``, ``alpha_scaling`` of the slab sum; ``energy``: the wrapped accumulator (default
    ``EnergyAccumulator(cell, **rest)``)."""

    def __init__(self, cell, energy=None, **kwargs):
        slab = {k: kwargs.pop(k) for k in ("gmax", "nlatvec", "alpha_scaling") if k in kwargs}
        self.ewald = Ewald(cell, **slab)
        self.energy = EnergyAccumulator(cell, **kwargs) if energy is None else energy
        self.mol = cell

    @property
    def last_route(self):
        return self.ewald.last_route

    def _assemble(self, base, ee, ei):
        out = dict(base)
        out["ee"], out["ei"] = ee, ei
        out["total"] = out["ke"] + out["ecp"] + ee + ei + self.ewald.ewald_ion_ion
        return out

    def __call__(self, configs, wf):
        ee, ei, _ = self.ewald.energy(configs, wf)
        return self._assemble(self.energy(configs, wf), ee, ei)

    def avg(self, configs, wf):
        ee, ei, _ = self.ewald.energy(configs, wf, mean=True)
        return self._assemble({k: np.mean(v, axis=0) for k, v in self.energy(configs, wf).items()}, ee, ei)

    def nonlocal_tmoves(self, configs, wf, e, tau, **kw):
        return self.energy.nonlocal_tmoves(configs, wf, e, tau, **kw)

    def has_nonlocal_moves(self):
        return self.energy.has_nonlocal_moves()

    def keys(self):
        return set(KEYS)

    def shapes(self):
        return {k: () for k in KEYS}
