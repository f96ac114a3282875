"""Shared code of the sweep-shape tests (test_sweep_shapes_cpu.py, test_gpu_sweep_shapes.py, golden/make_golden_sweep_shapes.py): a short,
fixed list of small systems, each built to reach one line of the fused sweeps that no other system of the suite reaches — the LMAX = 3
instantiations (a basis whose highest shell is f), n_up != n_dn, an empty spin channel, different orbital-tile counts per spin, more
than 32 atoms, a species whose atoms fill one work item and part of another, the default route of 16 .. 31 electrons per spin — and the
oracle side of every case.  Plain module, no GPU.  The helpers are those of tests/conditioning.py; ``ShapeCase`` is its ``Case`` with
other inputs, so both sides of a case are built and judged by the same code as the conditioning cases.

Orbitals are ``systems.random_mf`` (well conditioned: cond(D) 1 .. 1e3), Jastrow parameters those of ``helpers.oracle_wf``.  Open and
multi-determinant cases: 13 walkers (one full block of k_sweep_r8 and a partly filled one), 3 sweeps, sweep 1 forced; their oracle side
runs live (<= 3 s a chain) and is cached per case.  Periodic cases: 4 walkers, 2 sweeps, sweep 1 forced; their oracle side (~10 s a case)
is the committed fixture g52_sweep_shapes.npz.
"""

import copy
import functools

import numpy as np

import conditioning as cond
import helpers
from pyqmc_amd import systems

FIXTURE = "g52_sweep_shapes"
EPS = 2.2e-16
W, NS, FORCED = 13, 3, (1,)
PBC_W, PBC_NS = 4, 2
_F_O = [[3, [0.95, 1.0]]]
_F_C = [[3, [0.761, 1.0]]]
_S_H = [[0, [0.35, 1.0]]]  # h33s: one uncontracted s function per atom
_DF_H = [[2, [0.9, 1.0]], [3, [0.95, 1.0]]]  # h-atom-df: d and f functions behind the hydrogen table


def _water(f=False, nelec=None):
    sym, xyz = zip(*systems._WATER)
    basis = {"O": systems._O_BASIS + _F_O, "H": systems._H_BASIS} if f else None
    return systems.Mol(sym, xyz, nelec=nelec, basis=basis)


def _w4(f=False):
    m = systems.water_cluster(2, 2, 1)
    basis = {"O": systems._O_BASIS + _F_O, "H": systems._H_BASIS} if f else None
    return systems.Mol(m._names, m._coords, nelec=(17, 15), basis=basis)


def _h_grid(natom, nelec, basis=None):
    grid = np.array([(ix, iy, iz) for ix in range(3) for iy in range(3) for iz in range(4)], dtype=float) * 2.6
    xyz = grid + 0.3 * np.random.default_rng(2).standard_normal((36, 3))
    return systems.Mol(["H"] * natom, xyz[:natom], nelec=nelec, basis=basis)


# name -> (builder, nelec, natm, nao, highest l, tape seed): what test_sweep_shapes_cpu.py pins
OPEN_CASES = {
    "water-f": (lambda: _water(f=True), (4, 4), 3, 30, 3, 3),                 # LMAX 3 of r8 and res16; launch-per-move on f shells
    "water-53": (lambda: _water(nelec=(5, 3)), (5, 3), 3, 23, 2, 3),          # n_up != n_dn
    "water-f-53": (lambda: _water(f=True, nelec=(5, 3)), (5, 3), 3, 30, 3, 3),
    "h-atom": (lambda: systems.Mol(["H"], [(0.1, -0.2, 0.3)], nelec=(1, 0)), (1, 0), 1, 5, 1, 3),  # N = 1, empty spin channel
    # k_sweep_res takes no basis below 20 padded rows (res_setup, pqa_res.hip: `kt_cap < 20`; the hydrogen table has 5 AOs, one 16-row
    # chunk): through it N = 1 and the empty spin channel are hit by the same atom with a d and an f shell added (17 AOs, LMAX 3 as well)
    "h-atom-df": (lambda: systems.Mol(["H"], [(0.1, -0.2, 0.3)], nelec=(1, 0), basis={"H": systems._H_BASIS + _DF_H}), (1, 0), 1, 17, 3, 3),
    # natom > 32 (second ion pass), 4 full + 1 half item per shell type, two orbital tiles per spin
    "h36": (lambda: _h_grid(36, (18, 18)), (18, 18), 36, 180, 1, 3),
    "h36-1917": (lambda: _h_grid(36, (19, 17)), (19, 17), 36, 180, 1, 3),
    # The same grid cut to what k_sweep_r8's 80 KB of LDS take beside its two-tile partials (59 136 B): r8_setup refuses h36 at
    # `h->r8.lds > 80 * 1024` (86 224 B: every atom costs 61 doubles of Jastrow tables, every work item 272 B).  33 atoms with one s
    # function each is 81 904 B: still natom > 32 (nion = 2 and the Ic clamp of lanes 1 .. 31), 4 full items + 1 partial one, two tiles per
    # spin, default route = k_sweep_r8.  17 + 17 and not 17 + 16: a spin with one tile has KW = 4 and larger partials (61 184 B).
    "h33s": (lambda: _h_grid(33, (17, 17), {"H": _S_H}), (17, 17), 33, 33, 0, 3),
    "h33s-1917": (lambda: _h_grid(33, (19, 17), {"H": _S_H}), (19, 17), 33, 33, 0, 3),
    "w4-1715": (lambda: _w4(), (17, 15), 12, 92, 2, 3),                       # nt = (2, 1), half-filled O items, default route = r8
    "w4f-1715": (lambda: _w4(f=True), (17, 15), 12, 120, 3, 3),               # LMAX 3 together with nt = (2, 1)
}
# (case, route) pairs outside the route's scope -> the case that hits the same line through that route.  h36 / h36-1917 run k_sweep_res
# and the launch-per-move sweep, h-atom k_sweep_r8 and the launch-per-move sweep; the replacements run all three routes.
REPLACEMENT = {("h36", "r8"): "h33s", ("h36-1917", "r8"): "h33s-1917", ("h36", "default"): "h33s", ("h-atom", "res16"): "h-atom-df"}
DEFAULT_ROUTE_CASES = ("h36", "w4-1715")  # 16 .. 31 electrons per spin with no switch set: k_sweep_r8 by r8_plan
MD_CASES = {
    "water-f-md": (lambda: _water(f=True), (4, 4), 3, 30, 3, 3),              # k_sweep_ww<3>
    "c2-high-l-md": (systems.carbon_dimer_high_l, (4, 4), 2, 98, 5, 3),      # k_sweep_ww<5>
}
# name -> ((carbon table, random_kmf keywords), nelec, natm, nao, highest l, tape seed)
PBC_CASES = {
    "cubic-f": ((systems._C_BASIS + _F_C, {}), (16, 16), 8, 160, 3, 3),       # k_sweep_res<., 3, PBC>
    # k_sweep_res<., 3, PBC, CX>.  A twisted cell's tile holds the real and the imaginary AO rows, 2 nao, of which res_setup (pqa_res.hip)
    # takes at most 256 (`rows4 <= rows_cap`, two tiles of 16 complex orbitals) and 80 * rows * 8 B within its 160 KB of LDS: the 160 AOs
    # of cubic-f are 320 rows.  The carbon table without its second p and its d shell (s, s, p, f: 96 AOs, 192 rows) is inside.
    "c3-f": ((systems._C_BASIS[:3] + _F_C, {"complex_coeff": True, "twist": helpers.TWIST_CASES["prim"][1]}), (16, 16), 8, 96, 3, 3),
}
ALL_CASES = tuple(OPEN_CASES) + tuple(MD_CASES) + tuple(PBC_CASES)


def table(name):
    """(nelec, natm, nao, highest l, tape seed) of a case as the tables above state them."""
    return (OPEN_CASES.get(name) or MD_CASES.get(name) or PBC_CASES[name])[1:]


class ShapeCase(cond.Case):
    """``conditioning.Case`` (builders of both sides, tapes, judge) with the inputs of a case of this module."""

    def __init__(self, name):
        from pyqmc_amd import pbc

        self.name, self.dets, self.three, self.periodic, self.complex = name, None, False, name in PBC_CASES, False
        self.seed = table(name)[4]
        self.W, self.ns, self.forced = (PBC_W, PBC_NS, FORCED) if self.periodic else (W, NS, FORCED)
        if name in OPEN_CASES:
            self.mol = OPEN_CASES[name][0]()
            self.mf = systems.random_mf(self.mol)
        elif name in MD_CASES:
            self.mol = MD_CASES[name][0]()
            self.mf = systems.random_mf(self.mol, nvirt=6)
            self.dets = cond.DETS_ALL_ILL
        else:
            basis, kws = PBC_CASES[name][0]
            p = systems.diamond_primitive()
            prim = systems.Cell(p._names, p._coords, p.a, basis={"C": basis})
            self.mol = pbc.get_supercell(prim, helpers.PBC_SLATER_CASES["fcc2cubic"])
            self.mf = pbc.random_kmf(self.mol, **kws)
            self.complex = bool(kws)

    def permuted(self, seed):
        """``Case.permuted``; with n_up != n_dn the OCCUPIED columns of each spin in another order (``conditioning.permuted_mf`` permutes
        all max(n_up, n_dn) columns of both spins, which moves an unoccupied column of the smaller spin among its occupied ones: another
        wave function)."""
        nup, ndn = self.mol.nelec
        if self.periodic or self.dets is not None or nup == ndn:
            return super().permuted(seed)
        r = np.random.default_rng(seed)
        mo = np.array(self.mf.mo_coeff)
        for s, n in enumerate((nup, ndn)):
            mo[s][:, :n] = mo[s][:, r.permutation(n)]
        return systems.MeanField(mo, np.array(self.mf.mo_occ)), None

    def judge(self, inverse, phase, logpsi, cfg, mf=None, dets=None):
        """``Case.judge`` that skips an empty spin channel (the oracle's orbital evaluation does not take zero points)."""
        if min(self.mol.nelec) > 0:
            return super().judge(inverse, phase, logpsi, cfg, mf, dets)
        owf = self.oracle_wf(mf, dets)
        fn = cond.oracle_slater_matrices(owf)
        jast = owf.wf_factors[1].recompute(cfg.copy())[1]
        return cond.chain_errors(lambda c, s: fn(c, s) if self.mol.nelec[s] else np.zeros((len(c.configs), 1, 0, 0)), inverse, logpsi - jast, cfg)


@functools.lru_cache(maxsize=None)
def case(name):
    return ShapeCase(name)


def highest_l(mol):
    return max(int(sh[0]) for n in mol._names for sh in mol._basis[n])


def oracle_run(name, permuted=False):
    """One oracle chain of a case on its tapes (``permuted``: with the occupied columns in another order, ``Case.permuted(1)``) — the
    dictionary of ``conditioning.oracle_run``: decisions, margins, x (and wrap, psi_phase), the
    chain-error summary inv / log / q0m1 (/ phase), cond, cond_min, ke_upd_vs_fresh, grad2_upd_vs_fresh, acceptance (unforced sweeps)."""
    from oracle import energy as oen, vmc as ovmc

    c = case(name)
    mf, dets = c.permuted(1) if permuted else (c.mf, c.dets)
    dets = c.dets if dets is None else dets
    start, gauss, unif, tstep = c.tapes()
    owf = c.oracle_wf(mf, dets)
    N = gauss.shape[1]
    record, margins = [], []
    emol = copy.copy(c.mol)
    emol._ecp = {}
    _, cfg = ovmc.vmc_worker(emol, owf, start, tstep, gauss, unif, with_energy=False, record=record, margins=margins)
    inv, ph, logpsi = cond.oracle_state_all(owf)
    err = c.judge(inv, ph, logpsi, cfg, mf, dets)
    out = {"decisions": np.asarray(record).reshape(c.ns, N, c.W), "margins": np.asarray(margins).reshape(c.ns, N, c.W),
           "x": np.array(cfg.configs), "cond": float(err["cond"].max()), "cond_min": float(err["cond_min"].min()), **cond.summary(err)}
    if c.periodic:
        out["wrap"] = np.array(cfg.wrap)
    if c.complex:
        out["psi_phase"] = np.array(ph)
    ke_u, g2_u = oen.kinetic(cfg, owf)
    fresh = c.oracle_wf(mf, dets)
    fresh.recompute(cfg.copy())
    ke_f, g2_f = oen.kinetic(cfg.copy(), fresh)
    out["ke_upd_vs_fresh"], out["grad2_upd_vs_fresh"] = cond.rel_rows(ke_u, ke_f), cond.rel_rows(g2_u, g2_f)
    return out


SCALARS = ("inv", "log", "q0m1", "cond", "cond_min", "ke_upd_vs_fresh", "grad2_upd_vs_fresh", "min_margin", "acceptance", "spread_x")
PBC_KEYS = SCALARS + ("decisions", "margins", "x", "wrap", "x_permuted", "wrap_permuted", "decisions_equal_permuted")
COMPLEX_KEYS = ("psi_phase", "phase")


def combine(name, a, b):
    """The oracle side of a case from its run ``a`` and the run ``b`` with the occupied columns permuted."""
    c = case(name)
    out = dict(a)
    keep = np.ones(c.ns, dtype=bool)
    keep[list(c.forced)] = False
    out["min_margin"] = float(np.abs(a["margins"])[keep].min())
    out["acceptance"] = float(a["decisions"][keep].mean())
    out["decisions_equal_permuted"] = bool(np.array_equal(a["decisions"], b["decisions"]))
    out["spread_x"] = float(np.max(np.abs(a["x"] - b["x"])))
    out["x_permuted"] = b["x"]
    if c.periodic:
        out["wrap_permuted"] = b["wrap"]
    return out


def compute_case(name):
    return combine(name, oracle_run(name), oracle_run(name, permuted=True))


@functools.lru_cache(maxsize=None)
def oracle_case(name):
    """The oracle side of a case: computed once per process (open and multi-determinant cases) or read from the fixture (periodic)."""
    if name not in PBC_CASES:
        return compute_case(name)
    g = helpers.golden(FIXTURE)
    keys = PBC_KEYS + (COMPLEX_KEYS if case(name).complex else ())
    out = {k: (g[f"{name}/{k}"] if g[f"{name}/{k}"].ndim else g[f"{name}/{k}"].item()) for k in keys}
    out["decisions"] = out["decisions"].astype(bool)
    return out


def yardstick(o, key):
    """What a device figure is measured in: the oracle's own figure on the same chain, but not less than cond(D) * 2.2e-16 (cond(D) from
    the oracle's Slater matrices).  These chains are short and well conditioned: the oracle's own error can sit at one rounding while any
    backward-stable result may sit at cond * eps.  ``key`` "x": what two float64 oracle runs differ by, with no floor — except where
    the two runs are the same run (h-atom, h-atom-df: one orbital, no columns to permute, the difference is exactly 0), where it is
    cond * eps (= one rounding, cond(D) being 1) times the largest coordinate."""
    floor = o["cond"] * EPS
    if key == "x":
        return o["spread_x"] if o["spread_x"] > 0 else floor * float(np.max(np.abs(o["x"])))
    return max(o.get(key, 0.0), floor)
