"""Shared code of the ECP-shape tests (test_ecp_shapes_cpu.py, test_gpu_ecp_shapes.py, golden/make_golden_ecp_shapes.py): the cases of
tests/sweep_shapes.py (f-shell bases, n_up != n_dn, an empty spin channel, more than 32 atoms, uneven orbital-tile counts) and the two
ill-conditioned water cases of tests/conditioning.py with a pseudopotential table under which EVERY species has a non-local channel that
counts, ECP tapes, and the oracle's ECP row (oracle.energy.ecp_ea) with what a device row is measured in.  Plain module, no GPU.

The project's hydrogen (and helium) table has a non-local channel with coefficient 0: the point lists of a hydrogen-only system are built
and its Slater ratios computed, then multiplied by zero — its ECP row is the local channel alone (test_ecp_shapes_cpu.py pins that).
``ECP`` is the project's table with the hydrogen l = 0 term [[1.0, 0.5]] (v_0 = 0.5 exp(-r^2), range ~7 bohr at the 1e-22 cut of
pqa_create.hip); O and C keep theirs, so the periodic (carbon-only) cases are unchanged.  systems.py is untouched.

A device row is measured as max_w |dev - oracle| / max(1, A_w) with A_w = sum |ratio| |v_l| |P_l| + sum |v_local|, the absolute sum of
the walker's terms: the row is a cancelling sum (|row| / A_w goes down to 9e-4 on these cases).  The yardstick of a case is, in that
measure, the largest of (a) the oracle's row on its updated state after its chain against its fresh row, (b) the oracle's row with the
occupied columns permuted against the unpermuted one, (c) cond(D) * 2.2e-16 — the ECP counterpart of sweep_shapes.yardstick, from the
oracle only, taken at the oracle chain's final coordinates on the mask of threshold 10 (the deterministic mask of the 36-atom grids costs
the oracle 3 - 6 s a pass and gives the same figures: h36 (a) 2.07e-15 against 2.09e-15, (b) 3.0e-16 against 3.7e-16).
"""

import copy
import functools

import numpy as np

import conditioning as cond
import helpers
import sweep_shapes as ss
from pyqmc_amd import systems

EPS = ss.EPS
TAPE_SEED = 21
THRESHOLDS = (-1.0, 10.0)  # the deterministic mask (every point) and the stochastic one of the default threshold
YARDSTICK_THRESHOLD = 10.0
FIXTURE = "g53_ecp_shapes"
_H = systems._ECP["H"]
ECP = dict(systems._ECP, H=(_H[0], [_H[1][0], [0, [[], [], [[1.0, 0.5]]]]]))

OPEN_CASES, MD_CASES, PBC_CASES = tuple(ss.OPEN_CASES), tuple(ss.MD_CASES), tuple(ss.PBC_CASES)
COND_CASES = ("water-1e-5", "water-1e-7")  # conditioning.CASES: cond(D) 3e6 and 3e8 after their 100-sweep chain
LIVE_CASES = OPEN_CASES + MD_CASES
HYDROGEN_CASES = tuple(n for n in OPEN_CASES if set(ss.case(n).mol._names) == {"H"})
ONE_ELECTRON = ("h-atom", "h-atom-df")
# c2-high-l-md: two carbon cores whose l = 0 term (52 exp(-7.8 r^2)) selects within ~1 bohr, and eight electrons of random orbitals: the
# pass probabilities of its walkers at threshold 10 leave several of them without a point whatever the seed (at the final coordinates the
# chance of none is 0.63 .. 0.99 for seven of the 13 walkers: all 13 draw a point once in 1e8 seeds; seeds 21 .. 29 tried).  Its
# condition at threshold 10 is therefore the one-electron cases': walkers with and walkers without points.
SPARSE = ("c2-high-l-md",)
RANGE_CASES = ("h36", "h36-1917", "h33s", "h33s-1917")  # grids wider than the hydrogen table's range
TERM_CUT, TERM_SEEN = 1e-22, 1e-20  # an atom is out of range where all its terms are below the first; the device must see one above the second


def with_table(mol, table=None):
    """``mol`` rebuilt by ``systems.Mol(..., ecp=table)`` (default: the test table).  Nothing else of it changes."""
    return systems.Mol(mol._names, mol._coords, nelec=mol.nelec, basis=mol._basis, ecp=ECP if table is None else table, charges=mol._q)


@functools.lru_cache(maxsize=None)
def case(name):
    """The case of sweep_shapes / conditioning with the test table on both sides (``Case.oracle_wf`` / ``gpu_wf`` build from ``mol``)."""
    c = copy.copy(cond.case(name) if name in COND_CASES else ss.case(name))
    if not c.periodic:  # (the periodic cells hold carbon only: their table is the project's)
        c.mol = with_table(c.mol)
    return c


def necp(mol):
    from oracle import energy as oen

    return len(oen.ecp_atoms(mol))


@functools.lru_cache(maxsize=None)
def ecp_tapes(name, seed=TAPE_SEED):
    """Rotations (ns, N, necp, 3, 3) and mask uniforms (ns, N, necp, W) of a case, one step per sweep: the layout
    ``vmc_sweeps(ecp_rot=, ecp_unif=)`` replays, one step of it what ``energy(rot=, unif=)`` takes.  The walker-major evaluations at the
    start coordinates take step 0, the evaluations behind the sweeps end on step ns - 1."""
    c = case(name)
    N, k = int(np.sum(c.mol.nelec)), necp(c.mol)
    rng = np.random.default_rng(seed)
    return helpers.rotations(rng, c.ns, N, k), rng.random((c.ns, N, k, c.W))


def _largest_term(mol, ia, r):
    """(W,) the largest |c| r^n exp(-a r^2) over every term of every channel of atom ``ia`` (what pqa_create.hip's range is cut by)."""
    from oracle import energy as oen

    out = np.zeros(len(r))
    for n, a, c in oen.ecp_channels(mol._ecp[mol.atom_pure_symbol(ia)]):
        if len(c):
            out = np.maximum(out, np.max(np.abs(c) * r[:, None] ** n * np.exp(-a * r[:, None] ** 2), axis=1))
    return out


def ecp_parts(mol, cfg, owf, threshold, rot, unif):
    """The ECP row of ``owf``'s CURRENT state at ``cfg`` (oracle.energy.ecp_ea per electron and atom; rot (N, necp, 3, 3), unif
    (N, necp, W)), per walker: ``row``, ``local``, ``points`` = sum mask * naip, ``points_seen`` (the same over the pairs with a term
    above 1e-20), ``A`` = sum |ratio| |v_l| |P_l| + sum |v_local|; and over all walkers ``min_tie`` = min |prob - uniform|, ``pairs_out``
    / ``pairs_in``: the (walker, electron, atom) triples whose every term is below 1e-22 / that have one above."""
    from oracle import energy as oen

    x = cfg.configs
    W, N = x.shape[:2]
    row, local = np.zeros(W, dtype=getattr(owf, "dtype", float)), np.zeros(W)
    A, points, seen = np.zeros(W), np.zeros(W, dtype=np.int64), np.zeros(W, dtype=np.int64)
    tie, n_out, n_in = np.inf, 0, 0
    for e in range(N):
        for k, ia in enumerate(oen.ecp_atoms(mol)):
            d = oen.ecp_ea(mol, cfg, owf, e, ia, threshold, rot[e, k], unif[e, k])
            m, naip = d["mask"], d["P_l"].shape[1]
            row += d["total"]
            local += d["local"]
            A += np.abs(d["local"])
            A[m] += np.einsum("ij,ik,ijk->i", np.abs(d["ratio"]), np.abs(d["v_l"]), np.abs(d["P_l"]))
            r_vec = x[:, e, :] - np.asarray(mol.atom_coords()[ia])
            if hasattr(mol, "a"):
                from oracle.pbc import minimal_image

                r_vec = minimal_image(mol.lattice_vectors())(r_vec)
            big = _largest_term(mol, ia, np.linalg.norm(r_vec, axis=-1))
            points += m * naip
            seen += (m & (big > TERM_SEEN)) * naip
            n_out, n_in = n_out + int((big < TERM_CUT).sum()), n_in + int((big >= TERM_CUT).sum())
            if threshold > 0:
                tie = min(tie, float(np.min(np.abs(d["prob"] - unif[e, k]))))
    return {"row": row, "local": local, "nonlocal": row - local, "A": A, "points": points, "points_seen": seen, "min_tie": tie,
            "pairs_out": n_out, "pairs_in": n_in}


def oracle_ecp(c, cfg, threshold, rot, unif, mf=None, dets=None, mol=None):
    """``ecp_parts`` on a freshly recomputed oracle wave function of case ``c`` at ``cfg`` (``mf`` / ``dets``: another mean field /
    determinant list of the same wave function; ``mol``: the same molecule with another table)."""
    owf = c.oracle_wf(mf, dets)
    owf.recompute(cfg.copy())
    return ecp_parts(c.mol if mol is None else mol, cfg.copy(), owf, threshold, rot, unif)


def measure(row, o):
    """max_w |row - oracle row| / max(1, A_w)."""
    return float(np.max(np.abs(np.asarray(row) - o["row"]) / np.maximum(1.0, o["A"])))


def measure_pair(a, b, o):
    """Two device rows at the same coordinates against each other, in the same measure."""
    return float(np.max(np.abs(np.asarray(a) - np.asarray(b)) / np.maximum(1.0, o["A"])))


def oracle_chain(name):
    """The oracle's chain of a case on its sweep tapes, without energies -> (the wave function in its UPDATED state, final configs)."""
    from oracle import vmc as ovmc

    if name in COND_CASES:  # (the chain does not read the table: conditioning's own run)
        r = cond.oracle_run(name)
        return r["owf"], r["cfg"]
    c = case(name)
    start, gauss, unif, tstep = c.tapes()
    owf = c.oracle_wf()
    emol = copy.copy(c.mol)
    emol._ecp = {}
    _, cfg = ovmc.vmc_worker(emol, owf, start, tstep, gauss, unif, with_energy=False)
    return owf, cfg


def slater_cond(c, cfg):
    """max over walkers, spins and unique determinants of cond(D), from the oracle's Slater matrices at ``cfg``."""
    fn = cond.oracle_slater_matrices(c.oracle_wf())
    return float(max(np.linalg.cond(fn(cfg, s)).max() for s in (0, 1) if c.mol.nelec[s]))


_at = {}


def oracle_at(name, x, threshold, step, wrap=None):
    """``oracle_ecp`` of a case at the coordinates ``x`` on step ``step`` of its ECP tapes, computed once per process and coordinates."""
    c = case(name)
    key = (name, float(threshold), int(step), np.ascontiguousarray(x).tobytes(), None if wrap is None else np.ascontiguousarray(wrap).tobytes())
    if key not in _at:
        rot, unif = ecp_tapes(name)
        _at[key] = oracle_ecp(c, c.configs(x, wrap) if c.periodic else c.configs(x), threshold, rot[step], unif[step])
    return _at[key]


@functools.lru_cache(maxsize=None)
def compute_yardstick(name):
    """-> {"updated": (a), "permuted": (b), "cond": cond(D), "yardstick": max((a), (b), cond * eps), "x" (and "wrap"): the chain's final
    coordinates}, on the mask of YARDSTICK_THRESHOLD and the last step of the ECP tapes."""
    c = case(name)
    owf, cfg = oracle_chain(name)
    x, wrap = np.array(cfg.configs), np.array(cfg.wrap) if c.periodic else None
    rot, unif = (t[-1] for t in ecp_tapes(name))
    fresh = oracle_at(name, x, YARDSTICK_THRESHOLD, c.ns - 1, wrap)
    upd = ecp_parts(c.mol, cfg.copy(), owf, YARDSTICK_THRESHOLD, rot, unif)
    mf, dets = c.permuted(1)
    perm = oracle_ecp(c, cfg, YARDSTICK_THRESHOLD, rot, unif, mf, dets)
    out = {"updated": measure(upd["row"], fresh), "permuted": measure(perm["row"], fresh), "cond": slater_cond(c, cfg), "x": x}
    out["yardstick"] = max(out["updated"], out["permuted"], out["cond"] * EPS)
    if c.periodic:
        out["wrap"] = wrap
    return out


# the fixture's keys: per threshold tag "<case>/<tag>/<key>", and "<case>/yardstick", ".../updated", ".../permuted", ".../cond"
PBC_KEYS = ("row", "local", "A", "points", "points_seen")


def tag(threshold):
    return "det" if threshold <= 0 else "thr10"


def compute_pbc_case(name):
    """What the fixture holds of a periodic case: the yardstick and, per threshold, the fresh oracle's row, local part, A and point count
    at the coordinates and wrap counters g52 stores (the oracle chain's final ones), on step 0 of the ECP tapes."""
    y = compute_yardstick(name)
    g = ss.oracle_case(name)
    assert np.array_equal(y["wrap"], g["wrap"]) and np.max(np.abs(y["x"] - g["x"])) < 1e-9  # the chain g52 was recorded from
    out = {f"{name}/{k}": y[k] for k in ("yardstick", "updated", "permuted", "cond")}
    for thr in THRESHOLDS:
        o = oracle_at(name, g["x"], thr, 0, g["wrap"])
        out.update({f"{name}/{tag(thr)}/{k}": o[k] for k in PBC_KEYS})
    return out


def yardstick(name):
    """The yardstick of a case: computed once per process (open, multi-determinant and conditioning cases) or read from the fixture."""
    if name in PBC_CASES:
        return float(helpers.golden(FIXTURE)[f"{name}/yardstick"])
    return compute_yardstick(name)["yardstick"]


def pbc_oracle(name, threshold):
    g = helpers.golden(FIXTURE)
    return {k: g[f"{name}/{tag(threshold)}/{k}"] for k in PBC_KEYS}


# ---------------------------------------------------------------- the batched integrator (oracle/ecp_batched.py)
BATCHED_CASES = ("water-f-53", "w4f-1715", "h33s-1917")
BATCHED_SEED, BATCHED_TAU = 22, 0.02


def batched_rule(mol):
    """(naip per ECP atom, nselect_deterministic, nselect_random) of ``EnergyAccumulator(use_old_ecp=False)``: the reference's defaults
    (jax_ecp.py:43-69) — six points an atom here, the six likeliest kept and one of the others sampled."""
    from oracle import ecp_batched as ob

    naip = ob.default_naip(mol)
    nsd = int(naip.max())
    return naip, nsd, max(min(1, int(naip.sum()) - nsd), 0)


@functools.lru_cache(maxsize=None)
def batched_tapes(name):
    """Rotations (N, necp, 3, 3) and selection uniforms (N, W, nselect_random) of the energy, and the same per electron for the T-move
    tables (rotations (N, necp, 3, 3), uniforms (N, W, nselect_random): electron e takes its own row)."""
    c = case(name)
    N, k, nsr = int(np.sum(c.mol.nelec)), necp(c.mol), batched_rule(c.mol)[2]
    rng = np.random.default_rng(BATCHED_SEED)
    return helpers.rotations(rng, N, k), rng.random((N, c.W, nsr)), helpers.rotations(rng, N, k), rng.random((N, c.W, nsr))


def tmove_electrons(mol):
    """The first and the last electron of each spin."""
    nup, ndn = mol.nelec
    return sorted({0, nup - 1, nup, nup + ndn - 1})


_batched = {}


def batched_at(name, x):
    """The batched integrator of the oracle on a fresh wave function at ``x`` -> {"row", "local", "A" (sum |ratio| |v_l P_l| + sum
    |v_local| per walker), "tmoves": {e: (weight (W, P), positions (W, P, 3), sum_l |e^{-tau v_l} - 1| P_l (W, P))}}."""
    from oracle import ecp_batched as ob

    key = (name, np.ascontiguousarray(x).tobytes())
    if key in _batched:
        return _batched[key]
    c = case(name)
    cfg = c.configs(x)
    owf = c.oracle_wf()
    owf.recompute(cfg.copy())
    naip, nsd, nsr = batched_rule(c.mol)
    rot, unif, tm_rot, tm_unif = batched_tapes(name)
    W, N = x.shape[:2]
    row, local, A = np.zeros(W), np.zeros(W), np.zeros(W)
    for e in range(N):  # ecp_batched.ecp with the absolute sum beside it
        epos, vl, pl, loc, prob = ob.selected(c.mol, cfg, e, naip, nsd, nsr, rot[e], unif[e])
        ratio = owf.testvalue(e, cfg.make_irreducible(e, epos))[0]
        row += loc
        row += np.einsum("na,nal->n", ratio, vl[:, :, :-1])
        local += loc
        A += np.abs(loc) + np.einsum("na,nal->n", np.abs(ratio), np.abs(vl[:, :, :-1]))
    assert np.array_equal(row, ob.ecp(c.mol, cfg, owf, naip, nsd, nsr, rot, unif))
    tm = {}
    for e in tmove_electrons(c.mol):  # ecp_batched.tmoves without the ratios (the device entry returns weights and positions)
        epos, vl, pl, _, _ = ob.selected(c.mol, cfg, e, naip, nsd, nsr, tm_rot[e], tm_unif[e])
        ew = np.zeros_like(pl)
        m = pl > 0
        ew[m] = np.exp(-BATCHED_TAU * vl[m] / pl[m]) - 1
        tm[e] = (np.einsum("ijk,ijk->ij", ew, pl), epos, np.einsum("ijk,ijk->ij", np.abs(ew), pl))
    _batched[key] = {"row": row, "local": local, "A": A, "tmoves": tm}
    return _batched[key]
