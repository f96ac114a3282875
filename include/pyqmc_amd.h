/* pyqmc_amd — C ABI of the MI355X (gfx950) walker-batched trial-wave-function evaluator.
 *
 * The reference (WagnerGroup/pyqmc 0.8.0) has NO FFI: its boundary is the duck-typed
 * Python wave-function protocol (doc/source/wavefunction.rst:5-40).  Each entry point
 * below names the reference method it stands in for; pyqmc_amd/wf.py binds them with
 * ctypes behind classes with the reference's names (Slater, JastrowSpin, MultiplyWF),
 * and INTEGRATION.md shows the stub a pyqmc maintainer would add.
 *
 * Conventions
 *  - return 0 = ok, <0 = error (text via pqa_last_error).
 *  - every buffer is caller-owned, C-contiguous fp64 unless typed otherwise, and may be a
 *    host pointer OR a device pointer (copies use hipMemcpyDefault).  No pointer is
 *    retained after the call returns.
 *  - walker indices (widx) are checked against the walker count by every entry that takes
 *    them, host or device pointer, before anything is launched; an index outside is an error.
 *  - one handle = one walker shard on one device, one HIP stream, not re-entrant
 *    (same as the reference objects, which hold mutable per-walker state).
 *  - electrons are ordered all spin-up then all spin-down (slater.py:236-239).
 */
#ifndef PYQMC_AMD_H
#define PYQMC_AMD_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct pqa_handle pqa_handle_t;

/* Flat description of a Slater-Jastrow trial wave function (all pointers: host memory). */
typedef struct {
  /* geometry */
  int32_t natom;
  int32_t nelec_up, nelec_dn;
  const double* atom_xyz;    /* natom*3, bohr */
  const double* atom_charge; /* natom, valence charges (energy.py:40-45) */
  /* contracted GTO shells in AO order (numba/gto.py:435-470); coefficients already
     normalised (gto.py:375-405) */
  int32_t nshell, nprim, nao;
  const int32_t* shell_atom;     /* nshell */
  const int32_t* shell_l;        /* nshell, l <= 5 (twisted cells: l <= 3) */
  const int32_t* shell_prim_off; /* nshell+1 */
  const int32_t* shell_ao_off;   /* nshell */
  const double* prim_exp;        /* nprim */
  const double* prim_coef;       /* nprim */
  /* molecular orbitals, row-major [ao][mo] (orbitals.py:56-60), truncated to used columns */
  int32_t nmo_up, nmo_dn;
  const double* mo_up;
  const double* mo_dn;
  /* determinant expansion packed like determinant_tools.create_packed_objects (:39-71) */
  int32_t ndet, ndet_up, ndet_dn;
  const double* det_coeff;   /* ndet */
  const int32_t* det_occ_up; /* ndet_up*nelec_up */
  const int32_t* det_occ_dn; /* ndet_dn*nelec_dn */
  const int32_t* det_map;    /* 2*ndet */
  /* two-body Jastrow (jastrowspin.py:31-54); basis kinds: 0 = PolyPade(beta), 1 = CutoffCusp(gamma)
     (func3d.py:52-210) */
  int32_t na, nb; /* 0/0 = no Jastrow factor */
  const int32_t* a_kind;
  const double* a_param;
  const int32_t* b_kind;
  const double* b_param;
  double rcut_a, rcut_b;
  const double* acoeff; /* natom*na*2 */
  const double* bcoeff; /* nb*3 */
  /* semi-local ECPs (eval_ecp.py:149-200).  Channels of ECP atom k are
     [ecp_chan_off[k], ecp_chan_off[k+1]): non-local l = 0,1,.. first, LOCAL channel last
     (the reference's v_l column order).  Terms: sum coef * r^n * exp(-exp r^2). */
  int32_t necp;
  const int32_t* ecp_atom;     /* necp: atom index */
  const int32_t* ecp_chan_off; /* necp+1 */
  const int32_t* ecp_term_off; /* nchan_total+1 */
  const int32_t* ecp_term_n;
  const double* ecp_term_exp;
  const double* ecp_term_coef;
  int32_t has_slater; /* 0: Jastrow-only handle */
  /* three-body (electron-electron-ion) Jastrow (three_body_jastrow.py:19-63): its own a/b radial bases and
     ccoeff (natom, na3, na3, nb3, 3) as stored in wf.parameters["ccoeff"] (symmetrised in k,l by the library,
     :94-96).  na3 = 0: no three-body factor. */
  int32_t na3, nb3;
  const int32_t* a3_kind;
  const double* a3_param;
  const int32_t* b3_kind;
  const double* b3_param;
  double rcut_a3, rcut_b3;
  const double* ccoeff;
  /* periodic boundary conditions (PeriodicConfigs coord.py:137-252, MinimalImageDistance distance.py:83-159).
     pbc = 0: open system.  1: lattice vectors mutually orthogonal — displacements are folded in fractional
     coordinates (diagonal_dist / orthogonal_dist, :143-159).  2: general cell — fold, then argmin over the 27
     neighbouring cells (general_dist, :129-141).  Walker positions handed to the library are expected inside
     the cell (enforce_pbc, pbc/pbc.py:18-49), as PeriodicConfigs keeps them. */
  int32_t pbc;
  double lattice[9]; /* rows = lattice vectors of the simulation cell, bohr */
  /* Periodic orbitals (PBCOrbitalEvaluatorKpoints orbitals.py:118-255 over the lattice-summed AOs of
     numba/pbcgto.py:99-653), evaluated as Gamma-point orbitals of the simulation cell: the displacement point - atom
     is folded into the cell-centred parallelepiped, then every AO is summed over the cell translations Ls[j],
     j < num_Ls[atom of the shell] (all with |Ls[j]| <= sqrt(atom_cut) + half the cell's longest body diagonal),
     skipping an image when r^2 > atom_cut[atom]
     (pbcgto.py:213-214) or r^2 > shell_cut[shell] (:222, :356); cut-offs as max_Ls (:565-583).  Bloch orbitals
     of a primitive cell at the k-points of a zero-twist supercell are brought to this form on the host by folding
     the (real) Bloch phases into mo_up / mo_dn (pyqmc_amd/pbc.py:fold_mo_coeff).  nL = 0 with pbc != 0: no
     orbital tables (Jastrow-only handle). */
  int32_t nL;
  const double* Ls;        /* nL*3, sorted by norm (pbcgto.py:602-603) */
  const int32_t* num_Ls;   /* natom */
  const double* atom_cut;  /* natom, r^2 */
  const double* shell_cut; /* nshell, r^2 */
  /* Optional: reproduce which images the reference looks at.  The reference folds a point into the PRIMITIVE cell
     (wrap W = floor(r . inv(lattice_prim)), orbitals.py:201) and sums only the first num_Ls[a] entries of its
     norm-sorted primitive translation list (pbcgto.py:603-616, max_Ls :549-591), which is not a superset of what
     the cut-offs admit.  With member != NULL an image of atom A displaced by the cell translation
     (f + Ls[j]) (f = the fold applied to point - atom) is kept only if the primitive translation
     atom_n[A] + n(f) + img_n[j] - W is marked in member[member_class[A]], a (2M+1)^3 byte grid indexed
     [n0+M][n1+M][n2+M].  member = NULL: every image inside the cut-offs counts. */
  double lattice_prim[9];
  const int32_t* img_n;        /* nL*3: Ls[j] in units of the primitive lattice vectors */
  const int32_t* atom_n;       /* natom*3: the primitive translation that separates atom A from its primitive-cell original */
  const uint8_t* member;       /* n_member_class * (2M+1)^3 */
  const int32_t* member_class; /* natom */
  int32_t member_M, n_member_class;
  /* Complex orbitals (slater.py:212-216: Bloch coefficients at k-points off the time-reversal-invariant set).  With
     complex_orbitals != 0, mo_up / mo_dn hold [Re C | Im C] (nao x nmo_*, nmo_* = twice the number of orbitals),
     determinant occupations still index orbitals, and every complex output of the Slater entry points (sign of
     recompute / value, ratios of pqa_slater_eval, inverse / phases of pqa_slater_get_state) is (re, im) interleaved,
     i.e. the buffers are numpy complex128 arrays of the documented shapes.  Implemented for the wave-function protocol
     entry points; the fused sweep / energy entries refuse complex handles. */
  int32_t complex_orbitals;
  /* Twisted boundary conditions (Bloch orbitals with psi(r + L) = exp(i k_t . L) psi(r) for the lattice vectors L of the
     simulation cell; orbitals.py:201-213 get_wrapphase_complex).  twisted != 0 needs pbc, complex_orbitals and the
     periodic orbital tables.  The AOs become complex lattice sums sum_L exp(i k_t . L) phi(r - R - L); a handle in this
     mode takes UNFOLDED positions everywhere (position inside the cell + wrap . lattice, i.e. the electron's true
     coordinate) — the orbital kernel folds a point itself and derives the wrap phase exp(i k_t . wrap . lattice) of
     the reference from the integer wrap it removed; Jastrow, ECP and Ewald kernels use minimal-image displacements
     and do not care.  The fused sweep leaves the walkers unfolded. */
  int32_t twisted;
  double twist_k[3]; /* cartesian, 1/bohr */
} pqa_system_t;

/* ---- lifetime --------------------------------------------------------------------- */
int pqa_create(const pqa_system_t* sys, int device, pqa_handle_t** out);
void pqa_destroy(pqa_handle_t* h);
const char* pqa_last_error(const pqa_handle_t* h); /* h may be NULL: last create error */
int pqa_device_count(void);

/* wf.parameters[...] (slater.py:193-210, jastrowspin.py:48-53): names "det_coeff",
   "mo_coeff_alpha", "mo_coeff_beta", "acoeff", "bcoeff", "ccoeff".  Takes effect immediately for
   evaluations; cached walker state is refreshed by the next recompute, as in the reference. */
int pqa_set_param(pqa_handle_t* h, const char* name, const double* data, int64_t n);
int pqa_get_param(pqa_handle_t* h, const char* name, double* out, int64_t n);
/* pqa_get_param also answers "radial_table_info" (n = 2): the size in doubles of the radial tables the value-only
   orbital kernel reads for contracted shells of open systems and the largest fit error found when they were built,
   relative to sum |c| of the contraction (0, 0 with PQA_RADTAB=0 or a periodic system). */

/* ---- orbital evaluation (orbitals.py:85-96; numba/gto.py:89-254) --------------------- */
/* out (ncomp, npts, nao); ncomp 1 = value, 4 = +gradient, 5 = +laplacian */
int pqa_eval_ao(pqa_handle_t* h, const double* pts, int64_t npts, int ncomp, double* out);
/* out (ncomp, npts, nmo_spin); ncomp 1 or 5.  use_mfma=1: fused AO->MO MFMA kernel (product
   path); 0: plain VALU contraction of pqa_eval_ao output (A/B check only). */
int pqa_eval_mo(pqa_handle_t* h, int spin, const double* pts, int64_t npts, int ncomp, int use_mfma, double* out);

/* ---- Slater factor ------------------------------------------------------------------- */
/* Slater.recompute (slater.py:227-260) -> (sign, log|psi|) each (W) */
int pqa_slater_recompute(pqa_handle_t* h, const double* configs, int64_t W, double* sign, double* logabs);
/* Slater.value (slater.py:293-299) */
int pqa_slater_value(pqa_handle_t* h, double* sign, double* logabs);
/* _testrow/_testrowderiv (slater.py:301-380): multi-determinant ratios of replacing electron e's
   row by the orbitals at pts.  pts (nrow, npt, 3); row r belongs to walker widx[r] (NULL: r);
   out (ncomp, nrow*npt) with ncomp 1 (value: testvalue :429-446) or 5 (value, d/dx,d/dy,d/dz, laplacian:
   gradient_value :403-418, gradient_laplacian :420-427).  keep_saved (npt==1, widx==NULL, ncomp==5):
   keep the MO rows on the device for the next pqa_slater_update(use_saved=1). */
int pqa_slater_eval(pqa_handle_t* h, int e, const double* pts, int64_t nrow, int npt, const int32_t* widx,
                    int ncomp, int keep_saved, double* out);
/* Slater.updateinternals (slater.py:262-291) + Sherman-Morrison (slater.py:88-94); mask (W) bytes */
int pqa_slater_update(pqa_handle_t* h, int e, const double* epos, const uint8_t* mask, int use_saved);
/* any non-finite log-determinant of spin `spin`?  (the reference's trigger for a full recompute inside
   updateinternals, slater.py:269-275) */
int pqa_slater_has_zero(pqa_handle_t* h, int spin, int* flag);
/* test access: _inverse[s] (W, ndet_s, n, n) in the reference's [orbital, electron] order and
   _dets[s] (2, W, ndet_s) */
int pqa_slater_get_state(pqa_handle_t* h, int spin, double* inverse, double* dets);

/* ---- Jastrow factor ------------------------------------------------------------------ */
/* JastrowSpin.recompute / value (jastrowspin.py:56-109, 251-255) -> U (W) */
int pqa_jastrow_recompute(pqa_handle_t* h, const double* configs, int64_t W, double* logval);
int pqa_jastrow_value(pqa_handle_t* h, double* logval);
/* mode 0: testvalue (jastrowspin.py:387-419): out (nrow*npt) ratios
   mode 1: gradient_value (:296-340): out (4, nrow): dU/dx,dU/dy,dU/dz, ratio      (npt == 1)
   mode 2: gradient_laplacian (:342-385): out (4, nrow): grad U, lap U + |grad U|^2 (npt == 1) */
int pqa_jastrow_eval(pqa_handle_t* h, int e, const double* pts, int64_t nrow, int npt, const int32_t* widx,
                     int mode, double* out);
/* JastrowSpin.updateinternals (jastrowspin.py:111-137): also moves the handle's copy of the walkers */
int pqa_jastrow_update(pqa_handle_t* h, int e, const double* epos, const uint8_t* mask);
/* test access: _avalues (W,natom,na,2), _bvalues (W,nb,3), _configscurrent (W,N,3); any may be NULL */
int pqa_jastrow_get_state(pqa_handle_t* h, double* avalues, double* bvalues, double* configs);

/* ---- three-body Jastrow factor (ThreeBodyJastrow, three_body_jastrow.py) -------------- */
/* recompute :66-104 / value :191-195 -> U3 (W) */
int pqa_j3_recompute(pqa_handle_t* h, const double* configs, int64_t W, double* logval);
int pqa_j3_value(pqa_handle_t* h, double* logval);
/* testvalue :323-341 (mode 0), gradient_value :454-539 (mode 1), gradient_laplacian :541-655 (mode 2);
   argument and output layout as pqa_jastrow_eval */
int pqa_j3_eval(pqa_handle_t* h, int e, const double* pts, int64_t nrow, int npt, const int32_t* widx, int mode, double* out);
/* updateinternals :149-189: the factor keeps no partial sums here, so this only moves the stored walker
   coordinates when the handle has no two-body factor to do it */
int pqa_j3_update(pqa_handle_t* h, int e, const double* epos, const uint8_t* mask);

/* ---- Gaussian-process Jastrow factor (GPSJastrow, gps2.py) ----------------------------- */
/* The factor keeps a state of its own on the handle: its own copy of the walkers and its own walker count, independent of the
   Slater / Jastrow state, which these calls neither read nor write.  Any handle serves, also one created without a Slater and
   without a Jastrow factor; it supplies the electron count and the cell (minimal image in periodic handles).
   Support points xsupport (nsup, 2, 3), weights alpha (nsup), width f.  Call it again to change any of them: the stored
   Gaussians are NOT rebuilt (gps2.py rebuilds them in recompute only); a different nsup invalidates the state. */
int pqa_gps_set(pqa_handle_t* h, int nsup, const double* xsupport, const double* alpha, double f);
/* recompute :21-34 / value :40-43 -> log Psi (W) */
int pqa_gps_recompute(pqa_handle_t* h, const double* configs, int64_t W, double* logval);
int pqa_gps_value(pqa_handle_t* h, double* logval);
/* testvalue :76-93 (mode 0), gradient_value :95-108 (mode 1), gradient_laplacian :123-136 (mode 2); argument and output layout
   as pqa_jastrow_eval.  nrow = 0 returns at once. */
int pqa_gps_eval(pqa_handle_t* h, int e, const double* pts, int64_t nrow, int npt, const int32_t* widx, int mode, double* out);
/* updateinternals :68-74: epos (W, 3), mask (W) or NULL.  The sums over the electrons of the touched walkers are formed afresh. */
int pqa_gps_update(pqa_handle_t* h, int e, const double* epos, const uint8_t* mask);
/* pgradient :139-173: d_alpha (W, nsup), d_xsupport (W, nsup, 2, 3), d_f (W) */
int pqa_gps_pgradient(pqa_handle_t* h, double* d_alpha, double* d_xsupport, double* d_f);
/* test access: e_cs (W, nsup, N, 2) and the unit's walkers (W, N, 3); either may be NULL */
int pqa_gps_get_state(pqa_handle_t* h, double* e_cs, double* configs);

/* ---- AO-pair (geminal) Jastrow factor (GeminalJastrow, geminaljastrow.py) -------------------------- */
/* log Psi = sum_{i>j} a_i^T G a_j with a_i the AO values at electron i and G = triu(gcoeff) + triu(gcoeff)^T.  As the GPS factor
   it keeps a state of its own on the handle (its walkers, their AO values and the sums over the electrons), independent of the
   Slater / Jastrow state, which these calls neither read nor write.  The handle must carry basis tables (created with orbital
   coefficients, which the factor ignores) and real AOs: open systems and periodic cells at the Gamma point; twisted and complex
   handles are refused.
   gcoeff (n) in numpy.triu_indices(nao) order; n must be nao (nao + 1) / 2 (:81-84).  The stored AO values are not touched. */
int pqa_geminal_set(pqa_handle_t* h, const double* gcoeff, int64_t n);
/* recompute :70-88 / value :102-118 -> log Psi (W) */
int pqa_geminal_recompute(pqa_handle_t* h, const double* configs, int64_t W, double* logval);
int pqa_geminal_value(pqa_handle_t* h, double* logval);
/* testvalue :206-236 (mode 0), gradient_value :155-160 (mode 1), gradient_laplacian :173-188 (mode 2); argument and output layout
   as pqa_jastrow_eval.  nrow = 0 returns at once.  keep_saved (mode 1, widx NULL): the AO values at pts are kept for the
   pqa_geminal_update of the same electron that follows. */
int pqa_geminal_eval(pqa_handle_t* h, int e, const double* pts, int64_t nrow, int npt, const int32_t* widx, int mode, int keep_saved,
                     double* out);
/* testvalue_many :238-256: electrons es (ne) each moved to the one point pts (nrow, 3) of its row -> out (nrow, ne) */
int pqa_geminal_testvalue_many(pqa_handle_t* h, const int32_t* es, int ne, const double* pts, int64_t nrow, const int32_t* widx,
                               double* out);
/* updateinternals :90-100: epos (W, 3), mask (W) or NULL.  The sums over the electrons of the touched walkers are formed afresh.
   use_saved: take the AO values the last evaluation kept (it must have been mode 1 with keep_saved for this electron) instead of
   evaluating them at epos; both routes give bitwise the same state. */
int pqa_geminal_update(pqa_handle_t* h, int e, const double* epos, const uint8_t* mask, int use_saved);
/* pgradient :190-204: d_gcoeff (W, nao (nao + 1) / 2) */
int pqa_geminal_pgradient(pqa_handle_t* h, double* d_gcoeff);
/* test access: ao_val (W, N, nao) and the unit's walkers (W, N, 3); either may be NULL */
int pqa_geminal_get_state(pqa_handle_t* h, double* ao_val, double* configs);

/* ---- fused device-resident path --------------------------------------------------------- */
/* MultiplyWF.recompute (multiplywf.py:81-88) for all factors of the handle; also fills the
   per-electron orbital cache used by the fused sweep/energy. */
int pqa_wf_recompute(pqa_handle_t* h, const double* configs, int64_t W, double* sign, double* logabs);
int pqa_wf_value(pqa_handle_t* h, double* sign, double* logabs);
int pqa_get_configs(pqa_handle_t* h, double* configs);

/* Slater.pgradient (slater.py:462-542): d Psi / Psi with respect to the determinant coefficients, d_det (W, ndet)
   (:495-505), and to the orbital coefficients of each spin, d_mo_* (W, nao, nmo_s) (:507-533, _testcol :382-388),
   from the resident state (call after recompute / updateinternals).  Any output may be NULL.  Complex handles (complex
   orbitals / twisted cells): every output is complex, (re, im) interleaved, nmo_s counting orbitals — the holomorphic
   derivative the reference forms in complex arithmetic; twisted cells take the (complex) AO values of the unfolded
   walkers with their wrap phases. */
int pqa_slater_pgradient(pqa_handle_t* h, double* d_det, double* d_mo_up, double* d_mo_dn);

/* ThreeBodyJastrow.pgradient (three_body_jastrow.py:657-719): dU/dccoeff, d_ccoeff (W, natom, na3, na3, nb3, 3), from the
   stored walker coordinates. */
int pqa_j3_pgradient(pqa_handle_t* h, double* d_ccoeff);

/* testvalue_many (Slater slater.py:448-460, JastrowSpin jastrowspin.py:421-455, ThreeBodyJastrow
   three_body_jastrow.py:343-372, MultiplyWF multiplywf.py:112-114; used by the density-matrix accumulators
   observables/obdm.py:175, tbdm.py:239): for ONE auxiliary position per row, the ratio Psi(electron es[i] moved there)/Psi
   for each of the ne listed electrons.  pts (nrow,3); widx (nrow) walker index per row or NULL (nrow = W);
   factors: bit 0 Slater, bit 1 two-body Jastrow, bit 2 three-body Jastrow (their product is returned);
   out (nrow, ne) doubles, or (nrow, ne, 2) = (re, im) on a handle with complex orbitals. */
int pqa_testvalue_many(pqa_handle_t* h, const int32_t* es, int ne, const double* pts, int64_t nrow, const int32_t* widx,
                       int factors, double* out);

/* Periodic Coulomb energy: tables of the Ewald sum (Ewald.__init__ / set_up_reciprocal_ewald_sum / set_ewald_constants,
   observables/ewald.py:95-190; built by pyqmc_amd/ewald.py).  gpoints (ng,3): reciprocal vectors of the positive half
   space with weight > 1e-10 (:372-388); gweight (ng) = 4 pi exp(-G^2/4 alpha^2) / (V G^2); ion_cos/ion_sin (ng): real and
   imaginary part of sum_I Z_I exp(i G.R_I) (:233-234); ee_const / ei_const: self + charged-system terms for this electron
   count (:180-184); ii: ion-ion energy incl. its constants (:353).  The real-space sum runs over the 27 cells of
   nlatvec = 1 (:113-123).  gidx (ng,3) int32 / recip (3,3): optional integer decomposition gpoints = gidx . recip
   (recip = 2 pi inv(lattice)^T, :374-388); with it the structure factors e^{iG.x} are built from three base phases per
   electron by complex multiplication instead of one sincos per (G, electron).  NULL: direct sincos.
   Required before pqa_energy / energies in pqa_vmc_sweeps on a handle with pbc != 0. */
int pqa_set_ewald(pqa_handle_t* h, double alpha, int32_t ng, const double* gpoints, const double* gweight,
                  const double* ion_cos, const double* ion_sin, double ee_const, double ei_const, double ii,
                  const int32_t* gidx, const double* recip);

/* Wrap counters (PeriodicConfigs.wrap, coord.py:137-189) accumulated by the accepted moves of the LAST pqa_vmc_sweeps
   call: wrap (W, nelec, 3) int32, to be added to the caller's counters.  The walkers themselves stay folded into the
   cell (make_irreducible, mc.py:121). */
int pqa_get_wrap(pqa_handle_t* h, int32_t* wrap);

/* MultiplyWF.gradient / gradient_value / gradient_laplacian (multiplywf.py:116-129) of a real Slater x two-body-Jastrow product
   living on this handle, electron e moved to pts (W, 3), in ONE call: out (9, W) = the five Slater ratio rows of pqa_slater_eval
   (value, d/dx, d/dy, d/dz, laplacian, all relative to the current determinant) followed by the four Jastrow rows of
   pqa_jastrow_eval in mode jmode (1: grad U (3), value ratio; 2: grad U (3), laplacian).  keep_saved as pqa_slater_eval.
   pqa_wf_update: MultiplyWF.updateinternals (multiplywf.py:102-106) — Sherman-Morrison + Jastrow sums for the walkers of `mask`
   (NULL: all), and *has_zero = 1 if a determinant of e's spin is zero / not finite AFTER the update: what slater.py:269-275 tests
   before the NEXT update of that spin (the caller carries the flag; pqa_slater_has_zero is the stand-alone test). */
int pqa_wf_eval(pqa_handle_t* h, int e, const double* pts, int jmode, int keep_saved, double* out);
int pqa_wf_update(pqa_handle_t* h, int e, const double* epos, const uint8_t* mask, int use_saved, int* has_zero);

/* EnergyAccumulator.__call__ (accumulators.py:60-75) on the device-resident walkers:
   out (6, W) rows ke, ee, ei, ecp, grad2, total (kinetic energy.py:57-65, Coulomb :28-54, ECP
   eval_ecp.py:21-146).  threshold as eval_ecp.ecp_mask (:135-146).  rot (N, necp, 3, 3) and
   unif (N, necp, W) replay the reference's random draws; NULL -> device Philox stream `seed`. */
int pqa_energy(pqa_handle_t* h, double threshold, const double* rot, const double* unif, uint64_t seed, double* out);

/* EnergyAccumulator(naip=...) (accumulators.py:48-51 -> eval_ecp.ecp(..., naip), eval_ecp.py:21, :228-252 get_P_l): the
   quadrature rule of the ECP integrator of pqa_energy / the energy pass of pqa_vmc_sweeps / pqa_dmc_steps.  naip one of 6, 12,
   18, 26, 32, 50 — the grids of Mitas, Shirley & Ceperley the reference tabulates (eval_ecp.py:278-336) — for every ECP atom;
   0 restores the reference's default (naip=None: 6 points for atoms with at most one non-local channel, 12 otherwise,
   eval_ecp.py:239-240).  Any other value is refused, as get_rot does (eval_ecp.py:266-267).  The T-move candidates
   (pqa_tmoves, pqa_dmc_steps) keep the default rule: the reference's nonlocal_tmoves does not pass naip (accumulators.py:82-84). */
int pqa_set_ecp_naip(pqa_handle_t* h, int32_t naip);

/* EnergyAccumulator(use_old_ecp=False) (accumulators.py:57-58) -> jax_ecp.ECPAccumulator (jax_ecp.py:22-142): the batched
   formulation of the ECP integral.  For every electron ALL ECP atoms' quadrature points form one table (evaluate_vl,
   jax_ecp.py:160-222: naip[k] points at ECP atom k, 0 or one of the six grids; no range cut-off, no stochastic mask), of which
   nselect_deterministic points of largest sum_l v_l^2 are evaluated with weight 1 and nselect_random are sampled from the
   rest with weight 1 / (nselect_random p) (downselect_move_info, jax_ecp.py:225-290); nothing is dropped when the two add up
   to the table size.  enable = 1 switches the ECP part of pqa_energy and of the energy passes of pqa_vmc_sweeps /
   pqa_dmc_steps to it, 0 back to the semi-local integrator (eval_ecp.py).  In this mode pqa_energy's `unif` is the
   (N, W, nselect_random) table of selection uniforms (jax_ecp.py:255) and `rot` (N, necp, 3, 3) as before; pqa_vmc_sweeps
   draws both from the device streams (its tapes keep the semi-local layout and are refused); pqa_dmc_steps also takes its
   T-MOVE candidates from this integrator (nonlocal_tmoves, jax_ecp.py:110-135: every electron's selected points whose weight is
   not exactly 0) and takes or draws the tapes in the batched layout (pqa_dmc_tapes_t).
   pqa_ecp_batched_nselected: slots per electron (the P of the outputs below).
   pqa_ecp_batched_moves: ECPAccumulator.nonlocal_tmoves (jax_ecp.py:110-135) for electron e — the selected points' positions
   pos (W, P, 3) and T-move weights weight (W, P) = sum_l [P_l > 0] (exp(-tau v_l / P_l) - 1) P_l; rot (necp, 3, 3),
   unif (W, nselect_random) or NULL -> device stream `seed`.  The ratios come from pqa_wf_testvalue at `pos`. */
int pqa_set_ecp_batched(pqa_handle_t* h, int32_t enable, const int32_t* naip, int32_t nselect_deterministic, int32_t nselect_random);
int pqa_ecp_batched_nselected(pqa_handle_t* h);
int pqa_ecp_batched_moves(pqa_handle_t* h, int e, double tau, const double* rot, const double* unif, uint64_t seed,
                          double* weight, double* pos);

/* EnergyAccumulator.nonlocal_tmoves -> eval_ecp.compute_tmoves (eval_ecp.py:43-80) for electron e of the resident
   walkers: the candidate T-moves over every ECP atom's quadrature points (P = pqa_tmove_npoints() per walker).
   rot (necp,3,3), unif (necp,W): the reference's per-atom random rotation / mask uniforms.  Outputs: ratio (W,P)
   Psi(candidate)/Psi (1 where the walker fails the ECP mask for that atom), weight (W,P) = sum_l (exp(-tau v_l)-1)
   (2l+1)P_l w_i (0 there), pos (W,P,3) candidate positions (current position there).  ratio = NULL: positions and weights
   only — complex handles take their (complex) ratios from pqa_wf_testvalue at those positions. */
/* The next pqa_dmc_steps call starts from the energies (E_L, |grad|^2) its predecessor's last step left on the device instead of
   evaluating the starting configuration again — what dmc_propagate carries from step to step (dmc.py:148-149, :199-200); for callers
   that make one call per step to run host accumulators in between (pyqmc_amd.dmc with OBDM / TBDM accumulators).  One-shot; refused
   when the wave-function state changed since that call (recompute, update, resample, sweep, parameter change).  With tapes the
   index-0 energy draws of the call are unused. */
int pqa_dmc_continue(pqa_handle_t* h, int on);
/* 1 while the energies of the last pqa_dmc_steps call still describe the resident walkers' state (pqa_dmc_continue would be honoured), else 0:
   a per-step caller whose host accumulators may have touched the state asks before it continues (pyqmc_amd.dmc; dmc.py:196-212). */
int pqa_dmc_can_continue(pqa_handle_t* h);
int pqa_tmove_npoints(pqa_handle_t* h);
int pqa_tmoves(pqa_handle_t* h, int e, double tau, double threshold, const double* rot, const double* unif, double* ratio,
               double* weight, double* pos);

/* vmc_worker move loop (mc.py:112-137) fused on the device, nsteps sweeps over all electrons,
   optionally followed each sweep by the energy accumulator (mc.py:142-148).
   gauss (nsteps,N,W,3) standard normals and unif (nsteps,N,W): replay tapes, or NULL -> Philox(seed).
   ecp_rot (nsteps,N,necp,3,3) / ecp_unif (nsteps,N,necp,W): same for the ECP draws.
   acceptance (nsteps): mean acceptance per sweep.  energy_mean (nsteps,6): walker means of
   ke,ee,ei,ecp,grad2,total (NULL: no energy evaluation).  accept_rec (nsteps,N,W) bytes, may be NULL. */
int pqa_vmc_sweeps(pqa_handle_t* h, double tstep, int nsteps, const double* gauss, const double* unif,
                   double threshold, const double* ecp_rot, const double* ecp_unif, uint64_t seed,
                   double* acceptance, double* energy_mean, uint8_t* accept_rec);

/* branch (pyqmc/method/dmc.py:342-376) without the recompute that follows it in the reference (:155): walker w of the
   resident ensemble becomes a copy of walker newinds[w] — coordinates, inverses, determinant signs / logs, orbital-row
   cache and Jastrow sums are gathered on the device (the counterpart of configs.resample(newinds) coord.py:64-70,
   191-198 for the wave-function state).  newinds (W) int32 in [0, W). */
int pqa_resample(pqa_handle_t* h, const int32_t* newinds);

/* Distributed branching (pyqmc/method/dmc.py:342-376 over ranks): after every rank has computed the
   identical global comb, a walker whose new owner differs from its old one travels as coordinates only.
   pqa_get_walkers: coordinates (n,N,3) of the resident walkers idx[k] (duplicates allowed) into `out` — host memory or a
   device buffer handed straight to RCCL.
   pqa_branch_exchange: the rank's new ensemble = the resident walkers keep_src[0..nkeep) (their whole wave-function state is
   gathered on the device, as pqa_resample) followed by nrecv received walkers with coordinates recv_x (nrecv,N,3; host or
   device), for which ALONE the state is recomputed (the reference recomputes every walker after a branch, dmc.py:155).
   nkeep + nrecv must equal the resident walker count. */
int pqa_get_walkers(pqa_handle_t* h, const int32_t* idx, int64_t n, double* out);
int pqa_branch_exchange(pqa_handle_t* h, const int32_t* keep_src, int64_t nkeep, const double* recv_x, int64_t nrecv);

/* dmc_propagate's step loop (pyqmc/method/dmc.py:123-221) fused on the device, open or periodic systems, real and
   (round 3) complex wave functions.  Complex: no node constraint in the drift-diffusion (dmc.py:64-66 is real-only),
   weights from Re E_L, T-move amplitudes from Re[Psi(R')/Psi(R)] (the reference's propose_tmoves orders complex
   amplitudes, which is undefined; golden g30 pins this rule), and step_avg has EIGHT numbers per step: the seven below,
   then the weighted mean of Im ecp (= Im total).  Per step: per step (1) one T-move per electron (compute_tmoves eval_ecp.py:43-80, propose_tmoves dmc.py:73-120,
   masked updateinternals :160-168), (2) one drift-diffusion move per electron with Umrigar's limited drift
   (limdrift :22-35) and fixed-node rejection (propose_drift_diffusion :38-70), (3) the energy accumulator, the
   branching factor compute_S (:224-235), weights *= exp(tau r2_acc/r2_prop (S_new+S_old)/2) and the weighted step
   averages (:196-215).  No branching: the caller combs between calls, as rundmc does (:342-376).
   The walkers must be resident and current (pqa_wf_recompute); the starting energy is evaluated first (:146-149).
   weights (W) in/out.  step_avg (nsteps,7) [complex: (nsteps,8)]: sum_w w_w row_w / sum_w w_w for rows ke, ee, ei, ecp,
   grad2, total (real parts), then the mean weight.  step_acc (nsteps,2): acceptance and T-move acceptance (accepted / (W nelec)).
   tapes NULL -> device Philox streams keyed by (seed, walker, electron, step); otherwise every pointer the system
   needs must be set (the ECP ones only when the system has ECP atoms):
     gauss (nsteps,N,W,3) standard normals, unif (nsteps,N,W)                      drift-diffusion moves
     tm_rot (nsteps,N,necp,3,3), tm_unif (nsteps,N,necp,W), tm_u1, tm_u2 (nsteps,N,W)  T-move grid, mask, selection, acceptance
     ecp_rot (nsteps+1,N,necp,3,3), ecp_unif (nsteps+1,N,necp,W)                  energy draws; index 0 = starting energy
   With pqa_set_ecp_batched on, the members keep their names and the uniforms of the ECP integrator take its layout — what
   pqa_energy's `unif` has in that mode: ecp_unif (nsteps+1,N,W,nselect_random) and tm_unif (nsteps,N,W,nselect_random) are the
   selection uniforms of downselect_move_info (jax_ecp.py:255), one rotation per (electron, ECP atom) as before (atoms without
   points ignore theirs); both may be NULL where nothing is dropped (nselect_deterministic + nselect_random >= the table size)
   or nselect_random = 0.  gauss, unif, tm_u1 and tm_u2 are unchanged.  Without tapes the T-move selection uniforms come from
   a Philox stream of their own, not the energy evaluations': the evaluation that closes step i and the T-moves of step i + 1
   are keyed by the same (seed, step, walker, electron nselect_random + j). */
typedef struct {
  const double* gauss;
  const double* unif;
  const double* tm_rot;
  const double* tm_unif;
  const double* tm_u1;
  const double* tm_u2;
  const double* ecp_rot;
  const double* ecp_unif;
} pqa_dmc_tapes_t;
int pqa_dmc_steps(pqa_handle_t* h, double tstep, int nsteps, double branchcut, double e_trial, double e_est,
                  double threshold, double* weights, const pqa_dmc_tapes_t* tapes, uint64_t seed, double* step_avg,
                  double* step_acc);

/* ---- density matrices and parameter-gradient moments ---------------------------- */
/* Auxiliary one-electron Metropolis walk of the density-matrix estimators (sample_onebody,
   pyqmc/observables/obdm.py:215-250) on a handle whose orbitals are the estimator's basis (built from orb_coeff alone):
   n walkers distributed as f(r) = sum_i |phi_i(r)|^2 (orbitals of `spin`), nsamples proposals r + sqrt(tstep) z each,
   accepted with probability f(r')/f(r).  The walk stays on the device (one orbital launch + one accept kernel per
   sample).  pos (n,3) in/out; periodic handles take and return UNFOLDED coordinates (the orbital kernel folds every point
   itself and gives twisted cells their wrap phase, orbitals.py:201-213).  gauss (nsamples,n,3) standard normals and unif
   (nsamples,n): replay tapes in the reference's draw order, or both NULL -> Philox(seed).  The last nkeep samples
   (positions, orbital rows, densities) stay resident in `slot` (0 or 1) for pqa_obdm_accumulate / pqa_tbdm_accumulate;
   keep_pos (nkeep,n,3) receives their positions (may be NULL), accept (nsamples,n) the decisions as 0/1 (may be NULL). */
int pqa_dm_walk(pqa_handle_t* h, int slot, int spin, int64_t n, int nsamples, double tstep, double* pos, const double* gauss,
                const double* unif, uint64_t seed, int nkeep, double* keep_pos, double* accept);
/* Basis orbitals at the configurations' electrons (OBDMAccumulator.evaluate_orbitals obdm.py:199-201, tbdm.py:203-212):
   pts (npts,3) = (nconf, nelec_listed, 3), kept on the device in `slot`. */
int pqa_dm_points(pqa_handle_t* h, int slot, int spin, const double* pts, int64_t npts);
/* One sweep of the one-body estimator (obdm.py:170-190) for kept sample k of `slot`: configuration n uses auxiliary walker
   assign[n]; ratio (nconf,nelec) = Psi(r_e -> r')/Psi from wf.testvalue_many (interleaved complex if ratio_complex).
   first != 0 starts new accumulators value (nconf,norb,norb), norm (nconf,norb); otherwise adds. */
int pqa_obdm_accumulate(pqa_handle_t* h, int slot, int k, int64_t nconf, int nelec, const int32_t* assign, const double* ratio,
                        int ratio_complex, int first);
/* One sweep of the two-body estimator (tbdm.py:232-277): slot 0 / 1 hold the walks and electron orbitals of the first /
   second spin of the sector.  ratio (nconf,nea,neb) = Psi(r_a -> r1', r_b -> r2')/Psi, 0 for a pair naming one electron
   twice; ijkl (4,ntuple) int32.  Accumulates value (nconf,ntuple), norm_a (nconf,norb_a), norm_b (nconf,norb_b). */
int pqa_tbdm_accumulate(pqa_handle_t* h, int k, int64_t nconf, int nea, int neb, const int32_t* assign_a, const int32_t* assign_b,
                        const double* ratio, int ratio_complex, const int32_t* ijkl, int ntuple, int first);
/* One sweep of the two-body estimator with the pair ratios formed on the device (tbdm.py:232-246) instead of handed in: wf holds
   the wave function with the configurations as its resident walkers (wf's W = nconf), ev the estimator's orbitals as above.  For
   walker w the auxiliary points r1 = kept sample k of slot 0, walker assign_a[w], and r2 = the same of slot 1 with assign_b[w], are
   read on the device (periodic handles keep them unfolded: the orbital kernel folds, the Jastrow distances are minimal images);
   ratio[w][a][b] = Psi(r_a -> r1, r_b -> r2)/Psi for a over the whole spin block spin_a and b over spin_b of wf, in closed form from
   wf's resident state (pqa_tbdm.hip: single-move rows v = phi . inverse, a 2 x 2 determinant of them for equal spins, the
   determinant-weighted sum for several determinants, times exp of the two-body Jastrow difference), 0 for a pair naming one
   electron twice.  wf's state is not modified.  The ratios of a walker chunk (walker_chunk walkers; 0: the estimator units' own
   bound) are contracted on ev's stream by the kernel of pqa_tbdm_accumulate, after which ev holds exactly what that call
   accumulates (pqa_dm_fetch reads it); ratio (W,nea,neb) host receives the ratios, or NULL: nothing but the two assignments
   crosses the bus.  ijkl = NULL with ntuple = 0: ratios only, nothing is accumulated and pqa_dm_points is not needed.
   Fused scope: wf real and untwisted with a Slater factor (one or more determinants), with or without the two-body Jastrow, no
   three-body factor, open or periodic at Gamma; ev real, on the same device.  Everything else is refused (<0): those pair ratios go
   through the protocol route (pyqmc_amd.TBDMAccumulator: testvalue, updateinternals, testvalue_many). */
int pqa_tbdm_sweep(pqa_handle_t* wf, pqa_handle_t* ev, int k, int spin_a, int spin_b, const int32_t* assign_a, const int32_t* assign_b,
                   const int32_t* ijkl, int ntuple, int first, int64_t walker_chunk, double* ratio);
/* pqa_tbdm_sweep for complex and twisted wave-function handles and complex evaluators: the same steps, streams, events and chunks,
   with ratio (W,nea,neb) interleaved complex,
     v_D(q)[i] = sum_k phi_occ_D[k](q) T_D[i][k] (complex, no conjugation),   S_ab(D) = v_D(r1)[a] v_D(r2)[b] (- v_D(r2)[a] v_D(r1)[b]
     for equal spins, S_aa an exact 0 + 0i),   R_ab = (sum_D w_D S_ab(D) / sum_D w_D) exp(dU_ab),
   w_D the complex determinant weights relative to the largest |determinant| and dU_ab the real Jastrow difference of pqa_tbdm_sweep.
   A twisted wf keeps its walkers unfolded; r1 / r2 are folded by its orbital kernel, which puts the wrap phase on the row.  ev ends
   as pqa_tbdm_accumulate with complex ratios leaves it (a complex value, real norms; pqa_dm_fetch reads them).  Scope: wf a Slater
   handle with a state (one or more determinants; real, complex or twisted; with or without the two-body Jastrow; no three-body
   factor), both spin blocks non-empty, ev a second handle on the same device, real or complex; a twisted ev needs a twisted wf.
   Everything else is refused (<0) and goes through the protocol route.  wf's state is not modified. */
int pqa_tbdm_sweep_c(pqa_handle_t* wf, pqa_handle_t* ev, int k, int spin_a, int spin_b, const int32_t* assign_a, const int32_t* assign_b,
                     const int32_t* ijkl, int ntuple, int first, int64_t walker_chunk, double* ratio);
/* The whole one-body estimator of one evaluation (obdm.py:139-193) with the ratios formed on the device: wf holds the wave function
   with the configurations as its resident walkers (wf's W = nconf), ev the estimator's orbitals, whose `slot` holds the last
   nsweeps (or more) samples of a pqa_dm_walk.  es (ne) host: the listed electrons, any order, either spin, none twice.  Their
   coordinates are gathered from wf's resident walkers on the device and ev's orbitals are evaluated there into the slot (what
   pqa_dm_points does from a host array).  Sweep s = 0 .. nsweeps-1 uses kept sample s: walker w takes the auxiliary walker
   assign[s][w] (assign (nsweeps,W) host), or, with assign = NULL, floor(u naux) with u from Philox keyed by (seed; walker, sweep);
   assign_out (nsweeps,W) host receives the assignments used (may be NULL).  ratio[s][w][e] = Psi(r_e -> r')/Psi in closed form from
   wf's resident state (pqa_obdm.hip: the single-move rows v = phi . inverse, the determinant-weighted sum for several determinants,
   times exp of the two-body Jastrow difference); ratio (nsweeps,W,ne) host receives them, or NULL.  wf's state is not modified.
   mean = 0: ev's per-walker accumulators end as nsweeps pqa_obdm_accumulate calls leave them (first != 0 starts them, otherwise the
   sweeps are added; pqa_dm_fetch reads them).  mean != 0 (first must be set): value_mean (norb,norb) and norm_mean (norb) host
   receive the means over walkers and sweeps, value_mean = sum_s B_s^T T_s / (W nsweeps) on the fp64 matrix cores with the walkers
   as the k dimension; no per-walker (norb,norb) array exists in this mode.  walker_chunk: walkers per scratch chunk (0: the
   estimator units' own bound; the mean mode takes whole 64-walker slices).  Every sum has a fixed order that does not depend on
   the chunk.  Fused scope: wf real and untwisted with a Slater factor (one or more determinants), with or without the two-body
   Jastrow, no three-body factor, open or periodic at Gamma; ev real, on the same device; ne >= 1.  Everything else is refused (<0):
   those go through the protocol route (pyqmc_amd.OBDMAccumulator: testvalue_many, pqa_obdm_accumulate). */
int pqa_obdm_sweeps(pqa_handle_t* wf, pqa_handle_t* ev, int slot, const int32_t* es, int ne, int nsweeps, const int32_t* assign,
                    uint64_t seed, int mean, int first, int64_t walker_chunk, double* ratio, int32_t* assign_out, double* value_mean,
                    double* norm_mean);
/* The mean mode of pqa_obdm_sweeps with walker weights (the mixed estimator of DMC): weights (W) host, finite and >= 0 with a
   positive sum, otherwise refused;
     value_mean = sum_s sum_w w_w b_s[w] (x) t_s[w] / (nsweeps sum_w w_w),   norm_mean likewise.
   One body with pqa_obdm_sweeps: the weight multiplies the B operand of the matrix-core product as it is loaded and the norm term as
   it is added, sum_w w_w comes from one fixed-order tree, and slices, chunk rounding and the slice-order reduction are those of the
   unweighted mean.  So one chunk or several, and two calls, give the same bits, and unit weights give the bits of
   pqa_obdm_sweeps(mean = 1).  assign = NULL / assign_out as there; the ratios are not offered.  Same scope. */
int pqa_obdm_sweeps_w(pqa_handle_t* wf, pqa_handle_t* ev, int slot, const int32_t* es, int ne, int nsweeps, const int32_t* assign,
                      uint64_t seed, int64_t walker_chunk, const double* weights, int32_t* assign_out, double* value_mean,
                      double* norm_mean);
/* pqa_obdm_sweeps for complex and twisted wave-function handles and complex evaluators: the same steps, streams, chunks and fixed
   summation orders, with ratio (nsweeps,W,ne) and value_mean (norb,norb) interleaved complex and norm_mean (norb) real;
     value[j][k] += (phi_j(r')/F) conj(sum_e R_e phi_k(r_e)),   R_e = (sum_D w_D v_D(r')[e] / sum_D w_D) exp(A_e(r')),
   w_D the complex determinant weights relative to the largest |determinant|.  mean = 0: ev's per-walker accumulators end as nsweeps
   pqa_obdm_accumulate calls with complex ratios leave them.  mean != 0: value_mean = B^T T / (W nsweeps) from planar panels,
   Re = Br^T Tr - Bi^T Ti, Im = Br^T Ti + Bi^T Tr on the fp64 matrix cores.  weights != NULL (mean mode only): the weighted mean of
   pqa_obdm_sweeps_w; unit weights give the bits of the unweighted call.  Scope: wf a Slater handle with a state (one or more
   determinants; real, complex or twisted; with or without the two-body Jastrow; no three-body factor), ev a second handle on the
   same device, real or complex; a twisted ev needs a twisted wf (an untwisted periodic handle holds folded walkers, so the wrap
   phase of phi_k(r_e) would be lost).  es, nsweeps, first, assign and weights follow pqa_obdm_sweeps / pqa_obdm_sweeps_w.  Everything
   else is refused (<0) and goes through the protocol route.  wf's state is not modified. */
int pqa_obdm_sweeps_c(pqa_handle_t* wf, pqa_handle_t* ev, int slot, const int32_t* es, int ne, int nsweeps, const int32_t* assign,
                      uint64_t seed, int mean, int first, int64_t walker_chunk, const double* weights, double* ratio,
                      int32_t* assign_out, double* value_mean, double* norm_mean);
/* pqa_dm_points for the listed electrons es (ne) of wf's resident walkers: their coordinates are gathered on the device and ev's
   orbitals of the spin of the slot's walk (pqa_dm_walk comes first) are evaluated there into `slot`, rows (W, ne, norb) — the first
   stage of pqa_obdm_sweeps, with its scope checks.  wf's state is not modified. */
int pqa_dm_points_resident(pqa_handle_t* wf, pqa_handle_t* ev, int slot, const int32_t* es, int ne);
/* pqa_dm_points_resident with the scope of pqa_obdm_sweeps_c / pqa_tbdm_sweep_c: complex and twisted wf, complex ev (rows
   (W, ne, 2 norb), real block | imaginary block); a twisted ev needs a twisted wf, whose unfolded walkers give phi_k(r_e) its wrap
   phase. */
int pqa_dm_points_resident_c(pqa_handle_t* wf, pqa_handle_t* ev, int slot, const int32_t* es, int ne);
/* The fused density-matrix entries for wave functions with a THREE-BODY Jastrow factor.  pqa_obdm_sweeps_j3 has pqa_obdm_sweeps_c's
   parameter list (weights NULL: unweighted) with real ratio (nsweeps, W, ne) and value_mean (norb, norb); pqa_tbdm_sweep_j3 has
   pqa_tbdm_sweep's; pqa_dm_points_resident_j3 is pqa_dm_points_resident in their scope.  With C symmetrised in (k, l) the pair term
     t(x, s; y, u) = sum_I sum_klm C[I][k][l][m][s + u] a_k(|x - R_I|) a_l(|y - R_I|) b_m(|x - y|)
   is symmetric, U3 = sum_{i<j} t(i, j), P_e = sum_{j != e} t(e, j), and with one table G_s(q)[j] = t(q, s; r_j, s_j) per auxiliary
   point and moving spin, SG its sum over j,
     A3_e(r')  = SG_{s_e}(r') - G_{s_e}(r')[e] - P_e,                    R_e  = (Slater ratio) exp(A_e + A3_e)
     dU3_ab    = SG_{s1}(r1) + SG_{s2}(r2) + t(r1, s1; r2, s2) - G_{s1}(r1)[a] - G_{s1}(r1)[b] - G_{s2}(r2)[a] - G_{s2}(r2)[b]
                 - P_a - P_b + t(r_a, s1; r_b, s2),                      R_ab = S_ab exp(dU_ab + dU3_ab)
   with the Slater and two-body parts of pqa_obdm_sweeps / pqa_tbdm_sweep.  One kernel (k_j3_moves, one wave per walker) forms the
   three-body differences of a walker chunk ahead of the ratio kernel.  Scope: wf a real, untwisted Slater handle with a state (one
   or more determinants; with or without the two-body factor; with or without the three-body factor — without one the launches and
   the bits are those of pqa_obdm_sweeps / _w / pqa_tbdm_sweep), open or periodic at Gamma, whose three-body tables of one walker fit
   160 KiB of LDS; ev a second, real handle on the same device.  Everything else is refused (<0) with a message that names the entry
   and the protocol route.  Modes, chunks, assignments and weights follow the siblings.  wf's state is not modified. */
int pqa_obdm_sweeps_j3(pqa_handle_t* wf, pqa_handle_t* ev, int slot, const int32_t* es, int ne, int nsweeps, const int32_t* assign,
                       uint64_t seed, int mean, int first, int64_t walker_chunk, const double* weights, double* ratio,
                       int32_t* assign_out, double* value_mean, double* norm_mean);
int pqa_tbdm_sweep_j3(pqa_handle_t* wf, pqa_handle_t* ev, int k, int spin_a, int spin_b, const int32_t* assign_a, const int32_t* assign_b,
                      const int32_t* ijkl, int ntuple, int first, int64_t walker_chunk, double* ratio);
int pqa_dm_points_resident_j3(pqa_handle_t* wf, pqa_handle_t* ev, int slot, const int32_t* es, int ne);
/* Device bytes ev holds for pqa_obdm_sweeps: scratch = the mean mode's panels, partial tiles and sums plus a walker chunk's ratios;
   per_walker = the per-walker accumulators (value, norms), which the mean mode never allocates.  These are the buffers' capacities,
   so after a pqa_obdm_sweeps_c call they are the complex sizes (five panels, 2 norb^2 + norb partials, interleaved ratios and values). */
int pqa_obdm_bytes(pqa_handle_t* ev, int64_t* scratch, int64_t* per_walker);
/* Read an accumulator times `scale`: which = 0 value (ncol = entries per configuration, doubled when complex), 1 norm /
   norm_a, 2 norm_b (ncol = orbitals).  mean = 0: (nconf,ncol); mean != 0: (ncol,) averaged over the configurations on
   the device (the accumulators' avg(), obdm.py:195-197). */
int pqa_dm_fetch(pqa_handle_t* h, int which, int ncol, double scale, int mean, double* out);
/* The weighted walker mean of an accumulator times `scale`: out (ncol) = scale sum_n w_n acc[n][.] / sum_n w_n with `which` / ncol
   as in pqa_dm_fetch and weights (nconf) host, finite and >= 0 with a positive sum.  A block sums a run of 64 consecutive columns
   over a slice of configurations (k_wcol_means, pqa_estim.hpp), the slices are added in order: no atomics, two calls give the same
   bits. */
int pqa_dm_fetch_w(pqa_handle_t* h, int which, int ncol, double scale, const double* weights, double* out);
/* C (P,Q) = A^T B for A (n,P), B (n,Q) on the fp64 matrix cores: the moment matrix dpidpj = dp^T diag(w f) dp of
   StochasticReconfiguration.avg (stochastic_reconfiguration.py:106-114). */
int pqa_gram(pqa_handle_t* h, int64_t n, int P, int Q, const double* A, const double* B, double* C);

/* The random numbers the fused sweeps (pqa_vmc_sweeps, pqa_dmc_steps without tapes) draw for sweep `step` of `seed`:
   gauss (N,W,3) standard normals and unif (N,W) Metropolis uniforms of walkers 0..W-1 — Philox4x32-10 keyed by
   (seed; walker, electron, stream, step).  Test entry: lets the CPU oracle replay a device-RNG trajectory (the role
   np.random.seed plays for the reference's vmc_worker, mc.py:119,131). */
int pqa_philox_tapes(pqa_handle_t* h, uint64_t seed, int step, int64_t W, double* gauss, double* unif);
/* The same for pqa_dmc_steps without tapes: every array of pqa_dmc_tapes_t for `nsteps` steps of `seed`, restricted to walkers
   0..W-1, in the tape layouts above (the members of `out` point to caller-allocated HOST arrays of those shapes; tm_* may be
   NULL for systems without ECPs) — T-move grid rotations, mask uniforms, selection / acceptance uniforms, drift-diffusion
   normals and uniforms, and the energy evaluations' quadrature rotations and mask uniforms (index 0 = starting energy).
   With pqa_set_ecp_batched on it writes the batched layouts: ecp_unif / tm_unif are the selection uniforms of the energy
   evaluations and of the T-move tables (two different streams), written only where the selection drops points (NULL allowed
   otherwise).
   Test entry: the CPU oracle's dmc_propagate (pyqmc/method/dmc.py:123-221) replays a device-RNG block walker by walker. */
int pqa_philox_dmc_tapes(pqa_handle_t* h, uint64_t seed, int nsteps, int64_t W, pqa_dmc_tapes_t* out);

/* ---- total spin ----------------------------------------------------------------------- */
/* S2Accumulator.__call__ (pyqmc/observables/s2_accumulator.py): per walker S^2 = Sz(Sz+1) + N_dn - sum_{i up, j dn}
   Psi(R^{i<->j})/Psi(R), where R^{i<->j} puts up electron i at r_j and down electron j at r_i.  The swap ratios come in closed
   form from the resident state (orbitals of each spin at the other spin's electrons times the inverses, the Jastrow sums of
   every electron), which the call does not modify.  s2 (W); ratios (W, N_up, N_dn) = the swap ratios, or NULL.  Fused scope:
   real handles with a Slater factor (one or more determinants), with or without the two-body Jastrow, open or periodic at
   Gamma; N_dn = 0 (or N_up = 0) returns Sz(Sz+1) + N_dn without a launch.  Complex / twisted handles and handles with a
   three-body Jastrow factor are refused (<0): the swap ratios of those go through the protocol route
   (pyqmc_amd.S2Accumulator). */
int pqa_s2(pqa_handle_t* h, double* s2, double* ratios);

/* ---- symmetry operators ------------------------------------------------------------------ */
/* SymmetryAccumulator / SymmetryAccumulatorPBC.__call__ (pyqmc/observables/accumulators.py:237-283, :286-341): per operator o
   and walker w the ratio Psi(S_o R)/Psi(R), where S_o R moves every electron to x' = (x - origin_o) @ S_o + origin_o (row
   vectors: the reference's einsum("ijk,kl->ijl", x, S)) and, in a periodic cell, folds it back into the cell (enforce_pbc).
   ops (nop,3,3) row-major; origins (nop,3), or NULL for the origin 0; ratio (nop, W).  Read-only on the resident state (after
   the layout sync): inverses, determinants, Jastrow sums, coordinates and wrap stay as they were.  Fused scope: real handles
   with a Slater factor (one or more determinants), with or without the two-body Jastrow, open or periodic at Gamma.  Complex /
   twisted handles and handles with a three-body Jastrow factor are refused (<0): those go through the protocol route
   (pyqmc_amd.SymmetryAccumulator). */
int pqa_symmetry(pqa_handle_t* h, int nop, const double* ops, const double* origins, double* ratio);

/* ---- structure factor --------------------------------------------------------------- */
/* SqAccumulator (pyqmc/observables/accumulators.py:191-234): per walker w and wave vector q
     sq[w][q]     = |sum_j       exp(i q.r_j)|^2 / N,
     spinsq[w][q] = |sum_j s_j * exp(i q.r_j)|^2 / N      (s_j = +1 for the nelec_up first electrons, -1 for the rest),
   periodic points folded into the cell first (twisted handles keep unfolded coordinates).  nqv vectors q (nqv,3) Cartesian.
   With qn (nqv,3) and recip (3x3, rows b_a): q = sum_a qn[.][a] b_a, and every phase comes from a power recurrence of the three
   base phases exp(i b_a.r) (the q grids of SqAccumulator); with qn = NULL (recip ignored) one sincos per (q, electron).  The
   caller asserts that q and qn @ recip agree.  mean = 0: sq, spinsq (W, nqv); mean = 1: walker means (nqv), reduced on the
   device in a fixed order (no atomics: two calls give the same bits).  Every handle kind; read-only on the resident state
   (coordinates are read in place from whichever layout holds them: no layout sync, no change to anything a sweep reads). */
int pqa_sq(pqa_handle_t* h, int nqv, const double* q, const int* qn, const double* recip, int mean, double* sq, double* spinsq);
/* pqa_sq(mean = 1) with walker weights: sq, spinsq (nqv) = sum_w w_w value[w][.] / sum_w w_w; weights (W) host, finite and >= 0
   with a positive sum.  Every handle kind, read-only, reduced in a fixed order (no atomics: two calls give the same bits). */
int pqa_sq_w(pqa_handle_t* h, int nqv, const double* q, const int* qn, const double* recip, const double* weights, double* sq,
             double* spinsq);

/* ---- slab (2D) Ewald energy ------------------------------------------------------------------------ */
/* Ewald (pyqmc/observables/ewald2d.py; Yeh and Berkowitz, J. Chem. Phys. 111, 3155): Coulomb energy of a cell that is periodic along
   its first two lattice vectors and open along the third, of the resident walkers.  Per pair with minimal-image displacement
   d = (dx, dy, z) (all three lattice vectors, as the handle's other pair terms):
     real    sum_L erfc(alpha |d + L|) / |d + L|                       over the nlat in-plane displacements lat,
     recip   2 sum_k cos(k.d) (pi / (A k)) [e^{kz} erfc(k / 2 alpha + alpha z) + e^{-kz} erfc(k / 2 alpha - alpha z)],
     charge  -(2 pi / A) [z erf(alpha z) + exp(-alpha^2 z^2) / (alpha sqrt(pi))],
   the reciprocal weight in a scaled form that cannot overflow (pqa_ewald2d.hip).  Electron-electron pairs carry charge 1 and
   ee adds nelec * self_const; electron-ion pairs carry -q_I (the atom axis is contracted in all three terms; the reference's
   real-space contraction runs over the electron axis).  The ion-ion term is position independent and stays with the
   caller.  The tables (pyqmc_amd.ewald2d.ewald2d_tables):
     alpha, area        partition parameter, area of the in-plane cell
     self_const         -alpha / sqrt(pi) + sum_k gweight_k - sqrt(pi) / (A alpha)
     nk, kn, knorm, kpref, recip
                        k_j = kn[j][0] recip[0] + kn[j][1] recip[1] (recip: the two in-plane reciprocal rows, 2 x 3), |k_j| = knorm[j] > 0,
                        kpref[j] = (pi / (A knorm[j])) exp(-(knorm[j] / 2 alpha)^2)
     nlat, lat          in-plane real-space displacements (nlat, 3), nlat >= 1: (2 nlatvec + 1)^2 of them for any nlatvec
     nion, ion_xyz, ion_charge
                        ions (nion, 3) / (nion); nion = 0: the handle's atoms and charges
     walker_chunk       walkers per scratch chunk; 0: the estimator units' own bound
   mean = 0: ee, ei (W) per walker; mean = 1: the walker means (one double each), reduced on the device in a fixed order that does
   not depend on the chunk size (no atomics: two calls give the same bits).  Every handle kind with pbc != 0 (coordinates are
   folded into the cell first: twisted handles keep unfolded ones); open-boundary handles are refused (<0).  Read-only on the
   resident state: the coordinates are read in place from whichever layout holds them. */
typedef struct {
  double alpha, area, self_const;
  int32_t nk;
  const int32_t* kn;
  const double* knorm;
  const double* kpref;
  double recip[6];
  int32_t nlat;
  const double* lat;
  int32_t nion;
  const double* ion_xyz;
  const double* ion_charge;
  int64_t walker_chunk;
} pqa_ewald2d_t;
int pqa_ewald2d(pqa_handle_t* h, const pqa_ewald2d_t* tab, int mean, double* ee, double* ei);

/* ---- correlated evaluation of parameter sets (line minimisation) ---------------------------------- */
/* correlated_compute_worker (pyqmc/method/linemin.py:378-409): the resident walkers evaluated at K sets of the two-body Jastrow
   coefficients acoeff (K, natom, na, 2) and bcoeff (K, nb, 3).  Row k equals, within rounding, what this sequence gives on the same
   handle: upload set k's acoeff / bcoeff; pqa_wf_recompute -> logpsi[k] (W); pqa_energy(threshold, rot, unif, seed) -> en[k]
   (6, W), with the same draws for every k (the reference resets numpy's random state before every set, linemin.py:394-397).
   The Jastrow factor is linear in its coefficients, so the Slater part is evaluated once per call (a Slater-only energy pass:
   Coulomb / Ewald, local ECP channel, ECP points with their Slater-weighted values) and each set only contracts basis-resolved
   Jastrow rows (per electron grad / laplacian, per ECP point B(q) - B(r_e)) with its coefficients; logpsi[k] = log|Psi| + U_k - U
   from the basis sums the handle keeps.  The handle's coefficients, walkers, inverses and basis sums are not written; as
   pqa_energy it syncs a lane-per-walker layout back and drops saved gradient_value rows, as pqa_wf_value it refreshes stale basis
   sums.  Real single-determinant Slater x two-body Jastrow handles with the semi-local ECP integrator, open or periodic; anything
   else is refused. */
int pqa_correlated(pqa_handle_t* h, int K, const double* acoeff, const double* bcoeff, double threshold, const double* rot,
                   const double* unif, uint64_t seed, double* logpsi, double* en);

/* The same evaluation for one or more determinants, with the determinant coefficients varying between the sets as well
   (correlated_compute_worker, linemin.py:378-409, for the Slater.parameters["det_coeff"] of slater.py:301-380 and
   determinant_tools.compute_value, determinant_tools.py:74-88): det_coeff (K, ndet), acoeff (K, natom, na, 2), bcoeff (K, nb, 3);
   NULL for a coefficient array means that every set uses the handle's own.  Row k equals, within rounding, upload set k's
   det_coeff / acoeff / bcoeff; pqa_wf_recompute -> logpsi[k]; pqa_energy(threshold, rot, unif, seed) -> en[k] (6, W: ke, ee, ei,
   ecp, grad2, total).  The Slater factor is linear in det_coeff and nothing about a determinant changes between the sets: with
   omega_d the weight of determinant d without its coefficient and rho_u the row products of unique determinant u (gradient,
   laplacian, ECP point), set k has S_k = sum_d c_kd omega_d, grad D / D = sum_d c_kd omega_d rho_u(d) / S_k, and
   logpsi[k] = log|Psi| - log|S_0| + log|S_k| - U_0 + U_k.  One Slater-only energy pass supplies Coulomb / Ewald, the local ECP
   channel and the ECP point lists with their orbital rows; the determinant sums of all sets are one product per walker on the fp64
   matrix cores (k_corr_md, csrc/pqa_correlated.hip), the Jastrow part is pqa_correlated's.  Every sum has a fixed order: two calls
   give the same bits, and the result does not depend on walker_chunk (walkers per output chunk; 0: at most 256 MiB).  Writes as
   pqa_correlated: none to the walkers, inverses, determinants or coefficients.  Real Slater x two-body Jastrow handles, open or
   periodic (untwisted), no three-body factor, the semi-local ECP integrator or no ECP; anything else, and an LDS plan that does
   not fit, is refused. */
int pqa_correlated_md(pqa_handle_t* h, int K, const double* det_coeff, const double* acoeff, const double* bcoeff, double threshold,
                      const double* rot, const double* unif, uint64_t seed, long walker_chunk, double* logpsi, double* en);

/* The same evaluation for handles with a three-body Jastrow factor (three_body_jastrow.py:19-655), whose coefficients vary between
   the sets as well: pqa_correlated_md's arguments with ccoeff (K, natom, na3, na3, nb3, 3) after bcoeff; NULL for an array means
   that every set uses the handle's own.  Each set's ccoeff is symmetrised as the handle's is, C = (c + c^T_kl) / 2.  U3 is linear
   in C, and C enters only through its contraction with the a-functions of the moving electron: per electron (and per ECP point,
   values only) the wave builds the C-independent tables M_c[I][l][m][s'] = sum_{j != e, spin s'} a_l(r_jI) {b_m, grad b_m, lap b_m}
   (r_e - r_j) once, and every set contracts them and the a-triples of r_eI with its own coefficients to P_e, grad P_e, lap P_e (the
   J3 instantiations of k_corr_md); grad U3 and lap U3 join the two-body terms of the set, an ECP point's exponent gains
   P_e(q) - P_e(r_e), and logpsi[k] gains U3_k - U3_0 with U3 = 1/2 sum_e P_e(r_e), both from the same kernel.  Fixed summation
   orders: two calls give the same bits, whatever walker_chunk.  Writes as pqa_correlated_md: none to the walkers, inverses,
   determinants, coefficients or the three-body value.  Real, untwisted Slater x two-body x three-body Jastrow handles with one or
   more determinants, open or periodic at Gamma, the semi-local ECP integrator or no ECP; anything else, and an LDS plan that does
   not fit, is refused. */
int pqa_correlated_j3(pqa_handle_t* h, int K, const double* det_coeff, const double* acoeff, const double* bcoeff, const double* ccoeff,
                      double threshold, const double* rot, const double* unif, uint64_t seed, long walker_chunk, double* logpsi, double* en);

/* ---- stochastic-reconfiguration moments from the resident state ----------------------------------- */
/* StochasticReconfiguration.avg (stochastic_reconfiguration.py:49-118) on the resident walkers, without the walkers or the
   derivative arrays crossing the bus.  Column i of the serialised derivative matrix dp (W, P) is entry pos[i] (flat C-order index)
   of the parameter src[i] names: 0 det_coeff (ndet), 1 acoeff (natom, na, 2), 2 bcoeff (nb, 3), 3 ccoeff (natom, na3, na3, nb3, 3);
   src and pos are host arrays of P entries.  The energy pass is pqa_energy's (threshold, rot, unif, seed as there: the per-walker
   energies are the same bits).  With the weights w (W, host or device; NULL: 1 / W; normalised by their sum) and the Pathak-Wagner
   weight f of grad2 at nodal_cutoff (x = 1 / (grad2 cutoff^2); f = x (9 - 15 x + 7 x^2) where x < 1, else 1):
     en_mean (6)         sum_w w E_k for ke, ee, ei, ecp, grad2, total,
     moments (P + 2, P)  row-major: rows 0 .. P-1 dpidpj = sum_w dp_i (w f dp_j), row P dpH = sum_w E (w f dp_j) with E the total
                         energy, row P + 1 dppsi = sum_w (w f dp_j),
     en_walker (W, 6)    the per-walker energies, or NULL: nothing of size W leaves the device.
   The product runs on the fp64 matrix cores over walker chunks of at most 256 MiB of gathered columns; the walker sums have a fixed
   order (two calls give the same bits) and dpidpj is exactly symmetric.  The walkers, inverses, determinants and coefficients are
   not written; as pqa_energy the call syncs a lane-per-walker layout back and drops saved gradient_value rows, as pqa_wf_value it
   refreshes stale basis sums.  Real handles (open or periodic, one or more determinants, with or without the three-body factor,
   either ECP integrator); complex / twisted handles, a column of a factor the handle lacks, and moments beyond 256 MiB are refused
   (<0): those go through the protocol route.  Orbital coefficients are not a source here: pqa_sr_moments_orb below takes them. */
int pqa_sr_moments(pqa_handle_t* h, int P, const int32_t* src, const int32_t* pos, double nodal_cutoff, const double* weights,
                   double threshold, const double* rot, const double* unif, uint64_t seed, double* en_mean, double* moments,
                   double* en_walker);

/* pqa_sr_moments with the orbital coefficients as sources: everything above, and
     src 4 mo_coeff_alpha, 5 mo_coeff_beta   pos: flat C-order index into (nao, nmo_s);
     walker_chunk       walkers per chunk; 0: as many as keep a chunk's gathered columns and AO rows, (P + 2 + N nao) doubles per walker,
                        within 256 MiB (a smaller value makes a small case run several chunks);
     dp_walker (W, P)   host array or NULL: the compact derivative matrix dp the moments were formed from (tests and tools).
   The derivative of walker w and spin s, G[a][m] = sum_u wu[u] sum_e ao[e][a] T_u[e][col_u(m)] with wu[u] the sum of
   det_coeff[di] d_det[w][di] over the determinants whose spin-s part is u (Slater.pgradient, slater.py:507-533), is formed as
   G = ao^T B with B[e][m] = sum_u wu[u] T_u[e][col_u(m)]: one fp64 matrix-core product per walker and spin whatever the number of
   determinants (k_sr_orb), its entries stored straight into the selected columns.  No (W, nao, nmo) or (W N, nao) array exists:
   the AO values are evaluated per walker chunk.  Sums run k-steps ascending, determinants ascending: two calls give the same bits.
   Without a source 4 / 5 the result is pqa_sr_moments' bit for bit.  Writes go to scratch only, as there.  Orbital sources need a
   real open-boundary handle with at most 64 electrons and 64 orbitals of the spin and at least one electron of it; periodic (per-k
   parameter layout), complex and twisted handles, a pos outside (nao, nmo_s) or named twice are refused (<0): those go through the
   protocol route. */
int pqa_sr_moments_orb(pqa_handle_t* h, int P, const int32_t* src, const int32_t* pos, double nodal_cutoff, const double* weights,
                       double threshold, const double* rot, const double* unif, uint64_t seed, int64_t walker_chunk, double* en_mean,
                       double* moments, double* en_walker, double* dp_walker);

/* pqa_sr_moments for complex columns: complex or twisted handles (complex determinant derivatives, complex local energy) and the
   imaginary-part tail of the reference's serialised derivative matrix (LinearTransform.serialize_gradients, accumulators.py:134-150).
     src / pos (P)      as pqa_sr_moments: sources 0 det_coeff, 1 acoeff, 2 bcoeff, 3 ccoeff (orbital sources 4 / 5 are refused);
     ntail, tail        tail column t is i times primary column tail[t]; Pt = P + ntail columns in all.  An index outside 0 .. P - 1
                        or named twice is refused;
     walker_chunk       walkers per chunk; 0: as many as keep the two planes of a chunk's gathered columns within 256 MiB;
     en_mean (7)        weighted means of ke, ee, ei, Re ecp, grad2, Re total, Im ecp (Im total = Im ecp; a real handle: 0);
     moments            (Pt + 2, Pt) complex, (re, im) interleaved: rows dpidpj (Pt), dpH, dppsi.  No conjugation anywhere:
                        dpidpj = dp^T diag(w f) dp is complex symmetric, exactly;
     en_walker (W, 7)   the per-walker rows, or NULL;
     dp_walker (W, Pt)  complex interleaved host array or NULL: the derivative matrix the moments were formed from (tests and tools).
   With A = [dp | E | 1] = Ar + i Ai the product is Re M = Ar^T s Ar - Ai^T s Ai, Im M = Ar^T s Ai + Ai^T s Ar on the fp64 matrix
   cores; a 32-column block without a column that can have an imaginary part (every Jastrow column, the 1 column, everything of a real
   handle) stages no imaginary panel, so a block pair costs 1, 2 or 4 matrix instructions per step.  Fixed summation order (two calls
   give the same bits); state left alone and saved gradient_value rows dropped as in pqa_sr_moments.  Real handles are accepted (their
   imaginary parts are exactly zero).  Complex moments beyond 256 MiB are refused (<0): those go through the protocol route. */
int pqa_sr_moments_c(pqa_handle_t* h, int P, const int32_t* src, const int32_t* pos, int ntail, const int32_t* tail, double nodal_cutoff,
                     const double* weights, double threshold, const double* rot, const double* unif, uint64_t seed, int64_t walker_chunk,
                     double* en_mean, double* moments, double* en_walker, double* dp_walker);

/* ---- variance of the local energy at parameter sets (variance optimisation) ------------------------------------------------------ */
/* optvariance.py:44-54 on the resident walkers, for K sets of two-body Jastrow coefficients acoeff (K,natom,na,2),
   bcoeff (K,nb,3).  eoff (W) = Enref total - Enref ke per walker.  For set k:
     ke[k][w]  kinetic energy with set k (NULL: not written),
     var[k]    population variance (ddof 0) over w of eoff[w] + ke[k][w],
     dvar[k]   (P) d var[k] / d c, acoeff entries then bcoeff entries in their array order (NULL: not computed).
   Only the kinetic energy is evaluated (the Jastrow rows of pqa_correlated, no Coulomb, no ECP); ke agrees with pqa_correlated's ke
   row.  The walker reductions run on the device in a fixed order (two calls give the same bits).  The handle's coefficients,
   walkers, inverses and basis sums are not written (a lane-per-walker layout is synced back, as pqa_energy does).  Real
   single-determinant Slater x two-body Jastrow handles, open or periodic, with or without ECP; anything else is refused. */
int pqa_variance(pqa_handle_t* h, int K, const double* acoeff, const double* bcoeff, const double* eoff, double* ke, double* var,
                 double* dvar);

/* ---- mixture sampling of several wave functions (excited states) ------------------------------------------------------------------ */
/* sample_overlap_worker (pyqmc/method/sample_many.py:130-186) without its accumulator: nsteps Metropolis sweeps of the walkers resident
   on the K handles hs[0..K-1] with the distribution sum_k |Psi_k|^2, all on the device.  Every electron move does what the protocol
   route (MultiplyWF.gradient / gradient_value / value / updateinternals per handle) does: the proposal x + gauss + tstep limdrift(mean_k
   grad_k), the acceptance t_prob sum_k |ratio_k|^2 w_k / sum_k w_k with w_k = exp(2 (log|Psi_k| - log|Psi_0|)) against unif, and the
   Sherman-Morrison + Jastrow updates of all K handles under the one accept mask; a handle whose determinants of the moved spin had
   vanished (slater.py:269-275) has its Slater state rebuilt from the moved walkers instead.  gauss (nsteps*N, W, 3) already scaled by
   sqrt(tstep) and unif (nsteps*N, W) are the reference's draws in its order.  After each sweep n, overlap[n] (K, K) is the walker mean
   of psi_i psi_j / rho (compute_weights, :42-55); weights (K, K, W) or NULL receives the last sweep's per-walker values; acc_ratio or
   NULL the accepted fraction of all moves.  Scope: real Slater x two-body Jastrow handles (pqa_wf_eval's), any number of
   determinants, open boundaries, one device, equal W, N and nelec_up, distinct handles, K <= 8; anything else is refused and the
   caller takes the protocol route.  All K handles' work runs on hs[0]'s stream.  Afterwards every handle holds the state the
   protocol route would leave (walkers, inverses, determinants, Jastrow sums); saved gradient_value rows are dropped.  Errors are
   reported on hs[0]. */
int pqa_overlap_sweeps(pqa_handle_t* const* hs, int K, double tstep, int nsteps, const double* gauss, const double* unif,
                       double* overlap, double* weights, double* acc_ratio);

/* ---- estimators over the mixture of several wave functions (excited-state optimisation) ------------------------------------------- */
/* StochasticReconfigurationMultipleWF.avg (stochastic_reconfiguration.py:195-227) and EnergyAccumulatorMultipleWF.avg
   (accumulators_multiwf.py:29-60) on the walkers resident on the K handles hs[0..K-1] (which hold the same walkers, e.g. after
   pqa_overlap_sweeps), without the walkers, the per-walker energies or the derivative arrays crossing the bus.  With compute_weights'
   (sample_many.py:42-55) a_k = phase_k exp(log|Psi_k| - max_j log|Psi_j|), rho = mean_k a_k^2 and weights[i][j][c] = a_i (a_j / rho)
   per walker c (its nan_to_num rules included; the code is pqa_overlap_sweeps'):
     overlap (K, K)      mean_c weights[i][j][c],
     en (6, K, K)        en[r][i][j] = sum_c (E_j^r(c) - offset) weights[i][j][c] / W for the rows r = ke, ee, ei, ecp, grad2, total of
                         state j's local energy,
     moments             state after state, for the states with P[i] > 0, (P[i] + 2K, P[i]) row-major: rows 0 .. P[i]-1
                         dpipj = sum_c dp_p dp_q weights[i][i][c] / W; rows P[i] + j: dp[:, j] = sum_c dp_p weights[i][j][c] / W; rows
                         P[i] + K + j: dpH[:, j] = sum_c E_j dp_p weights[i][j][c] / W with E_j state j's total energy (no offset),
     u_walker (K, W)     a_k / sqrt(rho) per walker, or NULL,
     en_walker (K, W, 6) every state's per-walker energies, or NULL: nothing of size W leaves the device.
   Column q of state i's derivative matrix dp (W, P[i]) is entry pos[q] (flat C-order index) of the parameter src[q] names on hs[i]:
   0 det_coeff (ndet), 1 acoeff (natom, na, 2), 2 bcoeff (nb, 3); src and pos hold sum_i P[i] entries, state after state; P[i] = 0: the
   state has no columns (all zero: only overlap and en are formed).  Each handle runs pqa_energy's pass with its own key seeds[k], or,
   with rot / unif given, its own set of draws (K sets as pqa_energy takes them, one after the other): the per-walker energies are the
   bits pqa_energy gives for that key.  The weights have rank one per walker, so all moments of a state are one product
   A^T diag(1 / (rho W)) A[:, :P] with A = [a_i dp | a_0 .. a_{K-1} | E_0 a_0 .. E_{K-1} a_{K-1}]: it runs on the fp64 matrix cores over
   walker chunks of at most 256 MiB of gathered columns (walker_chunk > 0: at most that many walkers per chunk); the walker sums have
   a fixed order (two calls give the same bits; the result does not depend on walker_chunk) and dpipj is exactly symmetric.
   Scope: pqa_overlap_sweeps' (real Slater x two-body Jastrow handles, any number of determinants, open boundaries, one device, equal
   W, N and nelec_up, distinct handles, K <= 8) and sources 0 - 2; periodic, twisted, complex or three-body handles, other sources and
   moments of a state beyond 256 MiB are refused (<0): those go through the protocol route.  All K handles' work runs on hs[0]'s
   stream; errors are reported on hs[0].  The walkers, inverses, determinants and coefficients are not written; as pqa_sr_moments the
   call syncs a lane-per-walker layout back, drops saved gradient_value rows and refreshes stale basis sums.

   pqa_mix_wtdp: StochasticReconfigurationWfbyWf.avg (ensemble_optimization_wfbywf.py:57-66): wtdp[j][k][p] = sum_c dp_p(c)
   weights[j][k][c] / W with the derivatives dp (W, P) of the LAST state hs[K-1] (src, pos as above, P >= 1), and overlap (K, K).  No
   energy pass.  The thin product of the K (K + 1) / 2 weight columns with j <= k against dp, on the same kernels; wtdp[j][k] and
   wtdp[k][j] are the same row (equal bits).  Scope, stream, determinism and writes as pqa_mix_moments. */
int pqa_mix_moments(pqa_handle_t* const* hs, int K, const int32_t* P, const int32_t* src, const int32_t* pos, double offset,
                    double threshold, const double* rot, const double* unif, const uint64_t* seeds, int64_t walker_chunk,
                    double* overlap, double* en, double* moments, double* u_walker, double* en_walker);
int pqa_mix_wtdp(pqa_handle_t* const* hs, int K, int P, const int32_t* src, const int32_t* pos, int64_t walker_chunk, double* overlap,
                 double* wtdp);

/* ---- superposition of several wave functions (AddWF) ------------------------------------------------------------------------------- */
/* Psi = sum_k coeffs[k] Psi_k (pyqmc/wf/addwf.py) over the walkers resident on the K handles hs[0..K-1], which hold the same walkers.
   With w_k = coeffs[k] Psi_k / Psi per walker (sum_k w_k = 1), formed as c_k sign_k exp(log|Psi_k| - max_j log|Psi_j|) over their sum
   (the maximum is the walker's own, not the ensemble's as in the reference: no 0 / 0 when walkers differ by hundreds in log|Psi|).
   Scope of all three, pqa_overlap_sweeps': real Slater x two-body Jastrow handles (pqa_wf_eval's), any number of determinants, open
   boundaries, one device, equal W, N and nelec_up, distinct handles, K <= 8, real coeffs; anything else is refused and the caller takes
   the protocol route.  All K handles' work runs on hs[0]'s stream; saved gradient_value rows are dropped; errors are reported on hs[0].

   pqa_add_weights: sign (W) and logabs (W) of Psi and w (K, W); any of the three may be NULL.  Each handle's own value stays on the
   device.

   pqa_add_sweeps: nsteps sweeps of vmc_worker (pyqmc/method/mc.py:112-137) over |Psi|^2, all on the device.  Every electron move does what
   the protocol route (AddWF.gradient_value twice, updateinternals with saved_values) does: with v_k = Psi_k(R') / Psi_k(R) the drift
   sum_k rho_k grad_k, rho_k = w_k v_k / sum_j w_j v_j, under MultiplyWF.gradient_value's non-finite rules per handle; the proposal
   x + gauss + tstep limdrift(drift); the acceptance t_prob |sum_k w_k v_k|^2 against unif; the Sherman-Morrison + Jastrow updates of all K
   handles under the one accept mask, a handle whose determinants of the moved spin had vanished (slater.py:269-275) having its Slater
   state rebuilt from the moved walkers instead.  gauss (nsteps*N, W, 3) already scaled by sqrt(tstep) and unif (nsteps*N, W) are the
   reference's draws in its order.  acc (nsteps) or NULL receives each sweep's accepted fraction.  Afterwards every handle holds the state
   the protocol route would leave (walkers, inverses, determinants, Jastrow sums).

   pqa_add_energy: out (6, W) = ke, ee, ei, ecp, grad2, total of Psi (the rows of pqa_energy).  Every handle runs its own energy pass
   (pqa_energy's; semi-local ECP integrator only) with the SAME rot / unif, or the same seed where they are NULL: E_L = sum_k w_k E_L,k
   holds only for one set of ECP rotations and mask draws.  ke = sum_k w_k ke_k, ecp = sum_k w_k ecp_k, ee and ei are hs[0]'s, total =
   ke + ee + ei + ecp + the ion-ion energy; grad2 = sum_e |sum_k w_k grad_e Psi_k / Psi_k|^2 from an electron loop at the current
   positions.  The handles' rows and the combination stay on the device; only out comes back.  The walker state is not written. */
int pqa_add_weights(pqa_handle_t* const* hs, int K, const double* coeffs, double* sign, double* logabs, double* w);
int pqa_add_sweeps(pqa_handle_t* const* hs, int K, const double* coeffs, double tstep, int nsteps, const double* gauss,
                   const double* unif, double* acc);
int pqa_add_energy(pqa_handle_t* const* hs, int K, const double* coeffs, double threshold, const double* rot, const double* unif,
                   uint64_t seed, double* out);

/* ---- measurement -------------------------------------------------------------------- */
/* HIP-event timing on the handle's own stream (torch.cuda.Event only sees torch's stream). */
int pqa_timer_start(pqa_handle_t* h);
int pqa_timer_stop(pqa_handle_t* h, double* elapsed_ms); /* synchronises the stream */
int pqa_sync(pqa_handle_t* h);
/* per-kernel-class accounting: enable=1 brackets every launch of the orbital (AO->MO MFMA) kernel
   with events; query returns launches, total ms, total points*ncomp processed since enable. */
int pqa_profile_enable(pqa_handle_t* h, int enable);
int pqa_profile_query(pqa_handle_t* h, int64_t* launches, double* total_ms, double* point_comps);
/* same accounting for the streaming kernel of the fused lane-per-walker sweep: the flush launches of the blocked
   Sherman-Morrison update (rows outside the current electron block, once per block of KB moves; none when KB = n) */
int pqa_profile_query_commit(pqa_handle_t* h, int64_t* launches, double* total_ms);
/* and for the partial-sum kernel of the fused sweep (k_move_part_lw: Slater ratio sums + the Jastrow distance sums of the
   proposal, jastrowspin.py:296-340): launches bracketed (the proposal-side launch of every prof-stride-th electron), their
   total ms, and the number of partial-sum groups per walker the launch geometry uses at the resident walker count */
int pqa_profile_query_part(pqa_handle_t* h, int64_t* launches, double* total_ms, int* groups);
/* the per-walker energy rows of the LAST evaluation on the resident walkers, in pqa_energy's layout ([6][W]: ke, ee, ei, ecp, grad2,
   total; complex wave functions [7][W]) — also of the evaluation that ended the last step of pqa_vmc_sweeps / pqa_dmc_steps, which
   return walker means only.  Fails when no evaluation has run at the resident walker count. */
int pqa_energy_last(pqa_handle_t* h, double* out);
/* points evaluated by the ECP integrator in the last pqa_energy call (data dependent) */
int pqa_last_ecp_points(pqa_handle_t* h, int64_t* npoints);

#ifdef __cplusplus
}
#endif
#endif
