// Correlated evaluation of K Jastrow parameter sets on the resident walkers (correlated_compute_worker, pyqmc/method/linemin.py:378-409).
//
// The reference sets each parameter set, recomputes the whole wave function and runs the energy accumulator, with the random state
// reset before every set.  Only the two-body Jastrow coefficients differ between the sets here, and U is linear in them:
// U = sum_p c_p B_p(R), and so are grad_e U, lap_e U and the ECP exponent U(e -> q) - U(e).  The call therefore splits into
//   once per call   the Slater-only energy pass (energy_dev with EnergyOpts::slater_only): Coulomb / Ewald, the local ECP channel and
//                   the ECP point lists with their Slater-weighted values s_q = (D(e -> q) / D) w_q (b_econ), the same draws for all
//                   sets; the log values from the basis sums the handle keeps (k_corr_u);
//   per walker      k_corr_energy: per electron grad D / D and lap D / D (from the orbital-row cache), the basis-resolved Jastrow rows
//                   (grad_e B_p, lap_e B_p) in LDS, and for every ECP point the row B_p(q) - B_p(r_e) (jas_rows / jas_diff_rows,
//                   pqa_estim.hpp); each row is contracted with the (P x K) coefficient matrix, one set per lane, and combined per set:
//                   ke_k = -1/2 sum_e [lap D/D + 2 grad D/D . grad U_k + lap U_k + |grad U_k|^2],  grad2_k = sum_e |grad D/D + grad U_k|^2,
//                   ecp_k = local + sum_q s_q exp(dU_k(q)),  total_k = ke_k + ee + ei + ecp_k + ii.
// The handle's coefficients are never changed.  Outputs are written per walker chunk of at most 256 MiB.
// Several determinants, with det_coeff varying between the sets too: pqa_correlated_md / k_corr_md, further down; with a three-body
// factor whose ccoeff varies as well: pqa_correlated_j3, the J3 instantiations of k_corr_md.
// The three entries are one-line calls into one host driver, correlated_run, which an entry descriptor (CorrEntry) steers: one scope
// table, one staging of the coefficient sets, one argument struct (CorrArgs) and one plan of the scratch.  The kernels stay two:
// k_corr_energy is the default route, and its single-determinant ratios (slater_ratios) are not the bits of k_corr_md with one
// determinant.  What they share is factored once: the contractions of the Jastrow rows (jas_contract4 / jas_contract1,
// pqa_estim.hpp), the energy rows (corr_write_rows) and, between the two three-body contractions, the column walk (j3_column).
#include "pqa_estim.hpp"

namespace {

// U[k][w] = sum_i bvalues[w][i] c_b[k][i] + sum_i avalues[w][i] c_a[k][i] for k < K1: one wave per walker, the summation order of
// jas_value_wave (k_jastrow_value), so the row of the handle's own coefficients reproduces its Jastrow value bit for bit.
__global__ __launch_bounds__(64) void k_corr_u(const double* __restrict__ aval, const double* __restrict__ bval,
                                               const double* __restrict__ ca /*[K1][Pa]*/, const double* __restrict__ cb /*[K1][Pb]*/,
                                               int Pa, int Pb, int K1, long W, double* __restrict__ U /*[K1][W]*/) {
  const long w = blockIdx.x;
  const int lane = threadIdx.x;
  const double* bv = bval + (size_t)w * Pb;
  const double* av = aval + (size_t)w * Pa;
  for (int k = 0; k < K1; ++k) {
    double u = 0.0;
    for (int i = lane; i < Pb; i += 64) u += bv[i] * cb[(size_t)k * Pb + i];
    for (int i = lane; i < Pa; i += 64) u += av[i] * ca[(size_t)k * Pa + i];
    u = wave_sum(u);
    if (lane == 0) U[(size_t)k * W + w] = u;
  }
}

// The arguments of k_corr_energy and of k_corr_md (further down), filled by corr_args and the driver.
struct CorrArgs {
  long w0, Wc, W;           // first walker of the chunk, walkers in it, resident walkers
  int K, K1, P, Pa;         // sets, columns of cd and c3t (K + 1), Jastrow coefficients per set (acoeff then bcoeff), of which acoeff
  const double* ct;         // [P][K] Jastrow coefficient matrix
  const double* kc;         // [4][W] rows ke, ee, ei, grad2 of the Slater-only pass (ee, ei used)
  const double* local;      // [W] local ECP channel
  const double* econ[2];    // per spin: Slater-weighted point values (k_corr_energy)
  const double* wgt[2];     // per spin: point weights (k_corr_md)
  const double* emo[2];     // per spin: orbital rows of the points [n][nmo_s] (k_corr_md)
  const double* pts[2];     // per spin: point positions [n][3]
  const int* pte[2];        // per spin: electron of the point
  const long* off;          // [2][nseg W + 1] list offsets (k_ecp_sum's order)
  int nseg, has_ecp;
  double ii;
  double* out;              // [K][6][Wc]
  // k_corr_md only
  int DP, RS, GS;           // LDS strides: unique determinants of a component, a row of rho (= 2 mod 32), a row of num
  const double* cd;         // [ndet][K1] determinant coefficient matrix (column K: the handle's own)
  // its three-body instantiations (J3) only
  const double* c3t;        // [P3][K1] symmetrised three-body coefficient matrix (column K: the handle's own)
  double* u3;               // [K1][W] three-body log value U3_k = 1/2 sum_e P_e^k(r_e)
};

// The six energy rows of set k, walker w (column bw of the chunk): ke, ee, ei, ecp = local + tot, grad2, total.
__device__ __forceinline__ void corr_write_rows(const CorrArgs& A, long w, long bw, int k, double ke, double g2, double tot) {
  const double ee = A.kc[A.W + w], ei = A.kc[2 * A.W + w], ec = A.has_ecp ? A.local[w] + tot : 0.0;
  double* o = A.out + (size_t)k * 6 * A.Wc + bw;
  o[0] = ke; o[A.Wc] = ee; o[2 * A.Wc] = ei; o[3 * A.Wc] = ec; o[4 * A.Wc] = g2; o[5 * A.Wc] = ke + ee + ei + ec + A.ii;
}

// One wave per walker (grid.x), lanes = parameter sets kb + lane (grid.y: chunks of 64 sets).  LDS: rows R[4][P] (ke_electron).
template <bool PBC>
__global__ __launch_bounds__(64) void k_corr_energy(SysDev S, SlaterState st, JastrowState js, CorrArgs A) {
  extern __shared__ double R[];
  const int lane = threadIdx.x;
  const long bw = blockIdx.x, w = A.w0 + bw;
  const int k = blockIdx.y * 64 + lane;
  const bool act = k < A.K;
  const int P = A.P, Pa = A.Pa, N = S.nelec;
  const double* xw = js.x + (size_t)w * N * 3;
  const double irb = 1.0 / S.rcut_b, ira = 1.0 / S.rcut_a;
  double ke = 0.0, g2 = 0.0;
  for (int e = 0; e < N; ++e)
    ke_electron<PBC>(S, st, xw, w, e, P, Pa, ira, irb, R, A.ct, A.K, k, act, [&](double lap, double tx, double ty, double tz) {
      ke += -0.5 * lap;
      g2 += tx * tx + ty * ty + tz * tz;
    });
  // ECP: every point of the walker in k_ecp_sum's order (spin up then down, segment by segment); row B_p(q) - B_p(r_e)
  double tot = 0.0;
  if (A.has_ecp) {
    const size_t SS = (size_t)A.nseg * A.W + 1;
    for (int sp = 0; sp < 2; ++sp)
      for (int seg = 0; seg < A.nseg; ++seg) {
        const long* o = A.off + sp * SS + (size_t)seg * A.W + w;
        for (long pt = o[0]; pt < o[1]; ++pt) {
          const int e = A.pte[sp][pt], s = e >= S.nup;
          const double qx = A.pts[sp][3 * pt], qy = A.pts[sp][3 * pt + 1], qz = A.pts[sp][3 * pt + 2];
          jas_diff_rows<PBC>(S, xw, e, s, qx, qy, qz, P, Pa, ira, irb, R);
          if (act) tot += A.econ[sp][pt] * exp(jas_contract1(S, R, A.ct, A.K, k, s, Pa));
          __syncthreads();
        }
      }
  }
  if (act) corr_write_rows(A, w, bw, k, ke, g2, tot);
}

// ---------------------------------------------------------------------------------------------------------------------------------
// Several determinants (pqa_correlated_md): det_coeff varies between the sets as well.  Nothing about a determinant changes between
// the sets, the Slater factor is linear in det_coeff and U in acoeff / bcoeff.  For walker w and full determinant d with unique spin
// determinants u_up(d), u_dn(d) (det_map):
//   omega_d      = sign_up sign_dn exp(log_up + log_dn - ref)            det_weight (pqa_slater.hpp) without det_coeff[d], ref = det_ref
//   rho_u[e][c]  = sum_j cache[w][i][c][occ_u[j]] T_u[i][j]              electron e = (spin s, index i), unique determinant u of s,
//                                                                        c = value, d/dx, d/dy, d/dz, laplacian (slater_ratios<5>'s
//                                                                        products before it mixes determinants); for an ECP point q
//                                                                        of e the same with the point's orbital row b_emo[s][q][.]
// and for set k with determinant coefficients c_k, S_k = sum_d c_kd omega_d:
//   G_k[e][c]    = sum_d c_kd omega_d rho_{u_s(d)}[e][c] / S_k           grad D / D (c = x, y, z) and lap D / D of set k; the kernel
//                                                                        divides by the value component's sum instead of S_k, the
//                                                                        quotient ke_electron and the reference's gradient_laplacian
//                                                                        form: rho[value] = 1 for an exact inverse, and where a sweep's
//                                                                        rank-1 updates left rounding in T the quotient cancels it
//   r_k(q)       = sum_d c_kd omega_d rho_{u_s(d)}(q) / S_k              Slater ratio Psi_S,k(e -> q) / Psi_S,k
//   log|Psi_k|   = log|Psi| - log|S_0| + log|S_k| - U_0 + U_k            0: the handle's own coefficients (column K of the matrices)
//   lap_e        = G_k[e][lap] + lap U_k + |grad U_k|^2 + 2 G_k[e][xyz] . grad U_k,   ke_k = -1/2 sum_e lap_e,
//   grad2_k      = sum_e |G_k[e][xyz] + grad U_k|^2,   ecp_k = local + sum_q wgt_q r_k(q) exp(dU_k(q)),   ee, ei, ii as they are.
// The determinant part is one product ((5 N + npts) x ndet) . (ndet x K) per walker, the only cost that grows as ndet K: it runs on
// v_mfma_f64_16x16x4_f64.
//
// k_corr_md: one wave per walker (grid.x), set columns kb .. kb + 63 (grid.y).  One wave, not four: the Jastrow rows come from
// jas_rows / jas_diff_rows, the one-wave helpers k_corr_energy and k_var_ke share.
//   phase 0  omega_d into LDS (det_ref first); lane = set: S_k, determinants ascending.
//   per tile of 16 electrons (both spins in index order) or 16 ECP points of one list segment:
//   phase 1  rho_u[row][c] for every unique determinant of the row's spin on the vector unit (slots ascending), into LDS
//            [row][c][u], row stride = 2 mod 32 doubles: the 16 rows x 2 k-steps a half-wave reads lie 32 banks apart;
//   phase 2  num[c][row][k] = sum_d (omega_d rho_{u(d)}[row][c]) C[d][k] through mfma_tiles / mfma_tile: the A operand is gathered
//            through det_map on load (zero beyond ndet and the row tail), the B operand is the coefficient matrix in L2 (zero
//            beyond K); the five component accumulators of a tile are independent; the tile goes to LDS [c][row][column] for the
//            transpose to lane = set;
//   phase 3  per row the Jastrow rows and their contraction with ct, one set per lane, combined with num[c] / num[value] (an
//            electron) or num / S_k (a point) as above; the ECP
//            points in k_ecp_sum's order (spin up then down, segment by segment, points ascending).
// Every sum has a fixed order (k-steps, determinants, electrons, points ascending): two calls give the same bits, whatever the chunk.
__device__ __forceinline__ double md_omega(const SysDev& S, const SlaterState& st, long w, int d, double ref) {
  const double su = st.dsign[0][w * S.ndet_s[0] + S.det_map[d]];
  const double sd = st.dsign[1][w * S.ndet_s[1] + S.det_map[S.ndet + d]];
  const double l = det_logsum(S, st, w, d);
  return su * sd * ((l == -INFINITY) ? 0.0 : exp(l - ref));
}

// S[k][w] = sum_d cd[d][k] omega_d for k < K1 (determinants ascending, as k_corr_md's phase 0).  One wave per walker; LDS: ndet doubles.
__global__ __launch_bounds__(64) void k_corr_md_s(SysDev S, SlaterState st, const double* __restrict__ cd, int K1, long W,
                                                   double* __restrict__ out /*[K1][W]*/) {
  extern __shared__ double om[];
  const long w = blockIdx.x;
  const int lane = threadIdx.x;
  const double ref = det_ref(S, st, w);
  for (int d = lane; d < S.ndet; d += 64) om[d] = md_omega(S, st, w, d, ref);
  __syncthreads();
  for (int k = lane; k < K1; k += 64) {
    double s = 0.0;
    for (int d = 0; d < S.ndet; ++d) s += cd[(size_t)d * K1 + k] * om[d];
    out[(size_t)k * W + w] = s;
  }
}

// LDS of k_corr_md in doubles: omega [ndet (even)], rho [16][RS], num [5][16][GS], R [4][P]
inline size_t corr_md_lds(int ndet, int RS, int GS, int P) { return (size_t)((ndet + 1) & ~1) + (size_t)16 * RS + (size_t)80 * GS + (size_t)4 * P; }

// ---------------------------------------------------------------------------------------------------------------------------------
// Three-body factor (pqa_correlated_j3): ccoeff varies between the sets too.  U3 is linear in C (symmetrised in (k, l) by the host as
// set_c3 does), and C enters jas3_eval only through its contraction with the moving electron's a-functions (pqa_jastrow.hpp).  For
// electron e of spin s_e at r (its own position, or an ECP point q), with d_eI = r - R_I and partner spin s':
//   M_c[I][l][m][s'] = sum_{j != e, spin s'} a_l(r_jI) {b_m, (b_m'/r) d_x, d_y, d_z, lap b_m}(r - r_j)        c = 0 .. 4, C-independent
//   t_c[I][k]        = sum_{l m s'} C_k[I][k][l][m][s_e + s'] M_c[I][l][m][s']                                 per set (lane)
//   P_e      = sum_{I k} a_k t_0,     grad P_e = sum_{I k} (a_k'/r) d_eI t_0 + a_k t_{1..3},
//   lap P_e  = sum_{I k} (lap a_k) t_0 + 2 (a_k'/r) d_eI . t_{1..3} + a_k t_4                                  a_k = a_k(r_eI)
// the sums of jas3_eval_n regrouped.  grad U3 = grad P_e and lap U3 = lap P_e join the two-body rows' sums of the set, an ECP point
// adds P_e(q) - P_e(r_e) to the exponent, and U3_k = 1/2 sum_e P_e(r_e) goes to u3 for the log value (column K, the handle's own
// coefficients, through the same code: the difference U3_k - U3_0 cancels what the regrouping rounds differently from the handle's
// value).  The whole wave builds the tables once per electron or point; each lane then walks its own set's column of c3t, a read
// coalesced over the lanes as ct's.  An ECP point needs the value table alone, so the five table slots hold up to five positions of
// one electron at a time (consecutive points of the list, and r_e itself when the electron is new): the lane reads each coefficient
// once for all of them (c3t lives in L2: P3 K1 doubles, 189 KB for water at K = 40; measured 10 - 20 % of a call: DESIGN section 47).
// Sums run over partners, ions, k, l, m, s' ascending, whatever the grouping.  No per-lane arrays beyond t_c: nothing depends on an
// unrolled length, so there is one instantiation for every na3, nb3 <= PQA_MAXBAS3.
// LDS (doubles): aj [N][natom][na3] a_l(r_jI) of every electron, once per walker; M [5][natom][na3][nb3][2]; at [5][natom][na3] the
// a-triples (slots 0 .. 2) or the a-values of five positions; de [natom][3]; bj [N][5][nb3] the partners' b-functions.
struct J3Lds { double *aj, *M, *at, *de, *bj; };

inline size_t corr_j3_lds(int N, int natom, int na3, int nb3) {
  return (size_t)N * natom * na3 + (size_t)5 * natom * na3 * nb3 * 2 + (size_t)5 * natom * na3 + (size_t)3 * natom + (size_t)5 * N * nb3;
}

__device__ __forceinline__ J3Lds j3_lds(const SysDev& S, double* p) {
  J3Lds L;
  L.aj = p;
  L.M = L.aj + (size_t)S.nelec * S.natom * S.na3;
  L.at = L.M + (size_t)5 * S.natom * S.na3 * S.nb3 * 2;
  L.de = L.at + (size_t)5 * S.natom * S.na3;
  L.bj = L.de + (size_t)3 * S.natom;
  return L;
}

// aj of the walker whose coordinates are xw (one wave; complete for every lane on return)
template <bool PBC>
__device__ __forceinline__ void j3_partner_a(const SysDev& S, const double* xw, const J3Lds& L) {
  const int lane = threadIdx.x, A = S.natom, na = S.na3;
  const double ira = 1.0 / S.rcut_a3;
  for (int q = lane; q < S.nelec * A; q += 64) {
    const int j = q / A, I = q - j * A;
    double d[3];
    const double r = jrow_dist<PBC>(S, xw[3 * j] - S.atom_xyz[3 * I], xw[3 * j + 1] - S.atom_xyz[3 * I + 1], xw[3 * j + 2] - S.atom_xyz[3 * I + 2], d);
    const bool in = r < S.rcut_a3;
    const RadShared sh = rad_shared<0>(in ? r : 0.5 * S.rcut_a3, ira);
    for (int l = 0; l < na; ++l) {
      double v = 0.0, g, lp;
      if (in) rad_fn<0>(S.a3_kind[l], S.a3_param[l], S.a3_aux[l], S.rcut_a3, sh, v, g, lp);
      L.aj[(size_t)q * na + l] = v;
    }
  }
  __syncthreads();
}

// M[c][I][l][m][s'] = sum_{j of spin s'} aj[j][I][l] bj[j][c][m] for the slots c < nc (partners ascending; bj is zero for j = e and
// outside the cutoff).  Lanes over the table entries; starts and ends with a barrier.
__device__ __forceinline__ void j3_table_sums(const SysDev& S, int nc, const J3Lds& L) {
  const int lane = threadIdx.x, N = S.nelec, A = S.natom, na = S.na3, nb = S.nb3, nlm = na * nb * 2, TS = A * nlm;
  __syncthreads();
  for (int t = lane; t < nc * TS; t += 64) {
    const int c = t / TS, rem = t - c * TS, I = rem / nlm, r2 = rem - I * nlm;
    const int l = r2 / (2 * nb), m = (r2 >> 1) % nb, sp = r2 & 1;
    const int j0 = sp ? S.nup : 0, j1 = sp ? N : S.nup;
    double acc = 0.0;
    for (int j = j0; j < j1; ++j) acc += L.aj[((size_t)j * A + I) * na + l] * L.bj[((size_t)j * 5 + c) * nb + m];
    L.M[t] = acc;
  }
  __syncthreads();
}

// The tables of electron e placed at (rx, ry, rz): M_0 .. M_4, the a-triples and d_eI.  One wave; complete for every lane on return.
template <bool PBC>
__device__ __forceinline__ void j3_tables(const SysDev& S, const double* xw, int e, double rx, double ry, double rz, const J3Lds& L) {
  constexpr int NC = 5;
  const int lane = threadIdx.x, N = S.nelec, A = S.natom, na = S.na3, nb = S.nb3;
  const double ira = 1.0 / S.rcut_a3, irb = 1.0 / S.rcut_b3;
  __syncthreads();  // (the lanes' contractions with the previous tables are over)
  for (int I = lane; I < A; I += 64) {
    double d[3];
    const double r = jrow_dist<PBC>(S, rx - S.atom_xyz[3 * I], ry - S.atom_xyz[3 * I + 1], rz - S.atom_xyz[3 * I + 2], d);
    const bool in = r < S.rcut_a3;
    const RadShared sh = rad_shared<2>(in ? r : 0.5 * S.rcut_a3, ira);
    L.de[3 * I] = d[0]; L.de[3 * I + 1] = d[1]; L.de[3 * I + 2] = d[2];
    for (int k = 0; k < na; ++k) {
      double v = 0.0, g = 0.0, lp = 0.0;
      if (in) rad_fn<2>(S.a3_kind[k], S.a3_param[k], S.a3_aux[k], S.rcut_a3, sh, v, g, lp);
      L.at[I * na + k] = v; L.at[(A + I) * na + k] = g; L.at[(2 * A + I) * na + k] = lp;
    }
  }
  for (int j = lane; j < N; j += 64) {
    double d[3];
    const double r = jrow_dist<PBC>(S, rx - xw[3 * j], ry - xw[3 * j + 1], rz - xw[3 * j + 2], d);
    const bool in = j != e && r < S.rcut_b3;
    const RadShared sh = rad_shared<2>(in ? r : 0.5 * S.rcut_b3, irb);
    double* row = L.bj + (size_t)j * NC * nb;
    for (int m = 0; m < nb; ++m) {
      double v = 0.0, g = 0.0, lp = 0.0;
      if (in) rad_fn<2>(S.b3_kind[m], S.b3_param[m], S.b3_aux[m], S.rcut_b3, sh, v, g, lp);
      row[m] = v; row[nb + m] = g * d[0]; row[2 * nb + m] = g * d[1]; row[3 * nb + m] = g * d[2]; row[4 * nb + m] = lp;
    }
  }
  j3_table_sums(S, NC, L);
}

// Value tables of np <= 5 positions pos(c) (pointers to x, y, z) of electron e: slot c of M and of at as above.
template <bool PBC, class F>
__device__ __forceinline__ void j3_point_tables(const SysDev& S, const double* xw, int e, int np, F&& pos, const J3Lds& L) {
  const int lane = threadIdx.x, N = S.nelec, A = S.natom, na = S.na3, nb = S.nb3;
  const double ira = 1.0 / S.rcut_a3, irb = 1.0 / S.rcut_b3;
  __syncthreads();  // (the lanes' contractions with the previous tables are over)
  for (int q = lane; q < np * A; q += 64) {
    const int c = q / A, I = q - c * A;
    const double* p = pos(c);
    double d[3];
    const double r = jrow_dist<PBC>(S, p[0] - S.atom_xyz[3 * I], p[1] - S.atom_xyz[3 * I + 1], p[2] - S.atom_xyz[3 * I + 2], d);
    const bool in = r < S.rcut_a3;
    const RadShared sh = rad_shared<0>(in ? r : 0.5 * S.rcut_a3, ira);
    for (int k = 0; k < na; ++k) {
      double v = 0.0, g, lp;
      if (in) rad_fn<0>(S.a3_kind[k], S.a3_param[k], S.a3_aux[k], S.rcut_a3, sh, v, g, lp);
      L.at[(c * A + I) * na + k] = v;
    }
  }
  for (int q = lane; q < np * N; q += 64) {
    const int c = q / N, j = q - c * N;
    const double* p = pos(c);
    double d[3];
    const double r = jrow_dist<PBC>(S, p[0] - xw[3 * j], p[1] - xw[3 * j + 1], p[2] - xw[3 * j + 2], d);
    const bool in = j != e && r < S.rcut_b3;
    const RadShared sh = rad_shared<0>(in ? r : 0.5 * S.rcut_b3, irb);
    for (int m = 0; m < nb; ++m) {
      double v = 0.0, g, lp;
      if (in) rad_fn<0>(S.b3_kind[m], S.b3_param[m], S.b3_aux[m], S.rcut_b3, sh, v, g, lp);
      L.bj[((size_t)j * 5 + c) * nb + m] = v;
    }
  }
  j3_table_sums(S, np, L);
}

// t[c] = sum_{l m s'} c3t[(I, k, l, m, edown + s')][kcol] M_c[I][l][m][s'] for the five table slots c: the walk down column kcol of c3t
// that both contractions make for ion I and function k (l m, then s', ascending).
__device__ __forceinline__ void j3_column(const SysDev& S, int edown, const J3Lds& L, const double* __restrict__ c3t, int K1, int kcol, int I,
                                          int k, double (&t)[5]) {
  const int A = S.natom, na = S.na3, nb = S.nb3, nlm = na * nb * 2, TS = A * nlm;
  const double* Mp = L.M + (size_t)I * nlm;
  const double* cp = c3t + ((size_t)(I * na + k) * na * nb * 3 + edown) * K1 + kcol;
#pragma unroll
  for (int c = 0; c < 5; ++c) t[c] = 0.0;
  for (int lm = 0; lm < na * nb; ++lm)
#pragma unroll
    for (int sp = 0; sp < 2; ++sp) {
      const double cc = cp[(size_t)(lm * 3 + sp) * K1];
#pragma unroll
      for (int c = 0; c < 5; ++c) t[c] += cc * Mp[(size_t)c * TS + lm * 2 + sp];
    }
}

// Column kcol of c3t against the value tables of np <= 5 positions: out[c] = P_e(position c); one read of each coefficient serves
// them all (slots beyond np hold leftovers, and so do their out[c]).
__device__ __forceinline__ void j3_contract_points(const SysDev& S, int edown, const J3Lds& L, const double* __restrict__ c3t, int K1, int kcol,
                                                   double (&out)[5]) {
  const int A = S.natom, na = S.na3;
#pragma unroll
  for (int c = 0; c < 5; ++c) out[c] = 0.0;
  for (int I = 0; I < A; ++I)
    for (int k = 0; k < na; ++k) {
      double t[5];
      j3_column(S, edown, L, c3t, K1, kcol, I, k, t);
#pragma unroll
      for (int c = 0; c < 5; ++c) out[c] += L.at[(c * A + I) * na + k] * t[c];
    }
}

// Column kcol of c3t against the tables of j3_tables: out[0] = P_e, out[1 .. 3] = grad P_e, out[4] = lap P_e.
__device__ __forceinline__ void j3_contract(const SysDev& S, int edown, const J3Lds& L, const double* __restrict__ c3t, int K1, int kcol,
                                            double (&out)[5]) {
  const int A = S.natom, na = S.na3;
#pragma unroll
  for (int c = 0; c < 5; ++c) out[c] = 0.0;
  for (int I = 0; I < A; ++I) {
    for (int k = 0; k < na; ++k) {
      double t[5];
      j3_column(S, edown, L, c3t, K1, kcol, I, k, t);
      const double a = L.at[I * na + k], ag = L.at[(A + I) * na + k], al = L.at[(2 * A + I) * na + k];
      const double dx = L.de[3 * I], dy = L.de[3 * I + 1], dz = L.de[3 * I + 2];
      out[0] += a * t[0];
      out[1] += ag * dx * t[0] + a * t[1];
      out[2] += ag * dy * t[0] + a * t[2];
      out[3] += ag * dz * t[0] + a * t[3];
      out[4] += al * t[0] + 2.0 * ag * (dx * t[1] + dy * t[2] + dz * t[3]) + a * t[4];
    }
  }
}

// J3: the three-body instantiations (pqa_correlated_j3).  Block column blockIdx.y covers the K1 = K + 1 columns of c3t: the lane of
// column K (the handle's own coefficients) takes part in the three-body value alone.
template <bool PBC, bool J3>
__global__ __launch_bounds__(64) void k_corr_md(SysDev S, SlaterState st, JastrowState js, CorrArgs A) {
  extern __shared__ double sm[];
  const int lane = threadIdx.x, i16 = lane & 15, kq = lane >> 4;
  const long bw = blockIdx.x, w = A.w0 + bw;
  const int kb = blockIdx.y * 64, k = kb + lane;
  const bool act = k < A.K;
  const int ndet = S.ndet, N = S.nelec, P = A.P, Pa = A.Pa, DP = A.DP, RS = A.RS, GS = A.GS;
  const int ntile = ((A.K - kb < 64 ? A.K - kb : 64) + 15) / 16;  // 16-set column tiles of this block
  double* om = sm;
  double* rho = om + ((ndet + 1) & ~1);
  double* G = rho + (size_t)16 * RS;
  double* R = G + (size_t)80 * GS;
  const double* xw = js.x + (size_t)w * N * 3;
  const double irb = 1.0 / S.rcut_b, ira = 1.0 / S.rcut_a;
  const bool act3 = J3 && k < A.K1;  // (three-body value: the sets and the handle's own column)
  J3Lds L3{};
  double u3 = 0.0;
  if constexpr (J3) {
    L3 = j3_lds(S, R + (size_t)4 * P);
    j3_partner_a<PBC>(S, xw, L3);
  }
  // phase 0
  const double ref = det_ref(S, st, w);
  for (int d = lane; d < ndet; d += 64) om[d] = md_omega(S, st, w, d, ref);
  __syncthreads();
  double Sk = 0.0;
  if (act)
    for (int d = 0; d < ndet; ++d) Sk += A.cd[(size_t)d * A.K1 + k] * om[d];
  const double invS = 1.0 / Sk;
  auto bop = [&](int col) {
    return [&A, col](int kd, bool kin) { return (kin && col < A.K) ? A.cd[(size_t)kd * A.K1 + col] : 0.0; };
  };
  // kinetic terms: tiles of 16 electrons
  double ke = 0.0, g2 = 0.0;
  for (int e0 = 0; e0 < N; e0 += 16) {
    const int rows = N - e0 < 16 ? N - e0 : 16;
    for (int q = lane; q < 16 * DP; q += 64) {  // phase 1
      const int row = q / DP, u = q - row * DP, e = e0 + row;
      if (row >= rows) continue;
      const int s = e >= S.nup, D = S.ndet_s[s];
      if (u >= D) continue;
      const int i = e - s * S.nup, n = s ? S.ndn : S.nup, nmo = S.nmo[s];
      const double* T = st.T[s] + (((size_t)w * D + u) * n + i) * n;
      const int* occ = S.det_occ[s] + (size_t)u * n;
      const double* ch = st.cache[s] + ((size_t)w * n + i) * 5 * nmo;
      double a[5] = {0.0, 0.0, 0.0, 0.0, 0.0};
      for (int j = 0; j < n; ++j) {
        const double t = T[j];
        const int o = occ[j];
#pragma unroll
        for (int c = 0; c < 5; ++c) a[c] += ch[c * nmo + o] * t;
      }
#pragma unroll
      for (int c = 0; c < 5; ++c) rho[row * RS + c * DP + u] = a[c];
    }
    __syncthreads();
    {  // phase 2
      const int erow = e0 + i16;
      const bool rin = i16 < rows;
      const int* dm = S.det_map + ((rin && erow >= S.nup) ? ndet : 0);
      const double* rr = rho + i16 * RS;
      for (int t = 0; t < ntile; ++t) {
        d4 acc[5];
        mfma_tiles<5>(ndet, kq, [&](int c, int kd, bool kin) { return (kin && rin) ? om[kd] * rr[c * DP + dm[kd]] : 0.0; },
                      bop(kb + t * 16 + i16), acc);
#pragma unroll
        for (int c = 0; c < 5; ++c)
#pragma unroll
          for (int r = 0; r < 4; ++r) G[(c * 16 + kq + 4 * r) * GS + t * 16 + i16] = acc[c][r];
      }
    }
    __syncthreads();
    for (int row = 0; row < rows; ++row) {  // phase 3
      const int e = e0 + row, s = e >= S.nup;
      jas_rows<PBC>(S, xw, e, s, xw[3 * e], xw[3 * e + 1], xw[3 * e + 2], P, Pa, ira, irb, R);
      double p3[5] = {0.0, 0.0, 0.0, 0.0, 0.0};
      if constexpr (J3) {
        j3_tables<PBC>(S, xw, e, xw[3 * e], xw[3 * e + 1], xw[3 * e + 2], L3);
        if (act3) {
          j3_contract(S, s, L3, A.c3t, A.K1, k, p3);
          u3 += 0.5 * p3[0];
        }
      }
      if (act) {
        const double v = G[row * GS + lane];
        const double G0 = G[(16 + row) * GS + lane] / v, G1 = G[(32 + row) * GS + lane] / v, G2 = G[(48 + row) * GS + lane] / v;
        const double L = G[(64 + row) * GS + lane] / v;
        jas_contract4(S, R, A.ct, A.K, k, s, P, Pa, [&](double gx, double gy, double gz, double lp) {
          if constexpr (J3) { gx += p3[1]; gy += p3[2]; gz += p3[3]; lp += p3[4]; }
          const double lj = lp + gx * gx + gy * gy + gz * gz;
          const double lap = L + lj + 2.0 * (G0 * gx + G1 * gy + G2 * gz);
          const double tx = G0 + gx, ty = G1 + gy, tz = G2 + gz;
          ke += -0.5 * lap;
          g2 += tx * tx + ty * ty + tz * tz;
        });
      }
      __syncthreads();
    }
  }
  // ECP: tiles of 16 points of one list segment
  double tot = 0.0;
  int last_e = -1;      // (J3: the electron whose P_e(r_e) the lane holds in p_old, reused while consecutive points share it)
  double p_old = 0.0;
  if (A.has_ecp && (!J3 || kb < A.K)) {  // (a block with the handle's own column alone has no set to evaluate)
    const size_t SS = (size_t)A.nseg * A.W + 1;
    for (int sp = 0; sp < 2; ++sp) {
      const int n = sp ? S.ndn : S.nup, nmo = S.nmo[sp], D = S.ndet_s[sp];
      const int* dm = S.det_map + sp * ndet;
      for (int seg = 0; seg < A.nseg; ++seg) {
        const long* o = A.off + sp * SS + (size_t)seg * A.W + w;
        const long p0 = o[0], p1 = o[1];
        for (long pb = p0; pb < p1; pb += 16) {
          const int rows = p1 - pb < 16 ? (int)(p1 - pb) : 16;
          for (int q = lane; q < 16 * DP; q += 64) {  // phase 1
            const int row = q / DP, u = q - row * DP;
            if (row >= rows || u >= D) continue;
            const int i = A.pte[sp][pb + row] - sp * S.nup;
            const double* T = st.T[sp] + (((size_t)w * D + u) * n + i) * n;
            const int* occ = S.det_occ[sp] + (size_t)u * n;
            const double* mo = A.emo[sp] + (size_t)(pb + row) * nmo;
            double a = 0.0;
            for (int j = 0; j < n; ++j) a += mo[occ[j]] * T[j];
            rho[row * RS + u] = a;
          }
          __syncthreads();
          {  // phase 2
            const bool rin = i16 < rows;
            const double* rr = rho + i16 * RS;
            for (int t = 0; t < ntile; ++t) {
              const d4 acc = mfma_tile(ndet, kq, [&](int kd, bool kin) { return (kin && rin) ? om[kd] * rr[dm[kd]] : 0.0; },
                                       bop(kb + t * 16 + i16));
#pragma unroll
              for (int r = 0; r < 4; ++r) G[(kq + 4 * r) * GS + t * 16 + i16] = acc[r];
            }
          }
          __syncthreads();
          // (J3) groups of consecutive points of one electron share the five table slots, the first slot for r_e when the electron is new
          double pv[5] = {0.0, 0.0, 0.0, 0.0, 0.0};
          int gnext = 0, gslot = 0;  // first row behind the current group; the slot of the row at hand
          for (int row = 0; row < rows; ++row) {  // phase 3
            const long pt = pb + row;
            const int e = A.pte[sp][pt];
            double dp3 = 0.0;
            if constexpr (J3) {
              if (row == gnext) {
                const int o = e != last_e;
                int g = 1;
                while (g + o < 5 && row + g < rows && A.pte[sp][pt + g] == e) ++g;
                j3_point_tables<PBC>(S, xw, e, g + o, [&](int c) { return c < o ? xw + 3 * e : A.pts[sp] + 3 * (pt + c - o); }, L3);
                if (act) {
                  j3_contract_points(S, sp, L3, A.c3t, A.K1, k, pv);
                  if (o) p_old = pv[0];
                }
                last_e = e; gnext = row + g; gslot = o;
              }
              dp3 = (gslot == 0 ? pv[0] : gslot == 1 ? pv[1] : gslot == 2 ? pv[2] : gslot == 3 ? pv[3] : pv[4]) - p_old;
              ++gslot;
            }
            jas_diff_rows<PBC>(S, xw, e, sp, A.pts[sp][3 * pt], A.pts[sp][3 * pt + 1], A.pts[sp][3 * pt + 2], P, Pa, ira, irb, R);
            if (act) {
              double du = jas_contract1(S, R, A.ct, A.K, k, sp, Pa);
              if constexpr (J3) du += dp3;
              tot += A.wgt[sp][pt] * (G[row * GS + lane] * invS) * exp(du);
            }
            __syncthreads();
          }
        }
      }
    }
  }
  if constexpr (J3)
    if (act3) A.u3[(size_t)k * A.W + w] = u3;
  if (act) corr_write_rows(A, w, bw, k, ke, g2, tot);
}

// ---------------------------------------------------------------------------------------------------------------------------------
// host: one driver for the three entries

// What an entry is: its name (in messages), whether det_coeff is read (k_corr_md with k_corr_md_s and the determinant term of the log
// value; else k_corr_energy), whether ccoeff is read (the J3 instantiations; implies det), and whether a NULL coefficient array
// means the handle's own (else acoeff and bcoeff are required).
struct CorrEntry {
  const char* name;
  bool det, j3, own;
};

// Scope: a real Slater x two-body Jastrow handle with the semi-local ECP integrator or no ECP.  !det: one determinant, possibly
// twisted; det: one or more determinants, untwisted, no three-body factor; j3: the same with a three-body factor, which the handle
// must then have.  The first row that applies is the reason.
int correlated_scope(pqa_handle* h, const CorrEntry& en) {
  if (!en.det) TRY(linear_jastrow_scope(h, en.name));  // (the single-determinant handle and its LDS row block: pqa_variance's rule)
  const char* const needs = en.j3 ? "needs a Slater x two-body x three-body Jastrow handle" : "needs a Slater x two-body Jastrow handle";
  const char* const per_set = " (others: set, recompute and evaluate per set)";
  const struct { bool refuse; const char *why, *hint; } rows[] = {
      {en.det && (!h->has_slater || !h->has_j2), needs, per_set},
      {en.det && (h->cplx || h->twist), "complex orbitals / twisted cell", per_set},
      {en.det && !en.j3 && h->has_j3, "three-body Jastrow factor", per_set},
      {en.j3 && !h->has_j3, needs, per_set},
      {en.det && h->necp > 0 && h->ecpb_on, "batched ECP integrator", per_set},
      // the single-determinant entry alone also refuses the ECP pass with a wave per point (en.ecp_wave), and the batched integrator
      // whether or not there is an ECP: the other two take both, and the difference stands as it is
      {!en.det && (h->ecpb_on || h->en.ecp_wave), "needs the semi-local ECP integrator's thread-per-point pass", " (evaluate per set)"},
  };
  for (const auto& r : rows)
    if (r.refuse) FAIL(std::string(en.name) + ": " + r.why + r.hint);
  return 0;
}

using CorrKernel = void (*)(SysDev, SlaterState, JastrowState, CorrArgs);
const CorrKernel corr_kernels[3][2] = {  // [k_corr_energy, k_corr_md, its J3 instantiation][open, periodic]
    {k_corr_energy<false>, k_corr_energy<true>}, {k_corr_md<false, false>, k_corr_md<true, false>}, {k_corr_md<false, true>, k_corr_md<true, true>}};

// The fields every entry's kernel reads, after the Slater-only energy pass: the shapes, the pass's rows and its ECP point lists.
CorrArgs corr_args(pqa_handle* h, int K, int P, int Pa) {
  CorrArgs A{};
  A.W = h->W; A.K = K; A.K1 = K + 1; A.P = P; A.Pa = Pa; A.kc = (const double*)h->b_kc.p; A.ii = h->ii_energy; A.has_ecp = h->necp > 0;
  if (A.has_ecp) {
    A.local = (const double*)h->b_elocal.p; A.off = (const long*)h->b_eoff.p; A.nseg = h->en.last_nseg;
    for (int s = 0; s < 2; ++s) {
      A.econ[s] = (const double*)h->b_econ[s].p; A.wgt[s] = (const double*)h->b_ewgt[s].p; A.emo[s] = (const double*)h->b_emo[s].p;
      A.pts[s] = (const double*)h->b_epts[s].p; A.pte[s] = (const int*)h->b_epte[s].p;
    }
  }
  return A;
}

// The host driver of the three entries (en: which).  det_coeff and ccoeff are read where the entry says so; walker_chunk_arg is 0 for
// the entry without that argument.
int correlated_run(pqa_handle_t* h, const CorrEntry& en, int K, const double* det_coeff, const double* acoeff, const double* bcoeff,
                   const double* ccoeff, double threshold, const double* rot, const double* unif, uint64_t seed, long walker_chunk_arg,
                   double* logpsi, double* energy) {
  const std::string fn = en.name;
  HIPCHK(hipSetDevice(h->device));
  if (h->W == 0) FAIL("state not initialised (call pqa_wf_recompute)");
  if (K < 1) FAIL(fn + ": K must be at least 1");
  if (!logpsi || !energy || (!en.own && (!acoeff || !bcoeff)))
    FAIL(fn + (en.own ? ": logpsi and en must not be NULL" : ": acoeff, bcoeff, logpsi and en must not be NULL"));
  if (walker_chunk_arg < 0) FAIL(fn + ": walker_chunk must be 0 (the 256 MiB rule) or positive");
  TRY(correlated_scope(h, en));
  const long W = h->W;
  const int ndet = en.det ? h->ndet : 0, Pa = h->natom * h->na * 2, Pb = h->nb * 3, P = Pa + Pb, K1 = K + 1;
  const int P3 = en.j3 ? h->natom * h->na3 * h->na3 * h->nb3 * 3 : 0;
  // the LDS plan: refused where it does not fit, never truncated (k_corr_energy: the rows R[4][P] alone, which the scope has checked)
  const int DP = std::max(h->ndet_s[0], h->ndet_s[1]), RS = ((5 * DP + 29) / 32) * 32 + 2;
  const int ncol = ((std::min(K, 64) + 15) / 16) * 16, GS = ncol + ((ncol % 32 == 0) ? 16 : 0);
  const size_t lds = (en.det ? corr_md_lds(ndet, RS, GS, P) + (en.j3 ? corr_j3_lds(h->N, h->natom, h->na3, h->nb3) : 0) : (size_t)4 * P) * sizeof(double);
  if (lds > 160 * 1024)
    FAIL(fn + (en.j3 ? ": the determinant rows, Jastrow rows and three-body tables of a 16-row tile exceed the LDS of a CU (others: set, recompute and evaluate per set)"
                     : ": the determinant rows and Jastrow rows of a 16-row tile exceed the LDS of a CU (others: set, recompute and evaluate per set)"));
  const CorrKernel kernel = corr_kernels[en.j3 ? 2 : en.det ? 1 : 0][h->S.pbc ? 1 : 0];
  const char* const kname = en.det ? "k_corr_md" : "k_corr_energy";
  if (lds > 64 * 1024) TRY(raise_lds_limit(h, (const void*)kernel));
  // log|Psi| at the handle's own coefficients (as pqa_wf_value: refreshes the basis sums a fused sweep left stale)
  std::vector<double> lg0((size_t)W);
  TRY(pqa_wf_value(h, nullptr, lg0.data()));
  // [K1][n] rows of each coefficient array: rows 0 .. K-1 the sets (host or device memory; NULL: the handle's own), row K the handle's own
  HIPCHK(hipStreamSynchronize(h->stream));
  auto rows_in = [&](std::vector<double>& dst, const double* src, const double* own, int n) -> int {
    dst.resize((size_t)K1 * n);
    if (!n) return 0;
    HIPCHK(hipMemcpy(dst.data() + (size_t)K * n, own, (size_t)n * sizeof(double), hipMemcpyDeviceToHost));
    if (src) HIPCHK(hipMemcpy(dst.data(), src, (size_t)K * n * sizeof(double), hipMemcpyDefault));
    else
      for (int k = 0; k < K; ++k) std::copy(dst.begin() + (size_t)K * n, dst.end(), dst.begin() + (size_t)k * n);
    return 0;
  };
  std::vector<double> ca, cb, cdr, c3;
  TRY(rows_in(ca, acoeff, h->d_acoeff, Pa));
  TRY(rows_in(cb, bcoeff, h->d_bcoeff, Pb));
  TRY(rows_in(cdr, det_coeff, h->d_detcoeff, ndet));
  TRY(rows_in(c3, ccoeff, h->d_c3, P3));
  const std::vector<double> ct = pack_coef_sets(ca.data(), cb.data(), K, Pa, Pb);
  std::vector<double> cd((size_t)ndet * K1);  // [ndet][K1]
  for (int k = 0; k < K1; ++k)
    for (int d = 0; d < ndet; ++d) cd[(size_t)d * K1 + k] = cdr[(size_t)k * ndet + d];
  // three-body sets, symmetrised in (k, l) as set_c3 does (the handle's own, d_c3, already is): [P3][K1], column K the handle's own
  std::vector<double> c3t((size_t)P3 * K1);
  if (en.j3) {
    const int na3 = h->na3, m3 = h->nb3 * 3;
    for (int k = 0; k < K1; ++k) {
      const double* c = c3.data() + (size_t)k * P3;
      const bool sym = k < K && ccoeff;
      for (int I = 0; I < h->natom; ++I)
        for (int a = 0; a < na3; ++a)
          for (int l = 0; l < na3; ++l)
            for (int m = 0; m < m3; ++m) {
              const size_t p = (((size_t)I * na3 + a) * na3 + l) * m3 + m, q = (((size_t)I * na3 + l) * na3 + a) * m3 + m;
              c3t[p * K1 + k] = sym ? 0.5 * (c[p] + c[q]) : c[p];
            }
    }
  }
  // the Slater-only energy pass, once, with the ECP totals read on the host
  TRY(sync_aos(h));
  h->saved_valid = false;  // (as pqa_energy: the saved orbital rows of a gradient_value call are overwritten)
  EnergyOpts eo;
  eo.slater_only = true; eo.host_totals = true;
  TRY(energy_dev(h, threshold, rot, unif, seed, 0u, eo));
  CorrArgs A = corr_args(h, K, P, Pa);
  if (A.has_ecp && (h->en.last_tot[0] < 0 || h->en.last_tot[1] < 0)) FAIL(fn + ": ECP point totals were left on the device");
  // device scratch (b_out is sized by every user on entry), one plan for its size and its pieces: the coefficient rows for k_corr_u, U,
  // the Jastrow matrix and a chunk of outputs; with det the determinant matrix and S; with j3 the three-body matrix and U3
  const long Wc = walker_chunk_arg > 0 ? std::min(W, walker_chunk_arg) : walker_chunk(W, (size_t)K * 6 * sizeof(double));
  const size_t nu = (size_t)K1 * W;
  double *d_ca, *d_cb, *d_u, *d_ct, *d_o, *d_cd, *d_s, *d_c3t, *d_u3;
  const std::pair<double**, size_t> plan[] = {{&d_ca, (size_t)K1 * std::max(Pa, 1)}, {&d_cb, (size_t)K1 * std::max(Pb, 1)}, {&d_u, nu},
                                              {&d_ct, ct.size()}, {&d_o, (size_t)K * 6 * Wc}, {&d_cd, cd.size()}, {&d_s, en.det ? nu : 0},
                                              {&d_c3t, c3t.size()}, {&d_u3, en.j3 ? nu : 0}};
  size_t total = 0;
  for (const auto& pc : plan) total += pc.second;
  TRY(ensure(h, h->b_out, total * sizeof(double)));
  double* next = (double*)h->b_out.p;
  for (const auto& pc : plan) { *pc.first = next; next += pc.second; }
  TRY(copy_in(h, d_ca, ca.data(), ca.size() * sizeof(double)));
  TRY(copy_in(h, d_cb, cb.data(), cb.size() * sizeof(double)));
  TRY(copy_in(h, d_ct, ct.data(), ct.size() * sizeof(double)));
  TRY(copy_in(h, d_cd, cd.data(), cd.size() * sizeof(double)));
  TRY(copy_in(h, d_c3t, c3t.data(), c3t.size() * sizeof(double)));
  hipLaunchKernelGGL(k_corr_u, dim3((unsigned)W), dim3(64), 0, h->stream, (const double*)h->js.avalues, (const double*)h->js.bvalues,
                     (const double*)d_ca, (const double*)d_cb, Pa, Pb, K1, W, d_u);
  TRY(check_launch(h, "k_corr_u"));
  if (en.det) {
    hipLaunchKernelGGL(k_corr_md_s, dim3((unsigned)W), dim3(64), (size_t)ndet * sizeof(double), h->stream, h->S, h->st, (const double*)d_cd, K1, W, d_s);
    TRY(check_launch(h, "k_corr_md_s"));
  }
  A.ct = d_ct; A.out = d_o; A.DP = DP; A.RS = RS; A.GS = GS; A.cd = d_cd; A.c3t = d_c3t; A.u3 = d_u3;
  for (long w0 = 0; w0 < W; w0 += Wc) {
    A.w0 = w0; A.Wc = std::min(Wc, W - w0);
    const dim3 g((unsigned)A.Wc, (unsigned)(((en.j3 ? K1 : K) + 63) / 64));  // (J3: the handle's own column rides along for U3)
    hipLaunchKernelGGL(kernel, g, dim3(64), lds, h->stream, h->S, h->st, h->js, A);
    TRY(check_launch(h, kname));
    // [K][6][Wc] -> energy [K][6][W] columns w0 ..
    HIPCHK(hipMemcpy2DAsync(energy + w0, (size_t)W * sizeof(double), d_o, (size_t)A.Wc * sizeof(double), (size_t)A.Wc * sizeof(double),
                            (size_t)K * 6, hipMemcpyDefault, h->stream));
  }
  // log|Psi_k| = log|Psi| - U_0 + U_k, with det also - log|S_0| + log|S_k|, with j3 also - U3_0 + U3_k (0: the handle's own, row K)
  std::vector<double> u(nu), sv(en.det ? nu : 0), v3(en.j3 ? nu : 0);
  TRY(copy_out(h, u.data(), d_u, u.size() * sizeof(double)));
  if (en.det) TRY(copy_out(h, sv.data(), d_s, sv.size() * sizeof(double)));
  if (en.j3) TRY(copy_out(h, v3.data(), d_u3, v3.size() * sizeof(double)));
  std::vector<double> lp((size_t)K * W);
  for (int k = 0; k < K; ++k)
    for (long w = 0; w < W; ++w) {
      const size_t i = (size_t)k * W + w, i0 = (size_t)K * W + w;
      lp[i] = en.det ? lg0[w] + (std::log(std::fabs(sv[i])) - std::log(std::fabs(sv[i0]))) + (u[i] - u[i0]) : lg0[w] - u[i0] + u[i];
      if (en.j3) lp[i] += v3[i] - v3[i0];
    }
  HIPCHK(hipMemcpy(logpsi, lp.data(), lp.size() * sizeof(double), hipMemcpyDefault));
  return 0;
}

}  // namespace

extern "C" int pqa_correlated(pqa_handle_t* h, int K, const double* acoeff, const double* bcoeff, double threshold, const double* rot,
                              const double* unif, uint64_t seed, double* logpsi, double* en) {
  return correlated_run(h, {"pqa_correlated", false, false, false}, K, nullptr, acoeff, bcoeff, nullptr, threshold, rot, unif, seed, 0, logpsi, en);
}

extern "C" int pqa_correlated_md(pqa_handle_t* h, int K, const double* det_coeff, const double* acoeff, const double* bcoeff, double threshold,
                                 const double* rot, const double* unif, uint64_t seed, long walker_chunk_arg, double* logpsi, double* en) {
  return correlated_run(h, {"pqa_correlated_md", true, false, true}, K, det_coeff, acoeff, bcoeff, nullptr, threshold, rot, unif, seed, walker_chunk_arg,
                        logpsi, en);
}

extern "C" int pqa_correlated_j3(pqa_handle_t* h, int K, const double* det_coeff, const double* acoeff, const double* bcoeff, const double* ccoeff,
                                 double threshold, const double* rot, const double* unif, uint64_t seed, long walker_chunk_arg, double* logpsi,
                                 double* en) {
  return correlated_run(h, {"pqa_correlated_j3", true, true, true}, K, det_coeff, acoeff, bcoeff, ccoeff, threshold, rot, unif, seed, walker_chunk_arg,
                        logpsi, en);
}
