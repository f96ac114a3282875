// Pair ratios of the two-body density matrix (TBDMAccumulator, pyqmc/observables/tbdm.py:232-246) from the resident state, read-only
// on the wave function's handle, and their contraction on the orbital evaluator's handle without a trip through the host.
//
// For walker w and kept sample k the auxiliary points r1 = pos[slot 0][k][assign_a[w]], r2 = pos[slot 1][k][assign_b[w]] live on the
// evaluator handle; R[w][a][b] = Psi(r_a -> r1, r_b -> r2) / Psi for every electron a of spin block s1 and b of spin block s2.  The
// reference moves a to r1 (testvalue + updateinternals), reads the partners' ratios (testvalue_many) and moves a back; for a
// Slater x JastrowSpin product every pair ratio is in closed form in the resident state instead:
//
//   Slater:  with v_s(q)[i] = sum_k phi^s_{occ[k]}(q) T^s[i][k] (the single-move ratio; T the electron-major inverse, pqa_slater.hpp)
//              s1 != s2:  S_ab = v_s1(r1)[a] v_s2(r2)[b]                              (one row of each spin's determinant replaced)
//              s1 == s2:  S_ab = v(r1)[a] v(r2)[b] - v(r2)[a] v(r1)[b],  S_aa = 0     (two rows of one determinant: a 2 x 2 determinant)
//            several determinants: sum_D w_D S_ab(D) / sum_D w_D with the per-determinant tables and weights k_s2 uses (det_weight).
//   Jastrow: with A_e(q) = U(e -> q) - U, the single-move difference of k_testvalue_many, and u the two-body term of channel (s1, s2),
//              dU_ab = A_a(r1) + A_b(r2) + u(r1, r2) + u(r_a, r_b) - u(r1, r_b) - u(r_a, r2)
//            (A_a holds the pair (a, b) with b at its old place and A_b the same pair with a at its old place: the last three terms
//            trade those two for the pair at (r1, r2)).  R_ab = S_ab exp(dU_ab).
//
// Work per walker and sweep: value-only orbital rows at the two points (launch_orb: one pass over 2 W points for equal spins, one pass
// of W points per spin otherwise), 2 (s1 != s2) or 4 products of an orbital row with an inverse per unique determinant, O(N) Jastrow
// pairs per electron, the nea x neb combination.  The products have one or two right-hand sides, so the matrix cores have nothing to
// do here (a 16-column tile would carry 2 live columns); lanes run over the inverse's rows with a butterfly per row instead.
// The ratios of a walker chunk stay on the device: k_tbdm_acc (pqa_dm.hpp) consumes them on the evaluator's stream, ordered by events.
//
// Complex and twisted handles, complex evaluators (pqa_tbdm_sweep_c; the same host driver, tbdm_sweep, with DmEntry::cx set): the
// same formulas with everything complex except the Jastrow part,
//   v_s,D(q)[i] = sum_k phi^s_{occ_D[k]}(q) T^s_D[i][k]                      (complex x complex, no conjugation; T interleaved)
//   S_ab = sum_D w_D S_ab(D) / sum_D w_D,   w_D = det_weight_c               (complex quotient; S_aa an exact 0 + 0i)
//   R_ab = S_ab exp(dU_ab)                                                   (dU_ab real, as above)
// k_tbdm_pairs_c writes interleaved ratios and k_tbdm_acc reads them with rc = 1.  A twisted handle keeps its walkers unfolded; its
// orbital launch folds r1 / r2 and puts the wrap phase exp(i k_t . n . L) on the row, so a point moved by a lattice vector carries the
// Bloch phase of the moved electron.  A real handle through this entry reads its real tables and leaves imaginary parts exactly 0.
#include "pqa_estim.hpp"
#include "pqa_j3dm.hpp"

namespace {

// pts [2][wc][3]: r1 of the chunk's walkers, then r2.
__global__ __launch_bounds__(256) void k_tbdm_gather(const double* __restrict__ pos_a, const double* __restrict__ pos_b,
                                                     const int* __restrict__ assign_a, const int* __restrict__ assign_b, long w0, long wc,
                                                     double* __restrict__ pts) {
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  if (i >= 2 * wc) return;
  const bool second = i >= wc;
  const long w = w0 + (second ? i - wc : i);
  const double* p = second ? pos_b + 3 * (size_t)assign_b[w] : pos_a + 3 * (size_t)assign_a[w];
  pts[3 * i] = p[0]; pts[3 * i + 1] = p[1]; pts[3 * i + 2] = p[2];
}

// v[(d n + i) NP + p] = sum_k phi_p[occ_d[k]] T_d[i][k] for every unique determinant d of spin s and electron i: GS = 2^m >= min(n, 64)
// lanes share a row of the inverse (coalesced), 64 / GS rows go through at once, a butterfly over the group adds the partial sums.
template <int NP>
__device__ __forceinline__ void inverse_products(const SysDev& S, const SlaterState& st, int s, long w, const double* __restrict__ phi0,
                                                 const double* __restrict__ phi1, double* v) {
  const int lane = threadIdx.x, n = s ? S.ndn : S.nup, D = S.ndet_s[s];
  int GS = 1;
  while (GS < n && GS < 64) GS <<= 1;
  const int per = 64 / GS, g = lane / GS, j = lane & (GS - 1);
  const double* Tw = st.T[s] + (size_t)w * D * n * n;
  for (int r0 = 0; r0 < D * n; r0 += per) {
    const int r = r0 + g;  // row (d, i) of the walker's inverses
    const bool act = r < D * n;
    double p0 = 0.0, p1 = 0.0;
    if (act) {
      const int* occ = S.det_occ[s] + (size_t)(r / n) * n;
      for (int k = j; k < n; k += GS) {
        const double t = Tw[(size_t)r * n + k];
        const int o = occ[k];
        p0 += phi0[o] * t;
        if (NP == 2) p1 += phi1[o] * t;
      }
    }
    for (int off = 1; off < GS; off <<= 1) {
      p0 += __shfl_xor(p0, off, 64);
      if (NP == 2) p1 += __shfl_xor(p1, off, 64);
    }
    if (act && j == 0) {
      v[(size_t)r * NP] = p0;
      if (NP == 2) v[(size_t)r * NP + 1] = p1;
    }
  }
}

// One wave per walker of the chunk.  phi1 [wc][nmo_s1]: spin-s1 orbitals at r1, phi2 [wc][nmo_s2]: spin-s2 orbitals at r2;
// pts [2][wc][3]; jas: the handle has a two-body Jastrow factor; R [wc][nea][neb].
// Dynamic LDS (doubles): 3 N coordinates, nea + neb Jastrow sums, ndet weights (several determinants), the v tables
// ndet_s1 nea NP + (s1 != s2: ndet_s2 neb), NP = 2 for equal spins.
// J3 (pqa_tbdm_sweep_j3 on a three-body handle): D3 [wc][nea][neb], the three-body differences k_j3_moves left, join the exponent.
template <bool PBC, bool J3 = false>
__global__ __launch_bounds__(64) void k_tbdm_pairs(SysDev S, SlaterState st, JastrowState js, const double* __restrict__ phi1,
                                                   const double* __restrict__ phi2, const double* __restrict__ pts, long w0, long wc, int s1,
                                                   int s2, int jas, double* __restrict__ R, const double* __restrict__ D3) {
  extern __shared__ double lds[];
  const int N = S.nelec, lane = threadIdx.x, D = S.ndet;
  const long wl = blockIdx.x, w = w0 + wl;
  const int nea = s1 ? S.ndn : S.nup, neb = s2 ? S.ndn : S.nup, ea0 = s1 ? S.nup : 0, eb0 = s2 ? S.nup : 0;
  const bool same = s1 == s2;
  double* xs = lds;             // [N][3]
  double* A1 = lds + 3 * N;     // [nea]  A_a(r1) - u(r_a, r2)
  double* A2 = A1 + nea;        // [neb]  A_b(r2) - u(r1, r_b)
  double* wd = A2 + neb;        // [D]    determinant weights (D > 1)
  double* v1 = wd + (D > 1 ? D : 0);                               // [ndet_s1][nea][NP]
  double* v2 = same ? v1 : v1 + (size_t)S.ndet_s[s1] * nea;       // [ndet_s2][neb]
  const double* xw = js.x + (size_t)w * N * 3;
  for (int q = lane; q < 3 * N; q += 64) xs[q] = xw[q];
  const double r1x = pts[3 * wl], r1y = pts[3 * wl + 1], r1z = pts[3 * wl + 2];
  const double r2x = pts[3 * (wc + wl)], r2y = pts[3 * (wc + wl) + 1], r2z = pts[3 * (wc + wl) + 2];
  __syncthreads();
  const double irb = 1.0 / S.rcut_b, ira = 1.0 / S.rcut_a;
  const int chan = s1 + s2;  // column of the (s1, s2) pair in bcoeff: 0 uu, 1 ud, 2 dd
  double u12 = 0.0;
  if (jas) {
    // a lane owns one (electron, target) item: the nea electrons of s1 going to r1, then the neb electrons of s2 going to r2
    for (int t = lane; t < nea + neb; t += 64) {
      const bool fst = t < nea;
      const int e = fst ? ea0 + t : eb0 + (t - nea), se = fst ? s1 : s2;
      const double qx = fst ? r1x : r2x, qy = fst ? r1y : r2y, qz = fst ? r1z : r2z;  // where e goes
      const double ox = fst ? r2x : r1x, oy = fst ? r2y : r1y, oz = fst ? r2z : r1z;  // where its partner goes
      const double ex = xs[3 * e], ey = xs[3 * e + 1], ez = xs[3 * e + 2];
      double un = 0.0, uo = 0.0;
      for (int j = 0; j < N; ++j) {
        if (j == e) continue;
        const int col = se + (j >= S.nup);
        const double jx = xs[3 * j], jy = xs[3 * j + 1], jz = xs[3 * j + 2];
        un += pair_u<PBC>(S, qx - jx, qy - jy, qz - jz, col, irb);
        uo += pair_u<PBC>(S, ex - jx, ey - jy, ez - jz, col, irb);
      }
      un += ion_u<PBC>(S, qx, qy, qz, se, ira);
      uo += ion_u<PBC>(S, ex, ey, ez, se, ira);
      (fst ? A1[t] : A2[t - nea]) = (un - uo) - pair_u<PBC>(S, ex - ox, ey - oy, ez - oz, chan, irb);
    }
    u12 = pair_u<PBC>(S, r1x - r2x, r1y - r2y, r1z - r2z, chan, irb);
  }
  // determinant weights relative to the largest |determinant| (multi-determinant handles only)
  double den = 1.0;
  if (D > 1) {
    const double ref = det_ref(S, st, w);
    double t = 0.0;
    for (int Dd = lane; Dd < D; Dd += 64) {
      const double x = det_weight(S, st, w, Dd, ref);
      wd[Dd] = x;
      t += x;
    }
    den = wave_sum(t);
  }
  const double* p1 = phi1 + (size_t)wl * S.nmo[s1];
  const double* p2 = phi2 + (size_t)wl * S.nmo[s2];
  if (same) inverse_products<2>(S, st, s1, w, p1, p2, v1);
  else {
    inverse_products<1>(S, st, s1, w, p1, p1, v1);
    inverse_products<1>(S, st, s2, w, p2, p2, v2);
  }
  __syncthreads();
  double* Rw = R + (size_t)wl * nea * neb;
  for (int idx = lane; idx < nea * neb; idx += 64) {
    const int a = idx / neb, b = idx - a * neb;
    double ratio = 0.0;
    if (!(same && a == b)) {  // a pair naming one electron twice stays an exact 0
      for (int Dd = 0; Dd < D; ++Dd) {
        const int da = S.det_map[s1 * D + Dd], db = S.det_map[s2 * D + Dd];
        double sab;
        if (same) {
          const double* va = v1 + ((size_t)da * nea + a) * 2;
          const double* vb = v1 + ((size_t)da * nea + b) * 2;
          sab = va[0] * vb[1] - va[1] * vb[0];
        } else sab = v1[(size_t)da * nea + a] * v2[(size_t)db * neb + b];
        ratio += D > 1 ? wd[Dd] * sab : sab;
      }
      if (D > 1) ratio /= den;
      if (J3) {
        double dj = D3[(size_t)wl * nea * neb + idx];
        if (jas) {
          const int ia = ea0 + a, ib = eb0 + b;
          dj += A1[a] + A2[b] + u12 +
                pair_u<PBC>(S, xs[3 * ia] - xs[3 * ib], xs[3 * ia + 1] - xs[3 * ib + 1], xs[3 * ia + 2] - xs[3 * ib + 2], chan, irb);
        }
        ratio *= exp(dj);
      } else if (jas) {
        const int ia = ea0 + a, ib = eb0 + b;
        const double dj = A1[a] + A2[b] + u12 +
                          pair_u<PBC>(S, xs[3 * ia] - xs[3 * ib], xs[3 * ia + 1] - xs[3 * ib + 1], xs[3 * ia + 2] - xs[3 * ib + 2], chan, irb);
        ratio *= exp(dj);
      }
    }
    Rw[idx] = ratio;
  }
}

// inverse_products in complex arithmetic: v[((d n + i) NP + p) 2 + {0, 1}] as (re, im) pairs.  hc: the handle is complex (phi rows
// [re block | im block] of S.nmo[s] / 2 orbitals each, T interleaved); else the real tables are read and the imaginary parts are
// exactly 0 (inverse_rows_c of pqa_obdm.hip with two right-hand sides).  The butterfly adds both planes of both.
template <int NP>
__device__ __forceinline__ void inverse_products_c(const SysDev& S, const SlaterState& st, int s, long w, int hc, const double* __restrict__ phi0,
                                                   const double* __restrict__ phi1, double* v) {
  const int lane = threadIdx.x, n = s ? S.ndn : S.nup, D = S.ndet_s[s], nmo = S.nmo[s] / 2;
  int GS = 1;
  while (GS < n && GS < 64) GS <<= 1;
  const int per = 64 / GS, g = lane / GS, j = lane & (GS - 1);
  const double* Tw = st.T[s] + (size_t)w * D * n * n * (hc ? 2 : 1);
  for (int r0 = 0; r0 < D * n; r0 += per) {
    const int r = r0 + g;  // row (d, i) of the walker's inverses
    const bool act = r < D * n;
    cx p0 = {0.0, 0.0}, p1 = {0.0, 0.0};
    if (act) {
      const int* occ = S.det_occ[s] + (size_t)(r / n) * n;
      if (hc) {
        const double* Tr = Tw + (size_t)r * n * 2;
        for (int k = j; k < n; k += GS) {
          const cx t = {Tr[2 * k], Tr[2 * k + 1]};
          const int o = occ[k];
          p0 = cadd(p0, cmul(cx{phi0[o], phi0[nmo + o]}, t));
          if (NP == 2) p1 = cadd(p1, cmul(cx{phi1[o], phi1[nmo + o]}, t));
        }
      } else
        for (int k = j; k < n; k += GS) {
          const double t = Tw[(size_t)r * n + k];
          const int o = occ[k];
          p0.r += phi0[o] * t;
          if (NP == 2) p1.r += phi1[o] * t;
        }
    }
    for (int off = 1; off < GS; off <<= 1) {
      p0.r += __shfl_xor(p0.r, off, 64);
      p0.i += __shfl_xor(p0.i, off, 64);
      if (NP == 2) {
        p1.r += __shfl_xor(p1.r, off, 64);
        p1.i += __shfl_xor(p1.i, off, 64);
      }
    }
    if (act && j == 0) {
      double* o = v + (size_t)r * NP * 2;
      o[0] = p0.r; o[1] = p0.i;
      if (NP == 2) { o[2] = p1.r; o[3] = p1.i; }
    }
  }
}

// k_tbdm_pairs for complex and twisted handles: one wave per walker of the chunk, arguments as there, with hc: the wave function's
// handle is complex (phi rows [wc][S.nmo[s]] = [re block | im block], T and dsign interleaved; else the real tables are read and every
// imaginary part is exactly 0); R [wc][nea][neb] interleaved complex.  The Jastrow part is real and is k_tbdm_pairs' own, repeated here
// (a function shared by the two kernels changed k_tbdm_pairs' register allocation).
// Dynamic LDS (doubles): 3 N coordinates, nea + neb Jastrow sums, 2 ndet weights (several determinants), the v tables
// 2 (ndet_s1 nea NP + (s1 != s2: ndet_s2 neb)), NP = 2 for equal spins.
template <bool PBC>
__global__ __launch_bounds__(64) void k_tbdm_pairs_c(SysDev S, SlaterState st, JastrowState js, const double* __restrict__ phi1,
                                                     const double* __restrict__ phi2, const double* __restrict__ pts, long w0, long wc, int s1,
                                                     int s2, int jas, int hc, double* __restrict__ R) {
  extern __shared__ double lds[];
  const int N = S.nelec, lane = threadIdx.x, D = S.ndet;
  const long wl = blockIdx.x, w = w0 + wl;
  const int nea = s1 ? S.ndn : S.nup, neb = s2 ? S.ndn : S.nup, ea0 = s1 ? S.nup : 0, eb0 = s2 ? S.nup : 0;
  const bool same = s1 == s2;
  double* xs = lds;             // [N][3]
  double* A1 = lds + 3 * N;     // [nea]  A_a(r1) - u(r_a, r2)
  double* A2 = A1 + nea;        // [neb]  A_b(r2) - u(r1, r_b)
  double* wd = A2 + neb;        // [D][2] determinant weights (D > 1)
  double* v1 = wd + (D > 1 ? 2 * D : 0);                               // [ndet_s1][nea][NP][2]
  double* v2 = same ? v1 : v1 + (size_t)2 * S.ndet_s[s1] * nea;       // [ndet_s2][neb][2]
  const double* xw = js.x + (size_t)w * N * 3;
  for (int q = lane; q < 3 * N; q += 64) xs[q] = xw[q];
  const double r1x = pts[3 * wl], r1y = pts[3 * wl + 1], r1z = pts[3 * wl + 2];
  const double r2x = pts[3 * (wc + wl)], r2y = pts[3 * (wc + wl) + 1], r2z = pts[3 * (wc + wl) + 2];
  __syncthreads();
  const double irb = 1.0 / S.rcut_b, ira = 1.0 / S.rcut_a;
  const int chan = s1 + s2;  // column of the (s1, s2) pair in bcoeff: 0 uu, 1 ud, 2 dd
  double u12 = 0.0;
  if (jas) {
    // a lane owns one (electron, target) item: the nea electrons of s1 going to r1, then the neb electrons of s2 going to r2
    for (int t = lane; t < nea + neb; t += 64) {
      const bool fst = t < nea;
      const int e = fst ? ea0 + t : eb0 + (t - nea), se = fst ? s1 : s2;
      const double qx = fst ? r1x : r2x, qy = fst ? r1y : r2y, qz = fst ? r1z : r2z;  // where e goes
      const double ox = fst ? r2x : r1x, oy = fst ? r2y : r1y, oz = fst ? r2z : r1z;  // where its partner goes
      const double ex = xs[3 * e], ey = xs[3 * e + 1], ez = xs[3 * e + 2];
      double un = 0.0, uo = 0.0;
      for (int j = 0; j < N; ++j) {
        if (j == e) continue;
        const int col = se + (j >= S.nup);
        const double jx = xs[3 * j], jy = xs[3 * j + 1], jz = xs[3 * j + 2];
        un += pair_u<PBC>(S, qx - jx, qy - jy, qz - jz, col, irb);
        uo += pair_u<PBC>(S, ex - jx, ey - jy, ez - jz, col, irb);
      }
      un += ion_u<PBC>(S, qx, qy, qz, se, ira);
      uo += ion_u<PBC>(S, ex, ey, ez, se, ira);
      (fst ? A1[t] : A2[t - nea]) = (un - uo) - pair_u<PBC>(S, ex - ox, ey - oy, ez - oz, chan, irb);
    }
    u12 = pair_u<PBC>(S, r1x - r2x, r1y - r2y, r1z - r2z, chan, irb);
  }
  // determinant weights relative to the largest |determinant| (multi-determinant handles only): complex, summed in both planes
  cx den = {1.0, 0.0};
  if (D > 1) {
    const double ref = det_ref(S, st, w);
    cx t = {0.0, 0.0};
    for (int Dd = lane; Dd < D; Dd += 64) {
      const cx x = hc ? det_weight_c(S, st, w, Dd, ref) : cx{det_weight(S, st, w, Dd, ref), 0.0};
      wd[2 * Dd] = x.r; wd[2 * Dd + 1] = x.i;
      t = cadd(t, x);
    }
    den = wave_sum_cx(t);
  }
  const double* p1 = phi1 + (size_t)wl * S.nmo[s1];
  const double* p2 = phi2 + (size_t)wl * S.nmo[s2];
  if (same) inverse_products_c<2>(S, st, s1, w, hc, p1, p2, v1);
  else {
    inverse_products_c<1>(S, st, s1, w, hc, p1, p1, v1);
    inverse_products_c<1>(S, st, s2, w, hc, p2, p2, v2);
  }
  __syncthreads();
  double* Rw = R + (size_t)2 * wl * nea * neb;
  for (int idx = lane; idx < nea * neb; idx += 64) {
    const int a = idx / neb, b = idx - a * neb;
    cx ratio = {0.0, 0.0};
    if (!(same && a == b)) {  // a pair naming one electron twice stays an exact 0 + 0i
      for (int Dd = 0; Dd < D; ++Dd) {
        const int da = S.det_map[s1 * D + Dd], db = S.det_map[s2 * D + Dd];
        cx sab;
        if (same) {
          const double* va = v1 + ((size_t)da * nea + a) * 4;  // (v(r1)[a], v(r2)[a])
          const double* vb = v1 + ((size_t)da * nea + b) * 4;
          sab = csub(cmul(cx{va[0], va[1]}, cx{vb[2], vb[3]}), cmul(cx{va[2], va[3]}, cx{vb[0], vb[1]}));
        } else {
          const double* va = v1 + ((size_t)da * nea + a) * 2;
          const double* vb = v2 + ((size_t)db * neb + b) * 2;
          sab = cmul(cx{va[0], va[1]}, cx{vb[0], vb[1]});
        }
        ratio = cadd(ratio, D > 1 ? cmul(cx{wd[2 * Dd], wd[2 * Dd + 1]}, sab) : sab);
      }
      if (D > 1) ratio = cdiv(ratio, den);
      if (jas) {
        const int ia = ea0 + a, ib = eb0 + b;
        const double dj = A1[a] + A2[b] + u12 +
                          pair_u<PBC>(S, xs[3 * ia] - xs[3 * ib], xs[3 * ia + 1] - xs[3 * ib + 1], xs[3 * ia + 2] - xs[3 * ib + 2], chan, irb);
        ratio = cscale(ratio, exp(dj));
      }
    }
    Rw[2 * idx] = ratio.r; Rw[2 * idx + 1] = ratio.i;
  }
}

// The kernel variant of a call: the real ones share a signature, the complex ones have their own.
decltype(&k_tbdm_pairs<false, false>) tbdm_pairs_kernel(bool pbc, bool j3) {
  return pbc ? (j3 ? k_tbdm_pairs<true, true> : k_tbdm_pairs<true, false>) : (j3 ? k_tbdm_pairs<false, true> : k_tbdm_pairs<false, false>);
}
decltype(&k_tbdm_pairs_c<false>) tbdm_pairs_c_kernel(bool pbc) { return pbc ? k_tbdm_pairs_c<true> : k_tbdm_pairs_c<false>; }

// pqa_tbdm_sweep, pqa_tbdm_sweep_c and pqa_tbdm_sweep_j3
int tbdm_sweep(pqa_handle* h, pqa_handle* ev, const DmEntry& en, int k, int spin_a, int spin_b, const int32_t* assign_a,
               const int32_t* assign_b, const int32_t* ijkl, int ntuple, int first, int64_t chunk, double* ratio) {
  TRY(dm_pair_scope(h, ev, en));
  const std::string fn = en.name;
  const bool cx = en.cx;
  const bool j3 = en.j3 && h->has_j3;  // (the three-body differences are formed and added)
  if (spin_a < 0 || spin_a > 1 || spin_b < 0 || spin_b > 1) FAIL(fn + ": spins must be 0 or 1");
  if (!assign_a || !assign_b) FAIL(fn + ": assign_a / assign_b is NULL");
  const bool accumulate = ijkl != nullptr || ntuple != 0;
  if (accumulate && (!ijkl || ntuple <= 0)) FAIL(fn + ": ijkl and ntuple must be given together");
  if (!accumulate && !ratio) FAIL(fn + ": nothing to do (no index tuples and no ratio array)");
  const long W = h->W;
  const int N = h->N, nea = spin_a ? h->ndn : h->nup, neb = spin_b ? h->ndn : h->nup;
  if (nea == 0 || neb == 0) FAIL(fn + ": a spin block without electrons (use the protocol route)");
  auto& da = ev->dm[0];
  auto& db = ev->dm[1];
  if (k < 0 || k >= da.nkeep || k >= db.nkeep) FAIL(fn + ": sample was not kept by pqa_dm_walk");
  for (long w = 0; w < W; ++w)
    if (assign_a[w] < 0 || assign_a[w] >= da.n || assign_b[w] < 0 || assign_b[w] >= db.n) FAIL(fn + ": assignment outside the auxiliary walkers");
  // na2 / nb2: the doubles of an orbital row of the evaluator ([re block | im block] when it is complex), na / nb: its orbitals;
  // cz: doubles per ratio
  const int hc = h->cplx ? 1 : 0, oc = ev->cplx ? 1 : 0, cz = cx ? 2 : 1;
  const int na2 = ev->nmo[da.spin], nb2 = ev->nmo[db.spin], na = oc ? na2 / 2 : na2, nb = oc ? nb2 / 2 : nb2;
  const size_t lds_acc = (size_t)2 * ((size_t)nea * nb + (size_t)na * nb) * sizeof(double);
  if (accumulate) {
    if (da.ncfg != W * nea || db.ncfg != W * neb) FAIL(fn + ": pqa_dm_points was called with other numbers of points (the handle's walkers must be the configurations)");
    if (lds_acc > 64 * 1024) FAIL(fn + ": orbital basis too large for the per-walker LDS tiles");
    TRY(on_ev(h, ev, dm_prepare(ev, W, ntuple, cx ? 1 : 0, first, na, nb)));
    TRY(on_ev(h, ev, ensure(ev, ev->dm_ijkl, (size_t)4 * ntuple * sizeof(int))));
    TRY(on_ev(h, ev, copy_in(ev, ev->dm_ijkl.p, ijkl, (size_t)4 * ntuple * sizeof(int))));
  }
  TRY(on_ev(h, ev, ensure(ev, ev->dm_assign[0], (size_t)W * sizeof(int))));
  TRY(on_ev(h, ev, ensure(ev, ev->dm_assign[1], (size_t)W * sizeof(int))));
  TRY(on_ev(h, ev, copy_in(ev, ev->dm_assign[0].p, assign_a, (size_t)W * sizeof(int))));
  TRY(on_ev(h, ev, copy_in(ev, ev->dm_assign[1].p, assign_b, (size_t)W * sizeof(int))));
  // scratch per walker: the ratios, the orbital rows at the two points, the points
  const bool same = spin_a == spin_b;
  const int nm1 = h->nmo[spin_a], nm2 = h->nmo[spin_b];
  const long Wc = chunk > 0 ? std::min<long>(W, chunk) : walker_chunk(W, ((size_t)(cz + (j3 ? 1 : 0)) * nea * neb + nm1 + nm2 + 6) * sizeof(double));
  size_t lds_j3 = 0;
  if (j3) {
    TRY(j3_moves_lds<true>(h, fn, same ? nea : nea + neb, &lds_j3));
    TRY(ensure(h, h->b_j3dm, (size_t)Wc * nea * neb * sizeof(double)));
  }
  TRY(on_ev(h, ev, ensure(ev, ev->dm_ratio, (size_t)Wc * nea * neb * cz * sizeof(double))));
  TRY(ensure(h, h->b_tbpts, (size_t)6 * Wc * sizeof(double)));
  TRY(ensure(h, h->b_orbphi[0], (size_t)Wc * (same ? 2 * nm1 : nm1) * sizeof(double)));
  if (!same) TRY(ensure(h, h->b_orbphi[1], (size_t)Wc * nm2 * sizeof(double)));
  const int D = h->ndet;
  const size_t lds = ((size_t)3 * N + nea + neb + (D > 1 ? cz * D : 0) + cz * ((size_t)h->ndet_s[spin_a] * nea * (same ? 2 : 1) +
                      (same ? 0 : (size_t)h->ndet_s[spin_b] * neb))) * sizeof(double);
  if (lds > 160 * 1024) FAIL(fn + ": more determinants than one LDS block holds (use the protocol route)");
  const auto pairs = tbdm_pairs_kernel(h->S.pbc, j3);
  const auto pairs_c = tbdm_pairs_c_kernel(h->S.pbc);
  if (lds > 64 * 1024) TRY(raise_lds_limit(h, cx ? (const void*)pairs_c : (const void*)pairs));
  if (!h->tb_ev[0])
    for (hipEvent_t& e : h->tb_ev) TRY(new_event(h, &e, hipEventDisableTiming));
  const hipEvent_t produced = h->tb_ev[0], consumed = h->tb_ev[1];
  // the evaluator's queued work (walks, points, the uploads above) is done before the producer reads its arrays
  HIPCHK(hipEventRecord(consumed, ev->stream));
  TpTuneGuard tune(h), tune_ev(ev);
  double* d_pts = (double*)h->b_tbpts.p;
  double* d_R = (double*)ev->dm_ratio.p;
  const int* d_aa = (const int*)ev->dm_assign[0].p;
  const int* d_ab = (const int*)ev->dm_assign[1].p;
  for (long w0 = 0; w0 < W; w0 += Wc) {
    const long wc = std::min(Wc, W - w0);
    HIPCHK(hipStreamWaitEvent(h->stream, consumed, 0));  // (the previous chunk's ratios have been contracted)
    hipLaunchKernelGGL(k_tbdm_gather, dim3((unsigned)((2 * wc + 255) / 256)), dim3(256), 0, h->stream,
                       (const double*)da.keep_pos.p + (size_t)k * da.n * 3, (const double*)db.keep_pos.p + (size_t)k * db.n * 3, d_aa, d_ab, w0,
                       wc, d_pts);
    TRY(check_launch(h, "k_tbdm_gather"));
    double* phi1 = (double*)h->b_orbphi[0].p;
    double* phi2 = same ? phi1 + (size_t)wc * nm1 : (double*)h->b_orbphi[1].p;
    if (same) TRY(launch_orb(h, spin_a, plain_points(d_pts, 2 * wc), 2 * wc, 1, phi1));
    else {
      TRY(launch_orb(h, spin_a, plain_points(d_pts, wc), wc, 1, phi1));
      TRY(launch_orb(h, spin_b, plain_points(d_pts + 3 * wc, wc), wc, 1, phi2));
    }
    if (j3) TRY(launch_j3_moves<true>(h, lds_j3, (const double*)d_pts, nullptr, 0, w0, wc, spin_a, spin_b, 3, (double*)h->b_j3dm.p));
    if (cx)
      hipLaunchKernelGGL(pairs_c, dim3((unsigned)wc), dim3(64), lds, h->stream, h->S, h->st, h->js, (const double*)phi1, (const double*)phi2,
                         (const double*)d_pts, w0, wc, spin_a, spin_b, (int)h->has_j2, hc, d_R);
    else
      hipLaunchKernelGGL(pairs, dim3((unsigned)wc), dim3(64), lds, h->stream, h->S, h->st, h->js, (const double*)phi1, (const double*)phi2,
                         (const double*)d_pts, w0, wc, spin_a, spin_b, (int)h->has_j2, d_R,
                         j3 ? (const double*)h->b_j3dm.p : (const double*)nullptr);
    TRY(check_launch(h, "k_tbdm_pairs"));
    if (ratio)
      HIPCHK(hipMemcpyAsync(ratio + (size_t)w0 * nea * neb * cz, d_R, (size_t)wc * nea * neb * cz * sizeof(double), hipMemcpyDefault, h->stream));
    HIPCHK(hipEventRecord(produced, h->stream));
    HIPCHK(hipStreamWaitEvent(ev->stream, produced, 0));
    if (accumulate) {
      hipLaunchKernelGGL((k_tbdm_acc<>), dim3((unsigned)wc), dim3(256), lds_acc, ev->stream,
                         (const double*)da.keep_row.p + (size_t)k * da.n * na2, (const double*)da.keep_f.p + (size_t)k * da.n,
                         (const double*)db.keep_row.p + (size_t)k * db.n * nb2, (const double*)db.keep_f.p + (size_t)k * db.n, d_aa + w0, d_ab + w0,
                         (const double*)da.cfg.p + (size_t)w0 * nea * na2, (const double*)db.cfg.p + (size_t)w0 * neb * nb2, (const double*)d_R,
                         cx ? 1 : 0, oc, nea, neb, na, nb, (const int*)ev->dm_ijkl.p, ntuple, first,
                         (double*)ev->dm_val.p + (size_t)w0 * ntuple * cz, (double*)ev->dm_norm[0].p + (size_t)w0 * na,
                         (double*)ev->dm_norm[1].p + (size_t)w0 * nb);
      TRY(on_ev(h, ev, check_launch(ev, "k_tbdm_acc")));
    }
    HIPCHK(hipEventRecord(consumed, ev->stream));
  }
  if (ratio) HIPCHK(hipStreamSynchronize(h->stream));  // (the caller's array is complete on return)
  return 0;
}

}  // namespace

extern "C" int pqa_tbdm_sweep(pqa_handle_t* h, pqa_handle_t* ev, int k, int spin_a, int spin_b, const int32_t* assign_a,
                              const int32_t* assign_b, const int32_t* ijkl, int ntuple, int first, int64_t chunk, double* ratio) {
  return tbdm_sweep(h, ev, DmEntry{"pqa_tbdm_sweep", false}, k, spin_a, spin_b, assign_a, assign_b, ijkl, ntuple, first, chunk, ratio);
}

// pqa_tbdm_sweep for complex and twisted wave-function handles and complex evaluators (real ones are taken too): ratio (W, nea, neb) is
// interleaved complex, and the evaluator's value accumulator is complex (pqa_dm_fetch as after pqa_tbdm_accumulate with complex ratios).
extern "C" int pqa_tbdm_sweep_c(pqa_handle_t* h, pqa_handle_t* ev, int k, int spin_a, int spin_b, const int32_t* assign_a,
                                const int32_t* assign_b, const int32_t* ijkl, int ntuple, int first, int64_t chunk, double* ratio) {
  return tbdm_sweep(h, ev, DmEntry{"pqa_tbdm_sweep_c", true}, k, spin_a, spin_b, assign_a, assign_b, ijkl, ntuple, first, chunk, ratio);
}

// pqa_tbdm_sweep for real handles with a three-body Jastrow factor (handles without one are taken too and give pqa_tbdm_sweep's bits):
// k_j3_moves forms the three-body difference of every pair of a walker chunk ahead of k_tbdm_pairs<., true>.
extern "C" int pqa_tbdm_sweep_j3(pqa_handle_t* h, pqa_handle_t* ev, int k, int spin_a, int spin_b, const int32_t* assign_a,
                                 const int32_t* assign_b, const int32_t* ijkl, int ntuple, int first, int64_t chunk, double* ratio) {
  return tbdm_sweep(h, ev, DmEntry{"pqa_tbdm_sweep_j3", false, true}, k, spin_a, spin_b, assign_a, assign_b, ijkl, ntuple, first, chunk, ratio);
}
