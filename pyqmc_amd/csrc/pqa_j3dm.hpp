// Three-body Jastrow differences of the density-matrix moves (pqa_obdm_sweeps_j3, pqa_tbdm_sweep_j3), from the resident walkers.
//
// With C symmetrised in (k, l) (S.c3) the pair term is symmetric,
//
//   t(x, s; y, u) = sum_I sum_klm C[I][k][l][m][s + u] a_k(|x - R_I|) a_l(|y - R_I|) b_m(|x - y|),
//   U3 = sum_{i<j} t(r_i, s_i; r_j, s_j),   P_e = sum_{j != e} t(r_e, s_e; r_j, s_j)        (jas3_eval<0> at r_e),
//
// and every listed electron of a walker goes to the same one or two auxiliary points, so with one table per point q and moving spin s
//
//   G_s(q)[j] = t(q, s; r_j, s_j),   SG_s(q) = sum_j G_s(q)[j]
//
// one-body:  A3_e(r')  = SG_{s_e}(r') - G_{s_e}(r')[e] - P_e
// two-body:  dU3_ab    = SG_{s1}(r1) + SG_{s2}(r2) + t(r1, s1; r2, s2) - G_{s1}(r1)[a] - G_{s1}(r1)[b] - G_{s2}(r2)[a] - G_{s2}(r2)[b]
//                        - P_a - P_b + t(r_a, s1; r_b, s2)                                   (a != b)
//
// k_j3_moves forms these per walker of a chunk and writes A3 [wc][ne] or dU3 [wc][nea][neb] to chunk scratch; k_obdm_rt<PBC, true> /
// k_tbdm_pairs<PBC, true> add them in the exponent where they add the two-body difference.
//
// One wave per walker.  A table and the pair terms of a listed electron are both ROWS of one matrix M[row][j] = t(mover of the row;
// electron j): rows 0 and 1 are the tables (mover at an auxiliary point), row 2 + t is listed electron t at its own place (entry j = e
// an exact 0).  The a-functions of every electron and of the points are staged in LDS first.  Rows go through in groups of
// R = max(1, 64 / N), in jas3_eval's two phases:
//   1. lanes over (row, ion, l, m, partner spin): E[I][l][m][u] = sum_k C[I][k][l][m][s + u] a_k(mover, I) into LDS — the only reads
//      of C, na3 per entry;
//   2. lanes over (row, j): the pair's b-functions once, then the ions one after the other, sum_l a_l(j, I) sum_m E[I][l][m][s_j] b_m:
//      na3 nb3 multiply-adds per (pair, ion) on LDS operands, E read at one address by all lanes of a row.
// Pairs beyond rcut_b3 and ions beyond rcut_a3 of either end are skipped.  Every sum has a fixed order that depends on neither the lane
// count nor the chunk: k, then m, l and the ions in index order inside an item, P_e over j in index order, SG by wave_sum over the
// lanes' strided partial sums.
//
// Dynamic LDS (j3dm_layout), doubles: 3 (N + 2) coordinates (the electrons, then the two points), N + 2 rows of a-values (natom na3,
// padded to an odd stride), E [R][natom][na3][nb3][2], M [(2 + nl)][N | 1] + 1 (the cross term), P [nl]; then (N + 2) natom bytes:
// inside-the-cutoff flags.  nl: listed electrons.
#pragma once
#include "pqa_estim.hpp"

// The two-body Jastrow terms of the density-matrix kernels (k_obdm_rt, k_tbdm_pairs and their complex variants).
// sum_l bcoeff[l][col] b_l(|d|) of one electron pair (minimal image in a periodic cell)
template <bool PBC>
__device__ __forceinline__ double pair_u(const SysDev& S, double dx, double dy, double dz, int col, double irb) {
  if (PBC) min_image_j(S, dx, dy, dz);
  double u = 0.0;
  jas_basis<true>(S, sqrt(dx * dx + dy * dy + dz * dz), irb, [&](int l, double v) { u += S.bcoeff[l * 3 + col] * v; });
  return u;
}
// sum_I sum_k acoeff[I][k][spin] a_k(|q - R_I|)
template <bool PBC>
__device__ __forceinline__ double ion_u(const SysDev& S, double qx, double qy, double qz, int spin, double ira) {
  double u = 0.0;
  for (int I = 0; I < S.natom; ++I) {
    double dx = qx - S.atom_xyz[3 * I], dy = qy - S.atom_xyz[3 * I + 1], dz = qz - S.atom_xyz[3 * I + 2];
    if (PBC) min_image_j(S, dx, dy, dz);
    jas_basis<false>(S, sqrt(dx * dx + dy * dy + dz * dz), ira, [&](int k, double v) { u += S.acoeff[(I * S.na + k) * 2 + spin] * v; });
  }
  return u;
}

struct J3dmLayout {
  int as, Ns, nrow, R, es;  // stride of an a-value row, of a row of M; rows of M; rows per group; entries of a row's E
  size_t o_al, o_E, o_M, o_P, ndbl, bytes;
};
__host__ __device__ inline J3dmLayout j3dm_layout(int N, int A, int na, int nb, int nl) {
  J3dmLayout L;
  L.as = (A * na) | 1;  // odd strides: lanes on consecutive electrons / rows hit different LDS banks
  L.Ns = N | 1;
  L.nrow = 2 + nl;
  L.o_al = (size_t)3 * (N + 2);
  L.R = N >= 64 ? 1 : 64 / N;
  L.es = A * na * nb * 2;
  L.o_E = L.o_al + (size_t)(N + 2) * L.as;
  L.o_M = L.o_E + (size_t)L.R * L.es;
  L.o_P = L.o_M + (size_t)L.nrow * L.Ns + 1;
  L.ndbl = L.o_P + nl;
  L.bytes = L.ndbl * sizeof(double) + (((size_t)(N + 2) * A + 7) & ~(size_t)7);
  return L;
}

// a_k(|p - R_I|) of the three-body basis for every ion into row[I na3 + k] (zeros beyond the cutoff) and in[I] = inside the cutoff;
// the items (point, ion) of npt points run over the lanes.  px: npt points [3], rows at stride `as`, flags at stride natom.
template <bool PBC>
__device__ __forceinline__ void j3dm_avalues(const SysDev& S, const double* px, int npt, int as, double* rows, unsigned char* in) {
  const int A = S.natom, na = S.na3;
  const double ira = 1.0 / S.rcut_a3;
  for (int q = threadIdx.x; q < npt * A; q += 64) {
    const int p = q / A, I = q - p * A;
    double dx = px[3 * p] - S.atom_xyz[3 * I], dy = px[3 * p + 1] - S.atom_xyz[3 * I + 1], dz = px[3 * p + 2] - S.atom_xyz[3 * I + 2];
    if (PBC) min_image(S, dx, dy, dz);
    const double r = sqrt(dx * dx + dy * dy + dz * dz);
    const bool inside = r < S.rcut_a3;
    const RadShared sh = rad_shared<0>(inside ? r : 0.5 * S.rcut_a3, ira);
    double* row = rows + (size_t)p * as + (size_t)I * na;
    for (int k = 0; k < na; ++k) {
      double v, t1, t2;
      rad_fn<0>(S.a3_kind[k], S.a3_param[k], S.a3_aux[k], S.rcut_a3, sh, v, t1, t2);
      row[k] = inside ? v : 0.0;
    }
    in[(size_t)p * A + I] = inside ? 1 : 0;
  }
}

template <bool PBC, bool TWO, int NB3>
__device__ __forceinline__ void j3_moves_wave(const SysDev& S, const JastrowState& js, const double* __restrict__ pts,
                                              const int* __restrict__ es, int ne, long w0, long wc, int s1, int s2, int spins,
                                              double* __restrict__ out, double* lds) {
  const int N = S.nelec, A = S.natom, na = S.na3, nb = S.nb3, lane = threadIdx.x;
  const long wl = blockIdx.x, w = w0 + wl;
  const int nea = TWO ? (s1 ? S.ndn : S.nup) : 0, neb = TWO ? (s2 ? S.ndn : S.nup) : 0, ea0 = s1 ? S.nup : 0, eb0 = s2 ? S.nup : 0;
  const bool same = s1 == s2;
  const int nl = TWO ? (same ? nea : nea + neb) : ne;
  const J3dmLayout L = j3dm_layout(N, A, na, nb, nl);
  // positions N and N + 1 are the auxiliary points (one-body: the same point twice, one per table)
  double* xs = lds;            // [N + 2][3]
  double* al = lds + L.o_al;   // [N + 2][as]
  double* E = lds + L.o_E;     // [R][A][na][nb][2]
  double* M = lds + L.o_M;     // [nrow][Ns] + 1
  double* P = lds + L.o_P;     // [nl]
  unsigned char* ain = reinterpret_cast<unsigned char*>(lds + L.ndbl);  // [N + 2][A]
  const double* xw = js.x + (size_t)w * N * 3;
  for (int q = lane; q < 3 * N; q += 64) xs[q] = xw[q];
  if (lane < 6) xs[3 * N + lane] = pts[3 * ((TWO && lane >= 3) ? wc + wl : wl) + (lane >= 3 ? lane - 3 : lane)];
  __syncthreads();
  j3dm_avalues<PBC>(S, xs, N + 2, L.as, al, ain);
  __syncthreads();
  // listed electron t and whether table k is needed
  auto listed = [&](int t) { return TWO ? (t < nea ? ea0 + t : eb0 + (t - nea)) : es[t]; };
  const bool on0 = TWO || (spins & 1), on1 = TWO || (spins & 2);
  // the mover of a row as a position of xs, and its spin
  auto mover = [&](int row, int& mp, int& ms) {
    mp = row < 2 ? N + row : listed(row - 2);
    ms = row < 2 ? (TWO ? (row ? s2 : s1) : row) : (mp >= S.nup);
  };
  const double irb = 1.0 / S.rcut_b3;
  const int nlm2 = na * nb * 2;
  for (int r0 = 0; r0 < L.nrow; r0 += L.R) {
    const int nr = L.nrow - r0 < L.R ? L.nrow - r0 : L.R;
    // phase 1: E[r][I][l][m][u] = sum_k C[I][k][l][m][ms + u] a_k(mover, I)
    for (int it = lane; it < nr * L.es; it += 64) {
      const int r = it / L.es, rem = it - r * L.es, I = rem / nlm2, q = rem - I * nlm2, l = q / (2 * nb), m = (q >> 1) % nb, u = q & 1;
      const int row = r0 + r;
      if (row < 2 && !(row ? on1 : on0)) continue;
      int mp, ms;
      mover(row, mp, ms);
      double e = 0.0;
      if (ain[(size_t)mp * A + I]) {
        const double* am = al + (size_t)mp * L.as + (size_t)I * na;
        const double* c = S.c3 + ((size_t)I * na * na * nb + (size_t)l * nb + m) * 3 + ms + u;
        for (int k = 0; k < na; ++k) e += c[(size_t)k * na * nb * 3] * am[k];
      }
      E[it] = e;
    }
    __syncthreads();
    // phase 2: M[row][j] = sum_I sum_l a_l(j, I) sum_m E[I][l][m][s_j] b_m(|mover - r_j|); in the first group one more item, the
    // cross term t(r1, s1; r2, s2): the mover of row 0 against the second point
    const int nit = nr * N + ((TWO && r0 == 0) ? 1 : 0);
    for (int it = lane; it < nit; it += 64) {
      const bool cross = it == nr * N;
      const int r = cross ? 0 : it / N, row = r0 + r;
      if (row < 2 && !(row ? on1 : on0)) continue;
      int mp, ms;
      mover(row, mp, ms);
      const int pp = cross ? N + 1 : it - r * N, ps = cross ? s2 : (pp >= S.nup);
      double val = 0.0;
      if (pp != mp) {
        double dx = xs[3 * mp] - xs[3 * pp], dy = xs[3 * mp + 1] - xs[3 * pp + 1], dz = xs[3 * mp + 2] - xs[3 * pp + 2];
        if (PBC) min_image(S, dx, dy, dz);
        const double d = sqrt(dx * dx + dy * dy + dz * dz);
        if (d < S.rcut_b3) {
          const RadShared sh = rad_shared<0>(d, irb);
          double b[NB3];
#pragma unroll
          for (int m = 0; m < NB3; ++m) {
            b[m] = 0.0;
            double t1, t2;
            if (m < nb) rad_fn<0>(S.b3_kind[m], S.b3_param[m], S.b3_aux[m], S.rcut_b3, sh, b[m], t1, t2);
          }
          const double* ap = al + (size_t)pp * L.as;
          const unsigned char *mi = ain + (size_t)mp * A, *pi = ain + (size_t)pp * A;
          const double* Er = E + (size_t)r * L.es + ps;
          for (int I = 0; I < A; ++I) {
            if (!(mi[I] && pi[I])) continue;
            const double* EI = Er + (size_t)I * nlm2;
            for (int l = 0; l < na; ++l) {
              double cb = 0.0;
#pragma unroll
              for (int m = 0; m < NB3; ++m)
                if (m < nb) cb += EI[(l * nb + m) * 2] * b[m];
              val += ap[(size_t)I * na + l] * cb;
            }
          }
        }
      }
      M[cross ? (size_t)L.nrow * L.Ns : (size_t)row * L.Ns + pp] = val;
    }
    __syncthreads();
  }
  // table sums, P of the listed electrons
  double sg0 = 0.0, sg1 = 0.0;
  for (int j = lane; j < N; j += 64) {
    if (on0) sg0 += M[j];
    if (on1) sg1 += M[L.Ns + j];
  }
  sg0 = wave_sum(sg0);
  sg1 = wave_sum(sg1);
  for (int t = lane; t < nl; t += 64) {
    const double* r = M + (size_t)(2 + t) * L.Ns;
    double p = 0.0;
    for (int j = 0; j < N; ++j) p += r[j];
    P[t] = p;
  }
  __syncthreads();
  if (!TWO) {
    for (int t = lane; t < ne; t += 64) {
      const int e = es[t], k = e >= S.nup;
      out[(size_t)wl * ne + t] = ((k ? sg1 : sg0) - M[(size_t)k * L.Ns + e]) - P[t];
    }
  } else {
    const double t12 = M[(size_t)L.nrow * L.Ns];
    double* ow = out + (size_t)wl * nea * neb;
    for (int idx = lane; idx < nea * neb; idx += 64) {
      const int a = idx / neb, b = idx - a * neb, ia = ea0 + a, ib = eb0 + b, ta = a, tb = same ? b : nea + b;
      double d = 0.0;
      if (ia != ib)
        d = (sg0 + sg1 + t12) - (M[ia] + M[ib]) - (M[L.Ns + ia] + M[L.Ns + ib]) - (P[ta] + P[tb]) + M[(size_t)(2 + ta) * L.Ns + ib];
      ow[idx] = d;
    }
  }
}

// One wave per walker of the chunk (w0 .. w0 + wc).  TWO = false (one-body): pts [wc][3], the listed electrons es [ne], spins: bit 0 / 1
// an up / down electron is listed; out [wc][ne] = A3.  TWO = true (two-body): pts [2][wc][3] (r1, then r2), the spin blocks s1, s2;
// out [wc][nea][neb] = dU3 (a pair naming one electron twice: 0).  Four or fewer b-functions take the half-length register arrays, as
// jas3_eval does.
template <bool PBC, bool TWO>
static __global__ __launch_bounds__(64) void k_j3_moves(SysDev S, JastrowState js, const double* __restrict__ pts, const int* __restrict__ es,
                                                        int ne, long w0, long wc, int s1, int s2, int spins, double* __restrict__ out) {
  extern __shared__ double lds[];
  if (S.nb3 <= 4) j3_moves_wave<PBC, TWO, 4>(S, js, pts, es, ne, w0, wc, s1, s2, spins, out, lds);
  else j3_moves_wave<PBC, TWO, PQA_MAXBAS3>(S, js, pts, es, ne, w0, wc, s1, s2, spins, out, lds);
}

// The LDS of k_j3_moves<., TWO> for nl listed electrons: checked against the CU's 160 KiB, the kernel's limit raised above 64 KiB.
template <bool TWO>
inline int j3_moves_lds(pqa_handle* h, const std::string& fn, int nl, size_t* bytes) {
  const J3dmLayout L = j3dm_layout(h->N, h->natom, h->na3, h->nb3, nl);
  if (L.bytes > 160 * 1024) FAIL(fn + ": the three-body tables of one walker do not fit one LDS block (use the protocol route)");
  if (L.bytes > 64 * 1024)
    TRY(raise_lds_limit(h, h->S.pbc ? reinterpret_cast<const void*>(k_j3_moves<true, TWO>) : reinterpret_cast<const void*>(k_j3_moves<false, TWO>)));
  *bytes = L.bytes;
  return 0;
}

template <bool TWO>
inline int launch_j3_moves(pqa_handle* h, size_t lds, const double* pts, const int* es, int ne, long w0, long wc, int s1, int s2, int spins,
                           double* out) {
  if (h->S.pbc)
    hipLaunchKernelGGL((k_j3_moves<true, TWO>), dim3((unsigned)wc), dim3(64), lds, h->stream, h->S, h->js, pts, es, ne, w0, wc, s1, s2, spins, out);
  else
    hipLaunchKernelGGL((k_j3_moves<false, TWO>), dim3((unsigned)wc), dim3(64), lds, h->stream, h->S, h->js, pts, es, ne, w0, wc, s1, s2, spins, out);
  return check_launch(h, "k_j3_moves");
}
