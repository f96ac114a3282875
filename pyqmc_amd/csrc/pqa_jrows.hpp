// Basis-resolved two-body Jastrow rows of one electron, shared by pqa_correlated.hip and pqa_variance.hip.
//
// U = sum_p c_p B_p(R) is linear in the coefficients (acoeff entries (atom, k, spin), then bcoeff entries (k, pair)), and so are
// grad_e U and lap_e U: jas_rows writes R[m * P + p] = grad_e B_p (m = 0, 1, 2) and lap_e B_p (m = 3) for electron e, and a caller
// contracts them with whichever coefficient set it needs.
#pragma once
#include "pqa_internal.hpp"

template <bool PBC>
__device__ __forceinline__ double jrow_dist(const SysDev& S, double dx, double dy, double dz, double (&d)[3]) {
  if (PBC) min_image_j(S, dx, dy, dz);
  d[0] = dx; d[1] = dy; d[2] = dz;
  return sqrt(dx * dx + dy * dy + dz * dz);
}

// Rows of electron e (spin s, position ex, ey, ez) of the walker whose coordinates are xw into the LDS block R[4][P].  One wave per
// walker calls it; the rows are complete for every lane on return.  ira / irb: 1 / rcut_a, 1 / rcut_b.
template <bool PBC>
__device__ __forceinline__ void jas_rows(const SysDev& S, const double* xw, int e, int s, double ex, double ey, double ez,
                                         int P, int Pa, double ira, double irb, double* R) {
  const int lane = threadIdx.x, N = S.nelec;
  for (int p = lane; p < 4 * P; p += 64) R[p] = 0.0;
  __syncthreads();
  // one-body rows: a lane owns an atom, so its entries (atom, k, spin of e) are written by it alone
  for (int I = lane; I < S.natom; I += 64) {
    double d[3];
    const double rr = jrow_dist<PBC>(S, ex - S.atom_xyz[3 * I], ey - S.atom_xyz[3 * I + 1], ez - S.atom_xyz[3 * I + 2], d);
    if (rr < S.rcut_a) {
      const RadShared sh = rad_shared<2>(rr, ira);
      for (int a = 0; a < S.na; ++a) {
        double v, gf, lpl;
        rad_fn<2>(S.a_kind[a], S.a_param[a], S.a_aux[a], S.rcut_a, sh, v, gf, lpl);
        const int p = (I * S.na + a) * 2 + s;
        R[p] = gf * d[0]; R[P + p] = gf * d[1]; R[2 * P + p] = gf * d[2]; R[3 * P + p] = lpl;
      }
    }
  }
  // two-body rows: columns s (same spin pair: 2s) and s + 1 of basis function l, summed over the other electrons
  for (int l = 0; l < S.nb; ++l) {
    double acc[2][4] = {{0.0, 0.0, 0.0, 0.0}, {0.0, 0.0, 0.0, 0.0}};
    for (int j = lane; j < N; j += 64) {
      if (j == e) continue;
      double d[3];
      const double rr = jrow_dist<PBC>(S, ex - xw[3 * j], ey - xw[3 * j + 1], ez - xw[3 * j + 2], d);
      if (rr < S.rcut_b) {
        const RadShared sh = rad_shared<2>(rr, irb);
        double v, gf, lpl;
        rad_fn<2>(S.b_kind[l], S.b_param[l], S.b_aux[l], S.rcut_b, sh, v, gf, lpl);
        const int c = j >= S.nup;
        acc[c][0] += gf * d[0]; acc[c][1] += gf * d[1]; acc[c][2] += gf * d[2]; acc[c][3] += lpl;
      }
    }
    for (int c = 0; c < 2; ++c)
      for (int m = 0; m < 4; ++m) {
        const double t = wave_sum(acc[c][m]);
        if (lane == 0) R[m * P + Pa + l * 3 + s + c] = t;
      }
  }
  __syncthreads();
}
