// Total spin <S^2> of the resident walkers (S2Accumulator, pyqmc/observables/s2_accumulator.py), read-only on the handle state.
//
// S^2_loc(R) = Sz(Sz+1) + N_dn - sum_{i up, j dn} Psi(R^{i<->j}) / Psi(R), where R^{i<->j} puts up electron i at r_j and down
// electron j at r_i.  The reference forms each swap ratio from four testvalue + updateinternals moves (swap, unwind); for a
// Slater x JastrowSpin product every ratio factorises exactly and is read off the resident state instead:
//
//   Slater:  the swap replaces one row of each spin's determinant, so with the electron-major inverses T (pqa_slater.hpp)
//              rho_up_a(i, j) = sum_k phi_up_{occ_a[k]}(r_j) T_up_a[i][k],   rho_dn_b(j, i) = sum_k phi_dn_{occ_b[k]}(r_i) T_dn_b[j][k]
//            and the multi-determinant ratio is sum_D w_D rho_up_{a(D)}(i, j) rho_dn_{b(D)}(j, i) / sum_D w_D (det_weight).
//   Jastrow: with g_u(x) / g_d(x) the one-body sum chi_u / chi_d at x plus the two-body sums against every OTHER electron
//            (u_uu / u_ud against up partners, u_ud / u_dd against down partners),
//              dJ_ij = g_u(r_j) - g_u(r_i) + g_d(r_i) - g_d(r_j) - [u_uu(r_ij) + u_dd(r_ij) - 2 u_ud(r_ij)]
//            (the bracket removes the i-j pair from the g sums: the pair keeps its distance and its channel under the swap).
//
// Work per walker: one value-only orbital pass per spin at the OTHER spin's electrons (launch_orb, chunked over walkers), the
// two rho products per 16x16 tile of (i, j) on v_mfma_f64_16x16x4_f64, O(N^2) Jastrow pairs, one wave reduction.
#include "pqa_estim.hpp"

namespace {

// One wave per walker.  phi_u [wc][n_dn][nmo_up]: up-spin orbitals at the down electrons; phi_d [wc][n_up][nmo_dn]: down-spin
// orbitals at the up electrons.  jas: the handle has a two-body Jastrow factor.  s2[w] = base - sum of the swap ratios,
// ratios [W][n_up][n_dn] (may be null).  Dynamic LDS: 5 N doubles (coordinates, g_u, g_d).
template <bool PBC>
__global__ __launch_bounds__(64) void k_s2(SysDev S, SlaterState st, JastrowState js, const double* __restrict__ phi_u,
                                           const double* __restrict__ phi_d, long w0, int jas, double base, double* __restrict__ s2,
                                           double* __restrict__ ratios) {
  extern __shared__ double lds[];
  const int N = S.nelec, nu = S.nup, nd = S.ndn, lane = threadIdx.x;
  const long wl = blockIdx.x, w = w0 + wl;
  double* xs = lds;          // [N][3]
  double* gu = lds + 3 * N;  // [N]
  double* gd = gu + N;       // [N]
  const double* xw = js.x + (size_t)w * N * 3;
  for (int q = lane; q < 3 * N; q += 64) xs[q] = xw[q];
  __syncthreads();
  if (jas) {
    const double irb = 1.0 / S.rcut_b, ira = 1.0 / S.rcut_a;
    for (int e = lane; e < N; e += 64) {
      const double ex = xs[3 * e], ey = xs[3 * e + 1], ez = xs[3 * e + 2];
      double u = 0.0, d = 0.0;
      for (int k = 0; k < N; ++k) {
        if (k == e) continue;
        double dx = ex - xs[3 * k], dy = ey - xs[3 * k + 1], dz = ez - xs[3 * k + 2];
        if (PBC) min_image_j(S, dx, dy, dz);
        const int c = k >= nu;  // channel column of an up electron at x: 0 uu / 1 ud; of a down one: 1 ud / 2 dd
        jas_basis<true>(S, sqrt(dx * dx + dy * dy + dz * dz), irb, [&](int l, double v) {
          u += S.bcoeff[l * 3 + c] * v;
          d += S.bcoeff[l * 3 + 1 + c] * v;
        });
      }
      for (int I = 0; I < S.natom; ++I) {
        double dx = ex - S.atom_xyz[3 * I], dy = ey - S.atom_xyz[3 * I + 1], dz = ez - S.atom_xyz[3 * I + 2];
        if (PBC) min_image_j(S, dx, dy, dz);
        jas_basis<false>(S, sqrt(dx * dx + dy * dy + dz * dz), ira, [&](int k, double v) {
          u += S.acoeff[(I * S.na + k) * 2] * v;
          d += S.acoeff[(I * S.na + k) * 2 + 1] * v;
        });
      }
      gu[e] = u;
      gd[e] = d;
    }
    __syncthreads();
  }
  // determinant weights relative to the largest |determinant| (multi-determinant handles only)
  const int D = S.ndet;
  double ref = 0.0, den = 1.0;
  if (D > 1) {
    ref = det_ref(S, st, w);
    double t = 0.0;
    for (int Dd = lane; Dd < D; Dd += 64) t += det_weight(S, st, w, Dd, ref);
    den = wave_sum(t);
  }
  const int nmu = S.nmo[0], nmd = S.nmo[1];
  const double* Tu = st.T[0] + (size_t)w * S.ndet_s[0] * nu * nu;
  const double* Td = st.T[1] + (size_t)w * S.ndet_s[1] * nd * nd;
  const double* Pu = phi_u + (size_t)wl * nd * nmu;
  const double* Pd = phi_d + (size_t)wl * nu * nmd;
  // MFMA operands: lane (i16, kq) holds A[row i16][k kq] and B[k kq][col i16]; the result D[row kq + 4 r][col i16] in acc[r].
  // Both products are laid out with the up electron as row and the down electron as column, so a lane holds matching entries.
  const int i16 = lane & 15, kq = lane >> 4;
  double tot = 0.0;
  for (int i0 = 0; i0 < nu; i0 += 16) {
    for (int j0 = 0; j0 < nd; j0 += 16) {
      const int ia = i0 + i16, ja = j0 + i16;
      double num[4] = {0.0, 0.0, 0.0, 0.0};
      for (int Dd = 0; Dd < D; ++Dd) {
        const int a = S.det_map[Dd], b = S.det_map[D + Dd];
        const double wD = D > 1 ? det_weight(S, st, w, Dd, ref) : 1.0;
        const double* Ta = Tu + (size_t)a * nu * nu;
        const int* oa = S.det_occ[0] + (size_t)a * nu;
        // rho_up(i, j) = sum_k T_up[i][k] phi_up_{occ[k]}(r_j),  rho_dn(j, i) = sum_k phi_dn_{occ[k]}(r_i) T_dn[j][k]
        const d4 cu = mfma_tile(nu, kq, [&](int k, bool kin) { return (ia < nu && kin) ? Ta[(size_t)ia * nu + k] : 0.0; },
                                [&](int k, bool kin) { return (ja < nd && kin) ? Pu[(size_t)ja * nmu + oa[k]] : 0.0; });
        const double* Tb = Td + (size_t)b * nd * nd;
        const int* ob = S.det_occ[1] + (size_t)b * nd;
        const d4 cd = mfma_tile(nd, kq, [&](int k, bool kin) { return (ia < nu && kin) ? Pd[(size_t)ia * nmd + ob[k]] : 0.0; },
                                [&](int k, bool kin) { return (ja < nd && kin) ? Tb[(size_t)ja * nd + k] : 0.0; });
#pragma unroll
        for (int r = 0; r < 4; ++r) num[r] += wD * cu[r] * cd[r];
      }
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int i = i0 + kq + 4 * r, j = j0 + i16;
        if (i >= nu || j >= nd) continue;
        double ratio = D > 1 ? num[r] / den : num[r];
        if (jas) {
          const int je = nu + j;
          double dj = gu[je] - gu[i] + gd[i] - gd[je];
          double dx = xs[3 * i] - xs[3 * je], dy = xs[3 * i + 1] - xs[3 * je + 1], dz = xs[3 * i + 2] - xs[3 * je + 2];
          if (PBC) min_image_j(S, dx, dy, dz);
          jas_basis<true>(S, sqrt(dx * dx + dy * dy + dz * dz), 1.0 / S.rcut_b, [&](int l, double v) {
            dj -= (S.bcoeff[l * 3] + S.bcoeff[l * 3 + 2] - 2.0 * S.bcoeff[l * 3 + 1]) * v;
          });
          ratio *= exp(dj);
        }
        tot += ratio;
        if (ratios) ratios[((size_t)w * nu + i) * nd + j] = ratio;
      }
    }
  }
  tot = wave_sum(tot);
  if (lane == 0) s2[w] = base - tot;
}

}  // namespace

extern "C" int pqa_s2(pqa_handle_t* h, double* s2, double* ratios) {
  TRY(sync_aos(h));
  HIPCHK(hipSetDevice(h->device));
  if (h->W == 0) FAIL("pqa_s2: state not initialised (call recompute)");
  if (!s2) FAIL("pqa_s2: s2 is NULL");
  TRY(readonly_scope(h, "pqa_s2"));
  const long W = h->W;
  const int nu = h->nup, nd = h->ndn, N = h->N;
  const double sz = 0.5 * (nu - nd), base = sz * (sz + 1.0) + nd;
  if (nu == 0 || nd == 0) {  // no up/down pair: S^2 = Sz(Sz+1) + N_dn exactly, nothing to launch
    std::vector<double> v((size_t)W, base);
    HIPCHK(hipMemcpy(s2, v.data(), (size_t)W * sizeof(double), hipMemcpyDefault));
    return 0;
  }
  const long Wc = walker_chunk(W, (size_t)(nd * h->nmo[0] + nu * h->nmo[1]) * sizeof(double));  // (orbital scratch)
  DevBuf& bu = h->b_orbphi[0];
  DevBuf& bd = h->b_orbphi[1];
  TRY(ensure(h, bu, (size_t)Wc * nd * h->nmo[0] * sizeof(double)));
  TRY(ensure(h, bd, (size_t)Wc * nu * h->nmo[1] * sizeof(double)));
  const size_t nrat = ratios ? (size_t)W * nu * nd : 0;
  TRY(ensure(h, h->b_s2out, ((size_t)W + nrat) * sizeof(double)));
  double* d_s2 = (double*)h->b_s2out.p;
  double* d_rat = ratios ? d_s2 + W : nullptr;
  TpTuneGuard tune(h);
  const size_t lds = (size_t)5 * N * sizeof(double);
  int rc = 0;
  for (long w0 = 0; w0 < W && !rc; w0 += Wc) {
    const long wc = std::min(Wc, W - w0);
    const double* x0 = h->js.x + (size_t)w0 * N * 3;
    PointAddr pdn{x0 + 3 * nu, nd, 3L * N};  // the down electrons of the chunk's walkers
    PointAddr pup{x0, nu, 3L * N};           // the up electrons
    rc = launch_orb(h, 0, pdn, wc * nd, 1, (double*)bu.p);
    if (!rc) rc = launch_orb(h, 1, pup, wc * nu, 1, (double*)bd.p);
    if (rc) break;
    if (h->S.pbc)
      hipLaunchKernelGGL((k_s2<true>), dim3((unsigned)wc), dim3(64), lds, h->stream, h->S, h->st, h->js, (const double*)bu.p,
                         (const double*)bd.p, w0, (int)h->has_j2, base, d_s2, d_rat);
    else
      hipLaunchKernelGGL((k_s2<false>), dim3((unsigned)wc), dim3(64), lds, h->stream, h->S, h->st, h->js, (const double*)bu.p,
                         (const double*)bd.p, w0, (int)h->has_j2, base, d_s2, d_rat);
    rc = check_launch(h, "k_s2");
  }
  if (rc) return rc;
  if (ratios) HIPCHK(hipMemcpyAsync(ratios, d_rat, nrat * sizeof(double), hipMemcpyDefault, h->stream));
  return copy_out(h, s2, d_s2, (size_t)W * sizeof(double));
}
