// Symmetry-operator ratios Psi(SR)/Psi(R) of the resident walkers (SymmetryAccumulator / SymmetryAccumulatorPBC,
// pyqmc/observables/accumulators.py:237-341), read-only on the handle state.
//
// The reference transforms every electron, x' = (x - o) @ S + o (row vectors; o = 0 for the open-boundary accumulator), folds
// periodic points back into the cell (enforce_pbc) and recomputes the wave function there.  For a Slater x JastrowSpin product
// the ratio is assembled from the resident state instead:
//
//   Slater:  with M_a[i][k] = phi_{occ_a[k]}(r_i) and the electron-major inverse T_a[i][k] = (M_a^{-1})[k][i] (pqa_slater.hpp),
//              rho_a = det(M'_a) / det(M_a) = det(B_a),   B_a[i][j] = sum_k T_a[i][k] phi_{occ_a[k]}(r'_j)
//            (det(M' M^{-1}) with rows and columns exchanged); B is formed on v_mfma_f64_16x16x4_f64 and its determinant taken by
//            an LU with partial pivoting in LDS (for symmetry-adapted orbitals B is a signed permutation or block-orthogonal matrix
//            whose diagonal can vanish), kept as (sign, log|rho|).  The multi-determinant ratio is
//              sum_D w_D rho_up_{a(D)} rho_dn_{b(D)} / sum_D w_D   (det_weight, combined in log form).
//   Jastrow: U(SR) - U(R), both in full (one-body sums and every pair, minimum images): a periodic S need not map minimal images
//            onto minimal images, so no distance is assumed invariant.  U(R) is evaluated by the same loop from the resident
//            coordinates rather than read from avalues / bvalues, which a fused sweep leaves stale (refreshing them would be a write).
//
// Work per operator and walker chunk (orbital scratch <= 256 MiB): k_sym_xform writes the transformed coordinates, one value-only
// orbital pass per spin at that spin's transformed electrons (launch_orb), k_sym_det per (walker, spin, unique determinant),
// k_sym_comb per walker.
#include "pqa_estim.hpp"

namespace {

struct SymOp {
  double m[9];  // row-major S: x'_l = sum_k (x_k - o_k) m[k][l] + o_l
  double o[3];
};

// x' of every point of the chunk (P = walkers x N), periodic points folded into the cell as enforce_pbc does: every orbital path
// then sees points like the resident walkers' own (Gamma orbitals and min_image_j distances are lattice periodic either way).
__global__ __launch_bounds__(256) void k_sym_xform(SysDev S, const double* __restrict__ x, long P, SymOp op, double* __restrict__ xt) {
  const long p = (long)blockIdx.x * 256 + threadIdx.x;
  if (p >= P) return;
  const double a0 = x[3 * p] - op.o[0], a1 = x[3 * p + 1] - op.o[1], a2 = x[3 * p + 2] - op.o[2];
  double y0 = a0 * op.m[0] + a1 * op.m[3] + a2 * op.m[6] + op.o[0];
  double y1 = a0 * op.m[1] + a1 * op.m[4] + a2 * op.m[7] + op.o[1];
  double y2 = a0 * op.m[2] + a1 * op.m[5] + a2 * op.m[8] + op.o[2];
  fold_cell(S, y0, y1, y2);
  xt[3 * p] = y0;
  xt[3 * p + 1] = y1;
  xt[3 * p + 2] = y2;
}

// One wave per (walker of the chunk, unique determinant a of spin s): rho_a = det(B_a) as (sign, log|rho|) -> rsign / rlog
// [wc][ndet_s].  phi [wc][n][nmo]: spin-s orbitals at the walker's transformed spin-s electrons.  Dynamic LDS: n (n + 1) doubles.
__global__ __launch_bounds__(64) void k_sym_det(SysDev S, SlaterState st, int s, const double* __restrict__ phi, long w0,
                                                double* __restrict__ rsign, double* __restrict__ rlog) {
  extern __shared__ double lds[];
  const int n = s ? S.ndn : S.nup, nmo = S.nmo[s], D = S.ndet_s[s], ld = n + 1;
  const long wl = blockIdx.x / D, w = w0 + wl;
  const int a = blockIdx.x % D, lane = threadIdx.x;
  double* M = lds;  // B [n][ld]
  const double* Ta = st.T[s] + ((size_t)w * D + a) * n * n;
  const int* occ = S.det_occ[s] + (size_t)a * n;
  const double* P = phi + (size_t)wl * n * nmo;
  // MFMA tiles (mfma_tile): lane (i16, kq) supplies A[row i16][k] and B[k][col i16]; C[row kq + 4 r][col i16] lands in c[r]
  const int i16 = lane & 15, kq = lane >> 4;
  for (int i0 = 0; i0 < n; i0 += 16) {
    for (int j0 = 0; j0 < n; j0 += 16) {
      const int ia = i0 + i16, ja = j0 + i16;
      // B[i][j] = sum_k T[i][k] phi_{occ[k]}(r'_j)
      const d4 c = mfma_tile(n, kq, [&](int k, bool kin) { return (ia < n && kin) ? Ta[(size_t)ia * n + k] : 0.0; },
                             [&](int k, bool kin) { return (ja < n && kin) ? P[(size_t)ja * nmo + occ[k]] : 0.0; });
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int i = i0 + kq + 4 * r;
        if (i < n && ja < n) M[i * ld + ja] = c[r];
      }
    }
  }
  __syncthreads();
  double sign = 1.0, logd = 0.0;
  for (int k = 0; k < n; ++k) {
    double v = -1.0;
    int idx = k;
    for (int r = k + lane; r < n; r += 64) {
      const double cv = fabs(M[r * ld + k]);
      if (cv > v) { v = cv; idx = r; }  // (ascending r: the lowest index among equals)
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
      const double ov = __shfl_xor(v, off, 64);
      const int oi = __shfl_xor(idx, off, 64);
      if (ov > v || (ov == v && oi < idx)) { v = ov; idx = oi; }
    }
    if (!(v > 0.0) || !(v <= DBL_MAX)) {  // singular (or not finite): the transformed configuration is a node, rho = 0
      sign = 0.0;
      logd = -INFINITY;
      break;
    }
    const int p = idx;
    if (p != k) {
      for (int cc = k + lane; cc < n; cc += 64) {
        const double t = M[k * ld + cc];
        M[k * ld + cc] = M[p * ld + cc];
        M[p * ld + cc] = t;
      }
      sign = -sign;
    }
    __syncthreads();
    const double piv = M[k * ld + k];
    logd += log(fabs(piv));
    if (piv < 0.0) sign = -sign;
    const double ip = 1.0 / piv;
    // trailing update of rows / columns k+1 .. n-1 (column k and row k are only read): m <= 64 columns as 64 / m row groups,
    // one column per lane; wider trailing blocks row by row, lanes over the columns
    const int m = n - k - 1;
    if (m > 0 && m <= 64) {
      const int R = 64 / m, lr = lane / m, lc = lane - lr * m;
      if (lr < R) {
        const int cc = k + 1 + lc;
        const double rk = M[k * ld + cc];
        for (int r = k + 1 + lr; r < n; r += R) M[r * ld + cc] -= (M[r * ld + k] * ip) * rk;
      }
    } else if (m > 64) {
      for (int r = k + 1; r < n; ++r) {
        const double f = M[r * ld + k] * ip;
        for (int cc = k + 1 + lane; cc < n; cc += 64) M[r * ld + cc] -= f * M[k * ld + cc];
      }
    }
    __syncthreads();
  }
  if (lane == 0) {
    rsign[(size_t)wl * D + a] = sign;
    rlog[(size_t)wl * D + a] = logd;
  }
}

// Jastrow log value U of the configuration xs [N][3] (LDS): this lane's share of the one-body sums and of the N (N - 1) / 2
// pairs (jastrowspin.py:80-105, the sums avalues / bvalues hold, contracted with the coefficients); the caller reduces.
template <bool PBC>
__device__ double jas_total_part(const SysDev& S, const double* xs, int lane) {
  const int N = S.nelec, nu = S.nup;
  const double irb = 1.0 / S.rcut_b, ira = 1.0 / S.rcut_a;
  double u = 0.0;
  for (int e = lane; e < N; e += 64) {
    const int sp = e >= nu;
    for (int I = 0; I < S.natom; ++I) {
      double dx = xs[3 * e] - S.atom_xyz[3 * I], dy = xs[3 * e + 1] - S.atom_xyz[3 * I + 1], dz = xs[3 * e + 2] - S.atom_xyz[3 * I + 2];
      if (PBC) min_image_j(S, dx, dy, dz);
      jas_basis<false>(S, sqrt(dx * dx + dy * dy + dz * dz), ira, [&](int k, double v) { u += S.acoeff[(I * S.na + k) * 2 + sp] * v; });
    }
  }
  // pair p -> (i, j), i < j, rows in order: row i starts at st(i) = i (2N - i - 1) / 2
  const long npair = (long)N * (N - 1) / 2;
  const double b2 = 2.0 * N - 1.0;
  for (long p = lane; p < npair; p += 64) {
    int i = (int)((b2 - sqrt(fmax(b2 * b2 - 8.0 * (double)p, 0.0))) * 0.5);
    i = max(0, min(i, N - 2));
    while (i > 0 && (long)i * (2 * N - i - 1) / 2 > p) --i;
    while (i < N - 2 && (long)(i + 1) * (2 * N - i - 2) / 2 <= p) ++i;
    const int j = (int)(p - (long)i * (2 * N - i - 1) / 2) + i + 1;
    double dx = xs[3 * i] - xs[3 * j], dy = xs[3 * i + 1] - xs[3 * j + 1], dz = xs[3 * i + 2] - xs[3 * j + 2];
    if (PBC) min_image_j(S, dx, dy, dz);
    // (written out, not through jas_basis: there the compiler contracts min_image_j's periodic projections in another order)
    const double r = sqrt(dx * dx + dy * dy + dz * dz);
    if (r < S.rcut_b) {
      const int c = (i >= nu) + (j >= nu);  // 0 up-up, 1 up-down, 2 down-down
      const RadShared sh = rad_shared<0>(r, irb);
      for (int l = 0; l < S.nb; ++l) {
        double v, gf, lp;
        rad_fn<0>(S.b_kind[l], S.b_param[l], S.b_aux[l], S.rcut_b, sh, v, gf, lp);
        u += S.bcoeff[l * 3 + c] * v;
      }
    }
  }
  return u;
}

// One wave per walker: exp(U(SR) - U(R)) sum_D w_D rho_up rho_dn / sum_D w_D -> out[wl].  xt [wc][N][3] transformed coordinates;
// rs[s] / rl[s] [wc][ndet_s] from k_sym_det (unused for a spin without electrons: rho = 1).  Dynamic LDS: 6 N doubles.
template <bool PBC>
__global__ __launch_bounds__(64) void k_sym_comb(SysDev S, SlaterState st, JastrowState js, const double* __restrict__ xt, long w0, int jas,
                                                 const double* __restrict__ rs0, const double* __restrict__ rl0,
                                                 const double* __restrict__ rs1, const double* __restrict__ rl1,
                                                 double* __restrict__ out) {
  extern __shared__ double lds[];
  const int N = S.nelec, lane = threadIdx.x;
  const long wl = blockIdx.x, w = w0 + wl;
  double du = 0.0;
  if (jas) {
    double* xs = lds;          // [N][3] R
    double* ys = lds + 3 * N;  // [N][3] SR
    const double* xw = js.x + (size_t)w * N * 3;
    const double* yw = xt + (size_t)wl * N * 3;
    for (int q = lane; q < 3 * N; q += 64) { xs[q] = xw[q]; ys[q] = yw[q]; }
    __syncthreads();
    du = wave_sum(jas_total_part<PBC>(S, ys, lane) - jas_total_part<PBC>(S, xs, lane));
  }
  const int D = S.ndet, da = S.ndet_s[0], db = S.ndet_s[1];
  const bool hu = S.nup > 0, hd = S.ndn > 0;
  // log of every determinant's transformed magnitude, relative to its largest one (no overflow far from symmetric walkers)
  double ref2 = -INFINITY;
  for (int Dd = lane; Dd < D; Dd += 64) {
    const int a = S.det_map[Dd], b = S.det_map[D + Dd];
    const double l = det_logsum(S, st, w, Dd) + (hu ? rl0[(size_t)wl * da + a] : 0.0) + (hd ? rl1[(size_t)wl * db + b] : 0.0);
    ref2 = fmax(ref2, l);
  }
  ref2 = wave_max(ref2);
  const double ref = det_ref(S, st, w);
  double num = 0.0, den = 0.0;
  if (ref2 > -INFINITY) {
    for (int Dd = lane; Dd < D; Dd += 64) {
      const int a = S.det_map[Dd], b = S.det_map[D + Dd];
      const double su = st.dsign[0][w * da + a], sd = st.dsign[1][w * db + b];
      const double sg = (hu ? rs0[(size_t)wl * da + a] : 1.0) * (hd ? rs1[(size_t)wl * db + b] : 1.0);
      const double l = det_logsum(S, st, w, Dd) + (hu ? rl0[(size_t)wl * da + a] : 0.0) + (hd ? rl1[(size_t)wl * db + b] : 0.0);
      if (l > -INFINITY) num += S.det_coeff[Dd] * su * sd * sg * exp(l - ref2);
      den += det_weight(S, st, w, Dd, ref);
    }
    num = wave_sum(num);
    den = wave_sum(den);
  }
  if (lane == 0) out[wl] = (ref2 > -INFINITY) ? num / den * exp(ref2 - ref + du) : 0.0;
}

}  // namespace

extern "C" int pqa_symmetry(pqa_handle_t* h, int nop, const double* ops, const double* origins, double* ratio) {
  TRY(sync_aos(h));
  HIPCHK(hipSetDevice(h->device));
  if (h->W == 0) FAIL("pqa_symmetry: state not initialised (call recompute)");
  if (nop < 0) FAIL("pqa_symmetry: negative operator count");
  if (nop > 0 && (!ops || !ratio)) FAIL("pqa_symmetry: ops / ratio is NULL");
  TRY(readonly_scope(h, "pqa_symmetry"));
  if (nop == 0) return 0;
  const long W = h->W;
  const int nu = h->nup, nd = h->ndn, N = h->N;
  const int nel[2] = {nu, nd};
  // scratch per walker: transformed coordinates, orbital values, determinant ratios
  const long Wc = walker_chunk(W, ((size_t)3 * N + (size_t)nu * h->nmo[0] + (size_t)nd * h->nmo[1] +
                                   2 * (size_t)(h->ndet_s[0] + h->ndet_s[1])) * sizeof(double));
  TRY(ensure(h, h->b_symx, (size_t)Wc * N * 3 * sizeof(double)));
  for (int s = 0; s < 2; ++s) {
    TRY(ensure(h, h->b_orbphi[s], (size_t)Wc * std::max(nel[s] * h->nmo[s], 1) * sizeof(double)));
    TRY(ensure(h, h->b_symdet[s], (size_t)2 * Wc * h->ndet_s[s] * sizeof(double)));
  }
  TRY(ensure(h, h->b_symout, (size_t)nop * W * sizeof(double)));
  for (int s = 0; s < 2; ++s) {
    const size_t lds = (size_t)nel[s] * (nel[s] + 1) * sizeof(double);
    if (lds > 64 * 1024) TRY(raise_lds_limit(h, (const void*)k_sym_det));  // (91 electrons of a spin and more: 128 x 129 doubles = 129 KiB)
  }
  const double* xs = (const double*)h->b_symx.p;
  double* d_out = (double*)h->b_symout.p;
  TpTuneGuard tune(h);
  int rc = 0;
  for (int o = 0; o < nop && !rc; ++o) {
    SymOp op;
    for (int q = 0; q < 9; ++q) op.m[q] = ops[9 * o + q];
    for (int q = 0; q < 3; ++q) op.o[q] = origins ? origins[3 * o + q] : 0.0;
    for (long w0 = 0; w0 < W && !rc; w0 += Wc) {
      const long wc = std::min(Wc, W - w0);
      const long P = wc * N;
      hipLaunchKernelGGL(k_sym_xform, dim3((unsigned)((P + 255) / 256)), dim3(256), 0, h->stream, h->S,
                         (const double*)(h->js.x + (size_t)w0 * N * 3), P, op, (double*)h->b_symx.p);
      rc = check_launch(h, "k_sym_xform");
      double* rs[2];
      double* rl[2];
      for (int s = 0; s < 2 && !rc; ++s) {
        rs[s] = (double*)h->b_symdet[s].p;
        rl[s] = rs[s] + (size_t)wc * h->ndet_s[s];
        if (nel[s] == 0) continue;
        PointAddr pa{xs + 3 * (s ? nu : 0), nel[s], 3L * N};  // the transformed spin-s electrons of the chunk's walkers
        rc = launch_orb(h, s, pa, wc * nel[s], 1, (double*)h->b_orbphi[s].p);
        if (rc) break;
        hipLaunchKernelGGL(k_sym_det, dim3((unsigned)(wc * h->ndet_s[s])), dim3(64), (size_t)nel[s] * (nel[s] + 1) * sizeof(double),
                           h->stream, h->S, h->st, s, (const double*)h->b_orbphi[s].p, w0, rs[s], rl[s]);
        rc = check_launch(h, "k_sym_det");
      }
      if (rc) break;
      const size_t lds = (size_t)6 * N * sizeof(double);
      double* dst = d_out + (size_t)o * W + w0;
      if (h->S.pbc)
        hipLaunchKernelGGL((k_sym_comb<true>), dim3((unsigned)wc), dim3(64), lds, h->stream, h->S, h->st, h->js, xs, w0, (int)h->has_j2,
                           rs[0], rl[0], rs[1], rl[1], dst);
      else
        hipLaunchKernelGGL((k_sym_comb<false>), dim3((unsigned)wc), dim3(64), lds, h->stream, h->S, h->st, h->js, xs, w0, (int)h->has_j2,
                           rs[0], rl[0], rs[1], rl[1], dst);
      rc = check_launch(h, "k_sym_comb");
    }
  }
  if (rc) return rc;
  return copy_out(h, ratio, d_out, (size_t)nop * W * sizeof(double));
}
