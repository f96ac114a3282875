// Code shared by the fused estimator units (pqa_s2, pqa_symmetry, pqa_sq, pqa_correlated, pqa_overlap, pqa_variance, pqa_tbdm, pqa_sr, pqa_obdm); no
// other unit includes it.
//
// Basis-resolved two-body Jastrow rows: U = sum_p c_p B_p(R) is linear in the coefficients (acoeff entries (atom, k, spin), then
// bcoeff entries (k, pair)), and so are grad_e U, lap_e U and U(e -> q) - U(e).  jas_rows writes R[m * P + p] = grad_e B_p
// (m = 0, 1, 2) and lap_e B_p (m = 3) for electron e, jas_diff_rows R[p] = B_p(e -> q) - B_p(e), and a caller contracts them with
// whichever coefficient set it needs: jas_contract4 (gradient and Laplacian: ke_electron for k_corr_energy and k_var_ke, and
// k_corr_md) and jas_contract1 (the value at an ECP point: k_corr_energy and k_corr_md).
//
// Weighted walker means (pqa_obdm, pqa_sq): the weight sum k_wsum (pqa_sr's too) and the column reduction k_wcol_means / k_wcol_fold.
#pragma once
#include "pqa_carver.hpp"
#include "pqa_internal.hpp"

// ---------------------------------------------------------------------------------------------------------------------------------
// device

template <bool PBC>
__device__ __forceinline__ double jrow_dist(const SysDev& S, double dx, double dy, double dz, double (&d)[3]) {
  if (PBC) min_image_j(S, dx, dy, dz);
  d[0] = dx; d[1] = dy; d[2] = dz;
  return sqrt(dx * dx + dy * dy + dz * dz);
}

// Values of the one-body (TWO = false) or two-body (TWO = true) Jastrow basis functions at distance r (irc: 1 / cutoff): f(l, v) for
// every basis function l in index order, nothing outside the cutoff.
template <bool TWO, class F>
__device__ __forceinline__ void jas_basis(const SysDev& S, double r, double irc, F&& f) {
  const double rc = TWO ? S.rcut_b : S.rcut_a;
  if (r < rc) {
    const RadShared sh = rad_shared<0>(r, irc);
    const int n = TWO ? S.nb : S.na;
    for (int l = 0; l < n; ++l) {
      double v, gf, lp;
      if (TWO) rad_fn<0>(S.b_kind[l], S.b_param[l], S.b_aux[l], rc, sh, v, gf, lp);
      else rad_fn<0>(S.a_kind[l], S.a_param[l], S.a_aux[l], rc, sh, v, gf, lp);
      f(l, v);
    }
  }
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

// Value-only rows R[p] = B_p(q) - B_p(r_e) of moving electron e (spin s) of the walker whose coordinates are xw to q (qx, qy, qz),
// into the first P doubles of R.  One wave per walker calls it; the rows are complete for every lane on return.
template <bool PBC>
__device__ __forceinline__ void jas_diff_rows(const SysDev& S, const double* xw, int e, int s, double qx, double qy, double qz,
                                              int P, int Pa, double ira, double irb, double* R) {
  const int lane = threadIdx.x, N = S.nelec;
  const double ex = xw[3 * e], ey = xw[3 * e + 1], ez = xw[3 * e + 2];
  for (int p = lane; p < P; p += 64) R[p] = 0.0;
  __syncthreads();
  for (int I = lane; I < S.natom; I += 64) {
    double d[3];
    const double rn = jrow_dist<PBC>(S, qx - S.atom_xyz[3 * I], qy - S.atom_xyz[3 * I + 1], qz - S.atom_xyz[3 * I + 2], d);
    const double ro = jrow_dist<PBC>(S, ex - S.atom_xyz[3 * I], ey - S.atom_xyz[3 * I + 1], ez - S.atom_xyz[3 * I + 2], d);
    const RadShared shn = rad_shared<0>(rn, ira), sho = rad_shared<0>(ro, ira);
    for (int a = 0; a < S.na; ++a) {
      double vn = 0.0, vo = 0.0, gf, lpl;
      if (rn < S.rcut_a) rad_fn<0>(S.a_kind[a], S.a_param[a], S.a_aux[a], S.rcut_a, shn, vn, gf, lpl);
      if (ro < S.rcut_a) rad_fn<0>(S.a_kind[a], S.a_param[a], S.a_aux[a], S.rcut_a, sho, vo, gf, lpl);
      R[(I * S.na + a) * 2 + s] = vn - vo;
    }
  }
  for (int l = 0; l < S.nb; ++l) {
    double acc[2] = {0.0, 0.0};
    for (int j = lane; j < N; j += 64) {
      if (j == e) continue;
      double d[3];
      const double rn = jrow_dist<PBC>(S, qx - xw[3 * j], qy - xw[3 * j + 1], qz - xw[3 * j + 2], d);
      const double ro = jrow_dist<PBC>(S, ex - xw[3 * j], ey - xw[3 * j + 1], ez - xw[3 * j + 2], d);
      double vn = 0.0, vo = 0.0, gf, lpl;
      if (rn < S.rcut_b) rad_fn<0>(S.b_kind[l], S.b_param[l], S.b_aux[l], S.rcut_b, rad_shared<0>(rn, irb), vn, gf, lpl);
      if (ro < S.rcut_b) rad_fn<0>(S.b_kind[l], S.b_param[l], S.b_aux[l], S.rcut_b, rad_shared<0>(ro, irb), vo, gf, lpl);
      acc[j >= S.nup] += vn - vo;
    }
    for (int c = 0; c < 2; ++c) {
      const double t = wave_sum(acc[c]);
      if (lane == 0) R[Pa + l * 3 + s + c] = t;
    }
  }
  __syncthreads();
}

// The rows jas_rows left for an electron of spin s, contracted with set k of ct [P][K] (a lane's own set): g = grad_e U_k and
// lp = lap_e U_k.  Only the entries of spin s are non-zero: the one-body entries p = 2 q + s, then the two-body entries
// p = Pa + (q >> 1) * 3 + s + (q & 1), ascending.  Every kernel that contracts these rows does it here, so they hold the same bits.
// The four sums are handed to f(gx, gy, gz, lp) and not returned: the callers combine them with G = grad D / D as G . g, which the
// compiler contracts into fused multiply-adds, and which product it fuses depends on where G's divisions stand.  With the sums
// returned into the caller the divisions are sunk next to their use before this function is inlined, and the contraction rounds
// differently from the loops written in place; with the use inside f it is formed as it always was.
template <class F>
__device__ __forceinline__ void jas_contract4(const SysDev& S, const double* R, const double* ct, int K, int k, int s, int P, int Pa, F&& f) {
  double gx = 0.0, gy = 0.0, gz = 0.0, lp = 0.0;
  for (int q = 0; q < S.natom * S.na; ++q) {
    const int p = 2 * q + s;
    const double c = ct[(size_t)p * K + k];
    gx += c * R[p]; gy += c * R[P + p]; gz += c * R[2 * P + p]; lp += c * R[3 * P + p];
  }
  for (int q = 0; q < 2 * S.nb; ++q) {
    const int p = Pa + (q >> 1) * 3 + s + (q & 1);
    const double c = ct[(size_t)p * K + k];
    gx += c * R[p]; gy += c * R[P + p]; gz += c * R[2 * P + p]; lp += c * R[3 * P + p];
  }
  f(gx, gy, gz, lp);
}

// The value-only form, for the row jas_diff_rows left: dU_k = U_k(e -> q) - U_k(e), the same entries in the same order.
__device__ __forceinline__ double jas_contract1(const SysDev& S, const double* R, const double* ct, int K, int k, int s, int Pa) {
  double du = 0.0;
  for (int q = 0; q < S.natom * S.na; ++q) { const int p = 2 * q + s; du += ct[(size_t)p * K + k] * R[p]; }
  for (int q = 0; q < 2 * S.nb; ++q) { const int p = Pa + (q >> 1) * 3 + s + (q & 1); du += ct[(size_t)p * K + k] * R[p]; }
  return du;
}

// Kinetic terms of electron e of walker w (one wave per walker; LDS R[4][P] for jas_rows).  G = grad D / D and L = lap D / D come
// from the orbital-row cache; on the lanes with act the rows are contracted with set k of ct [P][K] to g = grad_e U_k,
// lp = lap_e U_k, and f(lap, tx, ty, tz) receives lap = L + lp + |g|^2 + 2 G . g (the electron's lap Psi / Psi) and t = G + g.
// k_corr_energy and k_var_ke both form their kinetic energy here, so they hold the same bits.
template <bool PBC, class F>
__device__ __forceinline__ void ke_electron(const SysDev& S, const SlaterState& st, const double* xw, long w, int e, int P, int Pa,
                                            double ira, double irb, double* R, const double* ct, int K, int k, bool act, F&& f) {
  const int s = e >= S.nup, i = e - s * S.nup, n = s ? S.ndn : S.nup, nmo = S.nmo[s];
  double r[5];
  slater_ratios<5>(S, st, s, i, w, st.cache[s] + ((size_t)w * n + i) * 5 * nmo, r, nullptr);
  const double G0 = r[1] / r[0], G1 = r[2] / r[0], G2 = r[3] / r[0], L = r[4] / r[0];
  jas_rows<PBC>(S, xw, e, s, xw[3 * e], xw[3 * e + 1], xw[3 * e + 2], P, Pa, ira, irb, R);
  if (act)
    jas_contract4(S, R, ct, K, k, s, P, Pa, [&](double gx, double gy, double gz, double lp) {
      const double lj = lp + gx * gx + gy * gy + gz * gz;
      const double lap = L + lj + 2.0 * (G0 * gx + G1 * gy + G2 * gz);
      f(lap, G0 + gx, G1 + gy, G2 + gz);
    });
  __syncthreads();
}

// One 16 x 16 tile of a product C = A B over k < n on v_mfma_f64_16x16x4_f64.  Lane (i16, kq) = (lane & 15, lane >> 4) supplies
// a(k) = A[row i16][k] and b(k) = B[k][col i16] for its k = k0 + kq < n (zero beyond n; the row / column bounds are the
// callbacks'); C[row kq + 4 r][col i16] lands in element r of the result.
template <class FA, class FB>
__device__ __forceinline__ d4 mfma_tile(int n, int kq, FA&& a, FB&& b) {
  d4 c = {0.0, 0.0, 0.0, 0.0};
  for (int k0 = 0; k0 < n; k0 += 4) {
    const int k = k0 + kq;
    const bool kin = k < n;
    c = __builtin_amdgcn_mfma_f64_16x16x4f64(a(k, kin), b(k, kin), c, 0, 0, 0);
  }
  return c;
}

// NC tiles C_m = A_m B that share the B operand (k_corr_md: the components of a row tile against one coefficient tile): a(m, k, kin),
// b(k, kin) as above, k-steps ascending.  The NC accumulators are independent, so one tile's MFMA latency is covered by the others'.
template <int NC, class FA, class FB>
__device__ __forceinline__ void mfma_tiles(int n, int kq, FA&& a, FB&& b, d4 (&c)[NC]) {
#pragma unroll
  for (int m = 0; m < NC; ++m) c[m] = d4{0.0, 0.0, 0.0, 0.0};
  for (int k0 = 0; k0 < n; k0 += 4) {
    const int k = k0 + kq;
    const bool kin = k < n;
    const double bk = b(k, kin);
#pragma unroll
    for (int m = 0; m < NC; ++m) c[m] = __builtin_amdgcn_mfma_f64_16x16x4f64(a(m, k, kin), bk, c[m], 0, 0, 0);
  }
}

// Fixed-order sum over the 256 threads of a block (sh: 256 doubles of LDS); every thread gets the total.
__device__ __forceinline__ double block_sum256(double v, double* sh) {
  const int t = threadIdx.x;
  sh[t] = v;
  __syncthreads();
  for (int o = 128; o > 0; o >>= 1) {
    if (t < o) sh[t] += sh[t + o];
    __syncthreads();
  }
  const double r = sh[0];
  __syncthreads();
  return r;
}

// Weighted walker means (the mixed estimators of DMC: sum_w w_w res_w / sum_w w_w).
//
// sum of the W weights: one block, a fixed-order tree (pqa_sr launches it too)
template <int PQA_UNIT = 0>  // (a template so that only the units that launch it compile it)
static __global__ __launch_bounds__(256) void k_wsum(const double* __restrict__ wts, long W, double* __restrict__ out) {
  __shared__ double part[256];
  double a = 0.0;
  for (long w = threadIdx.x; w < W; w += 256) a += wts[w];
  a = block_sum256(a, part);
  if (threadIdx.x == 0) out[0] = a;
}

constexpr int kWcolCols = 64;    // columns per block of k_wcol_means: a wave reads 64 consecutive doubles of a row
constexpr long kWcolRows = 256;  // least rows per slice
constexpr long kWcolSlices = 256;  // most slices

inline long wcol_slice_rows(long rows) { return std::max<long>(kWcolRows, (rows + kWcolSlices - 1) / kWcolSlices); }
inline long wcol_slices(long rows) { const long rp = wcol_slice_rows(rows); return (rows + rp - 1) / rp; }
inline long wcol_slices_max(long rows) { return rows <= kWcolRows * kWcolSlices ? wcol_slices(rows) : kWcolSlices; }  // most slices of <= rows rows

// part[z][sl][c] = sum over the rows r of slice sl (rp rows each) of wts[r] in[z][r][c], for nz = gridDim.z row-major arrays
// in[z] (rows, cols).  A block takes kWcolCols consecutive columns and one slice: wave v adds rows lo + v, lo + v + 4, ... (every
// load of a wave is one contiguous 512-byte piece of a row), the four waves' sums are added in wave order.  No atomics; the order
// depends on (rows, rp) alone.
template <int PQA_UNIT = 0>  // (a template so that only the units that launch it compile it)
static __global__ __launch_bounds__(256) void k_wcol_means(const double* __restrict__ in, const double* __restrict__ wts, long rows, long cols,
                                                           long rp, long nsl, double* __restrict__ part) {
  __shared__ double sh[4][kWcolCols];
  const int lane = threadIdx.x & 63, v = threadIdx.x >> 6;
  const long c = (long)blockIdx.x * kWcolCols + lane, sl = blockIdx.y, z = blockIdx.z;
  const long lo = sl * rp, hi = (lo + rp < rows) ? lo + rp : rows;
  const double* p = in + (size_t)z * rows * cols;
  double s = 0.0;
  if (c < cols) {
#pragma unroll 4
    for (long r = lo + v; r < hi; r += 4) s += wts[r] * p[(size_t)r * cols + c];
  }
  sh[v][lane] = s;
  __syncthreads();
  if (v == 0 && c < cols) part[((size_t)z * nsl + sl) * cols + c] = ((sh[0][lane] + sh[1][lane]) + sh[2][lane]) + sh[3][lane];
}

// acc[z cols + c] = (first ? 0 : acc) + part[z][0][c] + part[z][1][c] + ... in slice order; last: times scale / wsum[0]
template <int PQA_UNIT = 0>  // (a template so that only the units that launch it compile it)
static __global__ __launch_bounds__(256) void k_wcol_fold(const double* __restrict__ part, long nsl, long cols, long nz, int first, int last,
                                                          double scale, const double* __restrict__ wsum, double* __restrict__ acc) {
  const long k = (long)blockIdx.x * 256 + threadIdx.x;
  if (k >= nz * cols) return;
  const long z = k / cols, c = k - z * cols;
  double s = first ? 0.0 : acc[k];
  for (long sl = 0; sl < nsl; ++sl) s += part[((size_t)z * nsl + sl) * cols + c];
  if (last) s = scale * s / wsum[0];
  acc[k] = s;
}

// ---------------------------------------------------------------------------------------------------------------------------------
// host

// The walker weights of a weighted mean: W finite doubles >= 0 with a positive sum.
inline int check_weights(pqa_handle* h, const char* fn, const double* weights, long W) {
  if (!weights) FAIL(std::string(fn) + ": weights is NULL");
  double s = 0.0;
  for (long w = 0; w < W; ++w) {
    if (!std::isfinite(weights[w]) || weights[w] < 0.0) FAIL(std::string(fn) + ": weights must be finite and >= 0");
    s += weights[w];
  }
  if (!(s > 0.0) || !std::isfinite(s)) FAIL(std::string(fn) + ": the weights must have a positive sum");
  return 0;
}

// Weighted column means of nz row-major arrays in[z] (rows, cols) on stream-ordered scratch: d_wts (rows) the weights of these
// rows, part (nz, wcol_slices(rows), cols) scratch, acc (nz cols) the running sums over calls (first starts them; last: times
// scale / wsum[0]).
template <int PQA_UNIT = 0>  // (a template so that only the units that call it compile the kernels)
inline int wcol_means_dev(pqa_handle* h, const double* in, const double* d_wts, long rows, long cols, int nz, int first, int last, double scale,
                          const double* d_wsum, double* part, double* acc) {
  const long rp = wcol_slice_rows(rows), nsl = wcol_slices(rows);
  hipLaunchKernelGGL((k_wcol_means<PQA_UNIT>), dim3((unsigned)((cols + kWcolCols - 1) / kWcolCols), (unsigned)nsl, (unsigned)nz), dim3(256), 0, h->stream,
                     in, d_wts, rows, cols, rp, nsl, part);
  TRY(check_launch(h, "k_wcol_means"));
  hipLaunchKernelGGL((k_wcol_fold<PQA_UNIT>), dim3((unsigned)(((long)nz * cols + 255) / 256)), dim3(256), 0, h->stream, (const double*)part, nsl, cols,
                     (long)nz, first, last, scale, d_wsum, acc);
  return check_launch(h, "k_wcol_fold");
}

// Per-walker scratch of an estimator is allocated for a walker chunk of at most this many bytes.
constexpr size_t kChunkScratchBytes = size_t(256) << 20;

inline long walker_chunk(long W, size_t bytes_per_walker) {  // walkers per chunk
  return std::max<long>(1, std::min<long>(W, (long)(kChunkScratchBytes / std::max<size_t>(bytes_per_walker, 1))));
}

// The periodic orbital launcher times its tile sizes on large launches and keeps the choice; an estimator's launches are not to
// change the choices the handle's sweeps made themselves, so the tuning is restored on every exit.
struct TpTuneGuard {
  pqa_handle* h;
  decltype(pqa_handle::tp_tune) saved;
  explicit TpTuneGuard(pqa_handle* h_) : h(h_) { memcpy(saved, h->tp_tune, sizeof(h->tp_tune)); }
  ~TpTuneGuard() { memcpy(h->tp_tune, saved, sizeof(h->tp_tune)); }
};

// Scope of the read-only estimators (pqa_s2, pqa_symmetry, the density matrices): a real, untwisted Slater handle without a three-body
// factor.  complex_ok admits complex and twisted handles, three_body_ok a three-body factor (the density matrices' _c / _j3 entries).
inline int readonly_scope(pqa_handle* h, const char* fn, bool complex_ok = false, bool three_body_ok = false) {
  const char* why = !h->has_slater                           ? "the handle has no Slater factor"
                    : (!complex_ok && (h->cplx || h->twist)) ? "complex orbitals / twisted cell"
                    : (!three_body_ok && h->has_j3)          ? "three-body Jastrow factor"
                                                             : nullptr;
  if (why) FAIL(std::string(fn) + ": " + why + " (outside the fused scope: use the protocol route)");
  return 0;
}

// What an entry of the density-matrix units (pqa_obdm, pqa_tbdm) is: its name (in messages) and whether it is the complex one (complex
// / twisted handles and evaluators admitted, complex ratios and values, the _c kernels; else the real kernels), or the three-body one
// (real handles with a three-body factor admitted: k_j3_moves ahead of the <., true> kernels; a handle without one runs exactly the
// real entry's launches).
struct DmEntry {
  const char* name;
  bool cx;
  bool j3 = false;
};

// Scope of the entries that read wf's resident walkers for the evaluator ev: two handles on one device, wf in the read-only scope of
// the entry with a state.  Real entries take real handles and evaluators.  The complex one takes complex and twisted ones too; a
// twisted evaluator needs a twisted wf, whose walkers are unfolded (an untwisted periodic handle holds folded walkers, and the wrap
// phase of phi_k(r_e) would be lost).  Leaves wf's walker-major arrays current.
inline int dm_pair_scope(pqa_handle* h, pqa_handle* ev, const DmEntry& en) {
  const std::string fn = en.name;
  if (!h) return -2;
  if (!ev) FAIL(fn + ": the orbital evaluator's handle is NULL");
  TRY(sync_aos(h));
  HIPCHK(hipSetDevice(h->device));
  if (h->W == 0) FAIL(fn + ": state not initialised (call recompute)");
  TRY(readonly_scope(h, en.name, en.cx, en.j3));
  if (ev == h) FAIL(fn + ": the wave function and the orbital evaluator must be two handles");
  if (en.cx) {
    if (ev->twist && !h->twist)
      FAIL(fn + ": twisted orbital evaluator on an untwisted handle, whose folded walkers have lost the wrap phase (use the protocol route)");
  } else if (ev->cplx || ev->twist) FAIL(fn + ": complex orbital evaluator (outside the fused scope: use the protocol route)");
  if (ev->device != h->device) FAIL(fn + ": the two handles are on different devices (use the protocol route)");
  return 0;
}

// The return code of a call on the evaluator's handle, with its error reported on the wave function's
inline int on_ev(pqa_handle* h, pqa_handle* ev, int rc) {
  if (rc) h->err = ev->err;
  return rc;
}

// Scope of the single-determinant linear-Jastrow entries (pqa_variance; pqa_correlated through correlated_scope): a real
// single-determinant Slater x two-body Jastrow handle whose row block R[4][P] fits the LDS.
inline int linear_jastrow_scope(pqa_handle* h, const char* fn) {
  if (!h->has_slater || !h->has_j2 || h->has_j3 || h->cplx || h->ndet != 1)
    FAIL(std::string(fn) + ": needs a real single-determinant Slater x two-body Jastrow handle (others: set, recompute and evaluate per set)");
  const int P = h->natom * h->na * 2 + h->nb * 3;
  if ((size_t)4 * P * sizeof(double) > 64 * 1024) FAIL(std::string(fn) + ": more Jastrow coefficients than one LDS row block holds");
  return 0;
}

// The [P][K] coefficient matrix of K sets, acoeff ca [K][Pa] and bcoeff cb [K][Pb]: acoeff entries, then bcoeff entries.
inline std::vector<double> pack_coef_sets(const double* ca, const double* cb, int K, int Pa, int Pb) {
  const int P = Pa + Pb;
  std::vector<double> ct((size_t)P * K);
  for (int k = 0; k < K; ++k) {
    for (int p = 0; p < Pa; ++p) ct[(size_t)p * K + k] = ca[(size_t)k * Pa + p];
    for (int p = 0; p < Pb; ++p) ct[(size_t)(Pa + p) * K + k] = cb[(size_t)k * Pb + p];
  }
  return ct;
}
