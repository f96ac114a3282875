// Stochastic-reconfiguration moments of the resident walkers (StochasticReconfiguration.avg, stochastic_reconfiguration.py:49-118).
//
// The protocol route brings the walkers and every factor's (W x parameters) derivative arrays to the host, gathers the optimised
// columns there and uploads [dp | E | 1] and w f dp again for one product (pqa_gram).  Everything the estimator needs is on the handle
// already, so this call leaves it there:
//   energy_dev       the energy pass of pqa_energy (same draws, same per-walker rows in b_en);
//   sources          det_coeff: k_pgrad_det (b_pgdet); acoeff / bcoeff: the basis sums the handle keeps (refreshed where a fused sweep
//                    left them stale); ccoeff: k_j3_pgrad (b_out) - only those the column description names;
//   k_sr_gather      per walker chunk of at most 256 MiB: the compact row-major A = [dp | E | 1] (Wc, P + 2) and the scale
//                    s_w = w_w f_w (w: the normalised weight, f: the Pathak-Wagner weight from grad2);
//   k_sr_syrk        A^T diag(s) A[:, :P] on v_mfma_f64_16x16x4_f64, walkers as the k dimension.  A block of four waves owns a 32 x 32
//                    tile (one 16 x 16 tile per wave) and a slice of the walkers; 16 walkers of both column panels are staged in LDS per
//                    step, the right-hand panel scaled by s as it is loaded (w f dp never exists in memory).  dpidpj is symmetric: of
//                    its tiles only those on or above the diagonal are computed;
//   k_sr_reduce      the slices' partial tiles summed in slice order (the same bits on every call), the lower triangle mirrored from
//                    the upper one (dpidpj is exactly symmetric), added to the running moments of the chunks before;
//   k_sr_means       the six weighted energy means, a fixed-order tree.
// Only the (P + 2) x P moments and the six means leave the device (and the (W, 6) per-walker energies when the caller asks for them).
//
// pqa_sr_moments_orb adds the orbital coefficients as sources (4: mo_coeff_alpha, 5: mo_coeff_beta).  Their derivative
//   G[a][m] = sum_u wu[u] sum_e ao[e][a] T_u[e][col_u(m)],   wu[u] = sum_{di: det_map[di] = u} det_coeff[di] d_det[di]
// (k_pgrad_mo) never exists as a (W, nao, nmo) array: the AO values do not depend on u, so per walker and spin
//   B[e][m] = sum_u wu[u] T_u[e][col_u(m)]   (n x nmo, zero where u does not occupy m),   G = ao^T B.
//   launch_ao        value-only AO rows of the chunk's electrons (b_ao: the chunk's (Wc N, nao) rows, nothing of size W N nao);
//   k_sr_orb         a block per walker: wu and B in LDS, G tile by tile on v_mfma_f64_16x16x4_f64, every entry stored through the
//                    inverse column map colof straight into the chunk's A (entries nobody optimises are dropped);
//   k_sr_gather      then fills the other columns and leaves the orbital ones alone.
//
// pqa_sr_moments_c takes complex and twisted handles (complex d_det, complex local energy) and the imaginary-part tail of the
// reference's serialised matrix, with kernels of its own (k_sr_gather_c, k_sr_syrk_c, k_sr_reduce_c below): planar real / imaginary
// panels, one to four matrix instructions per k-step by what the two column blocks of a tile can hold.
//
// k_sr_syrk, k_sr_reduce and the preparation of the sources (sr_sources) are pqa_srk.hpp's: pqa_mix forms its moments with them too.
#include "pqa_srk.hpp"

namespace {

// Pathak-Wagner weight (accumulators.nodal_regularization)
__device__ __forceinline__ double sr_nodal_f(double grad2, double cutoff) {
  const double x = 1.0 / (grad2 * (cutoff * cutoff));
  return x < 1.0 ? x * (9.0 + x * (-15.0 + 7.0 * x)) : 1.0;
}

// sum of the W weights: one block, a fixed-order tree
__global__ __launch_bounds__(256) void k_sr_wsum(const double* __restrict__ wts, long W, double* __restrict__ out) {
  __shared__ double part[256];
  double a = 0.0;
  for (long w = threadIdx.x; w < W; w += 256) a += wts[w];
  a = block_sum256(a, part);
  if (threadIdx.x == 0) out[0] = a;
}

// normalised weight of walker w (wts == nullptr: 1 / W)
__device__ __forceinline__ double sr_weight(const double* wts, const double* wsum, long W, long w) {
  return wts ? wts[w] / wsum[0] : 1.0 / (double)W;
}

// out[k] = sum_w w_w en[k][w] for the six energy rows: one block per row, a fixed-order tree
__global__ __launch_bounds__(256) void k_sr_means(const double* __restrict__ en /*[6][W]*/, const double* __restrict__ wts,
                                                  const double* __restrict__ wsum, long W, double* __restrict__ out) {
  __shared__ double part[256];
  const double* row = en + (size_t)blockIdx.x * W;
  double a = 0.0;
  for (long w = threadIdx.x; w < W; w += 256) a += sr_weight(wts, wsum, W, w) * row[w];
  a = block_sum256(a, part);
  if (threadIdx.x == 0) out[blockIdx.x] = a;
}

// One thread per (walker of the chunk, column of A): A[w][i] = derivative column i (i < P), the local energy (P), 1 (P + 1); the
// thread of column 0 also writes the walker's scale.  Orbital-coefficient columns (src > 3) are k_sr_orb's and are left alone.
__global__ __launch_bounds__(256) void k_sr_gather(SrSources S, const int* __restrict__ src, const int* __restrict__ pos, int P,
                                                   const double* __restrict__ en /*[6][W]*/, const double* __restrict__ wts,
                                                   const double* __restrict__ wsum, double cutoff, long W, long w0, long Wc,
                                                   double* __restrict__ A /*[Wc][P + 2]*/, double* __restrict__ scale /*[Wc]*/) {
  const int lda = P + 2;
  const long idx = (long)blockIdx.x * 256 + threadIdx.x;
  if (idx >= Wc * lda) return;
  const long bw = idx / lda, w = w0 + bw;
  const int i = (int)(idx - bw * lda);
  double v;
  bool mine = true;
  if (i < P) {
    const int s = src[i];
    mine = s <= 3;
    v = mine ? S.base[s][(size_t)w * S.stride[s] + pos[i]] : 0.0;
  } else
    v = i == P ? en[5 * W + w] : 1.0;
  if (mine) A[idx] = v;
  if (i == 0) scale[bw] = sr_weight(wts, wsum, W, w) * sr_nodal_f(en[4 * W + w], cutoff);
}

// doubles per row of B in LDS: whole 16-column tiles, and = 16 mod 32, so that rows kq and kq + 1 of an operand read (the two rows
// of a half-wave's ds_read_b64) land in different halves of the 64 banks
inline int sr_orb_ldb(int nmo) {
  const int mp = (nmo + 15) / 16 * 16;
  return mp % 32 == 16 ? mp : mp + 16;
}

// Orbital-coefficient columns of spin s for the walkers w0 .. of a chunk: grid = (walkers of the chunk), block = 64 x (waves: the
// 16-row AO tiles, at most 4).  LDS: B [kpad][ldb] (kpad: n in whole k-steps of 4; the padding is zero), wu [ndet_s].
//   wu, B     as k_pgrad_mo forms its weights; determinants ascending;
//   G = ao^T B  a wave owns an AO tile a0 and all (at most 4) orbital tiles: per k-step lane (i16, kq) loads ao[e0 + kq][a0 + i16] once
//             (coalesced along a) and B[e0 + kq][m0 + i16] per orbital tile; k-steps ascending.  The lane holds D[a0 + kq + 4 r][m0 + i16];
//   store     A[bw][colof[a nmo + m]] where the map names a column.
// ao: the chunk's AO rows [Wc N][nao]; d_det [W][ndet]; colmap [ndet_s][nmo]; colof [nao][nmo].
__global__ __launch_bounds__(256) void k_sr_orb(SysDev S, SlaterState st, int s, const double* __restrict__ ao, const double* __restrict__ d_det,
                                                const int* __restrict__ colmap, const int* __restrict__ colof, long w0, int lda, int ldb,
                                                double* __restrict__ A) {
  extern __shared__ double sr_orb_lds[];
  const long bw = blockIdx.x, w = w0 + bw;
  const int n = s ? S.ndn : S.nup, D = S.ndet_s[s], nmo = S.nmo[s], nao = S.nao;
  const int kpad = (n + 3) & ~3, nmt = (nmo + 15) >> 4, nat = (nao + 15) >> 4;
  double* B = sr_orb_lds;
  double* wu = B + kpad * ldb;
  for (int u = threadIdx.x; u < D; u += blockDim.x) {
    double acc = 0.0;
    for (int di = 0; di < S.ndet; ++di)
      if (S.det_map[s * S.ndet + di] == u) acc += S.det_coeff[di] * d_det[w * S.ndet + di];
    wu[u] = acc;
  }
  __syncthreads();
  const double* Tw = st.T[s] + (size_t)w * D * n * n;
  for (int idx = threadIdx.x; idx < kpad * ldb; idx += blockDim.x) {
    const int e = idx / ldb, m = idx - e * ldb;
    double acc = 0.0;
    if (e < n && m < nmo)
      for (int u = 0; u < D; ++u) {
        const int col = colmap[u * nmo + m];
        if (col >= 0) acc += wu[u] * Tw[((size_t)u * n + e) * n + col];
      }
    B[idx] = acc;
  }
  __syncthreads();
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, nwave = blockDim.x >> 6, i16 = lane & 15, kq = lane >> 4;
  const double* aow = ao + ((size_t)bw * S.nelec + (size_t)s * S.nup) * nao;
  double* Aw = A + (size_t)bw * lda;
  for (int at = wave; at < nat; at += nwave) {
    const int a = at * 16 + i16;
    d4 acc[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) acc[j] = d4{0.0, 0.0, 0.0, 0.0};
    for (int e0 = 0; e0 < kpad; e0 += 4) {
      const int e = e0 + kq;
      const double av = (a < nao && e < n) ? aow[(size_t)e * nao + a] : 0.0;
      const double* brow = B + e * ldb + i16;
#pragma unroll
      for (int j = 0; j < 4; ++j)
        if (j < nmt) acc[j] = __builtin_amdgcn_mfma_f64_16x16x4f64(av, brow[16 * j], acc[j], 0, 0, 0);
    }
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      if (j >= nmt) continue;
      const int m = 16 * j + i16;
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int ar = at * 16 + kq + 4 * r;
        if (ar < nao && m < nmo) {
          const int c = colof[ar * nmo + m];
          if (c >= 0) Aw[c] = acc[j][r];
        }
      }
    }
  }
}

// ---- complex columns (pqa_sr_moments_c) -------------------------------------------------------------------------------------------------
// dp is complex on a complex / twisted handle (d_det is; the Jastrow sums stay real) and the reference's serialised matrix carries, after
// the P primary columns, ntail columns i dp[:, tail[t]].  With A = [dp | E | 1] = Ar + i Ai (planar, (Wc, Pt + 2) each, Pt = P + ntail)
// the moments M = A^T diag(s) A[:, :Pt] (no conjugation: M is complex symmetric) are
//   Re M = Ar^T s Ar - Ai^T s Ai,   Im M = Ar^T s Ai + Ai^T s Ar.

// One thread per (walker of the chunk, column of A): primary column i gets (Re, Im) of its source entry (sources 1 - 3 are real; source 0
// of a complex handle is the interleaved b_pgdet), tail column t gets i times its twin: (-Im, Re).  Column Pt is (Re total, Im ecp),
// column Pt + 1 is (1, 0).  en: [7][W] on a complex handle, [6][W] on a real one (whose imaginary plane is zero).  dpz: the chunk's
// interleaved (Wc, Pt) dp for the caller that asked for it, or nullptr.
__global__ __launch_bounds__(256) void k_sr_gather_c(SrSources S, const int* __restrict__ src, const int* __restrict__ pos, int P,
                                                     const int* __restrict__ tail, int ntail, int cplx, const double* __restrict__ en,
                                                     const double* __restrict__ wts, const double* __restrict__ wsum, double cutoff, long W,
                                                     long w0, long Wc, double* __restrict__ Ar, double* __restrict__ Ai,
                                                     double* __restrict__ scale /*[Wc]*/, double* __restrict__ dpz) {
  const int Pt = P + ntail, lda = Pt + 2;
  const long idx = (long)blockIdx.x * 256 + threadIdx.x;
  if (idx >= Wc * lda) return;
  const long bw = idx / lda, w = w0 + bw;
  const int i = (int)(idx - bw * lda);
  double re, im = 0.0;
  if (i < Pt) {
    const int c = i < P ? i : tail[i - P], s = src[c];
    if (s == 0 && cplx) {
      const double* z = S.base[0] + 2 * ((size_t)w * S.stride[0] + pos[c]);
      re = z[0]; im = z[1];
    } else
      re = S.base[s][(size_t)w * S.stride[s] + pos[c]];
    if (i >= P) { const double t = re; re = -im; im = t; }
    if (dpz) { dpz[2 * ((size_t)bw * Pt + i)] = re; dpz[2 * ((size_t)bw * Pt + i) + 1] = im; }
  } else if (i == Pt) {
    re = en[5 * W + w];
    if (cplx) im = en[6 * W + w];
  } else
    re = 1.0;
  Ar[idx] = re;
  Ai[idx] = im;
  if (i == 0) scale[bw] = sr_weight(wts, wsum, W, w) * sr_nodal_f(en[4 * W + w], cutoff);
}

// The tile of one block of k_sr_syrk_c.  FI / FJ: the left / right column block holds a column that can have an imaginary part, so its
// imaginary panel is staged too.  MFMAs per k-step: 1 (neither), 2 (one of them), 4 (both): Lr Rr [- Li Ri] and [Lr Ri] [+ Li Rr].
template <bool FI, bool FJ>
__device__ __forceinline__ void sr_syrk_c_tile(const double* __restrict__ Ar, const double* __restrict__ Ai, const double* __restrict__ scale,
                                               long Wc, int Pt, long per, double* __restrict__ part, double* Lr, double* Li, double* Rr,
                                               double* Ri) {
  const int bj = blockIdx.x, bi = blockIdx.y, sl = blockIdx.z;
  const int lda = Pt + 2;
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6, i16 = lane & 15, kq = lane >> 4, wi = wave >> 1, wj = wave & 1;
  const long k_lo = (long)sl * per, k_hi = k_lo + per < Wc ? k_lo + per : Wc;
  // staging: thread t holds rows r0 and r0 + 8 of column c of each staged 16 x 32 panel
  const int c = t & 31, r0 = t >> 5;
  const int ca = bi * 32 + c, cb = bj * 32 + c;
  const bool ain = ca < lda, bin = cb < Pt;
  double vlr[2], vli[2], vrr[2], vri[2];
  auto fetch = [&](long k0) {
#pragma unroll
    for (int q = 0; q < 2; ++q) {
      const long row = k0 + r0 + 8 * q;
      const bool rin = row < k_hi;
      const double s = (rin && bin) ? scale[row] : 0.0;
      vlr[q] = (rin && ain) ? Ar[(size_t)row * lda + ca] : 0.0;
      if (FI) vli[q] = (rin && ain) ? Ai[(size_t)row * lda + ca] : 0.0;
      vrr[q] = (rin && bin) ? Ar[(size_t)row * lda + cb] * s : 0.0;
      if (FJ) vri[q] = (rin && bin) ? Ai[(size_t)row * lda + cb] * s : 0.0;
    }
  };
  d4 re = {0.0, 0.0, 0.0, 0.0}, im = {0.0, 0.0, 0.0, 0.0};
  if (k_lo < k_hi) fetch(k_lo);
  for (long k0 = k_lo; k0 < k_hi; k0 += kSrKB) {
#pragma unroll
    for (int q = 0; q < 2; ++q) {
      const int o = (r0 + 8 * q) * kSrLd + c;
      Lr[o] = vlr[q];
      if (FI) Li[o] = vli[q];
      Rr[o] = vrr[q];
      if (FJ) Ri[o] = vri[q];
    }
    __syncthreads();
    if (k0 + kSrKB < k_hi) fetch(k0 + kSrKB);  // (the next step's loads fly while this one multiplies)
#pragma unroll
    for (int kk = 0; kk < kSrKB / 4; ++kk) {
      const int oa = (kk * 4 + kq) * kSrLd + wi * 16 + i16, ob = (kk * 4 + kq) * kSrLd + wj * 16 + i16;
      const double lr = Lr[oa], rr = Rr[ob];
      re = __builtin_amdgcn_mfma_f64_16x16x4f64(lr, rr, re, 0, 0, 0);
      if (FI && FJ) re = __builtin_amdgcn_mfma_f64_16x16x4f64(-Li[oa], Ri[ob], re, 0, 0, 0);
      if (FJ) im = __builtin_amdgcn_mfma_f64_16x16x4f64(lr, Ri[ob], im, 0, 0, 0);
      if (FI) im = __builtin_amdgcn_mfma_f64_16x16x4f64(Li[oa], rr, im, 0, 0, 0);
    }
    __syncthreads();
  }
  const int ti = 2 * bi + wi, tj = 2 * bj + wj;
  if (ti > tj && ti * 16 + 15 < Pt) return;
  // lane holds D[row = kq + 4 r][col = i16]; the two planes of slice sl follow each other
  const size_t n = (size_t)lda * Pt;
  double* pr = part + (size_t)sl * 2 * n;
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const int p = ti * 16 + kq + 4 * r, q = tj * 16 + i16;
    if (p < lda && q < Pt) {
      pr[(size_t)p * Pt + q] = re[r];
      pr[n + (size_t)p * Pt + q] = im[r];
    }
  }
}

// part[sl][plane] (Pt + 2, Pt) = tile (32 bi .., 32 bj ..) of A^T diag(s) A[:, :Pt] over the walkers of slice sl, with k_sr_syrk's
// mapping: grid = (column blocks, row blocks, slices), block = 256, wave (wi, wj) owns the 16 x 16 tile (2 bi + wi, 2 bj + wj); blocks and
// wave tiles strictly below the diagonal are skipped unless they hold a row >= Pt.  flag[b]: column block b of A holds a column that
// can have an imaginary part; the choice of the tile's form is block-uniform.
__global__ __launch_bounds__(256) void k_sr_syrk_c(const double* __restrict__ Ar, const double* __restrict__ Ai, const double* __restrict__ scale,
                                                   const int* __restrict__ flag, long Wc, int Pt, long per, double* __restrict__ part) {
  __shared__ double Lr[kSrKB * kSrLd], Li[kSrKB * kSrLd], Rr[kSrKB * kSrLd], Ri[kSrKB * kSrLd];
  const int bj = blockIdx.x, bi = blockIdx.y;
  if (bi > bj && bi * 32 + 31 < Pt) return;
  const bool fi = flag[bi] != 0, fj = flag[bj] != 0;
  if (fi && fj) sr_syrk_c_tile<true, true>(Ar, Ai, scale, Wc, Pt, per, part, Lr, Li, Rr, Ri);
  else if (fi) sr_syrk_c_tile<true, false>(Ar, Ai, scale, Wc, Pt, per, part, Lr, Li, Rr, Ri);
  else if (fj) sr_syrk_c_tile<false, true>(Ar, Ai, scale, Wc, Pt, per, part, Lr, Li, Rr, Ri);
  else sr_syrk_c_tile<false, false>(Ar, Ai, scale, Wc, Pt, per, part, Lr, Li, Rr, Ri);
}

// mom (Pt + 2, Pt) complex interleaved = (first ? 0 : mom) + sum over the slices in slice order of both planes; element (i, j) of the
// symmetric block is read at (min, max): the tiles below the diagonal were never written.
__global__ __launch_bounds__(256) void k_sr_reduce_c(const double* __restrict__ part, int Pt, int nslice, int first, double* __restrict__ mom) {
  const long n = (long)(Pt + 2) * Pt;
  const long idx = (long)blockIdx.x * 256 + threadIdx.x;
  if (idx >= n) return;
  const int i = (int)(idx / Pt), j = (int)(idx - (long)i * Pt);
  const long from = (i < Pt && j < i) ? (long)j * Pt + i : idx;
  double sr = 0.0, si = 0.0;
  for (int sl = 0; sl < nslice; ++sl) {
    sr += part[(size_t)sl * 2 * n + from];
    si += part[(size_t)sl * 2 * n + n + from];
  }
  mom[2 * idx] = first ? sr : mom[2 * idx] + sr;
  mom[2 * idx + 1] = first ? si : mom[2 * idx + 1] + si;
}

}  // namespace

// Both entries.  fn: the entry's name (its messages); orb: sources 4 / 5 are accepted; chunk: walkers per chunk (0: the scratch rule);
// dp_walker: host (W, P) or NULL.
static int sr_moments(pqa_handle_t* h, const std::string& fn, bool orb, int P, const int32_t* src, const int32_t* pos, double nodal_cutoff,
               const double* weights, double threshold, const double* rot, const double* unif, uint64_t seed, long chunk, double* en_mean,
               double* moments, double* en_walker, double* dp_walker) {
  // argument checks first: they need nothing but the handle's host-side sizes
  if (P < 1) FAIL(fn + ": P must be at least 1");
  if (!src || !pos || !en_mean || !moments) FAIL(fn + ": src, pos, en_mean and moments must not be NULL");
  if (!(nodal_cutoff > 0.0)) FAIL(fn + ": nodal_cutoff must be positive");
  if (h->cplx) FAIL(fn + ": complex orbitals / twisted cell (outside the device scope: use the protocol route)");
  long size[4];
  sr_source_sizes(h, size);
  bool need[4] = {false, false, false, false};
  bool orb_spin[2] = {false, false};
  std::vector<int> colof[2];  // [nao][nmo_s]: the column of A an orbital-coefficient entry fills, or -1
  for (int i = 0; i < P; ++i) {
    if (orb && (src[i] == 4 || src[i] == 5)) {
      const int s = src[i] - 4, n = s ? h->ndn : h->nup;
      const char* why = !h->has_slater                ? "the handle has no Slater factor"
                        : h->twist                     ? "twisted cell"
                        : h->S.pbc != 0                ? "periodic cell (per-k parameter layout)"
                        : n == 0                       ? "a spin without electrons"
                        : (n > 64 || h->nmo[s] > 64)   ? "more than 64 electrons or orbitals of a spin"
                                                       : nullptr;
      if (why) FAIL(fn + ": orbital coefficients: " + why + " (outside the device scope: use the protocol route)");
      if (pos[i] < 0 || pos[i] >= (long)h->nao * h->nmo[s]) FAIL(fn + ": pos outside the (nao, nmo) orbital coefficients src names");
      if (colof[s].empty()) colof[s].assign((size_t)h->nao * h->nmo[s], -1);
      if (colof[s][pos[i]] >= 0) FAIL(fn + ": an orbital coefficient is named twice");
      colof[s][pos[i]] = i;
      orb_spin[s] = true;
      continue;
    }
    if (src[i] < 0 || src[i] > 3)
      FAIL(fn + (orb ? ": src must be 0 (det_coeff), 1 (acoeff), 2 (bcoeff), 3 (ccoeff), 4 (mo_coeff_alpha) or 5 (mo_coeff_beta)"
                     : ": src must be 0 (det_coeff), 1 (acoeff), 2 (bcoeff) or 3 (ccoeff)"));
    if (pos[i] < 0 || pos[i] >= size[src[i]]) FAIL(fn + ": pos outside the parameter src names (or the handle has no such factor)");
    need[src[i]] = true;
  }
  const bool has_orb = orb_spin[0] || orb_spin[1];
  if (chunk < 0) FAIL(fn + ": walker_chunk must not be negative");
  const size_t nmom = (size_t)(P + 2) * P;
  if (nmom * sizeof(double) > kChunkScratchBytes) FAIL(fn + ": the (P + 2) x P moments exceed the 256 MiB scratch limit (use the protocol route)");
  if (h->W == 0) FAIL("state not initialised (call pqa_wf_recompute)");
  TRY(sync_aos(h));
  HIPCHK(hipSetDevice(h->device));
  const long W = h->W;
  h->saved_valid = false;  // (as pqa_energy: the saved orbital rows of a gradient_value call are overwritten)
  TRY(energy_dev(h, threshold, rot, unif, seed, 0u));
  const double* d_en = (const double*)h->b_en.p;
  // derivative sources
  SrSources S{};
  need[0] = need[0] || has_orb;  // (the orbital columns need d_det for the determinant weights)
  TRY(sr_sources(h, need, S));
  // scratch: [moments | means (6) | weight sum (1) | weights (W) | per-walker energies (W, 6) | scale (Wc) | A (Wc, P + 2) |
  // partials (nslice, P + 2, P) | src, pos | colof of each spin]; with orbital columns a chunk's A and AO rows (b_ao) together stay
  // within the chunk limit
  const int lda = P + 2;
  long Wc = walker_chunk(W, ((size_t)lda + (has_orb ? (size_t)h->N * h->nao : 0)) * sizeof(double));
  if (chunk > 0) Wc = std::min(Wc, chunk);
  size_t orb_lds[2] = {0, 0};
  for (int s = 0; s < 2; ++s)
    if (orb_spin[s]) {
      const int n = s ? h->ndn : h->nup;
      orb_lds[s] = ((size_t)((n + 3) & ~3) * sr_orb_ldb(h->nmo[s]) + h->ndet_s[s]) * sizeof(double);
      if (orb_lds[s] > 150 * 1024) FAIL(fn + ": orbital coefficients: the determinant weights of one walker do not fit LDS (use the protocol route)");
    }
  const int nbi = (lda + 31) / 32, nbj = (P + 31) / 32;
  const long nslice = sr_slices(Wc, nbi, nbj, nmom);
  const size_t nw = weights ? (size_t)W : 0, nenw = en_walker ? (size_t)6 * W : 0;
  const size_t ndbl = nmom + 6 + 1 + nw + nenw + (size_t)Wc + (size_t)Wc * lda + (size_t)nslice * nmom;
  TRY(ensure(h, h->b_sr, ndbl * sizeof(double) + ((size_t)2 * P + colof[0].size() + colof[1].size()) * sizeof(int)));
  double* d_mom = (double*)h->b_sr.p;
  double* d_mean = d_mom + nmom;
  double* d_wsum = d_mean + 6;
  double* d_wts = d_wsum + 1;
  double* d_enw = d_wts + nw;
  double* d_scale = d_enw + nenw;
  double* d_A = d_scale + Wc;
  double* d_part = d_A + (size_t)Wc * lda;
  int* d_src = (int*)(d_part + (size_t)nslice * nmom);
  int* d_pos = d_src + P;
  TRY(copy_in(h, d_src, src, (size_t)P * sizeof(int)));
  TRY(copy_in(h, d_pos, pos, (size_t)P * sizeof(int)));
  int* d_colof[2] = {d_pos + P, d_pos + P + colof[0].size()};
  for (int s = 0; s < 2; ++s) TRY(copy_in(h, d_colof[s], colof[s].data(), colof[s].size() * sizeof(int)));
  if (has_orb) TRY(ensure(h, h->b_ao, (size_t)Wc * h->N * h->nao * sizeof(double)));
  const double* wts = nullptr;
  if (weights) {
    TRY(copy_in(h, d_wts, weights, (size_t)W * sizeof(double)));
    hipLaunchKernelGGL(k_sr_wsum, dim3(1), dim3(256), 0, h->stream, (const double*)d_wts, W, d_wsum);
    TRY(check_launch(h, "k_sr_wsum"));
    wts = d_wts;
  }
  hipLaunchKernelGGL(k_sr_means, dim3(6), dim3(256), 0, h->stream, d_en, wts, (const double*)d_wsum, W, d_mean);
  TRY(check_launch(h, "k_sr_means"));
  for (long w0 = 0; w0 < W; w0 += Wc) {
    const long wc = std::min(Wc, W - w0);
    const long ns = std::min<long>(nslice, std::max<long>(1, wc / 64));
    const long per = ((wc + ns - 1) / ns + kSrKB - 1) / kSrKB * kSrKB;  // walkers per slice, whole staging steps
    if (has_orb) {
      TRY(launch_ao(h, plain_points(h->js.x + (size_t)w0 * h->N * 3, wc * h->N), wc * h->N, 1, (double*)h->b_ao.p));
      const unsigned nwave = (unsigned)std::min(4, (h->nao + 15) / 16);
      for (int s = 0; s < 2; ++s) {
        if (!orb_spin[s]) continue;
        if (orb_lds[s] > 64 * 1024) TRY(raise_lds_limit(h, reinterpret_cast<const void*>(k_sr_orb)));
        hipLaunchKernelGGL(k_sr_orb, dim3((unsigned)wc), dim3(64 * nwave), orb_lds[s], h->stream, h->S, h->st, s, (const double*)h->b_ao.p,
                           (const double*)h->b_pgdet.p, (const int*)h->d_colmap[s], (const int*)d_colof[s], w0, lda, sr_orb_ldb(h->nmo[s]),
                           d_A);
        TRY(check_launch(h, "k_sr_orb"));
      }
    }
    hipLaunchKernelGGL(k_sr_gather, dim3((unsigned)((wc * lda + 255) / 256)), dim3(256), 0, h->stream, S, (const int*)d_src,
                       (const int*)d_pos, P, d_en, wts, (const double*)d_wsum, nodal_cutoff, W, w0, wc, d_A, d_scale);
    TRY(check_launch(h, "k_sr_gather"));
    if (dp_walker) {  // the chunk's dp = A[:, :P], before the next chunk overwrites it
      HIPCHK(hipMemcpy2DAsync(dp_walker + (size_t)w0 * P, (size_t)P * sizeof(double), d_A, (size_t)lda * sizeof(double),
                              (size_t)P * sizeof(double), (size_t)wc, hipMemcpyDeviceToHost, h->stream));
      HIPCHK(hipStreamSynchronize(h->stream));
    }
    hipLaunchKernelGGL(k_sr_syrk, dim3((unsigned)nbj, (unsigned)nbi, (unsigned)ns), dim3(256), 0, h->stream, (const double*)d_A,
                       (const double*)d_scale, wc, P, 2, 1, per, d_part);
    TRY(check_launch(h, "k_sr_syrk"));
    hipLaunchKernelGGL(k_sr_reduce, dim3((unsigned)((nmom + 255) / 256)), dim3(256), 0, h->stream, (const double*)d_part, P, 2, 0, (int)ns,
                       (int)(w0 == 0), 0, d_mom);
    TRY(check_launch(h, "k_sr_reduce"));
  }
  TRY(copy_in(h, moments, d_mom, nmom * sizeof(double)));
  if (en_walker) {
    transpose(h, d_en, d_enw, 6, W);  // rows (6, W) -> (W, 6)
    TRY(check_launch(h, "k_transpose"));
    TRY(copy_in(h, en_walker, d_enw, (size_t)6 * W * sizeof(double)));
  }
  return copy_out(h, en_mean, d_mean, 6 * sizeof(double));
}

extern "C" int pqa_sr_moments(pqa_handle_t* h, int P, const int32_t* src, const int32_t* pos, double nodal_cutoff, const double* weights,
                              double threshold, const double* rot, const double* unif, uint64_t seed, double* en_mean, double* moments,
                              double* en_walker) {
  return sr_moments(h, "pqa_sr_moments", false, P, src, pos, nodal_cutoff, weights, threshold, rot, unif, seed, 0, en_mean, moments, en_walker,
                    nullptr);
}

extern "C" int pqa_sr_moments_orb(pqa_handle_t* h, int P, const int32_t* src, const int32_t* pos, double nodal_cutoff, const double* weights,
                                  double threshold, const double* rot, const double* unif, uint64_t seed, int64_t walker_chunk,
                                  double* en_mean, double* moments, double* en_walker, double* dp_walker) {
  return sr_moments(h, "pqa_sr_moments_orb", true, P, src, pos, nodal_cutoff, weights, threshold, rot, unif, seed, (long)walker_chunk, en_mean,
                    moments, en_walker, dp_walker);
}

// The complex entry: the steps of sr_moments with complex columns (k_sr_gather_c, k_sr_syrk_c, k_sr_reduce_c).  Real handles are taken
// too (zero imaginary planes, six energy rows): a cross-check against pqa_sr_moments.
extern "C" int pqa_sr_moments_c(pqa_handle_t* h, int P, const int32_t* src, const int32_t* pos, int ntail, const int32_t* tail,
                                double nodal_cutoff, const double* weights, double threshold, const double* rot, const double* unif,
                                uint64_t seed, int64_t walker_chunk_arg, double* en_mean, double* moments, double* en_walker,
                                double* dp_walker) {
  const std::string fn = "pqa_sr_moments_c";
  // argument checks first: they need nothing but the handle's host-side sizes
  if (P < 1) FAIL(fn + ": P must be at least 1");
  if (!src || !pos || !en_mean || !moments) FAIL(fn + ": src, pos, en_mean and moments must not be NULL");
  if (ntail < 0 || ntail > P || (ntail > 0 && !tail)) FAIL(fn + ": ntail must be within 0 .. P, with tail given");
  if (!(nodal_cutoff > 0.0)) FAIL(fn + ": nodal_cutoff must be positive");
  const long size[4] = {h->has_slater ? (long)h->ndet : 0, h->has_j2 ? (long)h->natom * h->na * 2 : 0, h->has_j2 ? (long)h->nb * 3 : 0,
                        h->has_j3 ? (long)h->natom * h->na3 * h->na3 * h->nb3 * 3 : 0};
  bool need[4] = {false, false, false, false};
  for (int i = 0; i < P; ++i) {
    if (src[i] == 4 || src[i] == 5) FAIL(fn + ": orbital coefficients are not a source here (complex / periodic layouts: use the protocol route)");
    if (src[i] < 0 || src[i] > 3) FAIL(fn + ": src must be 0 (det_coeff), 1 (acoeff), 2 (bcoeff) or 3 (ccoeff)");
    if (pos[i] < 0 || pos[i] >= size[src[i]]) FAIL(fn + ": pos outside the parameter src names (or the handle has no such factor)");
    need[src[i]] = true;
  }
  {
    std::vector<char> seen((size_t)P, 0);
    for (int t = 0; t < ntail; ++t) {
      if (tail[t] < 0 || tail[t] >= P) FAIL(fn + ": tail names a primary column out of range");
      if (seen[tail[t]]) FAIL(fn + ": tail names a primary column twice");
      seen[tail[t]] = 1;
    }
  }
  if (walker_chunk_arg < 0) FAIL(fn + ": walker_chunk must not be negative");
  const int Pt = P + ntail, lda = Pt + 2;
  const size_t nmom = (size_t)lda * Pt;  // complex entries of the moments
  if (2 * nmom * sizeof(double) > kChunkScratchBytes) FAIL(fn + ": the (Pt + 2) x Pt complex moments exceed the 256 MiB scratch limit (use the protocol route)");
  if (h->W == 0) FAIL("state not initialised (call pqa_wf_recompute)");
  TRY(sync_aos(h));
  HIPCHK(hipSetDevice(h->device));
  const long W = h->W;
  const int cplx = h->cplx ? 1 : 0, nen = cplx ? 7 : 6;
  h->saved_valid = false;  // (as pqa_energy: the saved orbital rows of a gradient_value call are overwritten)
  TRY(energy_dev(h, threshold, rot, unif, seed, 0u));
  const double* d_en = (const double*)h->b_en.p;
  // derivative sources
  SrSources S{};
  if (need[0]) {
    TRY(slater_value_dev(h));  // sign (complex: phase) / log of the determinant expansion -> b_sign, b_log
    TRY(ensure(h, h->b_pgdet, (size_t)(cplx ? 2 : 1) * W * h->ndet * sizeof(double)));
    const dim3 gd((unsigned)((W * h->ndet + 255) / 256));
    if (cplx)
      hipLaunchKernelGGL((k_pgrad_det_c<>), gd, dim3(256), 0, h->stream, h->S, h->st, (const double*)h->b_sign.p, (const double*)h->b_log.p, W,
                         (double*)h->b_pgdet.p);
    else
      hipLaunchKernelGGL((k_pgrad_det<>), gd, dim3(256), 0, h->stream, h->S, h->st, (const double*)h->b_sign.p, (const double*)h->b_log.p, W,
                         (double*)h->b_pgdet.p);
    TRY(check_launch(h, "k_pgrad_det"));
    S.base[0] = (const double*)h->b_pgdet.p; S.stride[0] = size[0];
  }
  if (need[1] || need[2]) {
    TRY(jas_refresh(h));
    S.base[1] = h->js.avalues; S.stride[1] = size[1];
    S.base[2] = h->js.bvalues; S.stride[2] = size[2];
  }
  if (need[3]) {
    const size_t lds = ((size_t)h->N * h->natom * h->na3 + (size_t)h->N * (h->N - 1) / 2 * h->nb3) * sizeof(double);
    if (lds > 150 * 1024) FAIL("three-body parameter gradient: the a/b value tables of one walker do not fit LDS");
    TRY(ensure(h, h->b_out, (size_t)W * size[3] * sizeof(double)));
    if (lds > 64 * 1024) TRY(raise_lds_limit(h, reinterpret_cast<const void*>(k_j3_pgrad<>)));
    hipLaunchKernelGGL((k_j3_pgrad<>), dim3((unsigned)W), dim3(64), lds, h->stream, h->S, h->js, (double*)h->b_out.p);
    TRY(check_launch(h, "k_j3_pgrad"));
    S.base[3] = (const double*)h->b_out.p; S.stride[3] = size[3];
  }
  // one flag per 32-column block of A: does it hold a column that can have an imaginary part (source 0 of a complex handle, a tail
  // column, the E column of a complex handle)
  const int nbi = (lda + 31) / 32, nbj = (Pt + 31) / 32;
  std::vector<int> flag((size_t)nbi, 0);
  for (int i = 0; i < P; ++i)
    if (cplx && src[i] == 0) flag[i / 32] = 1;
  for (int i = P; i < Pt; ++i) flag[i / 32] = 1;
  if (cplx) flag[Pt / 32] = 1;
  // scratch: [moments (2 nmom) | means (7) | weight sum (1) | weights (W) | per-walker energies (W, nen) | scale (Wc) | Ar, Ai (Wc, Pt + 2) |
  // interleaved dp (Wc, Pt) when asked for | partials (nslice, 2, Pt + 2, Pt) | src, pos, tail, flag]
  long Wc = walker_chunk(W, (size_t)2 * lda * sizeof(double));
  if (walker_chunk_arg > 0) Wc = std::min<long>(Wc, (long)walker_chunk_arg);
  long nslice = std::min<long>(std::max<long>(1, 1024 / ((long)nbi * nbj)), std::max<long>(1, Wc / 64));
  nslice = std::max<long>(1, std::min<long>(nslice, (long)(kChunkScratchBytes / (2 * nmom * sizeof(double)))));
  const size_t nw = weights ? (size_t)W : 0, nenw = en_walker ? (size_t)nen * W : 0, ndp = dp_walker ? (size_t)2 * Wc * Pt : 0;
  const size_t ndbl = 2 * nmom + 7 + 1 + nw + nenw + (size_t)Wc + (size_t)2 * Wc * lda + ndp + (size_t)nslice * 2 * nmom;
  TRY(ensure(h, h->b_sr, ndbl * sizeof(double) + ((size_t)2 * P + ntail + nbi) * sizeof(int)));
  double* d_mom = (double*)h->b_sr.p;
  double* d_mean = d_mom + 2 * nmom;
  double* d_wsum = d_mean + 7;
  double* d_wts = d_wsum + 1;
  double* d_enw = d_wts + nw;
  double* d_scale = d_enw + nenw;
  double* d_Ar = d_scale + Wc;
  double* d_Ai = d_Ar + (size_t)Wc * lda;
  double* d_dp = d_Ai + (size_t)Wc * lda;
  double* d_part = d_dp + ndp;
  int* d_src = (int*)(d_part + (size_t)nslice * 2 * nmom);
  int* d_pos = d_src + P;
  int* d_tail = d_pos + P;
  int* d_flag = d_tail + ntail;
  TRY(copy_in(h, d_src, src, (size_t)P * sizeof(int)));
  TRY(copy_in(h, d_pos, pos, (size_t)P * sizeof(int)));
  TRY(copy_in(h, d_tail, tail, (size_t)ntail * sizeof(int)));
  TRY(copy_in(h, d_flag, flag.data(), (size_t)nbi * sizeof(int)));
  HIPCHK(hipStreamSynchronize(h->stream));  // (flag is a local: the copy has read it before it goes)
  const double* wts = nullptr;
  if (weights) {
    TRY(copy_in(h, d_wts, weights, (size_t)W * sizeof(double)));
    hipLaunchKernelGGL(k_sr_wsum, dim3(1), dim3(256), 0, h->stream, (const double*)d_wts, W, d_wsum);
    TRY(check_launch(h, "k_sr_wsum"));
    wts = d_wts;
  }
  hipLaunchKernelGGL(k_sr_means, dim3((unsigned)nen), dim3(256), 0, h->stream, d_en, wts, (const double*)d_wsum, W, d_mean);
  TRY(check_launch(h, "k_sr_means"));
  for (long w0 = 0; w0 < W; w0 += Wc) {
    const long wc = std::min(Wc, W - w0);
    const long ns = std::min<long>(nslice, std::max<long>(1, wc / 64));
    const long per = ((wc + ns - 1) / ns + kSrKB - 1) / kSrKB * kSrKB;  // walkers per slice, whole staging steps
    hipLaunchKernelGGL(k_sr_gather_c, dim3((unsigned)((wc * lda + 255) / 256)), dim3(256), 0, h->stream, S, (const int*)d_src, (const int*)d_pos, P,
                       (const int*)d_tail, ntail, cplx, d_en, wts, (const double*)d_wsum, nodal_cutoff, W, w0, wc, d_Ar, d_Ai, d_scale,
                       dp_walker ? d_dp : nullptr);
    TRY(check_launch(h, "k_sr_gather_c"));
    if (dp_walker)  // the chunk's dp, before the next chunk overwrites it
      TRY(copy_out(h, dp_walker + (size_t)2 * w0 * Pt, d_dp, (size_t)2 * wc * Pt * sizeof(double)));
    hipLaunchKernelGGL(k_sr_syrk_c, dim3((unsigned)nbj, (unsigned)nbi, (unsigned)ns), dim3(256), 0, h->stream, (const double*)d_Ar,
                       (const double*)d_Ai, (const double*)d_scale, (const int*)d_flag, wc, Pt, per, d_part);
    TRY(check_launch(h, "k_sr_syrk_c"));
    hipLaunchKernelGGL(k_sr_reduce_c, dim3((unsigned)((nmom + 255) / 256)), dim3(256), 0, h->stream, (const double*)d_part, Pt, (int)ns,
                       (int)(w0 == 0), d_mom);
    TRY(check_launch(h, "k_sr_reduce_c"));
  }
  TRY(copy_in(h, moments, d_mom, 2 * nmom * sizeof(double)));
  if (en_walker) {
    transpose(h, d_en, d_enw, nen, W);  // rows (nen, W) -> (W, nen)
    TRY(check_launch(h, "k_transpose"));
    HIPCHK(hipMemcpy2DAsync(en_walker, 7 * sizeof(double), d_enw, (size_t)nen * sizeof(double), (size_t)nen * sizeof(double), (size_t)W,
                            hipMemcpyDeviceToHost, h->stream));
  }
  TRY(copy_out(h, en_mean, d_mean, (size_t)nen * sizeof(double)));
  if (!cplx) {  // a real handle has no seventh row
    en_mean[6] = 0.0;
    if (en_walker)
      for (long w = 0; w < W; ++w) en_walker[7 * w + 6] = 0.0;
  }
  return 0;
}
