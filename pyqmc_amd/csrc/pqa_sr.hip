// Stochastic-reconfiguration moments of the resident walkers (StochasticReconfiguration.avg, stochastic_reconfiguration.py:49-118).
//
// The protocol route brings the walkers and every factor's (W x parameters) derivative arrays to the host, gathers the optimised
// columns there and uploads [dp | E | 1] and w f dp again for one product (pqa_gram).  Everything the estimator needs is on the handle
// already, so one host driver (sr_moments) leaves it there, for all three entries:
//   energy_dev       the energy pass of pqa_energy (same draws, same per-walker rows in b_en);
//   sr_sources       the derivative arrays the column description names (pqa_srk.hpp), and only those;
//   k_wsum, k_sr_means  the weight sum and the weighted energy means, fixed-order trees;
//   per walker chunk of at most 256 MiB:
//     gather         the compact row-major A = [dp | E | 1] (Wc, P + 2) and the scale s_w = w_w f_w (w: the normalised weight, f: the
//                    Pathak-Wagner weight from grad2);
//     product        A^T diag(s) A[:, :P] over slices of the chunk's walkers (w f dp never exists in memory);
//     reduce         the slices' partial tiles summed in slice order (the same bits on every call), the lower triangle mirrored from
//                    the upper one, added to the running moments of the chunks before.
// Only the (P + 2) x P moments and the energy means leave the device (and the per-walker energies / dp when the caller asks for them).
// The entries differ where their data do:
//   pqa_sr_moments      real handles, sources 0 - 3: k_sr_gather, k_sr_syrk, k_sr_reduce (the last two are pqa_srk.hpp's: pqa_mix forms
//                       its moments with them too).
//   pqa_sr_moments_orb  also the orbital coefficients (4: mo_coeff_alpha, 5: mo_coeff_beta).  Their derivative
//                         G[a][m] = sum_u wu[u] sum_e ao[e][a] T_u[e][col_u(m)],   wu[u] = sum_{di: det_map[di] = u} det_coeff[di] d_det[di]
//                       (k_pgrad_mo) never exists as a (W, nao, nmo) array: the AO values do not depend on u, so per walker and spin
//                         B[e][m] = sum_u wu[u] T_u[e][col_u(m)]   (n x nmo, zero where u does not occupy m),   G = ao^T B.
//                       Before the gather of a chunk, launch_ao writes the value-only AO rows of its electrons (b_ao: (Wc N, nao),
//                       nothing of size W N nao) and k_sr_orb, a block per walker, forms wu and B in LDS and G tile by tile on
//                       v_mfma_f64_16x16x4_f64, every entry stored through the inverse column map colof straight into A (entries
//                       nobody optimises are dropped); k_sr_gather leaves those columns alone.
//   pqa_sr_moments_c    complex and twisted handles (complex d_det, complex local energy; real handles are taken too) and the
//                       imaginary-part tail of the reference's serialised matrix: A as planar real / imaginary panels
//                       (k_sr_gather_c), one to four matrix instructions per k-step by what the two column blocks of a tile can hold
//                       (k_sr_syrk_c, by a flag per column block), both planes reduced (k_sr_reduce_c); seven energy slots.
#include "pqa_srk.hpp"

namespace {

// Pathak-Wagner weight (accumulators.nodal_regularization)
__device__ __forceinline__ double sr_nodal_f(double grad2, double cutoff) {
  const double x = 1.0 / (grad2 * (cutoff * cutoff));
  return x < 1.0 ? x * (9.0 + x * (-15.0 + 7.0 * x)) : 1.0;
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

// What an entry is: its name (in messages), whether sources 4 / 5 are accepted, whether its columns are complex (then with the ntail
// twins tail names), walkers per chunk (0: the scratch rule), dp_walker: host (W, P) doubles / (W, P + ntail) complex, or NULL.
struct SrEntry {
  const char* name;
  bool orb, cx;
  int ntail;
  const int32_t* tail;
  long chunk;
  double* dp_walker;
};

static int sr_moments(pqa_handle_t* h, const SrEntry& e, int P, const int32_t* src, const int32_t* pos, double nodal_cutoff, const double* weights,
                      double threshold, const double* rot, const double* unif, uint64_t seed, double* en_mean, double* moments, double* en_walker) {
  const std::string fn = e.name;
  const int ntail = e.ntail;
  // argument checks first: they need nothing but the handle's host-side sizes
  if (P < 1) FAIL(fn + ": P must be at least 1");
  if (!src || !pos || !en_mean || !moments) FAIL(fn + ": src, pos, en_mean and moments must not be NULL");
  if (e.cx && (ntail < 0 || ntail > P || (ntail > 0 && !e.tail))) FAIL(fn + ": ntail must be within 0 .. P, with tail given");
  if (!(nodal_cutoff > 0.0)) FAIL(fn + ": nodal_cutoff must be positive");
  if (h->cplx && !e.cx) FAIL(fn + ": complex orbitals / twisted cell (outside the device scope: use the protocol route)");
  bool need[4] = {false, false, false, false};
  bool orb_spin[2] = {false, false};
  std::vector<int> colof[2];  // [nao][nmo_s]: the column of A an orbital-coefficient entry fills, or -1
  for (int i = 0; i < P; ++i) {  // (column by column: the first bad column is the one reported, of whichever kind)
    const bool mo = src[i] == 4 || src[i] == 5;
    if (mo && e.orb) {
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
    if (mo && e.cx) FAIL(fn + ": orbital coefficients are not a source here (complex / periodic layouts: use the protocol route)");
    if (e.orb && (src[i] < 0 || src[i] > 3))
      FAIL(fn + ": src must be 0 (det_coeff), 1 (acoeff), 2 (bcoeff), 3 (ccoeff), 4 (mo_coeff_alpha) or 5 (mo_coeff_beta)");
    TRY(sr_check_columns(h, h, fn, 1, src + i, pos + i, 3, need));
  }
  const bool has_orb = orb_spin[0] || orb_spin[1];
  if (e.cx) {
    std::vector<char> seen((size_t)P, 0);
    for (int t = 0; t < ntail; ++t) {
      if (e.tail[t] < 0 || e.tail[t] >= P) FAIL(fn + ": tail names a primary column out of range");
      if (seen[e.tail[t]]) FAIL(fn + ": tail names a primary column twice");
      seen[e.tail[t]] = 1;
    }
  }
  if (e.chunk < 0) FAIL(fn + ": walker_chunk must not be negative");
  // Pt columns (the primary ones and the tail), cf planes of (Pt + 2) x Pt moments
  const int Pt = P + ntail, lda = Pt + 2, cf = e.cx ? 2 : 1;
  const size_t nmom = (size_t)lda * Pt;
  if (cf * nmom * sizeof(double) > kChunkScratchBytes)
    FAIL(fn + (e.cx ? ": the (Pt + 2) x Pt complex moments exceed the 256 MiB scratch limit (use the protocol route)"
                    : ": the (P + 2) x P moments exceed the 256 MiB scratch limit (use the protocol route)"));
  if (h->W == 0) FAIL("state not initialised (call pqa_wf_recompute)");
  TRY(sync_aos(h));
  HIPCHK(hipSetDevice(h->device));
  const long W = h->W;
  const int cplx = h->cplx ? 1 : 0, nen = cplx ? 7 : 6;  // rows of b_en
  const int nout = e.cx ? 7 : 6;                         // energy slots the entry returns (a real handle leaves the seventh zero)
  h->saved_valid = false;  // (as pqa_energy: the saved orbital rows of a gradient_value call are overwritten)
  TRY(energy_dev(h, threshold, rot, unif, seed, 0u));
  const double* d_en = (const double*)h->b_en.p;
  // derivative sources
  SrSources S{};
  need[0] = need[0] || has_orb;  // (the orbital columns need d_det for the determinant weights)
  TRY(sr_sources(h, need, S));
  // with orbital columns a chunk's A and AO rows (b_ao) together stay within the chunk limit
  long Wc = walker_chunk(W, ((size_t)cf * lda + (has_orb ? (size_t)h->N * h->nao : 0)) * sizeof(double));
  if (e.chunk > 0) Wc = std::min(Wc, e.chunk);
  size_t orb_lds[2] = {0, 0};
  for (int s = 0; s < 2; ++s)
    if (orb_spin[s]) {
      const int n = s ? h->ndn : h->nup;
      orb_lds[s] = ((size_t)((n + 3) & ~3) * sr_orb_ldb(h->nmo[s]) + h->ndet_s[s]) * sizeof(double);
      if (orb_lds[s] > 150 * 1024) FAIL(fn + ": orbital coefficients: the determinant weights of one walker do not fit LDS (use the protocol route)");
    }
  const int nbi = (lda + 31) / 32, nbj = (Pt + 31) / 32;
  const long nslice = sr_slices(Wc, nbi, nbj, cf * nmom);
  // complex columns: one flag per 32-column block of A: does it hold a column that can have an imaginary part (source 0 of a complex
  // handle, a tail column, the E column of a complex handle)
  std::vector<int> flag(e.cx ? (size_t)nbi : 0, 0);
  if (e.cx) {
    for (int i = 0; i < P; ++i)
      if (cplx && src[i] == 0) flag[i / 32] = 1;
    for (int i = P; i < Pt; ++i) flag[i / 32] = 1;
    if (cplx) flag[Pt / 32] = 1;
  }
  // scratch
  double *d_mom, *d_mean, *d_wsum, *d_wts, *d_enw, *d_scale, *d_A, *d_dp, *d_part;
  int *d_src, *d_pos, *d_tail, *d_flag, *d_colof[2];
  auto layout = [&](Carver c) {
    d_mom = c.take<double>(cf * nmom);
    d_mean = c.take<double>(nout);
    d_wsum = c.take<double>(1);
    d_wts = c.take<double>(weights ? W : 0);
    d_enw = c.take<double>(en_walker ? (size_t)nen * W : 0);  // per-walker energies (W, nen)
    d_scale = c.take<double>(Wc);
    d_A = c.take<double>((size_t)cf * Wc * lda);  // complex columns: the real plane, then the imaginary one
    d_dp = c.take<double>(e.cx && e.dp_walker ? (size_t)2 * Wc * Pt : 0);  // interleaved dp of a chunk
    d_part = c.take<double>((size_t)nslice * cf * nmom);
    d_src = c.take<int>(P);
    d_pos = c.take<int>(P);
    d_tail = c.take<int>(ntail);
    d_flag = c.take<int>(flag.size());
    for (int s = 0; s < 2; ++s) d_colof[s] = c.take<int>(colof[s].size());
    return c.size();
  };
  TRY(ensure(h, h->b_sr, layout(Carver())));
  layout(Carver(h->b_sr.p));
  double* d_Ai = d_A + (size_t)Wc * lda;
  TRY(copy_in(h, d_src, src, (size_t)P * sizeof(int)));
  TRY(copy_in(h, d_pos, pos, (size_t)P * sizeof(int)));
  TRY(copy_in(h, d_tail, e.tail, (size_t)ntail * sizeof(int)));
  TRY(copy_in(h, d_flag, flag.data(), flag.size() * sizeof(int)));
  for (int s = 0; s < 2; ++s) TRY(copy_in(h, d_colof[s], colof[s].data(), colof[s].size() * sizeof(int)));
  if (has_orb) TRY(ensure(h, h->b_ao, (size_t)Wc * h->N * h->nao * sizeof(double)));
  const double* wts = nullptr;
  if (weights) {
    TRY(copy_in(h, d_wts, weights, (size_t)W * sizeof(double)));
    hipLaunchKernelGGL((k_wsum<>), dim3(1), dim3(256), 0, h->stream, (const double*)d_wts, W, d_wsum);
    TRY(check_launch(h, "k_wsum"));
    wts = d_wts;
  }
  hipLaunchKernelGGL(k_sr_means, dim3((unsigned)nen), dim3(256), 0, h->stream, d_en, wts, (const double*)d_wsum, W, d_mean);
  TRY(check_launch(h, "k_sr_means"));
  const dim3 gmom((unsigned)((nmom + 255) / 256));
  for (long w0 = 0; w0 < W; w0 += Wc) {
    const long wc = std::min(Wc, W - w0);
    const long ns = std::min<long>(nslice, std::max<long>(1, wc / 64));
    const long per = ((wc + ns - 1) / ns + kSrKB - 1) / kSrKB * kSrKB;  // walkers per slice, whole staging steps
    const dim3 ggather((unsigned)((wc * lda + 255) / 256)), gsyrk((unsigned)nbj, (unsigned)nbi, (unsigned)ns);
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
    // gather, and the chunk's dp for the caller that asked for it, before the next chunk overwrites it
    if (e.cx) {
      hipLaunchKernelGGL(k_sr_gather_c, ggather, dim3(256), 0, h->stream, S, (const int*)d_src, (const int*)d_pos, P, (const int*)d_tail, ntail,
                         cplx, d_en, wts, (const double*)d_wsum, nodal_cutoff, W, w0, wc, d_A, d_Ai, d_scale, e.dp_walker ? d_dp : nullptr);
      TRY(check_launch(h, "k_sr_gather_c"));
      if (e.dp_walker) TRY(copy_out(h, e.dp_walker + (size_t)2 * w0 * Pt, d_dp, (size_t)2 * wc * Pt * sizeof(double)));
    } else {
      hipLaunchKernelGGL(k_sr_gather, ggather, dim3(256), 0, h->stream, S, (const int*)d_src, (const int*)d_pos, P, d_en, wts,
                         (const double*)d_wsum, nodal_cutoff, W, w0, wc, d_A, d_scale);
      TRY(check_launch(h, "k_sr_gather"));
      if (e.dp_walker) {  // dp = A[:, :P]
        HIPCHK(hipMemcpy2DAsync(e.dp_walker + (size_t)w0 * P, (size_t)P * sizeof(double), d_A, (size_t)lda * sizeof(double),
                                (size_t)P * sizeof(double), (size_t)wc, hipMemcpyDeviceToHost, h->stream));
        HIPCHK(hipStreamSynchronize(h->stream));
      }
    }
    // product and reduce
    if (e.cx) {
      hipLaunchKernelGGL(k_sr_syrk_c, gsyrk, dim3(256), 0, h->stream, (const double*)d_A, (const double*)d_Ai, (const double*)d_scale,
                         (const int*)d_flag, wc, Pt, per, d_part);
      TRY(check_launch(h, "k_sr_syrk_c"));
      hipLaunchKernelGGL(k_sr_reduce_c, gmom, dim3(256), 0, h->stream, (const double*)d_part, Pt, (int)ns, (int)(w0 == 0), d_mom);
      TRY(check_launch(h, "k_sr_reduce_c"));
    } else {
      hipLaunchKernelGGL(k_sr_syrk, gsyrk, dim3(256), 0, h->stream, (const double*)d_A, (const double*)d_scale, wc, P, 2, 1, per, d_part);
      TRY(check_launch(h, "k_sr_syrk"));
      hipLaunchKernelGGL(k_sr_reduce, gmom, dim3(256), 0, h->stream, (const double*)d_part, P, 2, 0, (int)ns, (int)(w0 == 0), 0, d_mom);
      TRY(check_launch(h, "k_sr_reduce"));
    }
  }
  TRY(copy_in(h, moments, d_mom, cf * nmom * sizeof(double)));
  if (en_walker) {
    transpose(h, d_en, d_enw, nen, W);  // rows (nen, W) -> (W, nen), into the caller's (W, nout)
    TRY(check_launch(h, "k_transpose"));
    HIPCHK(hipMemcpy2DAsync(en_walker, (size_t)nout * sizeof(double), d_enw, (size_t)nen * sizeof(double), (size_t)nen * sizeof(double), (size_t)W,
                            hipMemcpyDeviceToHost, h->stream));
  }
  TRY(copy_out(h, en_mean, d_mean, (size_t)nen * sizeof(double)));
  if (nen < nout) {  // the complex entry on a real handle: there is no seventh row
    en_mean[6] = 0.0;
    if (en_walker)
      for (long w = 0; w < W; ++w) en_walker[7 * w + 6] = 0.0;
  }
  return 0;
}

extern "C" int pqa_sr_moments(pqa_handle_t* h, int P, const int32_t* src, const int32_t* pos, double nodal_cutoff, const double* weights,
                              double threshold, const double* rot, const double* unif, uint64_t seed, double* en_mean, double* moments,
                              double* en_walker) {
  return sr_moments(h, {"pqa_sr_moments", false, false, 0, nullptr, 0, nullptr}, P, src, pos, nodal_cutoff, weights, threshold, rot, unif, seed,
                    en_mean, moments, en_walker);
}

extern "C" int pqa_sr_moments_orb(pqa_handle_t* h, int P, const int32_t* src, const int32_t* pos, double nodal_cutoff, const double* weights,
                                  double threshold, const double* rot, const double* unif, uint64_t seed, int64_t walker_chunk,
                                  double* en_mean, double* moments, double* en_walker, double* dp_walker) {
  return sr_moments(h, {"pqa_sr_moments_orb", true, false, 0, nullptr, (long)walker_chunk, dp_walker}, P, src, pos, nodal_cutoff, weights,
                    threshold, rot, unif, seed, en_mean, moments, en_walker);
}

extern "C" int pqa_sr_moments_c(pqa_handle_t* h, int P, const int32_t* src, const int32_t* pos, int ntail, const int32_t* tail,
                                double nodal_cutoff, const double* weights, double threshold, const double* rot, const double* unif,
                                uint64_t seed, int64_t walker_chunk, double* en_mean, double* moments, double* en_walker, double* dp_walker) {
  return sr_moments(h, {"pqa_sr_moments_c", false, true, ntail, tail, (long)walker_chunk, dp_walker}, P, src, pos, nodal_cutoff, weights,
                    threshold, rot, unif, seed, en_mean, moments, en_walker);
}
