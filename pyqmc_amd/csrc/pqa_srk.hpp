// The product of the moment estimators (pqa_sr: StochasticReconfiguration.avg; pqa_mix: the mixture estimators of several states) and the
// preparation of its derivative columns; no other unit includes it.
//
// Both gather, per walker chunk, a compact row-major A = [derivative columns (P) | nx further columns] (Wc, P + nx) and a scale s (Wc)
// and need M = A^T diag(s) A[:, :P]:
//   sr_check_columns the column description (src, pos) of an entry against the handle's parameters;
//   sr_sources       the per-walker derivative arrays a column description names, left on the handle (det_coeff: pgrad_det_dev; acoeff /
//                    bcoeff: the basis sums the handle keeps, refreshed where a fused sweep left them stale; ccoeff: j3_pgrad_dev);
//   k_sr_syrk        M on v_mfma_f64_16x16x4_f64, walkers as the k dimension.  A block of four waves owns a 32 x 32 tile (one 16 x 16
//                    tile per wave) and a slice of the walkers; 16 walkers of both column panels are staged in LDS per step, the
//                    right-hand panel scaled by s as it is loaded.  The leading P x P block is symmetric: of its tiles only those on or
//                    above the diagonal are computed (sym), or none at all (!sym: a caller that needs the nx further rows only);
//   k_sr_reduce      the slices' partial tiles summed in slice order (the same bits on every call), the lower triangle mirrored from
//                    the upper one (the P x P block is exactly symmetric), added to the running moments of the chunks before (pqa_sr:
//                    as one term; pqa_mix: slice by slice, so that the chunking does not show in the result);
#pragma once
#include "pqa_estim.hpp"

namespace {

constexpr int kSrKB = 16;      // walkers staged per step of k_sr_syrk
constexpr int kSrLd = 48;      // doubles per staged row: 32 columns + 16 of padding, so rows kq and kq + 1 of an operand read land in
                               // different halves of the 64 LDS banks (no conflict within a half-wave's ds_read_b64)

struct SrSources {
  const double* base[4];  // det_coeff, acoeff, bcoeff, ccoeff derivatives, walker-major
  long stride[4];         // doubles per walker of each
};

// part[sl] (P + nx, P) += tile (32 bi .., 32 bj ..) of A^T diag(s) A[:, :P] over the walkers of slice sl.  grid = (column blocks,
// row blocks, slices), block = 256: wave (wi, wj) = (wave >> 1, wave & 1) owns the 16 x 16 tile (2 bi + wi, 2 bj + wj).  Blocks strictly
// below the diagonal (!sym: all blocks) are skipped unless they hold a row >= P (the nx further rows); a wave's tile of that kind is
// not stored.
__global__ __launch_bounds__(256) void k_sr_syrk(const double* __restrict__ A, const double* __restrict__ scale, long Wc, int P, int nx, int sym,
                                                 long per, double* __restrict__ part) {
  __shared__ double La[kSrKB * kSrLd], Lb[kSrKB * kSrLd];
  const int bj = blockIdx.x, bi = blockIdx.y, sl = blockIdx.z;
  if ((bi > bj || !sym) && bi * 32 + 31 < P) return;
  const int lda = P + nx;
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6, i16 = lane & 15, kq = lane >> 4, wi = wave >> 1, wj = wave & 1;
  const long k_lo = (long)sl * per, k_hi = k_lo + per < Wc ? k_lo + per : Wc;
  // staging: element e = t + 256 q of the two 16 x 32 panels: panel e >> 9, row (e >> 5) & 15, column e & 31
  const int c = t & 31, r0 = t >> 5;  // q advances the row by 8; q >= 2: the right-hand panel
  const int ca = bi * 32 + c, cb = bj * 32 + c;
  const bool ain = ca < lda, bin = cb < P;
  double v[4];
  auto fetch = [&](long k0) {
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const long row = k0 + r0 + 8 * (q & 1);
      const bool rin = row < k_hi;
      if (q < 2) v[q] = (rin && ain) ? A[(size_t)row * lda + ca] : 0.0;
      else v[q] = (rin && bin) ? A[(size_t)row * lda + cb] * scale[row] : 0.0;
    }
  };
  d4 acc = {0.0, 0.0, 0.0, 0.0};
  if (k_lo < k_hi) fetch(k_lo);
  for (long k0 = k_lo; k0 < k_hi; k0 += kSrKB) {
#pragma unroll
    for (int q = 0; q < 4; ++q) (q < 2 ? La : Lb)[(r0 + 8 * (q & 1)) * kSrLd + c] = v[q];
    __syncthreads();
    if (k0 + kSrKB < k_hi) fetch(k0 + kSrKB);  // (the next step's loads fly while this one multiplies)
#pragma unroll
    for (int kk = 0; kk < kSrKB / 4; ++kk) {
      const int row = kk * 4 + kq;
      acc = __builtin_amdgcn_mfma_f64_16x16x4f64(La[row * kSrLd + wi * 16 + i16], Lb[row * kSrLd + wj * 16 + i16], acc, 0, 0, 0);
    }
    __syncthreads();
  }
  const int ti = 2 * bi + wi, tj = 2 * bj + wj;
  if ((ti > tj || !sym) && ti * 16 + 15 < P) return;
  // lane holds D[row = kq + 4 r][col = i16]
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const int p = ti * 16 + kq + 4 * r, q = tj * 16 + i16;
    if (p < lda && q < P) part[((size_t)sl * lda + p) * P + q] = acc[r];
  }
}

// mom (P + nx, P), rows row0 .. = (first ? 0 : mom) + sum over the slices in slice order; element (i, j) of the symmetric block is read
// at (min, max): the tiles below the diagonal were never written.  row0: 0, or P for a product formed without its symmetric block.
// running: the slices are added to the moments of the chunks before one after the other (the sum over all slices of all chunks has ONE
// order, whatever the chunks), not as their own sum.
__global__ __launch_bounds__(256) void k_sr_reduce(const double* __restrict__ part, int P, int nx, int row0, int nslice, int first, int running,
                                                   double* __restrict__ mom) {
  const long n = (long)(P + nx) * P;
  const long idx = (long)row0 * P + (long)blockIdx.x * 256 + threadIdx.x;
  if (idx >= n) return;
  const int i = (int)(idx / P), j = (int)(idx - (long)i * P);
  const long from = (i < P && j < i) ? (long)j * P + i : idx;
  double s = (running && !first) ? mom[idx] : 0.0;
  for (int sl = 0; sl < nslice; ++sl) s += part[(size_t)sl * n + from];
  mom[idx] = (first || running) ? s : mom[idx] + s;
}

// Slices of a chunk's product: enough blocks to fill the device, at least 64 walkers each, partial tiles within the scratch limit.
inline long sr_slices(long Wc, int nbi, int nbj, size_t nmom) {
  const long nslice = std::min<long>(std::max<long>(1, 1024 / ((long)nbi * nbj)), std::max<long>(1, Wc / 64));
  return std::max<long>(1, std::min<long>(nslice, (long)(kChunkScratchBytes / (nmom * sizeof(double)))));
}

}  // namespace

// Entries of the four derivative sources of handle h (0 where it lacks the factor).
inline void sr_source_sizes(const pqa_handle* h, long (&size)[4]) {
  size[0] = h->has_slater ? (long)h->ndet : 0;
  size[1] = h->has_j2 ? (long)h->natom * h->na * 2 : 0;
  size[2] = h->has_j2 ? (long)h->nb * 3 : 0;
  size[3] = h->has_j3 ? (long)h->natom * h->na3 * h->na3 * h->nb3 * 3 : 0;
}

// The plain columns of an entry fn: every src[i] within 0 .. max_src (2: the mixture entries, 3: the SR entries) and pos[i] within the
// parameter of handle g it names -> need[src[i]].  A failure is reported on h.
inline int sr_check_columns(pqa_handle* h, const pqa_handle* g, const std::string& fn, int P, const int32_t* src, const int32_t* pos, int max_src,
                            bool (&need)[4]) {
  long size[4];
  sr_source_sizes(g, size);
  for (int i = 0; i < P; ++i) {
    if (src[i] < 0 || src[i] > max_src)
      FAIL(fn + (max_src < 3 ? ": src must be 0 (det_coeff), 1 (acoeff) or 2 (bcoeff) (three-body and orbital coefficients: the protocol route)"
                             : ": src must be 0 (det_coeff), 1 (acoeff), 2 (bcoeff) or 3 (ccoeff)"));
    if (pos[i] < 0 || pos[i] >= size[src[i]])
      FAIL(fn + (max_src < 3 ? ": pos outside the parameter src names" : ": pos outside the parameter src names (or the handle has no such factor)"));
    need[src[i]] = true;
  }
  return 0;
}

// The derivative arrays of the sources need[] names, for the resident walkers of handle h, on h's stream: S.base / S.stride (doubles
// per walker; S.base[0] of a complex handle is the interleaved (re, im) array of W x stride[0] pairs, as k_sr_gather_c reads it).
//   0  pgrad_det_dev -> b_pgdet (W, ndet), after the sign / log of the determinant expansion -> b_sign, b_log
//   1, 2  the Jastrow basis sums the handle keeps (refreshed when stale)
//   3  j3_pgrad_dev -> b_out
inline int sr_sources(pqa_handle* h, const bool (&need)[4], SrSources& S) {
  long size[4];
  sr_source_sizes(h, size);
  if (need[0]) {
    TRY(pgrad_det_dev(h));
    S.base[0] = (const double*)h->b_pgdet.p; S.stride[0] = size[0];
  }
  if (need[1] || need[2]) {
    TRY(jas_refresh(h));
    S.base[1] = h->js.avalues; S.stride[1] = size[1];
    S.base[2] = h->js.bvalues; S.stride[2] = size[2];
  }
  if (need[3]) {
    TRY(j3_pgrad_dev(h));
    S.base[3] = (const double*)h->b_out.p; S.stride[3] = size[3];
  }
  return 0;
}
