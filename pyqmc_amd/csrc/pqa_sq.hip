// Structure factor of the resident walkers (SqAccumulator, pyqmc/observables/accumulators.py:191-234), read-only on the handle.
//
// Per walker and q:  u = sum_{j up} e^{i q.r_j},  d = sum_{j dn} e^{i q.r_j},  Sq = |u + d|^2 / N,  spinSq = |u - d|^2 / N.
//
// The coordinates are read in place from whichever layout holds the live state: the walker-major array js.x, or, after a fused
// sweep (aos_stale), the lane-per-walker planes b_xt ([N*3][W]); the strides (sw, se, sc) select the layout as k_ewald's do, so
// no layout conversion runs and nothing a sweep reads is written.  Periodic points are folded into the cell (twisted handles keep
// unfolded coordinates; the reference's PeriodicConfigs hold folded ones).
//
// k_sq: a block takes WB walkers of a walker chunk (WB a power of two, chosen from the LDS per walker and the chunk size).
//   1. per (walker, electron, axis) one thread folds the point and writes to LDS either
//        recurrence (q = sum_a n_a b_a on the q grids): the powers m = 0..nmax of e^{i b_a.r} (complex products from e^{i b_a.r}),
//        direct (an arbitrary qlist):                     the coordinates.
//   2. per (q, walker) item one thread sums over the electrons, up and down separately:
//        recurrence: e^{i q.r} = prod_a (e^{i b_a.r})^{n_a}, negative n_a by conjugation: three 16-byte LDS reads and two complex
//                    products per (q, electron), no sincos;
//        direct:     one sincos of q.r per (q, electron).
//      Items are q-major (item = q * WB + walker): the lanes of a wave read the same table entry of WB different walkers, whose
//      tables start 16 bytes apart modulo the 256-byte bank width (stride padding), so those reads do not conflict.
//   It writes the per-walker values of the chunk ([2][wc][Q]).
// Per-walker mode copies each chunk out.  Mean mode sums every chunk on the device in a fixed order (k_sq_rows: column sums over
// fixed row slices; k_sq_fold: the slices in order, plus the previous chunks' running sum) and divides by W at the last chunk:
// no atomics, so two calls give the same bits.
#include "pqa_estim.hpp"

namespace {

constexpr size_t kSqLdsBlock = 40 << 10;              // LDS per block WB is sized for (four blocks of four waves per CU)
constexpr size_t kSqLdsMax = 160 << 10;               // LDS per CU: a larger phase table takes the direct path
constexpr int kSqThreads = 256;
constexpr int kSqRowSlices = 256;                     // mean mode: row slices of a chunk summed by k_sq_rows

struct SqArgs {
  int N, nup, Q, wbs, M;  // electrons, up electrons, q vectors, log2(walkers per block), powers per base phase (recurrence)
  long stride;            // doubles per walker table in LDS (stride * 8 = 16 mod 256)
  const double* q;        // [Q][3] Cartesian (direct)
  const int* qn;          // [Q][3] integer coordinates in the basis recip (recurrence)
  double recip[9];        // rows b_a
};

template <bool REC>
__global__ __launch_bounds__(kSqThreads) void k_sq(SysDev S, SqArgs A, const double* __restrict__ x, long sw, long se, long sc,
                                                   long w0, long wc, double* __restrict__ out) {
  extern __shared__ double lds[];
  const int WB = 1 << A.wbs, N = A.N, Q = A.Q;
  const long b0 = (long)blockIdx.x * WB;  // first walker of the block within the chunk
  const int nw = (int)min((long)WB, wc - b0);
  const int tid = threadIdx.x;
  for (int k = tid; k < nw * N * 3; k += kSqThreads) {  // walker fastest: neighbouring lanes read neighbouring walkers of the planes
    const int wl = k % nw, r = k / nw, e = r / 3, a = r % 3;
    const double* xp = x + (w0 + b0 + wl) * sw + (long)e * se;
    double px = xp[0], py = xp[sc], pz = xp[2 * sc];
    fold_cell(S, px, py, pz);
    double* tw = lds + (size_t)wl * A.stride;
    if (REC) {
      double sn, cs;
      sincos(A.recip[3 * a] * px + A.recip[3 * a + 1] * py + A.recip[3 * a + 2] * pz, &sn, &cs);
      double* t = tw + (size_t)r * A.M * 2;  // [e][a][m][re, im]
      double cr = 1.0, ci = 0.0;
      for (int m = 0; m < A.M; ++m) {
        t[2 * m] = cr; t[2 * m + 1] = ci;
        const double nr = cr * cs - ci * sn;
        ci = cr * sn + ci * cs;
        cr = nr;
      }
    } else {
      tw[r] = a == 0 ? px : (a == 1 ? py : pz);
    }
  }
  __syncthreads();
  for (int it = tid; it < Q * WB; it += kSqThreads) {
    const int q = it >> A.wbs, wl = it & (WB - 1);
    if (wl >= nw) continue;
    double ur = 0.0, ui = 0.0, dr = 0.0, di = 0.0;
    if (REC) {
      const int n0 = A.qn[3 * q], n1 = A.qn[3 * q + 1], n2 = A.qn[3 * q + 2];
      const int M = A.M;
      const double f0 = n0 < 0 ? -1.0 : 1.0, f1 = n1 < 0 ? -1.0 : 1.0, f2 = n2 < 0 ? -1.0 : 1.0;
      const double2* t = reinterpret_cast<const double2*>(lds + (size_t)wl * A.stride);
      const int o0 = abs(n0), o1 = M + abs(n1), o2 = 2 * M + abs(n2);
      auto term = [&](int e, double& sr, double& si) {
        const double2* te = t + (size_t)e * 3 * M;
        const double2 av = te[o0], bv = te[o1], cv = te[o2];
        const double ar = av.x, ai = f0 * av.y, br = bv.x, bi = f1 * bv.y, cr = cv.x, ci = f2 * cv.y;
        const double abr = ar * br - ai * bi, abi = ar * bi + ai * br;
        sr += abr * cr - abi * ci;
        si += abr * ci + abi * cr;
      };
      for (int e = 0; e < A.nup; ++e) term(e, ur, ui);
      for (int e = A.nup; e < N; ++e) term(e, dr, di);
    } else {
      const double qx = A.q[3 * q], qy = A.q[3 * q + 1], qz = A.q[3 * q + 2];
      const double* tw = lds + (size_t)wl * A.stride;
      auto term = [&](int e, double& sr, double& si) {
        double sn, cs;
        sincos(tw[3 * e] * qx + tw[3 * e + 1] * qy + tw[3 * e + 2] * qz, &sn, &cs);
        sr += cs;
        si += sn;
      };
      for (int e = 0; e < A.nup; ++e) term(e, ur, ui);
      for (int e = A.nup; e < N; ++e) term(e, dr, di);
    }
    const double sr = ur + dr, si = ui + di, tr = ur - dr, ti = ui - di;
    const long w = b0 + wl;
    out[w * Q + q] = (sr * sr + si * si) / N;
    out[(wc + w) * Q + q] = (tr * tr + ti * ti) / N;
  }
}

// mean mode, stage 1: column sums of v ([2][wc][Q]) over the row slices [r rp, (r + 1) rp): part [2][R][Q]
__global__ __launch_bounds__(64) void k_sq_rows(const double* __restrict__ v, long wc, int Q, long rp, int R, double* __restrict__ part) {
  const int q = blockIdx.x * 64 + threadIdx.x;
  if (q >= Q) return;
  const int r = blockIdx.y, z = blockIdx.z;
  const long lo = (long)r * rp, hi = min(wc, lo + rp);
  const double* p = v + (size_t)z * wc * Q + q;
  double s = 0.0;
  for (long w = lo; w < hi; ++w) s += p[(size_t)w * Q];
  part[((size_t)z * R + r) * Q + q] = s;
}

// mean mode, stage 2: acc[z Q + q] = (first chunk ? 0 : acc) + sum_r part[z][r][q], divided by W after the last chunk
__global__ __launch_bounds__(256) void k_sq_fold(const double* __restrict__ part, int R, int Q, int first, int last, double W,
                                                 double* __restrict__ acc) {
  const int k = blockIdx.x * 256 + threadIdx.x;
  if (k >= 2 * Q) return;
  const int z = k / Q, q = k % Q;
  double s = 0.0;
  for (int r = 0; r < R; ++r) s += part[((size_t)z * R + r) * Q + q];
  double v = (first ? 0.0 : acc[k]) + s;
  if (last) v /= W;
  acc[k] = v;
}

// pqa_sq (weights == NULL) and pqa_sq_w (the walker means with the weights `weights`)
int sq_run(pqa_handle* h, int nqv, const double* q, const int* qn, const double* recip, int mean, const double* weights, double* sq,
           double* spinsq, const std::string& fn) {
  HIPCHK(hipSetDevice(h->device));
  if (h->W == 0) FAIL(fn + ": state not initialised (call recompute)");
  if (nqv < 0) FAIL(fn + ": negative q count");
  if (weights) TRY(check_weights(h, fn.c_str(), weights, h->W));
  if (nqv == 0) return 0;
  if (!q || !sq || !spinsq) FAIL(fn + ": q / sq / spinsq is NULL");
  const long W = h->W;
  const int N = h->N, Q = nqv;
  // the live coordinates, in place: the sweep's planes [N*3][W] when the walker-major arrays are stale, else js.x [W][N][3]
  const bool planes = h->aos_stale;
  const double* x = planes ? (const double*)h->b_xt.p : h->js.x;
  const long sw = planes ? 1L : 3L * N, se = planes ? 3L * W : 3L, sc = planes ? W : 1L;

  bool rec = qn && recip;
  int nmax = 0;
  if (rec)
    for (long k = 0; k < 3L * Q; ++k) nmax = std::max(nmax, std::abs(qn[k]));
  auto stride_of = [&](bool r) {  // doubles per walker table, padded to 16 bytes past a multiple of 256
    const long raw = r ? 3L * N * (nmax + 1) * 2 : 3L * N;
    return (raw + 31) / 32 * 32 + 2;
  };
  if (rec && (size_t)stride_of(true) * sizeof(double) > kSqLdsMax) rec = false;  // (the table would not fit: one sincos per term)
  SqArgs A{};
  A.N = N; A.nup = h->nup; A.Q = Q; A.M = nmax + 1;
  A.stride = stride_of(rec);
  const size_t tab = (size_t)A.stride * sizeof(double);
  if (tab > kSqLdsMax) FAIL(fn + ": too many electrons for the coordinate table in LDS");
  if (rec)
    for (int k = 0; k < 9; ++k) A.recip[k] = recip[k];

  const long Wc = walker_chunk(W, (size_t)2 * Q * sizeof(double));  // (the per-walker values of a chunk)
  // walkers per block: as many as fit kSqLdsBlock (at most 64), fewer while a chunk would give fewer than 2048 blocks
  int wbs = 6;
  while (wbs > 0 && ((size_t)1 << wbs) * tab > kSqLdsBlock) --wbs;
  while (wbs > 0 && (Wc >> wbs) < 2048) --wbs;
  A.wbs = wbs;
  const int WB = 1 << wbs;
  const size_t lds = (size_t)WB * tab;
  if (lds > 64 * 1024) TRY(raise_lds_limit(h, rec ? (const void*)k_sq<true> : (const void*)k_sq<false>));

  TRY(ensure(h, h->b_sqq, (size_t)Q * 3 * (sizeof(double) + sizeof(int))));
  double* d_q = (double*)h->b_sqq.p;
  int* d_qn = (int*)(d_q + (size_t)Q * 3);
  TRY(copy_in(h, d_q, q, (size_t)Q * 3 * sizeof(double)));
  if (rec) TRY(copy_in(h, d_qn, qn, (size_t)Q * 3 * sizeof(int)));
  A.q = d_q;
  A.qn = d_qn;
  TRY(ensure(h, h->b_sqout, (size_t)2 * Wc * Q * sizeof(double)));
  double* d_out = (double*)h->b_sqout.p;
  const long R = std::min<long>(kSqRowSlices, Wc);
  double *d_wts = nullptr, *d_wsum = nullptr;
  if (weights) {  // sums [2][Q], then the W weights and their sum; partials of the weighted column sums [2][slices][Q]
    TRY(ensure(h, h->b_sqpart, (size_t)2 * wcol_slices_max(std::min(Wc, W)) * Q * sizeof(double)));
    TRY(ensure(h, h->b_sqacc, ((size_t)2 * Q + W + 1) * sizeof(double)));
    d_wts = (double*)h->b_sqacc.p + (size_t)2 * Q;
    d_wsum = d_wts + W;
    TRY(copy_in(h, d_wts, weights, (size_t)W * sizeof(double)));
    hipLaunchKernelGGL((k_wsum<>), dim3(1), dim3(256), 0, h->stream, (const double*)d_wts, W, d_wsum);
    TRY(check_launch(h, "k_wsum"));
  } else if (mean) {
    TRY(ensure(h, h->b_sqpart, (size_t)2 * R * Q * sizeof(double)));
    TRY(ensure(h, h->b_sqacc, (size_t)2 * Q * sizeof(double)));
  }
  for (long w0 = 0; w0 < W; w0 += Wc) {
    const long wc = std::min(Wc, W - w0);
    const unsigned nblk = (unsigned)((wc + WB - 1) / WB);
    if (rec)
      hipLaunchKernelGGL(k_sq<true>, dim3(nblk), dim3(kSqThreads), lds, h->stream, h->S, A, x, sw, se, sc, w0, wc, d_out);
    else
      hipLaunchKernelGGL(k_sq<false>, dim3(nblk), dim3(kSqThreads), lds, h->stream, h->S, A, x, sw, se, sc, w0, wc, d_out);
    TRY(check_launch(h, "k_sq"));
    if (!mean) {
      TRY(copy_out(h, sq + (size_t)w0 * Q, d_out, (size_t)wc * Q * sizeof(double)));
      TRY(copy_out(h, spinsq + (size_t)w0 * Q, d_out + (size_t)wc * Q, (size_t)wc * Q * sizeof(double)));
      continue;
    }
    if (weights) {  // sum_w w_w v[z][w][q] of the chunk in the fixed order of k_wcol_means, the chunks one after the other
      TRY(wcol_means_dev<>(h, d_out, d_wts + w0, wc, Q, 2, (int)(w0 == 0), (int)(w0 + wc == W), 1.0, d_wsum, (double*)h->b_sqpart.p,
                         (double*)h->b_sqacc.p));
      continue;
    }
    const long rp = (wc + R - 1) / R;
    const int Rc = (int)((wc + rp - 1) / rp);  // slices this chunk fills
    hipLaunchKernelGGL(k_sq_rows, dim3((unsigned)((Q + 63) / 64), (unsigned)Rc, 2), dim3(64), 0, h->stream, (const double*)d_out, wc, Q,
                       rp, Rc, (double*)h->b_sqpart.p);
    TRY(check_launch(h, "k_sq_rows"));
    hipLaunchKernelGGL(k_sq_fold, dim3((unsigned)((2 * Q + 255) / 256)), dim3(256), 0, h->stream, (const double*)h->b_sqpart.p, Rc, Q,
                       (int)(w0 == 0), (int)(w0 + wc == W), (double)W, (double*)h->b_sqacc.p);
    TRY(check_launch(h, "k_sq_fold"));
  }
  if (!mean) return 0;
  TRY(copy_out(h, sq, h->b_sqacc.p, (size_t)Q * sizeof(double)));
  return copy_out(h, spinsq, (const double*)h->b_sqacc.p + Q, (size_t)Q * sizeof(double));
}

}  // namespace

extern "C" int pqa_sq(pqa_handle_t* h, int nqv, const double* q, const int* qn, const double* recip, int mean, double* sq, double* spinsq) {
  return sq_run(h, nqv, q, qn, recip, mean, nullptr, sq, spinsq, "pqa_sq");
}

extern "C" int pqa_sq_w(pqa_handle_t* h, int nqv, const double* q, const int* qn, const double* recip, const double* weights, double* sq,
                        double* spinsq) {
  if (!h) return -2;
  if (!weights) FAIL("pqa_sq_w: weights is NULL");
  return sq_run(h, nqv, q, qn, recip, 1, weights, sq, spinsq, "pqa_sq_w");
}
