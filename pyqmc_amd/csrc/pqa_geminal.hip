// AO-pair (geminal) Jastrow factor (GeminalJastrow, pyqmc/wf/geminaljastrow.py): a unit of its own with state of its own on the
// handle, reached through the protocol entry points pqa_geminal_*.  It reads the handle's basis tables through launch_ao
// (pqa_orb_pbc.hip, unchanged) and the electron count, and nothing else: its walkers, their count, AO values and sums are
// independent of h->W and of the Slater / Jastrow state, which it never reads or writes.
//
// With a_i = chi(r_i) (nao values), T = sum_i a_i (electrons in ascending order) and the symmetric G = triu(p) + triu(p)^T:
//   log Psi       = sum_{i>j} a_i^T G a_j = 1/2 (T^T G T - sum_i a_i^T G a_i)
//   h_e           = (T - a_e) G                                  one nao-vector per row (walker, electron)
//   ratio(e -> q) = exp(chi(q) . h_e - a_e . h_e)
//   grad log      = grad chi(q) . h_e,      lap Psi / Psi = lap chi(q) . h_e + |grad log|^2
//   d log / d p_mn = T_m T_n - sum_i a_im a_in                   m <= n, numpy.triu_indices order
//
// Layout: A [W][N][nao], T [W][nao], G [nao][nao] row-major; AO planes as launch_ao writes them, [ncomp][P][nao].
//
// Kernels.  k_gem_gemm forms H = B G on the matrix cores (v_mfma_f64_16x16x4_f64) for rows B[r] = T[w_r] - A[w_r][e_r] (or the plain
// rows {a_i}, T of the value), built while the operand is staged: a 256-thread block owns 64 rows x 64 columns, wave v the column
// tile v of all four 16-row tiles, and G passes through LDS in chunks of 32 rows (K), so any nao fits.  Row, column and K tails are
// zero-filled in LDS and every wave issues every MFMA.  k_gem_dots then takes one wave per row: lanes stride over nao to the next
// multiple of 64 with the tail lanes clamped to nao - 1 and their h set to zero, h is read once per group of eight AO rows (the
// points of a testvalue, the components of a gradient) and the dots are closed by wave_sum.  The update writes the electron's AO
// row and position and rebuilds T of the touched walkers by a fresh ascending sum: no running corrections, so a chain of moves
// agrees with a recompute of the moved walkers.
#include "pqa_internal.hpp"
#include "pqa_stage.hpp"

namespace {

constexpr int kGemThreads = 256, kGemWaves = kGemThreads / PQA_WAVE;
constexpr int kGemM = 64, kGemN = 64, kGemK = 32;  // block tile of H (rows x columns) and the K-chunk of G staged in LDS
// LDS row pitches (doubles): a wave reads B as [16 rows][4 k] and G as [4 k][16 columns], 8 bytes a lane; with 64 banks of 4 bytes a
// half-wave is conflict-free when its 32 addresses cover 32 distinct doubles mod 32: B rows 2 apart, G rows 16 apart (mod 32)
constexpr int kGemLdb = kGemK + 2, kGemLdg = kGemN + 16;
constexpr int kGemItems = 8;  // AO rows one pass of k_gem_dots contracts with a row's h

// How row r of a GEMM / dot launch finds its operand.  mode 0: electron e of walker widx[r] (or r); mode 1: electron es[r % ne] of
// walker widx[r / ne] (or r / ne); both B = T[w] - A[w][e].  mode 2 (value): B = A[r] for r < nA, B = T[r - nA] beyond
struct GemRows {
  const double* T;  // [W][nao]
  const double* A;  // [W * N][nao]
  const int* widx;
  const int* es;
  int ne, e, N, mode;
  long nA;
};
// rows of T and of A (flat, w * N + e) the operand is made of (-1: none), and the sign A enters with
__device__ __forceinline__ void gem_row(const GemRows& R, long r, long& tw, long& aw, double& sa) {
  if (R.mode == 2) {
    tw = r < R.nA ? -1 : r - R.nA;
    aw = r < R.nA ? r : -1;
    sa = 1.0;
    return;
  }
  const long rr = R.mode == 1 ? r / R.ne : r;
  const int e = R.mode == 1 ? R.es[r % R.ne] : R.e;
  tw = R.widx ? R.widx[rr] : rr;
  aw = tw * R.N + e;
  sa = -1.0;
}

// G[m][n] = p[idx(min, max)], diagonal doubled; idx(m, n) = m nao - m (m - 1) / 2 + n - m for m <= n (numpy.triu_indices order)
__device__ __forceinline__ long gem_pair(int m, int n, int nao) { return (long)m * nao - (long)m * (m - 1) / 2 + (n - m); }
__global__ __launch_bounds__(kGemThreads) void k_gem_sym(const double* __restrict__ p, int nao, double* __restrict__ G) {
  const long i = (long)blockIdx.x * kGemThreads + threadIdx.x;
  if (i >= (long)nao * nao) return;
  const int m = (int)(i / nao), n = (int)(i % nao);
  const double v = p[gem_pair(min(m, n), max(m, n), nao)];
  G[i] = m == n ? 2.0 * v : v;
}

// H[r][:] = B[r] G for r < nrow.  grid (ceil(nrow / 64), ceil(nao / 64))
__global__ __launch_bounds__(kGemThreads) void k_gem_gemm(GemRows R, const double* __restrict__ G, long nrow, int nao, double* __restrict__ H) {
  __shared__ double sB[kGemM * kGemLdb];
  __shared__ double sG[kGemK * kGemLdg];
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, i16 = lane & 15, kq = lane >> 4;
  const long r0 = (long)blockIdx.x * kGemM;
  const int c0 = blockIdx.y * kGemN;
  // staging roles.  B: column tid & 31 of the rows (tid >> 5) + 8 j; G: column tid & 63 of the rows (tid >> 6) + 4 j
  const int bk = tid & 31, brow = tid >> 5, gc = tid & 63, gk = tid >> 6;
  const double *pT[8], *pA[8];
  double sA[8];
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    const long r = r0 + brow + 8 * j;
    pT[j] = pA[j] = nullptr;
    sA[j] = 0.0;
    if (r < nrow) {
      long tw, aw;
      gem_row(R, r, tw, aw, sA[j]);
      if (tw >= 0) pT[j] = R.T + (size_t)tw * nao;
      if (aw >= 0) pA[j] = R.A + (size_t)aw * nao;
    }
  }
  d4 acc[4];
#pragma unroll
  for (int t = 0; t < 4; ++t) acc[t] = d4{0.0, 0.0, 0.0, 0.0};
  for (int k0 = 0; k0 < nao; k0 += kGemK) {
    const bool kin = k0 + bk < nao;
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      double v = 0.0;
      if (kin && pT[j]) v = pT[j][k0 + bk];
      if (kin && pA[j]) v += sA[j] * pA[j][k0 + bk];
      sB[(brow + 8 * j) * kGemLdb + bk] = v;
    }
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      const int k = k0 + gk + 4 * j;
      sG[(gk + 4 * j) * kGemLdg + gc] = (k < nao && c0 + gc < nao) ? G[(size_t)k * nao + c0 + gc] : 0.0;
    }
    __syncthreads();
#pragma unroll
    for (int kk = 0; kk < kGemK; kk += 4) {
      const double b = sG[(kk + kq) * kGemLdg + wave * 16 + i16];
#pragma unroll
      for (int t = 0; t < 4; ++t) acc[t] = __builtin_amdgcn_mfma_f64_16x16x4f64(sB[(t * 16 + i16) * kGemLdb + kk + kq], b, acc[t], 0, 0, 0);
    }
    __syncthreads();
  }
  // the lane holds D[row = kq + 4 q][column = i16] of each tile
  const int col = c0 + wave * 16 + i16;
#pragma unroll
  for (int t = 0; t < 4; ++t)
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const long r = r0 + t * 16 + kq + 4 * q;
      if (r < nrow && col < nao) H[(size_t)r * nao + col] = acc[t][q];
    }
}

// One wave per row r: the dots of h = H[r] with AO rows, and with a_e.  P: points of the AO planes.
//   mode 0: the npt value rows of the row's points (row r / ne of the planes under GemRows mode 1) -> out[r * npt + q] = ratio
//   mode 1: planes (value, gradient) -> out[c * nrow + r] = gradient c, out[3 nrow + r] = ratio
//   mode 2: planes (value, gradient, Laplacian), the value unused -> gradient, out[3 nrow + r] = lap . h + |gradient|^2
__global__ __launch_bounds__(kGemThreads) void k_gem_dots(GemRows R, const double* __restrict__ H, const double* __restrict__ ao, long nrow, long P,
                                                          int nao, int npt, int mode, double* __restrict__ out) {
  const int lane = threadIdx.x & 63;
  const long r = (long)blockIdx.x * kGemWaves + (threadIdx.x >> 6);
  if (r >= nrow) return;
  long tw, aw;
  double sa;
  gem_row(R, r, tw, aw, sa);
  const double* hr = H + (size_t)r * nao;
  const double* ae = R.A + (size_t)aw * nao;
  const long pr = R.mode == 1 ? r / R.ne : r;
  const int nitem = mode == 0 ? npt : 4;
  const double* base = mode == 0 ? ao + (size_t)pr * npt * nao : ao + (size_t)((mode == 2 ? P : 0) + r) * nao;
  const size_t stride = mode == 0 ? (size_t)nao : (size_t)P * nao;
  double old = 0.0, res[4] = {0.0, 0.0, 0.0, 0.0};
  for (int j0 = 0; j0 < nitem; j0 += kGemItems) {
    double acc[kGemItems], o = 0.0;
#pragma unroll
    for (int j = 0; j < kGemItems; ++j) acc[j] = 0.0;
    for (int k0 = 0; k0 < nao; k0 += 64) {
      const int k = k0 + lane, kc = min(k, nao - 1);
      const double hv = k < nao ? hr[kc] : 0.0;  // tail lanes: clamped loads, zero weight
#pragma unroll
      for (int j = 0; j < kGemItems; ++j)
        if (j0 + j < nitem) acc[j] += base[(size_t)(j0 + j) * stride + kc] * hv;
      if (j0 == 0 && mode != 2) o += ae[kc] * hv;
    }
    if (j0 == 0 && mode != 2) old = wave_sum(o);
#pragma unroll
    for (int j = 0; j < kGemItems; ++j)
      if (j0 + j < nitem) {
        const double s = wave_sum(acc[j]);
        if (mode == 0) {
          if (lane == 0) out[(size_t)r * npt + j0 + j] = exp(s - old);
        } else if (j < 4)
          res[j] = s;
      }
  }
  if (mode == 0 || lane != 0) return;
  if (mode == 1) {
    out[r] = res[1]; out[nrow + r] = res[2]; out[2 * nrow + r] = res[3];
    out[3 * nrow + r] = exp(res[0] - old);
  } else {
    out[r] = res[0]; out[nrow + r] = res[1]; out[2 * nrow + r] = res[2];
    out[3 * nrow + r] = res[3] + res[0] * res[0] + res[1] * res[1] + res[2] * res[2];
  }
}

// T[w][k] = sum_i A[w][i][k], ascending; one thread per (w, k)
__global__ __launch_bounds__(kGemThreads) void k_gem_tsum(const double* __restrict__ A, long W, int N, int nao, double* __restrict__ T) {
  const long i = (long)blockIdx.x * kGemThreads + threadIdx.x;
  if (i >= W * nao) return;
  const long w = i / nao;
  const int k = (int)(i % nao);
  const double* a = A + (size_t)w * N * nao + k;
  double s = 0.0;
  for (int e = 0; e < N; ++e) s += a[(size_t)e * nao];
  T[i] = s;
}

// log Psi of the walkers w0 .. w0 + Wc from H = [rows {a_i} of those walkers; their T] G: one wave per walker
__global__ __launch_bounds__(kGemThreads) void k_gem_value(const double* __restrict__ A, const double* __restrict__ T, const double* __restrict__ H,
                                                           long Wc, int N, int nao, double* __restrict__ out) {
  const int lane = threadIdx.x & 63;
  const long w = (long)blockIdx.x * kGemWaves + (threadIdx.x >> 6);
  if (w >= Wc) return;
  const double* Aw = A + (size_t)w * N * nao;
  const double* Ha = H + (size_t)w * N * nao;
  const double* Ht = H + ((size_t)Wc * N + w) * nao;
  double acc = 0.0;
  for (int k0 = 0; k0 < nao; k0 += 64) {
    const int k = k0 + lane, kc = min(k, nao - 1);
    double s = T[(size_t)w * nao + kc] * Ht[kc];
    for (int i = 0; i < N; ++i) s -= Aw[(size_t)i * nao + kc] * Ha[(size_t)i * nao + kc];
    if (k < nao) acc += s;
  }
  acc = wave_sum(acc);
  if (lane == 0) out[w] = 0.5 * acc;
}

// electron e of the masked walkers: its AO row from row[w] (the value plane of an evaluation at epos), its position, and T by a
// fresh sum over the electrons; one thread per (w, k)
__global__ __launch_bounds__(kGemThreads) void k_gem_update(double* __restrict__ A, double* __restrict__ T, double* __restrict__ x, int e,
                                                            const double* __restrict__ row, const double* __restrict__ epos,
                                                            const uint8_t* __restrict__ mask, long W, int N, int nao) {
  const long i = (long)blockIdx.x * kGemThreads + threadIdx.x;
  if (i >= W * nao) return;
  const long w = i / nao;
  const int k = (int)(i % nao);
  if (mask && !mask[w]) return;
  const double n = row[i];
  double* a = A + (size_t)w * N * nao + k;
  double s = 0.0;
  for (int j = 0; j < N; ++j) s += j == e ? n : a[(size_t)j * nao];
  a[(size_t)e * nao] = n;
  T[i] = s;
  if (k == 0) {
    double* xe = x + ((size_t)w * N + e) * 3;
    xe[0] = epos[3 * w]; xe[1] = epos[3 * w + 1]; xe[2] = epos[3 * w + 2];
  }
}

// d log Psi / d p_mn = T_m T_n - sum_i a_im a_in of the walkers w0 + blockIdx.z: a lane per column n, four rows m a block (their a_im
// are uniform over the block); grid (ceil(nao / 64), ceil(nao / 4), walkers), block 64.  out [walker][pair]
constexpr int kGemPgRows = 4;
__global__ __launch_bounds__(64) void k_gem_pgrad(const double* __restrict__ A, const double* __restrict__ T, int N, int nao, long npair,
                                                  double* __restrict__ out) {
  const int n = blockIdx.x * 64 + threadIdx.x, m0 = blockIdx.y * kGemPgRows;
  if (blockIdx.x * 64 + 63 < m0) return;  // the whole block lies below the diagonal
  const long w = blockIdx.z;
  const double* Aw = A + (size_t)w * N * nao;
  const double* Tw = T + (size_t)w * nao;
  const int nc = min(n, nao - 1);
  int mc[kGemPgRows];
  double acc[kGemPgRows];
#pragma unroll
  for (int j = 0; j < kGemPgRows; ++j) {
    mc[j] = min(m0 + j, nao - 1);
    acc[j] = Tw[mc[j]] * Tw[nc];
  }
  for (int i = 0; i < N; ++i) {
    const double an = Aw[(size_t)i * nao + nc];
#pragma unroll
    for (int j = 0; j < kGemPgRows; ++j) acc[j] -= Aw[(size_t)i * nao + mc[j]] * an;
  }
#pragma unroll
  for (int j = 0; j < kGemPgRows; ++j) {
    const int m = m0 + j;
    if (m < nao && n < nao && n >= m) out[(size_t)w * npair + gem_pair(m, n, nao)] = acc[j];
  }
}

inline dim3 gem_grid1(long n, int per) { return dim3((unsigned)((n + per - 1) / per)); }

int gem_ready(pqa_handle* h, const char* fn, bool state) {
  if (!h->gem_set) FAIL(std::string(fn) + ": coefficients not set (call pqa_geminal_set)");
  if (state && h->gem_W == 0) FAIL(std::string(fn) + ": geminal state not initialised (call pqa_geminal_recompute)");
  return 0;
}

inline GemRows gem_rows(const pqa_handle* h, int mode) {
  GemRows R{};
  R.T = (const double*)h->b_gem_t.p; R.A = (const double*)h->b_gem_a.p;
  R.N = h->N; R.mode = mode; R.ne = 1;
  return R;
}

int gem_gemm(pqa_handle* h, const GemRows& R, long nrow, double* H) {
  const dim3 grid((unsigned)((nrow + kGemM - 1) / kGemM), (unsigned)((h->nao + kGemN - 1) / kGemN));
  hipLaunchKernelGGL(k_gem_gemm, grid, dim3(kGemThreads), 0, h->stream, R, (const double*)h->b_gem_g.p, nrow, h->nao, H);
  return check_launch(h, "k_gem_gemm");
}

// log Psi of every walker, in walker chunks that keep the rows of H below 256 MiB
int gem_value(pqa_handle* h, double* logval) {
  const long W = h->gem_W, N = h->N, nao = h->nao;
  const long Wc = std::max<long>(1, std::min<long>(W, ((long)1 << 25) / ((N + 1) * nao)));
  TRY(ensure(h, h->b_gem_h, (size_t)Wc * (N + 1) * nao * sizeof(double)));
  TRY(ensure(h, h->b_out, (size_t)W * sizeof(double)));
  for (long w0 = 0; w0 < W; w0 += Wc) {
    const long n = std::min(Wc, W - w0);
    GemRows R = gem_rows(h, 2);
    R.A += (size_t)w0 * N * nao; R.T += (size_t)w0 * nao; R.nA = n * N;
    TRY(gem_gemm(h, R, n * (N + 1), (double*)h->b_gem_h.p));
    hipLaunchKernelGGL(k_gem_value, gem_grid1(n, kGemWaves), dim3(kGemThreads), 0, h->stream, R.A, R.T, (const double*)h->b_gem_h.p, n, (int)N,
                       (int)nao, (double*)h->b_out.p + w0);
    TRY(check_launch(h, "k_gem_value"));
  }
  return copy_out(h, logval, h->b_out.p, (size_t)W * sizeof(double));
}

}  // namespace

extern "C" int pqa_geminal_set(pqa_handle_t* h, const double* gcoeff, int64_t n) {
  HIPCHK(hipSetDevice(h->device));
  if (!h->has_slater || h->nao < 1) FAIL("pqa_geminal_set: the handle has no basis tables (create it with orbital coefficients)");
  if (h->twist || h->cplx) FAIL("pqa_geminal_set: not implemented for twisted or complex handles (real AOs only)");
  const int64_t want = (int64_t)h->nao * (h->nao + 1) / 2;
  if (n != want)
    FAIL("pqa_geminal_set: Wrong number of parameters: got " + std::to_string(n) + ", nao (nao + 1) / 2 = " + std::to_string(want) + " for nao = " +
         std::to_string(h->nao));
  if (!gcoeff) FAIL("pqa_geminal_set: gcoeff is NULL");
  const size_t nn = (size_t)h->nao * h->nao;
  TRY(ensure(h, h->b_pts, (size_t)n * sizeof(double)));
  TRY(ensure(h, h->b_gem_g, nn * sizeof(double)));
  TRY(copy_in(h, h->b_pts.p, gcoeff, (size_t)n * sizeof(double)));
  hipLaunchKernelGGL(k_gem_sym, gem_grid1((long)nn, kGemThreads), dim3(kGemThreads), 0, h->stream, (const double*)h->b_pts.p, h->nao,
                     (double*)h->b_gem_g.p);
  TRY(check_launch(h, "k_gem_sym"));
  HIPCHK(hipStreamSynchronize(h->stream));
  h->gem_set = true;
  return 0;
}

extern "C" int pqa_geminal_recompute(pqa_handle_t* h, const double* configs, int64_t W, double* logval) {
  HIPCHK(hipSetDevice(h->device));
  TRY(gem_ready(h, "pqa_geminal_recompute", false));
  if (W < 1 || !configs || !logval) FAIL("pqa_geminal_recompute: W >= 1 with configs (W, N, 3) and logval (W)");
  const size_t N = h->N, nao = h->nao;
  h->gem_W = 0;
  h->gem_saved_valid = false;
  TRY(ensure(h, h->b_gem_x, (size_t)W * N * 3 * sizeof(double)));
  TRY(ensure(h, h->b_gem_a, (size_t)W * N * nao * sizeof(double)));
  TRY(ensure(h, h->b_gem_t, (size_t)W * nao * sizeof(double)));
  TRY(copy_in(h, h->b_gem_x.p, configs, (size_t)W * N * 3 * sizeof(double)));
  const long P = (long)(W * N);
  TRY(launch_ao(h, plain_points((const double*)h->b_gem_x.p, P), P, 1, (double*)h->b_gem_a.p));  // one plane [P][nao] = A
  hipLaunchKernelGGL(k_gem_tsum, gem_grid1((long)(W * nao), kGemThreads), dim3(kGemThreads), 0, h->stream, (const double*)h->b_gem_a.p, (long)W,
                     (int)N, (int)nao, (double*)h->b_gem_t.p);
  TRY(check_launch(h, "k_gem_tsum"));
  h->gem_W = W;
  return gem_value(h, logval);
}

extern "C" int pqa_geminal_value(pqa_handle_t* h, double* logval) {
  HIPCHK(hipSetDevice(h->device));
  TRY(gem_ready(h, "pqa_geminal_value", true));
  if (!logval) FAIL("pqa_geminal_value: logval is NULL");
  return gem_value(h, logval);
}

extern "C" int pqa_geminal_eval(pqa_handle_t* h, int e, const double* pts, int64_t nrow, int npt, const int32_t* widx, int mode, int keep_saved,
                                double* out) {
  HIPCHK(hipSetDevice(h->device));
  TRY(gem_ready(h, "pqa_geminal_eval", true));
  StagedPoints in;
  TRY(stage_eval(h, "pqa_geminal_eval", h->gem_W, e, pts, nrow, npt, widx, mode, &in));
  if (!in.P) return 0;
  if (!out) FAIL("pqa_geminal_eval: out is NULL");
  h->gem_saved_valid = false;
  const size_t nao = h->nao, P = (size_t)in.P, nout = mode == 0 ? P : (size_t)4 * nrow;
  const int ncomp = mode == 0 ? 1 : mode == 1 ? 4 : 5;
  TRY(ensure(h, h->b_gem_ao, (size_t)ncomp * P * nao * sizeof(double)));
  TRY(ensure(h, h->b_gem_h, (size_t)nrow * nao * sizeof(double)));
  TRY(ensure(h, h->b_out, nout * sizeof(double)));
  TRY(launch_ao(h, plain_points(in.pts, (long)P), (long)P, ncomp, (double*)h->b_gem_ao.p));
  GemRows R = gem_rows(h, 0);
  R.e = e; R.widx = in.widx;
  TRY(gem_gemm(h, R, nrow, (double*)h->b_gem_h.p));
  hipLaunchKernelGGL(k_gem_dots, gem_grid1(nrow, kGemWaves), dim3(kGemThreads), 0, h->stream, R, (const double*)h->b_gem_h.p,
                     (const double*)h->b_gem_ao.p, (long)nrow, (long)P, (int)nao, npt, mode, (double*)h->b_out.p);
  TRY(check_launch(h, "k_gem_dots"));
  if (keep_saved && mode == 1 && !widx) {  // the value plane, one row per walker
    TRY(ensure(h, h->b_gem_saved, (size_t)nrow * nao * sizeof(double)));
    TRY(copy_in(h, h->b_gem_saved.p, h->b_gem_ao.p, (size_t)nrow * nao * sizeof(double)));
    h->gem_saved_valid = true;
    h->gem_saved_e = e;
  }
  return copy_out(h, out, h->b_out.p, nout * sizeof(double));
}

extern "C" int pqa_geminal_testvalue_many(pqa_handle_t* h, const int32_t* es, int ne, const double* pts, int64_t nrow, const int32_t* widx,
                                          double* out) {
  HIPCHK(hipSetDevice(h->device));
  TRY(gem_ready(h, "pqa_geminal_testvalue_many", true));
  if (nrow <= 0 || ne <= 0) return 0;
  if (!out) FAIL("pqa_geminal_testvalue_many: out is NULL");
  const int* des;
  StagedPoints in;
  TRY(stage_electrons(h, "pqa_geminal_testvalue_many", es, ne, &des));
  TRY(stage_points(h, "pqa_geminal_testvalue_many", h->gem_W, pts, nrow, 1, widx, &in));
  h->gem_saved_valid = false;
  const size_t nao = h->nao, rows = (size_t)nrow * ne;
  TRY(ensure(h, h->b_gem_ao, (size_t)nrow * nao * sizeof(double)));
  TRY(ensure(h, h->b_gem_h, rows * nao * sizeof(double)));
  TRY(ensure(h, h->b_out, rows * sizeof(double)));
  TRY(launch_ao(h, plain_points(in.pts, (long)nrow), (long)nrow, 1, (double*)h->b_gem_ao.p));
  GemRows R = gem_rows(h, 1);
  R.es = des; R.ne = ne; R.widx = in.widx;
  TRY(gem_gemm(h, R, (long)rows, (double*)h->b_gem_h.p));
  hipLaunchKernelGGL(k_gem_dots, gem_grid1((long)rows, kGemWaves), dim3(kGemThreads), 0, h->stream, R, (const double*)h->b_gem_h.p,
                     (const double*)h->b_gem_ao.p, (long)rows, (long)nrow, (int)nao, 1, 0, (double*)h->b_out.p);
  TRY(check_launch(h, "k_gem_dots"));
  return copy_out(h, out, h->b_out.p, rows * sizeof(double));
}

extern "C" int pqa_geminal_update(pqa_handle_t* h, int e, const double* epos, const uint8_t* mask, int use_saved) {
  HIPCHK(hipSetDevice(h->device));
  TRY(gem_ready(h, "pqa_geminal_update", true));
  const long W = h->gem_W;
  const size_t nao = h->nao;
  const double* dx;
  const uint8_t* dm;
  TRY(stage_move(h, "pqa_geminal_update", W, e, epos, mask, &dx, &dm));
  const double* row = (const double*)h->b_gem_saved.p;
  if (!(use_saved && h->gem_saved_valid && h->gem_saved_e == e)) {
    // value and gradient planes, as the mode-1 evaluation whose value plane the other route keeps: the same instantiation of the
    // AO kernel on the same points, so both routes write bitwise the same row
    TRY(ensure(h, h->b_gem_ao, (size_t)4 * W * nao * sizeof(double)));
    TRY(launch_ao(h, plain_points(dx, W), W, 4, (double*)h->b_gem_ao.p));
    row = (const double*)h->b_gem_ao.p;
  }
  h->gem_saved_valid = false;
  hipLaunchKernelGGL(k_gem_update, gem_grid1(W * (long)nao, kGemThreads), dim3(kGemThreads), 0, h->stream, (double*)h->b_gem_a.p,
                     (double*)h->b_gem_t.p, (double*)h->b_gem_x.p, e, row, dx, dm, W, h->N, (int)nao);
  TRY(check_launch(h, "k_gem_update"));
  HIPCHK(hipStreamSynchronize(h->stream));
  return 0;
}

extern "C" int pqa_geminal_pgradient(pqa_handle_t* h, double* d_gcoeff) {
  HIPCHK(hipSetDevice(h->device));
  TRY(gem_ready(h, "pqa_geminal_pgradient", true));
  if (!d_gcoeff) FAIL("pqa_geminal_pgradient: d_gcoeff is NULL");
  const long W = h->gem_W, N = h->N, nao = h->nao, npair = nao * (nao + 1) / 2;
  // walker chunks: at most 256 MiB of derivatives on the device, and a grid z extent below 65536
  const long Wc = std::max<long>(1, std::min<long>(std::min<long>(W, 65535), ((long)1 << 25) / npair));
  TRY(ensure(h, h->b_out, (size_t)Wc * npair * sizeof(double)));
  for (long w0 = 0; w0 < W; w0 += Wc) {
    const long n = std::min(Wc, W - w0);
    const dim3 grid((unsigned)((nao + 63) / 64), (unsigned)((nao + kGemPgRows - 1) / kGemPgRows), (unsigned)n);
    hipLaunchKernelGGL(k_gem_pgrad, grid, dim3(64), 0, h->stream, (const double*)h->b_gem_a.p + (size_t)w0 * N * nao,
                       (const double*)h->b_gem_t.p + (size_t)w0 * nao, (int)N, (int)nao, npair, (double*)h->b_out.p);
    TRY(check_launch(h, "k_gem_pgrad"));
    TRY(copy_out(h, d_gcoeff + (size_t)w0 * npair, h->b_out.p, (size_t)n * npair * sizeof(double)));
  }
  return 0;
}

extern "C" int pqa_geminal_get_state(pqa_handle_t* h, double* ao_val, double* configs) {
  HIPCHK(hipSetDevice(h->device));
  TRY(gem_ready(h, "pqa_geminal_get_state", true));
  const size_t W = h->gem_W, N = h->N, nao = h->nao;
  HIPCHK(hipStreamSynchronize(h->stream));
  if (ao_val) HIPCHK(hipMemcpy(ao_val, h->b_gem_a.p, W * N * nao * sizeof(double), hipMemcpyDeviceToHost));
  if (configs) HIPCHK(hipMemcpy(configs, h->b_gem_x.p, W * N * 3 * sizeof(double), hipMemcpyDeviceToHost));
  return 0;
}
