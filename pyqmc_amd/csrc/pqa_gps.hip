// Gaussian-process Jastrow factor (GPSJastrow, pyqmc/wf/gps2.py): a unit of its own with state of its own on the handle, reached
// through the protocol entry points pqa_gps_*.  It reads the handle's cell (SysDev::pbc / pb) and electron count and nothing else:
// its walkers, their count and its sums are independent of h->W and of the Slater / Jastrow state, which it never reads or writes.
//
// With support pairs X[s][t] (t = 0, 1), weights alpha[s] and the width f, the state of a walker is
//   e[i][s][t] = exp(-f |r_i - X[s][t]|^2)          and          S[s][t] = sum_i e[i][s][t]   (electrons in ascending order),
// and with o_t = e[e][s][t], n_t = exp(-f |q - X[s][t]|^2), d_t = X[s][t] - q (minimal image in a periodic cell):
//   log Psi       = sum_s alpha_s sum_i e[i][s][0] (S[s][1] - e[i][s][1])
//   ratio(e -> q) = exp(sum_s alpha_s [(n_0 - o_0)(S[s][1] - o_1) + (n_1 - o_1)(S[s][0] - o_0)])
//   grad log      = 2 f sum_s alpha_s sum_t n_t d_t (S[s][1-t] - o_{1-t})
//   lap Psi / Psi = sum_s alpha_s sum_t n_t (4 f^2 |d_t|^2 - 6 f)(S[s][1-t] - o_{1-t}) + |grad log|^2.
//
// Layout: the item k = 2 s + t is the fastest index, e [W][N][K] and S [W][K] with K = 2 nsup, so that the lanes of a wave, which
// stride over the items, read and write consecutive doubles, and an item's partner k ^ 1 sits in the same 16 bytes.  One wave per
// walker (row), four rows per 256-thread block; the waves of a block share nothing (no LDS, no barrier).  The item loops run to
// the next multiple of 64 with the tail lanes clamped to item K - 1 and masked out of every store and sum, so that min_image's wave
// vote and wave_sum see all 64 lanes.  No cap on nsup: a lane takes the items k, k + 64, ...
//
// Minimal image: min_image (pqa_common.hpp), the full Wigner-Seitz reduction.  The two-body Jastrow's min_image_j skips the
// reduction in cells where every Jastrow cut-off is below the inradius (PbcDev::jas_fold, which a handle without a Jastrow factor
// sets); a Gaussian has no cut-off, so that shortcut does not apply here.  min_image folds the fractional displacement by
// floor(. + 1/2) first and so takes arguments any distance outside the cell: support points need no folding on the host.  The
// displacement is formed as electron - support, as the reference forms it, and negated where the formulas want X - q.
//
// The masked update writes the electron's column and position and rebuilds S of the touched walkers by a fresh ascending sum: no
// running corrections, so a chain of moves agrees with a recompute of the moved walkers.
#include "pqa_internal.hpp"
#include "pqa_stage.hpp"

namespace {

constexpr int kGpsThreads = 256, kGpsRows = kGpsThreads / PQA_WAVE;

struct GpsDev {
  int N, K;             // electrons; items (2 nsup)
  double f;
  const double* X;      // [K][3]
  const double* alpha;  // [nsup]
  double* x;            // [W][N][3]
  double* E;            // [W][N][K]
  double* S;            // [W][K]
};

// exp(-f |d|^2) of the minimal image d of (px, py, pz) - X[k]
__device__ __forceinline__ double gps_gauss(const SysDev& S, const GpsDev& G, int k, double px, double py, double pz, double (&d)[3],
                                            double& r2) {
  double dx = px - G.X[3 * k], dy = py - G.X[3 * k + 1], dz = pz - G.X[3 * k + 2];
  min_image(S, dx, dy, dz);
  d[0] = dx; d[1] = dy; d[2] = dz;
  r2 = dx * dx + dy * dy + dz * dz;
  return exp(-G.f * r2);
}

// e and S of every walker from its coordinates
__global__ __launch_bounds__(kGpsThreads) void k_gps_fill(SysDev S, GpsDev G, long W) {
  const int lane = threadIdx.x & 63, K = G.K;
  const long w = (long)blockIdx.x * kGpsRows + (threadIdx.x >> 6);
  if (w >= W) return;
  const double* xw = G.x + (size_t)w * G.N * 3;
  double* Ew = G.E + (size_t)w * G.N * K;
  for (int k0 = 0; k0 < K; k0 += 64) {
    const int k = k0 + lane, kc = min(k, K - 1);
    const bool in = k < K;
    double s = 0.0;
    for (int i = 0; i < G.N; ++i) {
      double d[3], r2;
      const double v = gps_gauss(S, G, kc, xw[3 * i], xw[3 * i + 1], xw[3 * i + 2], d, r2);
      if (in) Ew[(size_t)i * K + k] = v;
      s += v;
    }
    if (in) G.S[(size_t)w * K + k] = s;
  }
}

// log Psi of every walker from e and S
__global__ __launch_bounds__(kGpsThreads) void k_gps_value(GpsDev G, long W, double* __restrict__ out) {
  const int lane = threadIdx.x & 63, K = G.K;
  const long w = (long)blockIdx.x * kGpsRows + (threadIdx.x >> 6);
  if (w >= W) return;
  const double* Ew = G.E + (size_t)w * G.N * K;
  const double* Sw = G.S + (size_t)w * K;
  double acc = 0.0;
  for (int k0 = 0; k0 < K; k0 += 64) {
    const int k = k0 + lane, kc = min(k, K - 1);
    const double sp = Sw[kc ^ 1];
    double a = 0.0;
    for (int i = 0; i < G.N; ++i) a += Ew[(size_t)i * K + kc] * (sp - Ew[(size_t)i * K + (kc ^ 1)]);
    if (k < K && !(k & 1)) acc += G.alpha[k >> 1] * a;  // the items t = 0 carry the sum
  }
  acc = wave_sum(acc);
  if (lane == 0) out[w] = acc;
}

// electron e of the walkers widx[r] (or r) at npt points per row; modes as pqa_jastrow_eval
__global__ __launch_bounds__(kGpsThreads) void k_gps_eval(SysDev S, GpsDev G, int e, const double* __restrict__ pts, long nrow, int npt,
                                                          const int* __restrict__ widx, int mode, double* __restrict__ out) {
  const int lane = threadIdx.x & 63, K = G.K;
  const long r = (long)blockIdx.x * kGpsRows + (threadIdx.x >> 6);
  if (r >= nrow) return;
  const long w = widx ? widx[r] : r;
  const double* Ee = G.E + ((size_t)w * G.N + e) * K;
  const double* Sw = G.S + (size_t)w * K;
  const double f = G.f;
  for (int q = 0; q < npt; ++q) {
    const double* p = pts + (size_t)(r * npt + q) * 3;
    const double px = p[0], py = p[1], pz = p[2];
    double av = 0.0, gx = 0.0, gy = 0.0, gz = 0.0, al = 0.0;
    for (int k0 = 0; k0 < K; k0 += 64) {
      const int k = k0 + lane, kc = min(k, K - 1);
      const double ac = k < K ? G.alpha[kc >> 1] * (Sw[kc ^ 1] - Ee[kc ^ 1]) : 0.0;  // alpha_s (S[s][1-t] - o_{1-t})
      double d[3], r2;
      const double n = gps_gauss(S, G, kc, px, py, pz, d, r2);
      av += ac * (n - Ee[kc]);
      if (mode) {
        const double an = ac * n;
        gx -= an * d[0]; gy -= an * d[1]; gz -= an * d[2];  // d = q - X
        al += an * (4.0 * f * f * r2 - 6.0 * f);
      }
    }
    if (mode == 0) {
      av = wave_sum(av);
      if (lane == 0) out[r * npt + q] = exp(av);
      continue;
    }
    gx = 2.0 * f * wave_sum(gx); gy = 2.0 * f * wave_sum(gy); gz = 2.0 * f * wave_sum(gz);
    const double last = mode == 1 ? exp(wave_sum(av)) : wave_sum(al) + gx * gx + gy * gy + gz * gz;
    if (lane == 0) { out[r] = gx; out[nrow + r] = gy; out[2 * nrow + r] = gz; out[3 * nrow + r] = last; }
  }
}

// electron e of the masked walkers to epos [W][3]: its column of e, its position, and S by a fresh sum over the electrons
__global__ __launch_bounds__(kGpsThreads) void k_gps_update(SysDev S, GpsDev G, int e, const double* __restrict__ epos,
                                                            const uint8_t* __restrict__ mask, long W) {
  const int lane = threadIdx.x & 63, K = G.K;
  const long w = (long)blockIdx.x * kGpsRows + (threadIdx.x >> 6);
  if (w >= W || (mask && !mask[w])) return;
  const double px = epos[3 * w], py = epos[3 * w + 1], pz = epos[3 * w + 2];
  double* Ew = G.E + (size_t)w * G.N * K;
  for (int k0 = 0; k0 < K; k0 += 64) {
    const int k = k0 + lane, kc = min(k, K - 1);
    const bool in = k < K;
    double d[3], r2;
    const double n = gps_gauss(S, G, kc, px, py, pz, d, r2);
    double s = 0.0;
    for (int i = 0; i < G.N; ++i) s += i == e ? n : Ew[(size_t)i * K + kc];
    if (in) { Ew[(size_t)e * K + k] = n; G.S[(size_t)w * K + k] = s; }
  }
  if (lane == 0) {
    double* xe = G.x + ((size_t)w * G.N + e) * 3;
    xe[0] = px; xe[1] = py; xe[2] = pz;
  }
}

// parameter derivatives of log Psi (gps2.py:139-173), with c_k(i) = e[i][k] (S[k^1] - e[i][k^1]) and d = r_i - X[k] at the CURRENT
// support points:  d_alpha[s] = sum_i c_{2s}(i),  d_X[k] = 2 f alpha_s sum_i d c_k(i),  d_f = -sum_k alpha_s sum_i |d|^2 c_k(i)
__global__ __launch_bounds__(kGpsThreads) void k_gps_pgrad(SysDev S, GpsDev G, long W, double* __restrict__ d_alpha, double* __restrict__ d_X,
                                                           double* __restrict__ d_f) {
  const int lane = threadIdx.x & 63, K = G.K;
  const long w = (long)blockIdx.x * kGpsRows + (threadIdx.x >> 6);
  if (w >= W) return;
  const double* xw = G.x + (size_t)w * G.N * 3;
  const double* Ew = G.E + (size_t)w * G.N * K;
  const double* Sw = G.S + (size_t)w * K;
  double fa = 0.0;
  for (int k0 = 0; k0 < K; k0 += 64) {
    const int k = k0 + lane, kc = min(k, K - 1);
    const double a = G.alpha[kc >> 1], sp = Sw[kc ^ 1];
    double sa = 0.0, sx = 0.0, sy = 0.0, sz = 0.0, sr = 0.0;
    for (int i = 0; i < G.N; ++i) {
      const double c = Ew[(size_t)i * K + kc] * (sp - Ew[(size_t)i * K + (kc ^ 1)]);
      double d[3], r2;
      gps_gauss(S, G, kc, xw[3 * i], xw[3 * i + 1], xw[3 * i + 2], d, r2);
      sa += c; sx += d[0] * c; sy += d[1] * c; sz += d[2] * c; sr += r2 * c;
    }
    if (k < K) {
      if (!(k & 1)) d_alpha[(size_t)w * (K >> 1) + (k >> 1)] = sa;
      double* o = d_X + ((size_t)w * K + k) * 3;
      const double c2 = 2.0 * G.f * a;
      o[0] = c2 * sx; o[1] = c2 * sy; o[2] = c2 * sz;
      fa -= a * sr;
    }
  }
  fa = wave_sum(fa);
  if (lane == 0) d_f[w] = fa;
}

inline dim3 gps_grid(long rows) { return dim3((unsigned)((rows + kGpsRows - 1) / kGpsRows)); }

inline GpsDev gps_dev(const pqa_handle* h) {
  GpsDev G{};
  G.N = h->N; G.K = 2 * h->gps_nsup; G.f = h->gps_f;
  G.X = (const double*)h->b_gps_par.p; G.alpha = G.X + 3 * G.K;
  G.x = (double*)h->b_gps_x.p; G.E = (double*)h->b_gps_e.p; G.S = (double*)h->b_gps_s.p;
  return G;
}

int gps_ready(pqa_handle* h, const char* fn, bool state) {
  if (h->gps_nsup == 0) FAIL(std::string(fn) + ": support points not set (call pqa_gps_set)");
  if (state && h->gps_W == 0) FAIL(std::string(fn) + ": GPS state not initialised (call pqa_gps_recompute)");
  return 0;
}

int gps_value(pqa_handle* h, double* logval) {
  const long W = h->gps_W;
  TRY(ensure(h, h->b_out, (size_t)W * sizeof(double)));
  hipLaunchKernelGGL(k_gps_value, gps_grid(W), dim3(kGpsThreads), 0, h->stream, gps_dev(h), W, (double*)h->b_out.p);
  TRY(check_launch(h, "k_gps_value"));
  return copy_out(h, logval, h->b_out.p, (size_t)W * sizeof(double));
}

}  // namespace

extern "C" int pqa_gps_set(pqa_handle_t* h, int nsup, const double* xsupport, const double* alpha, double f) {
  HIPCHK(hipSetDevice(h->device));
  if (nsup < 1 || !xsupport || !alpha) FAIL("pqa_gps_set: nsup >= 1 with xsupport (nsup, 2, 3) and alpha (nsup)");
  if (nsup > (1 << 24)) FAIL("pqa_gps_set: more than 2^24 support pairs");
  if (nsup != h->gps_nsup) h->gps_W = 0;  // e and S are laid out by the support count: recompute
  TRY(ensure(h, h->b_gps_par, (size_t)7 * nsup * sizeof(double)));
  double* par = (double*)h->b_gps_par.p;
  TRY(copy_in(h, par, xsupport, (size_t)6 * nsup * sizeof(double)));
  TRY(copy_in(h, par + 6 * nsup, alpha, (size_t)nsup * sizeof(double)));
  HIPCHK(hipStreamSynchronize(h->stream));
  h->gps_nsup = nsup;
  h->gps_f = f;
  return 0;
}

extern "C" int pqa_gps_recompute(pqa_handle_t* h, const double* configs, int64_t W, double* logval) {
  HIPCHK(hipSetDevice(h->device));
  TRY(gps_ready(h, "pqa_gps_recompute", false));
  if (W < 1 || !configs || !logval) FAIL("pqa_gps_recompute: W >= 1 with configs (W, N, 3) and logval (W)");
  const size_t N = h->N, K = 2 * (size_t)h->gps_nsup;
  h->gps_W = 0;
  TRY(ensure(h, h->b_gps_x, (size_t)W * N * 3 * sizeof(double)));
  TRY(ensure(h, h->b_gps_e, (size_t)W * N * K * sizeof(double)));
  TRY(ensure(h, h->b_gps_s, (size_t)W * K * sizeof(double)));
  TRY(copy_in(h, h->b_gps_x.p, configs, (size_t)W * N * 3 * sizeof(double)));
  hipLaunchKernelGGL(k_gps_fill, gps_grid(W), dim3(kGpsThreads), 0, h->stream, h->S, gps_dev(h), (long)W);
  TRY(check_launch(h, "k_gps_fill"));
  h->gps_W = W;
  return gps_value(h, logval);
}

extern "C" int pqa_gps_value(pqa_handle_t* h, double* logval) {
  HIPCHK(hipSetDevice(h->device));
  TRY(gps_ready(h, "pqa_gps_value", true));
  if (!logval) FAIL("pqa_gps_value: logval is NULL");
  return gps_value(h, logval);
}

extern "C" int pqa_gps_eval(pqa_handle_t* h, int e, const double* pts, int64_t nrow, int npt, const int32_t* widx, int mode, double* out) {
  HIPCHK(hipSetDevice(h->device));
  TRY(gps_ready(h, "pqa_gps_eval", true));
  StagedPoints in;
  TRY(stage_eval(h, "pqa_gps_eval", h->gps_W, e, pts, nrow, npt, widx, mode, &in));
  if (!in.P) return 0;
  if (!out) FAIL("pqa_gps_eval: out is NULL");
  const size_t nout = mode == 0 ? (size_t)in.P : (size_t)4 * nrow;
  TRY(ensure(h, h->b_out, nout * sizeof(double)));
  hipLaunchKernelGGL(k_gps_eval, gps_grid(nrow), dim3(kGpsThreads), 0, h->stream, h->S, gps_dev(h), e, in.pts, (long)nrow, npt, in.widx, mode,
                     (double*)h->b_out.p);
  TRY(check_launch(h, "k_gps_eval"));
  return copy_out(h, out, h->b_out.p, nout * sizeof(double));
}

extern "C" int pqa_gps_update(pqa_handle_t* h, int e, const double* epos, const uint8_t* mask) {
  HIPCHK(hipSetDevice(h->device));
  TRY(gps_ready(h, "pqa_gps_update", true));
  const long W = h->gps_W;
  const double* dx;
  const uint8_t* dm;
  TRY(stage_move(h, "pqa_gps_update", W, e, epos, mask, &dx, &dm));
  hipLaunchKernelGGL(k_gps_update, gps_grid(W), dim3(kGpsThreads), 0, h->stream, h->S, gps_dev(h), e, dx, dm, W);
  TRY(check_launch(h, "k_gps_update"));
  HIPCHK(hipStreamSynchronize(h->stream));
  return 0;
}

extern "C" int pqa_gps_pgradient(pqa_handle_t* h, double* d_alpha, double* d_xsupport, double* d_f) {
  HIPCHK(hipSetDevice(h->device));
  TRY(gps_ready(h, "pqa_gps_pgradient", true));
  if (!d_alpha || !d_xsupport || !d_f) FAIL("pqa_gps_pgradient: d_alpha / d_xsupport / d_f is NULL");
  const size_t W = h->gps_W, ns = h->gps_nsup;
  TRY(ensure(h, h->b_out, W * (7 * ns + 1) * sizeof(double)));
  double* da = (double*)h->b_out.p;
  double *dx = da + W * ns, *df = dx + W * 6 * ns;
  hipLaunchKernelGGL(k_gps_pgrad, gps_grid((long)W), dim3(kGpsThreads), 0, h->stream, h->S, gps_dev(h), (long)W, da, dx, df);
  TRY(check_launch(h, "k_gps_pgrad"));
  TRY(copy_in(h, d_alpha, da, W * ns * sizeof(double)));
  TRY(copy_in(h, d_xsupport, dx, W * 6 * ns * sizeof(double)));
  return copy_out(h, d_f, df, W * sizeof(double));
}

extern "C" int pqa_gps_get_state(pqa_handle_t* h, double* e_cs, double* configs) {
  HIPCHK(hipSetDevice(h->device));
  TRY(gps_ready(h, "pqa_gps_get_state", true));
  const size_t W = h->gps_W, N = h->N, ns = h->gps_nsup;
  HIPCHK(hipStreamSynchronize(h->stream));
  if (e_cs) {  // [W][N][nsup][2] on the device -> the reference's (W, nsup, N, 2)
    std::vector<double> E(W * N * ns * 2);
    HIPCHK(hipMemcpy(E.data(), h->b_gps_e.p, E.size() * sizeof(double), hipMemcpyDeviceToHost));
    for (size_t w = 0; w < W; ++w)
      for (size_t i = 0; i < N; ++i)
        for (size_t s = 0; s < ns; ++s)
          for (size_t t = 0; t < 2; ++t) e_cs[((w * ns + s) * N + i) * 2 + t] = E[((w * N + i) * ns + s) * 2 + t];
  }
  if (configs) HIPCHK(hipMemcpy(configs, h->b_gps_x.p, W * N * 3 * sizeof(double), hipMemcpyDeviceToHost));
  return 0;
}
