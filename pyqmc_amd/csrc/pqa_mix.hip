// Estimators over the mixture sum_k |Psi_k|^2 of K resident wave functions, after pqa_overlap_sweeps has moved their walkers:
// StochasticReconfigurationMultipleWF.avg (stochastic_reconfiguration.py:195-227), EnergyAccumulatorMultipleWF.avg
// (accumulators_multiwf.py:29-60) and StochasticReconfigurationWfbyWf.avg (ensemble_optimization_wfbywf.py:57-66), without the walkers,
// the per-walker energies or the (W, P) derivative arrays crossing the bus.
//
// The weights of compute_weights (sample_many.py:42-55) have rank one per walker: with a_k = phase_k exp(log|Psi_k| - ref) and
// rho = mean_k a_k^2, weights[i][j][c] = a_i (a_j / rho).  Every sum of the estimator of state i is therefore a block of ONE product
//   M_i = A_i^T diag(s) A_i[:, :P_i],   A_i = [a_i dp(i) | a_0 .. a_{K-1} | E_0 a_0 .. E_{K-1} a_{K-1}]  (W, P_i + 2K),   s = 1 / (rho W):
//   rows 0 .. P_i-1        dpipj  = sum_c dp_p dp_q weights[i][i][c] / W
//   rows P_i .. P_i+K-1    dp[:, j]  = sum_c dp_p weights[i][j][c] / W
//   rows P_i+K ..          dpH[:, j] = sum_c E_j dp_p weights[i][j][c] / W      (E_j: state j's total energy, no offset)
// the shape pqa_sr's product has with 2K further rows instead of 2, so it runs on pqa_srk.hpp's k_sr_syrk / k_sr_reduce.
//   energy_dev       per handle, with its own key or draws: the rows pqa_energy gives (b_en of each handle);
//   sr_check_columns, sr_sources  per handle, the derivative arrays its columns name (sources 0 - 2; pqa_srk.hpp);
//   values_dev       per handle: sign, log of the Slater factor and the Jastrow exponent;
//   k_ovl_weights    weights (K, K, W), k_ovl_mean their walker means (pqa_multi.hpp: the kernels of pqa_overlap_sweeps);
//   k_mix_scale      a (K, W), s (W), and u = a / sqrt(rho) for a caller that asks for it;
//   k_mix_en         en[r][i][j] = sum_c (E_j^r - offset) weights[i][j][c] / W: one block per entry, a fixed-order tree;
//   k_mix_gather     per state and walker chunk of at most 256 MiB: the compact row-major A_i;
//   k_sr_syrk, k_sr_reduce  the product and the slices' sum in slice order, the symmetric block mirrored from its upper triangle.
// pqa_mix_wtdp is the thin product for the derivatives of the last state: A = [dp | weights[j][k], j <= k] (W, P + K (K + 1) / 2),
// s = 1 / W, only the rows below the symmetric block formed; (j, k) and (k, j) are one row.
#include "pqa_srk.hpp"
#include "pqa_multi.hpp"

namespace {

struct MixEn {
  const double* en[kMaxK];  // b_en (6, W) of every handle
};

// a[k][w] = psi_k, s[w] = (1 / rho) / W, u[k][w] = psi_k / sqrt(rho) (u == nullptr: not written)
__global__ __launch_bounds__(256) void k_mix_scale(OvlPtrs P, int K, long W, double* __restrict__ a, double* __restrict__ s,
                                                   double* __restrict__ u) {
  const long w = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (w >= W) return;
  double psi[kMaxK];
  const double rho = ovl_psi_rho(P, K, w, psi);
  for (int k = 0; k < K; ++k) a[(size_t)k * W + w] = psi[k];
  s[w] = (1.0 / rho) / (double)W;
  if (u) {
    const double q = sqrt(rho);
    for (int k = 0; k < K; ++k) u[(size_t)k * W + w] = psi[k] / q;
  }
}

// s[w] = 1 / W
__global__ __launch_bounds__(256) void k_mix_fill(long W, double* __restrict__ s) {
  const long w = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (w < W) s[w] = 1.0 / (double)W;
}

// out[(r K + i) K + j] = sum_w (E_j^r(w) - offset) wts[i][j][w] / W: one block per entry, a fixed-order tree
__global__ __launch_bounds__(256) void k_mix_en(MixEn E, const double* __restrict__ wts, int K, long W, double offset, double* __restrict__ out) {
  __shared__ double part[256];
  const int b = blockIdx.x, j = b % K, i = (b / K) % K, r = b / (K * K);
  const double* row = E.en[j] + (size_t)r * W;
  const double* wr = wts + ((size_t)i * K + j) * W;
  double acc = 0.0;
  for (long w = threadIdx.x; w < W; w += 256) acc += (row[w] - offset) * wr[w];
  acc = block_sum256(acc, part);
  if (threadIdx.x == 0) out[b] = acc / (double)W;
}

// One thread per (walker of the chunk, column of A_i): a_i dp (columns < P), a_j (P + j), E_j a_j (P + K + j)
__global__ __launch_bounds__(256) void k_mix_gather(SrSources S, const int* __restrict__ src, const int* __restrict__ pos, int P, int K, int state,
                                                    MixEn E, const double* __restrict__ a /*[K][W]*/, long W, long w0, long Wc,
                                                    double* __restrict__ A /*[Wc][P + 2K]*/) {
  const int lda = P + 2 * K;
  const long idx = (long)blockIdx.x * 256 + threadIdx.x;
  if (idx >= Wc * lda) return;
  const long bw = idx / lda, w = w0 + bw;
  const int i = (int)(idx - bw * lda);
  double v;
  if (i < P) {
    const int s = src[i];
    v = a[(size_t)state * W + w] * S.base[s][(size_t)w * S.stride[s] + pos[i]];
  } else if (i < P + K)
    v = a[(size_t)(i - P) * W + w];
  else
    v = E.en[i - P - K][5 * W + w] * a[(size_t)(i - P - K) * W + w];
  A[idx] = v;
}

// One thread per (walker of the chunk, column): dp (columns < P), weights[j][k] of pair q = i - P (pj[q] <= pk[q])
__global__ __launch_bounds__(256) void k_mix_gather_wt(SrSources S, const int* __restrict__ src, const int* __restrict__ pos, int P, int K, int npair,
                                                       const double* __restrict__ wts /*[K][K][W]*/, long W, long w0, long Wc,
                                                       double* __restrict__ A /*[Wc][P + npair]*/) {
  const int lda = P + npair;
  const long idx = (long)blockIdx.x * 256 + threadIdx.x;
  if (idx >= Wc * lda) return;
  const long bw = idx / lda, w = w0 + bw;
  const int i = (int)(idx - bw * lda);
  double v;
  if (i < P) {
    const int s = src[i];
    v = S.base[s][(size_t)w * S.stride[s] + pos[i]];
  } else {
    // pair q of the upper triangle, row after row: (0,0) (0,1) .. (0,K-1) (1,1) ..
    int q = i - P, j = 0;
    while (q >= K - j) { q -= K - j; ++j; }
    v = wts[((size_t)j * K + (j + q)) * W + w];
  }
  A[idx] = v;
}

// values of every handle, then the weights (K, K, W) and their walker means (K, K) on the first handle's stream
int mix_weights(const MultiCall& mc, double* d_w, double* d_ovl) {
  pqa_handle* h = mc.h;
  const long W = h->W;
  TRY(multi_values(mc.hs, mc.K));
  hipLaunchKernelGGL((k_ovl_weights<>), dim3((unsigned)((W + 255) / 256)), dim3(256), 0, h->stream, mc.P, mc.K, W, d_w);
  hipLaunchKernelGGL((k_ovl_mean<>), dim3((unsigned)(mc.K * mc.K)), dim3(256), 0, h->stream, (const double*)d_w, W, d_ovl);
  return check_launch(h, "k_ovl_weights / k_ovl_mean");
}

// Plan of one product: lda columns, P of them on the right.  The walkers are cut into slices of `per` walkers (whole staging steps)
// by W and the shape alone; a chunk is a whole number of slices, and k_sr_reduce adds the slices to the moments one after the other,
// so the sum over the walkers has one order whatever the chunks are.
struct MixPlan {
  int lda, nbi, nbj;
  long per, Wc, nslice;  // walkers per slice, walkers per chunk (nslice slices)
  size_t nmom;
};

MixPlan mix_plan(long W, int P, int nx, long chunk) {
  MixPlan p;
  p.lda = P + nx;
  p.nmom = (size_t)p.lda * P;
  p.nbi = (p.lda + 31) / 32;
  p.nbj = (P + 31) / 32;
  // most walkers of a chunk by the scratch limit, in whole staging steps (one step at least)
  const long wmax = std::max<long>(kSrKB, walker_chunk(W, (size_t)p.lda * sizeof(double)) / kSrKB * kSrKB);
  const long ns = sr_slices(W, p.nbi, p.nbj, p.nmom);
  p.per = std::min<long>(wmax, ((W + ns - 1) / ns + kSrKB - 1) / kSrKB * kSrKB);
  // slices per chunk: what the scratch limit and the caller's chunk allow (one at least), partial tiles within the scratch limit
  const long want = chunk > 0 ? std::min(wmax, chunk) : wmax;
  p.nslice = std::max<long>(1, std::min<long>(want / p.per, (long)(kChunkScratchBytes / (p.nmom * sizeof(double)))));
  p.nslice = std::min<long>(p.nslice, (W + p.per - 1) / p.per);
  p.Wc = p.nslice * p.per;
  return p;
}

// The product of one gathered chunk (wc <= p.Wc walkers) into the running moments d_mom (sym: with the symmetric block)
int mix_product(pqa_handle* h, const MixPlan& p, int P, int nx, int sym, long wc, bool first, const double* d_A, const double* d_s, double* d_part,
                double* d_mom) {
  const long ns = (wc + p.per - 1) / p.per;
  hipLaunchKernelGGL(k_sr_syrk, dim3((unsigned)p.nbj, (unsigned)p.nbi, (unsigned)ns), dim3(256), 0, h->stream, d_A, d_s, wc, P, nx, sym, p.per, d_part);
  TRY(check_launch(h, "k_sr_syrk"));
  const int row0 = sym ? 0 : P;
  const size_t nred = p.nmom - (size_t)row0 * P;
  hipLaunchKernelGGL(k_sr_reduce, dim3((unsigned)((nred + 255) / 256)), dim3(256), 0, h->stream, (const double*)d_part, P, nx, row0, (int)ns,
                     (int)first, 1, d_mom);
  return check_launch(h, "k_sr_reduce");
}

}  // namespace

extern "C" int pqa_mix_moments(pqa_handle_t* const* hs, int K, const int32_t* P, const int32_t* src, const int32_t* pos, double offset,
                               double threshold, const double* rot, const double* unif, const uint64_t* seeds, int64_t walker_chunk_arg,
                               double* overlap, double* en, double* moments, double* u_walker, double* en_walker) {
  MultiCall mc(hs, K, "pqa_mix_moments", false);  // (as pqa_sr_moments: nothing moves)
  pqa_handle* h = mc.h;
  if (!h) return -2;
  const std::string fn = mc.fn;
  // argument checks first: they need nothing but the handles' host-side sizes
  if (!P || !overlap || !en) FAIL(fn + ": P, overlap and en must not be NULL");
  if ((rot == nullptr) != (unif == nullptr)) FAIL(fn + ": rot and unif come together");
  if (!rot && !seeds) FAIL(fn + ": seeds must not be NULL without rot / unif");
  if (walker_chunk_arg < 0) FAIL(fn + ": walker_chunk must not be negative");
  long ptot = 0;
  int pmax = 0;
  for (int k = 0; k < K; ++k) {
    if (P[k] < 0) FAIL(fn + ": P must not be negative");
    ptot += P[k];
    pmax = std::max(pmax, (int)P[k]);
    if ((size_t)(P[k] + 2 * K) * P[k] * sizeof(double) > kChunkScratchBytes)
      FAIL(fn + ": the (P + 2K) x P moments of a state exceed the 256 MiB scratch limit (use the protocol route)");
  }
  if (ptot > 0 && (!src || !pos || !moments)) FAIL(fn + ": src, pos and moments must not be NULL when a state has columns");
  TRY(mc.open());
  bool need[kMaxK][4] = {};
  for (int k = 0, off = 0; k < K; off += P[k], ++k) TRY(sr_check_columns(h, hs[k], fn, P[k], src + off, pos + off, 2, need[k]));
  const long W = h->W;
  // every handle's energy pass (its own draws) and derivative sources
  MixEn E{};
  SrSources S[kMaxK] = {};
  size_t orot = 0, ounif = 0;
  TRY(multi_each(hs, K, [&](pqa_handle* g, int k) {
    TRY(energy_dev(g, threshold, rot ? rot + orot : nullptr, unif ? unif + ounif : nullptr, seeds ? seeds[k] : 0, 0u));
    TRY(sr_sources(g, need[k], S[k]));
    E.en[k] = (const double*)g->b_en.p;
    orot += (size_t)g->N * g->necp * 9;
    ounif += (size_t)g->N * g->necp * W;
    return 0;
  }));
  // plans of the states' products
  MixPlan plan[kMaxK];
  size_t amax = 0, pamax = 0, mmax = 0;
  for (int k = 0; k < K; ++k) {
    if (P[k] == 0) continue;
    plan[k] = mix_plan(W, P[k], 2 * K, (long)walker_chunk_arg);
    amax = std::max(amax, (size_t)plan[k].Wc * plan[k].lda);
    pamax = std::max(pamax, (size_t)plan[k].nslice * plan[k].nmom);
    mmax = std::max(mmax, plan[k].nmom);
  }
  // scratch on the first handle
  double *d_w, *d_a, *d_s, *d_u, *d_ovl, *d_en, *d_enw, *d_mom, *d_A, *d_part;
  int *d_src, *d_pos;
  auto layout = [&](Carver c) {
    d_w = c.take<double>((size_t)K * K * W);  // weights (K, K, W)
    d_a = c.take<double>((size_t)K * W);
    d_s = c.take<double>(W);
    d_u = c.take<double>(u_walker ? (size_t)K * W : 0);
    d_ovl = c.take<double>((size_t)K * K);
    d_en = c.take<double>((size_t)6 * K * K);
    d_enw = c.take<double>(en_walker ? (size_t)6 * W : 0);  // per-walker energies of one handle (W, 6)
    d_mom = c.take<double>(mmax);                            // moments of one state
    d_A = c.take<double>(amax);                              // A of one chunk
    d_part = c.take<double>(pamax);
    d_src = c.take<int>(pmax);  // src, pos of one state
    d_pos = c.take<int>(pmax);
    return c.size();
  };
  TRY(ensure(h, h->b_sr, layout(Carver())));
  layout(Carver(h->b_sr.p));
  TRY(mix_weights(mc, d_w, d_ovl));
  const unsigned gb = (unsigned)((W + 255) / 256);
  hipLaunchKernelGGL(k_mix_scale, dim3(gb), dim3(256), 0, h->stream, mc.P, K, W, d_a, d_s, u_walker ? d_u : nullptr);
  hipLaunchKernelGGL(k_mix_en, dim3((unsigned)(6 * K * K)), dim3(256), 0, h->stream, E, (const double*)d_w, K, W, offset, d_en);
  TRY(check_launch(h, "k_mix_scale / k_mix_en"));
  size_t moff = 0;
  for (int k = 0, off = 0; k < K; off += P[k], ++k) {
    if (P[k] == 0) continue;
    const MixPlan& p = plan[k];
    TRY(copy_in(h, d_src, src + off, (size_t)P[k] * sizeof(int)));
    TRY(copy_in(h, d_pos, pos + off, (size_t)P[k] * sizeof(int)));
    for (long w0 = 0; w0 < W; w0 += p.Wc) {
      const long wc = std::min(p.Wc, W - w0);
      hipLaunchKernelGGL(k_mix_gather, dim3((unsigned)((wc * p.lda + 255) / 256)), dim3(256), 0, h->stream, S[k], (const int*)d_src,
                         (const int*)d_pos, (int)P[k], K, k, E, (const double*)d_a, W, w0, wc, d_A);
      TRY(check_launch(h, "k_mix_gather"));
      TRY(mix_product(h, p, P[k], 2 * K, 1, wc, w0 == 0, d_A, d_s + w0, d_part, d_mom));
    }
    TRY(copy_in(h, moments + moff, d_mom, p.nmom * sizeof(double)));
    moff += p.nmom;
  }
  if (en_walker)
    for (int k = 0; k < K; ++k) {
      transpose(h, E.en[k], d_enw, 6, W);  // rows (6, W) -> (W, 6)
      TRY(check_launch(h, "k_transpose"));
      TRY(copy_in(h, en_walker + (size_t)k * 6 * W, d_enw, (size_t)6 * W * sizeof(double)));
    }
  if (u_walker) TRY(copy_in(h, u_walker, d_u, (size_t)K * W * sizeof(double)));
  TRY(copy_in(h, en, d_en, (size_t)6 * K * K * sizeof(double)));
  return copy_out(h, overlap, d_ovl, (size_t)K * K * sizeof(double));
}

extern "C" int pqa_mix_wtdp(pqa_handle_t* const* hs, int K, int P, const int32_t* src, const int32_t* pos, int64_t walker_chunk_arg,
                            double* overlap, double* wtdp) {
  MultiCall mc(hs, K, "pqa_mix_wtdp", false);
  pqa_handle* h = mc.h;
  if (!h) return -2;
  const std::string fn = mc.fn;
  if (P < 1) FAIL(fn + ": P must be at least 1");
  if (!src || !pos || !overlap || !wtdp) FAIL(fn + ": src, pos, overlap and wtdp must not be NULL");
  if (walker_chunk_arg < 0) FAIL(fn + ": walker_chunk must not be negative");
  const int npair = K * (K + 1) / 2;
  if ((size_t)(P + npair) * P * sizeof(double) > kChunkScratchBytes)
    FAIL(fn + ": the (P + K (K + 1) / 2) x P partial moments exceed the 256 MiB scratch limit (use the protocol route)");
  TRY(mc.open());
  pqa_handle* g = hs[K - 1];  // the derivatives are the last state's
  bool need[4] = {false, false, false, false};
  TRY(sr_check_columns(h, g, fn, P, src, pos, 2, need));
  const long W = h->W;
  SrSources S{};
  if (int rc = sr_sources(g, need, S)) {
    h->err = g->err;
    return rc;
  }
  const MixPlan p = mix_plan(W, P, npair, (long)walker_chunk_arg);
  // scratch on the first handle
  double *d_w, *d_s, *d_ovl, *d_mom, *d_A, *d_part;
  int *d_src, *d_pos;
  auto layout = [&](Carver c) {
    d_w = c.take<double>((size_t)K * K * W);  // weights (K, K, W)
    d_s = c.take<double>(W);
    d_ovl = c.take<double>((size_t)K * K);
    d_mom = c.take<double>(p.nmom);
    d_A = c.take<double>((size_t)p.Wc * p.lda);  // A of one chunk
    d_part = c.take<double>((size_t)p.nslice * p.nmom);
    d_src = c.take<int>(P);
    d_pos = c.take<int>(P);
    return c.size();
  };
  TRY(ensure(h, h->b_sr, layout(Carver())));
  layout(Carver(h->b_sr.p));
  TRY(copy_in(h, d_src, src, (size_t)P * sizeof(int)));
  TRY(copy_in(h, d_pos, pos, (size_t)P * sizeof(int)));
  TRY(mix_weights(mc, d_w, d_ovl));
  hipLaunchKernelGGL(k_mix_fill, dim3((unsigned)((W + 255) / 256)), dim3(256), 0, h->stream, W, d_s);
  TRY(check_launch(h, "k_mix_fill"));
  for (long w0 = 0; w0 < W; w0 += p.Wc) {
    const long wc = std::min(p.Wc, W - w0);
    hipLaunchKernelGGL(k_mix_gather_wt, dim3((unsigned)((wc * p.lda + 255) / 256)), dim3(256), 0, h->stream, S, (const int*)d_src, (const int*)d_pos,
                       P, K, npair, (const double*)d_w, W, w0, wc, d_A);
    TRY(check_launch(h, "k_mix_gather_wt"));
    TRY(mix_product(h, p, P, npair, 0, wc, w0 == 0, d_A, d_s + w0, d_part, d_mom));
  }
  std::vector<double> rows((size_t)npair * P);
  TRY(copy_in(h, rows.data(), d_mom + (size_t)P * P, rows.size() * sizeof(double)));
  TRY(copy_out(h, overlap, d_ovl, (size_t)K * K * sizeof(double)));
  for (int j = 0, q = 0; j < K; ++j)
    for (int k = j; k < K; ++k, ++q) {  // (j, k) and (k, j) are the same row
      memcpy(wtdp + ((size_t)j * K + k) * P, rows.data() + (size_t)q * P, (size_t)P * sizeof(double));
      memcpy(wtdp + ((size_t)k * K + j) * P, rows.data() + (size_t)q * P, (size_t)P * sizeof(double));
    }
  return 0;
}
