// Metropolis sweeps over the mixture sum_k |Psi_k|^2 of K resident wave functions (sample_overlap_worker, pyqmc/method/sample_many.py:
// 130-186, without the accumulator part): multi_sweeps of pqa_multi.hpp with
//   proposal   k_ovl_propose: the mean of the K drifts r[1:4]/r[0] + r[5:8] (MultiplyWF.gradient), limdrift
//   decision   k_ovl_decide: gradient_value's non-finite rules, t_prob sum_k |ratio_k|^2 w_k / sum_k w_k with
//              w_k = exp(2 (log|Psi_k| - log|Psi_0|)) from the values at the move's start, accept if greater than the uniform draw
//   after      every handle's value, then k_ovl_weights (compute_weights, sample_many.py:42-55: psi_i psi_j / rho per walker) and
//              k_ovl_mean (the walker mean, a fixed-order tree: block_sum256), both pqa_multi.hpp's (pqa_mix weights its estimators
//              with them)
// and after the last sweep k_ovl_fraction: the accepted fraction of all moves.
#include "pqa_multi.hpp"

#pragma clang fp contract(off)  // (as pqa_multi.hpp: this unit's own kernels too)

namespace {

__global__ __launch_bounds__(256) void k_ovl_propose(OvlPtrs P, int K, long W, double tstep, const double* __restrict__ gauss,
                                                     double* __restrict__ grad) {
  const long w = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (w >= W) return;
  double g[3] = {0.0, 0.0, 0.0};
  for (int k = 0; k < K; ++k) {
    const double* r = P.out[k];
    const double v = r[w];
    for (int d = 0; d < 3; ++d) g[d] = g[d] + (r[(1 + d) * W + w] / v + r[(5 + d) * W + w]);
  }
  for (int d = 0; d < 3; ++d) g[d] = g[d] / K;
  limdrift1(g);
  multi_propose(P, K, w, tstep, gauss, g, grad);
}

__global__ __launch_bounds__(256) void k_ovl_decide(OvlPtrs P, int K, long W, double tstep, const double* __restrict__ gauss,
                                                    const double* __restrict__ unif, const double* __restrict__ grad,
                                                    double* __restrict__ nacc) {
  const long w = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (w >= W) return;
  double ng[3] = {0.0, 0.0, 0.0}, ratio2[kMaxK];
  for (int k = 0; k < K; ++k) {
    const double* r = P.out[k];
    const double v = r[w];
    for (int d = 0; d < 3; ++d) {
      double dv = r[(1 + d) * W + w] / v;
      if (!(dv >= -DBL_MAX && dv <= DBL_MAX)) dv = 0.0;  // (MultiplyWF.gradient_value)
      ng[d] = ng[d] + (dv + r[(5 + d) * W + w]);
    }
    const double val = (v >= -DBL_MAX && v <= DBL_MAX) ? v : 1.0;
    const double q = val * r[8 * W + w];
    ratio2[k] = fabs(q) * fabs(q);
  }
  for (int d = 0; d < 3; ++d) ng[d] = ng[d] / K;
  limdrift1(ng);
  const double t_prob = multi_tprob(w, tstep, gauss, grad, ng);
  const double lg0 = P.lg[0][w] + P.ju[0][w];
  double num = 0.0, den = 0.0;
  for (int k = 0; k < K; ++k) {
    const double wk = exp(2.0 * ((P.lg[k][w] + P.ju[k][w]) - lg0));
    num = k ? num + ratio2[k] * wk : ratio2[k] * wk;
    den = k ? den + wk : wk;
  }
  multi_accept(P, K, w, t_prob * num / den > unif[w], nacc);
}

}  // namespace

extern "C" int pqa_overlap_sweeps(pqa_handle_t* const* hs, int K, double tstep, int nsteps, const double* gauss, const double* unif,
                                  double* overlap, double* weights, double* acc_ratio) {
  MultiCall mc(hs, K, "pqa_overlap_sweeps", true);
  pqa_handle* h = mc.h;
  if (!h) return -2;
  if (nsteps < 0) FAIL("pqa_overlap_sweeps: nsteps must not be negative");
  if (!gauss || !unif || !overlap) FAIL("pqa_overlap_sweeps: gauss, unif and overlap must not be NULL");
  TRY(mc.open());
  const long W = h->W;
  const OvlPtrs& P = mc.P;
  const dim3 gb((unsigned)((W + 255) / 256)), tb(256);
  hipStream_t st = h->stream;
  // scratch of its own: the weights (K K W), the per-sweep overlaps (nsteps K K), the accepted fraction
  const size_t nw = (size_t)K * K * W, no = (size_t)nsteps * K * K;
  SweepScratch sc{};
  TRY(multi_sweeps(
      mc, h->b_ovl, nw + no + 1, nsteps, gauss, unif, sc,
      [&](const double* g) {
        hipLaunchKernelGGL(k_ovl_propose, gb, tb, 0, st, P, K, W, tstep, g, sc.grad);
        return check_launch(h, "k_ovl_propose");
      },
      [&](const double* g, const double* u) {
        hipLaunchKernelGGL(k_ovl_decide, gb, tb, 0, st, P, K, W, tstep, g, u, (const double*)sc.grad, sc.acc);
        return check_launch(h, "k_ovl_decide");
      },
      [&](int n) {
        TRY(multi_values(hs, K));
        hipLaunchKernelGGL((k_ovl_weights<>), gb, tb, 0, st, P, K, W, sc.own);
        hipLaunchKernelGGL((k_ovl_mean<>), dim3((unsigned)(K * K)), tb, 0, st, (const double*)sc.own, W, sc.own + nw + (size_t)n * K * K);
        return check_launch(h, "k_ovl_weights / k_ovl_mean");
      }));
  double* d_a = sc.own + nw + no;
  const bool moved = nsteps > 0 && h->N > 0;
  if (moved) {
    hipLaunchKernelGGL((k_ovl_fraction<>), dim3(1), tb, 0, st, sc.acc, W, (double)W * nsteps * h->N, d_a);
    TRY(check_launch(h, "k_ovl_fraction"));
  }
  TRY(copy_in(h, overlap, sc.own + nw, no * sizeof(double)));
  if (weights && nsteps > 0) TRY(copy_in(h, weights, sc.own, nw * sizeof(double)));
  double a = 0.0;
  TRY(copy_out(h, &a, d_a, moved ? sizeof(double) : 0));
  if (acc_ratio) *acc_ratio = a;
  return 0;
}
