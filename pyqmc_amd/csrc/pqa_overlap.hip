// Metropolis sweeps over the mixture sum_k |Psi_k|^2 of K resident wave functions (sample_overlap_worker, pyqmc/method/sample_many.py:
// 130-186, without the accumulator part), every electron move of every sweep on the device with no host round trip of its data.
//
// Per electron e (spin s), all K handles' work ordered on the first handle's stream:
//   has-zero   the vanished-determinant test of slater.py:269-275 on spin s of every handle (k_has_zero), its flags copied to pinned
//              host words behind an event the host waits on only before the updates (the work below is queued behind it)
//   old rows   per handle: e's current position gathered (k_ovl_gather), launch_orb + k_slater_eval<5> + k_jastrow_eval (mode 1)
//   proposal   k_ovl_propose: the mean of the K drifts r[1:4]/r[0] + r[5:8] (MultiplyWF.gradient), limdrift, x + gauss + tstep grad
//   new rows   per handle: launch_orb into b_motmp (the saved rows), k_slater_eval<5>, k_jastrow_eval (mode 1); each handle's value
//              (k_slater_value + k_jastrow_value: pqa_wf_value's log|Psi_k|)
//   decision   k_ovl_decide: gradient_value's non-finite rules, t_prob sum_k |ratio_k|^2 w_k / sum_k w_k with
//              w_k = exp(2 (log|Psi_k| - log|Psi_0|)), accept if greater than the uniform draw; the mask into every handle's b_mask
//   update     per handle under that mask: k_sm_update with the saved rows + k_jastrow_update; a handle whose spin-s determinants
//              had vanished instead gets k_jastrow_update and a rebuild of its Slater state from the moved walkers (the protocol's
//              fallback: Slater.recompute(configs) then the Jastrow update)
// After each sweep: every handle's value, then k_ovl_weights (compute_weights, sample_many.py:42-55: psi_i psi_j / rho per walker)
// and k_ovl_mean (the walker mean, a fixed-order tree: block_sum256), both pqa_multi.hpp's (pqa_mix weights its estimators with them).
#include "pqa_multi.hpp"

#pragma clang fp contract(off)  // (as pqa_multi.hpp: this unit's own kernels too)

namespace {

// grad (W, 3) kept for the decision; new positions into every handle's b_newpos
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
  for (int d = 0; d < 3; ++d) {
    grad[3 * w + d] = g[d];
    const double x = (P.pts[0][3 * w + d] + gauss[3 * w + d]) + g[d] * tstep;
    for (int k = 0; k < K; ++k) P.newpos[k][3 * w + d] = x;
  }
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
  double gs[3], bs[3];
  for (int d = 0; d < 3; ++d) {
    gs[d] = gauss[3 * w + d];
    bs[d] = gs[d] + tstep * (grad[3 * w + d] + ng[d]);
  }
  const double forward = gs[0] * gs[0] + gs[1] * gs[1] + gs[2] * gs[2];
  const double backward = bs[0] * bs[0] + bs[1] * bs[1] + bs[2] * bs[2];
  const double t_prob = exp(1.0 / (2.0 * tstep) * (forward - backward));
  const double lg0 = P.lg[0][w] + P.ju[0][w];
  double num = 0.0, den = 0.0;
  for (int k = 0; k < K; ++k) {
    const double wk = exp(2.0 * ((P.lg[k][w] + P.ju[k][w]) - lg0));
    num = k ? num + ratio2[k] * wk : ratio2[k] * wk;
    den = k ? den + wk : wk;
  }
  const bool acc = t_prob * num / den > unif[w];
  for (int k = 0; k < K; ++k) P.mask[k][w] = acc;
  nacc[w] += acc ? 1.0 : 0.0;
}

}  // namespace

extern "C" int pqa_overlap_sweeps(pqa_handle_t* const* hs, int K, double tstep, int nsteps, const double* gauss, const double* unif,
                                  double* overlap, double* weights, double* acc_ratio) {
  if (!hs || K < 1 || !hs[0]) return -2;
  pqa_handle* h = hs[0];  // (errors are reported on the first handle)
  if (nsteps < 0) FAIL("pqa_overlap_sweeps: nsteps must not be negative");
  if (!gauss || !unif || !overlap) FAIL("pqa_overlap_sweeps: gauss, unif and overlap must not be NULL");
  TRY(multi_validate(hs, K, "pqa_overlap_sweeps"));
  HIPCHK(hipSetDevice(h->device));
  const long W = h->W;
  const int N = h->N;
  TRY(multi_begin(hs, K, "pqa_overlap_sweeps"));
  StreamShare share(hs, K);
  OvlPtrs P{};
  TRY(multi_buffers(hs, K, P));
  // scratch on the first handle: one sweep's tapes (N W 3 + N W), the old drift (3 W), acceptance counts (W), weights (K K W),
  // per-sweep overlaps (nsteps K K)
  const size_t ng = (size_t)N * W * 3, nu = (size_t)N * W, nw = (size_t)K * K * W, no = (size_t)std::max(nsteps, 1) * K * K;
  TRY(ensure(h, h->b_ovl, (ng + nu + 3 * (size_t)W + W + nw + no) * sizeof(double)));
  double* d_g = (double*)h->b_ovl.p;
  double* d_u = d_g + ng;
  double* d_grad = d_u + nu;
  double* d_acc = d_grad + 3 * (size_t)W;
  double* d_w = d_acc + W;
  double* d_o = d_w + nw;
  hipStream_t st = h->stream;
  HIPCHK(hipMemsetAsync(d_acc, 0, (size_t)W * sizeof(double), st));
  const unsigned gb = (unsigned)((W + 255) / 256);
  for (int n = 0; n < nsteps; ++n) {
    TRY(copy_in(h, d_g, gauss + (size_t)n * ng, ng * sizeof(double)));
    TRY(copy_in(h, d_u, unif + (size_t)n * nu, nu * sizeof(double)));
    for (int e = 0; e < N; ++e) {
      const int s = e >= h->nup;
      TRY(multi_flags(hs, K, s));
      hipLaunchKernelGGL(k_ovl_gather, dim3(gb), dim3(256), 0, st, P, K, N, e, W);
      TRY(check_launch(h, "k_has_zero / k_ovl_gather"));
      for (int k = 0; k < K; ++k) {
        int rc = rows_at(hs[k], e, P.pts[k]);
        if (rc) { h->err = hs[k]->err; return rc; }
      }
      hipLaunchKernelGGL(k_ovl_propose, dim3(gb), dim3(256), 0, st, P, K, W, tstep, (const double*)(d_g + (size_t)e * W * 3), d_grad);
      TRY(check_launch(h, "k_ovl_propose"));
      for (int k = 0; k < K; ++k) {
        int rc = rows_at(hs[k], e, P.newpos[k]);
        if (!rc) rc = values_dev(hs[k]);
        if (rc) { h->err = hs[k]->err; return rc; }
      }
      hipLaunchKernelGGL(k_ovl_decide, dim3(gb), dim3(256), 0, st, P, K, W, tstep, (const double*)(d_g + (size_t)e * W * 3),
                         (const double*)(d_u + (size_t)e * W), (const double*)d_grad, d_acc);
      TRY(check_launch(h, "k_ovl_decide"));
      TRY(multi_update(hs, K, e, s));
    }
    for (int k = 0; k < K; ++k) {
      int rc = values_dev(hs[k]);
      if (rc) { h->err = hs[k]->err; return rc; }
    }
    hipLaunchKernelGGL((k_ovl_weights<>), dim3(gb), dim3(256), 0, st, P, K, W, d_w);
    hipLaunchKernelGGL((k_ovl_mean<>), dim3((unsigned)(K * K)), dim3(256), 0, st, (const double*)d_w, W, d_o + (size_t)n * K * K);
    TRY(check_launch(h, "k_ovl_weights / k_ovl_mean"));
  }
  if (nsteps > 0) TRY(copy_in(h, overlap, d_o, (size_t)nsteps * K * K * sizeof(double)));
  if (weights && nsteps > 0) TRY(copy_in(h, weights, d_w, nw * sizeof(double)));
  std::vector<double> acc((size_t)W);
  TRY(copy_out(h, acc.data(), d_acc, (size_t)W * sizeof(double)));
  if (acc_ratio) {
    double a = 0.0;
    for (long w = 0; w < W; ++w) a += acc[w];
    *acc_ratio = nsteps > 0 && N > 0 ? a / ((double)W * nsteps * N) : 0.0;
  }
  return 0;
}
