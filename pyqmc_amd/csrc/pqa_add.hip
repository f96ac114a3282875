// The superposition Psi = sum_k c_k Psi_k of K resident wave functions (AddWF, pyqmc/wf/addwf.py): its value and weights, Metropolis sweeps
// over |Psi|^2 (vmc_worker, pyqmc/method/mc.py:112-137) and its local energy, on the device with no host round trip of per-walker data.
// With w_k = c_k Psi_k / Psi (sum_k w_k = 1) at the current walkers, and v_k the ratio Psi_k(R') / Psi_k(R) of moving electron e:
//   Psi(R') / Psi(R)         = sum_k w_k v_k
//   rho_k                    = w_k v_k / sum_j w_j v_j                        (the weights at R')
//   grad_e Psi / Psi at R'   = sum_k rho_k grad_e Psi_k / Psi_k
//   E_L                      = sum_k w_k E_L,k                                (H is linear)
//
// pqa_add_sweeps, per electron e (spin s), all K handles' work ordered on the first handle's stream (pqa_multi.hpp):
//   has-zero   multi_flags; e's current position gathered (k_ovl_gather); every handle's value (values_dev)
//   old rows   per handle: rows_at the current position
//   proposal   k_add_propose: w_k from the values, the drift sum_k rho_k g_k with AddWF.gradient_value's rules, limdrift,
//              x + gauss + tstep grad into every handle's b_newpos
//   new rows   per handle: rows_at the proposed position (the saved rows of the update)
//   decision   k_add_decide: the new drift likewise, val = sum_k w_k val_k, t_prob |val|^2 against the uniform draw; the mask into
//              every handle's b_mask, the walker's accepted moves of the sweep counted
//   update     multi_update
// After each sweep k_add_mean turns the counts into the accepted fraction (a fixed-order tree) and clears them.
#include "pqa_multi.hpp"

#pragma clang fp contract(off)  // (as pqa_multi.hpp: this unit's own kernels too)

namespace {

struct AddCoef {
  double c[kMaxK];
};

// t_k = c_k sign_k exp(log|Psi_k| - max_j log|Psi_j|) and their sum in k order: w_k = t_k / sum.  The reference value is the walker's own
// maximum, so walkers that differ by hundreds in log|Psi| keep finite weights.  Returns the maximum.
__device__ __forceinline__ double add_terms(const OvlPtrs& P, const AddCoef& C, int K, long w, double (&t)[kMaxK], double& sum) {
  double lv[kMaxK];
  double ref = 0.0;
  for (int k = 0; k < K; ++k) {
    lv[k] = P.lg[k][w] + P.ju[k][w];
    ref = k ? fmax(ref, lv[k]) : lv[k];
  }
  sum = 0.0;
  for (int k = 0; k < K; ++k) {
    t[k] = (C.c[k] * P.sign[k][w]) * exp(lv[k] - ref);
    sum = k ? sum + t[k] : t[k];
  }
  return ref;
}

// AddWF.gradient_value on the rows b_out of every handle: the gradient sum_k rho_k g_k and the value sum_k w_k val_k, where g_k and
// val_k carry MultiplyWF.gradient_value's non-finite rules (a non-finite Slater gradient counts 0, a non-finite Slater ratio 1) and
// rho_k is formed from the raw ratios (MultiplyWF.testvalue)
__device__ __forceinline__ void add_gradient_value(const OvlPtrs& P, int K, long W, long w, const double (&wk)[kMaxK], double (&g)[3],
                                                   double& val) {
  double den = 0.0;
  val = 0.0;
  for (int k = 0; k < K; ++k) {
    const double* r = P.out[k];
    const double v = r[w];
    const double vk = (v >= -DBL_MAX && v <= DBL_MAX) ? v : 1.0;
    const double t = wk[k] * (vk * r[8 * W + w]);
    val = k ? val + t : t;
    const double n = wk[k] * (v * r[8 * W + w]);
    den = k ? den + n : n;
  }
  for (int d = 0; d < 3; ++d) g[d] = 0.0;
  for (int k = 0; k < K; ++k) {  // (the rows read again: no per-component arrays, no scratch)
    const double* r = P.out[k];
    const double v = r[w];
    const double rho = (wk[k] * (v * r[8 * W + w])) / den;
    for (int d = 0; d < 3; ++d) {
      double dv = r[(1 + d) * W + w] / v;
      if (!(dv >= -DBL_MAX && dv <= DBL_MAX)) dv = 0.0;
      const double t = rho * (dv + r[(5 + d) * W + w]);
      g[d] = k ? g[d] + t : t;
    }
  }
}

// sign and log|Psi| of the sum and w (K, W); any output may be NULL
__global__ __launch_bounds__(256) void k_add_weights(OvlPtrs P, AddCoef C, int K, long W, double* __restrict__ sign,
                                                     double* __restrict__ logabs, double* __restrict__ wts) {
  const long w = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (w >= W) return;
  double t[kMaxK], sum;
  const double ref = add_terms(P, C, K, w, t, sum);
  if (sign) sign[w] = sum / fabs(sum);
  if (logabs) logabs[w] = log(fabs(sum)) + ref;
  if (wts)
    for (int k = 0; k < K; ++k) wts[(size_t)k * W + w] = t[k] / sum;
}

// the weights (K, W) and the old drift (W, 3) kept for the decision; new positions into every handle's b_newpos
__global__ __launch_bounds__(256) void k_add_propose(OvlPtrs P, AddCoef C, int K, long W, double tstep, const double* __restrict__ gauss,
                                                     double* __restrict__ wts, double* __restrict__ grad) {
  const long w = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (w >= W) return;
  double wk[kMaxK], sum, g[3], val;
  add_terms(P, C, K, w, wk, sum);
  for (int k = 0; k < K; ++k) {
    wk[k] = wk[k] / sum;
    wts[(size_t)k * W + w] = wk[k];
  }
  add_gradient_value(P, K, W, w, wk, g, val);
  limdrift1(g);
  for (int d = 0; d < 3; ++d) {
    grad[3 * w + d] = g[d];
    const double x = (P.pts[0][3 * w + d] + gauss[3 * w + d]) + g[d] * tstep;
    for (int k = 0; k < K; ++k) P.newpos[k][3 * w + d] = x;
  }
}

__global__ __launch_bounds__(256) void k_add_decide(OvlPtrs P, int K, long W, double tstep, const double* __restrict__ gauss,
                                                    const double* __restrict__ unif, const double* __restrict__ wts,
                                                    const double* __restrict__ grad, double* __restrict__ nacc) {
  const long w = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (w >= W) return;
  double wk[kMaxK], ng[3], val;
  for (int k = 0; k < K; ++k) wk[k] = wts[(size_t)k * W + w];
  add_gradient_value(P, K, W, w, wk, ng, val);
  limdrift1(ng);
  double gs[3], bs[3];
  for (int d = 0; d < 3; ++d) {
    gs[d] = gauss[3 * w + d];
    bs[d] = gs[d] + tstep * (grad[3 * w + d] + ng[d]);
  }
  const double forward = gs[0] * gs[0] + gs[1] * gs[1] + gs[2] * gs[2];
  const double backward = bs[0] * bs[0] + bs[1] * bs[1] + bs[2] * bs[2];
  const double t_prob = exp(1.0 / (2.0 * tstep) * (forward - backward));
  const bool acc = fabs(val) * fabs(val) * t_prob > unif[w];
  for (int k = 0; k < K; ++k) P.mask[k][w] = acc;
  nacc[w] += acc ? 1.0 : 0.0;
}

// out[0] = sum_w nacc[w] / denom in a fixed order (one block); the counts cleared for the next sweep
__global__ __launch_bounds__(256) void k_add_mean(double* __restrict__ nacc, long W, double denom, double* __restrict__ out) {
  __shared__ double part[256];
  double a = 0.0;
  for (long w = threadIdx.x; w < W; w += 256) {
    a += nacc[w];
    nacc[w] = 0.0;
  }
  a = block_sum256(a, part);
  if (threadIdx.x == 0) out[0] = a / denom;
}

// grad2[w] (+)= |sum_k w_k g_k|^2 of the electron whose rows are in b_out (g_k = grad D_k / D_k + grad U_k at the current position)
__global__ __launch_bounds__(256) void k_add_grad2(OvlPtrs P, int K, long W, const double* __restrict__ wts, int first,
                                                   double* __restrict__ grad2) {
  const long w = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (w >= W) return;
  double s2 = 0.0;
  for (int d = 0; d < 3; ++d) {
    double a = 0.0;
    for (int k = 0; k < K; ++k) {
      const double* r = P.out[k];
      const double t = wts[(size_t)k * W + w] * (r[(1 + d) * W + w] / r[w] + r[(5 + d) * W + w]);
      a = k ? a + t : t;
    }
    s2 = s2 + a * a;
  }
  grad2[w] = first ? s2 : grad2[w] + s2;
}

struct AddRows {
  const double* en[kMaxK];  // b_en (6, W) of every handle: ke, ee, ei, ecp, grad2, total
};

// out (6, W): ke = sum_k w_k ke_k, ee and ei of handle 0, ecp = sum_k w_k ecp_k, grad2 as k_add_grad2 left it in row 4,
// total = ke + ee + ei + ecp + ii (k_energy_assemble's order)
__global__ __launch_bounds__(256) void k_add_combine(AddRows E, int K, long W, const double* __restrict__ wts, double ii,
                                                     double* __restrict__ out) {
  const long w = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (w >= W) return;
  double ke = 0.0, ec = 0.0;
  for (int k = 0; k < K; ++k) {
    const double wk = wts[(size_t)k * W + w];
    const double a = wk * E.en[k][w], b = wk * E.en[k][3 * W + w];
    ke = k ? ke + a : a;
    ec = k ? ec + b : b;
  }
  const double ee = E.en[0][W + w], ei = E.en[0][2 * W + w];
  out[w] = ke; out[W + w] = ee; out[2 * W + w] = ei; out[3 * W + w] = ec;
  out[5 * W + w] = ke + ee + ei + ec + ii;
}

// what the three entry points do first: the handles checked, their states current, their streams shared from here on by the caller
int add_begin(pqa_handle* const* hs, int K, const double* coeffs, const char* fn, AddCoef& C) {
  pqa_handle* h = hs[0];
  if (!coeffs) FAIL(std::string(fn) + ": coeffs must not be NULL");
  TRY(multi_validate(hs, K, fn));
  HIPCHK(hipSetDevice(h->device));
  for (int k = 0; k < K; ++k) C.c[k] = coeffs[k];
  return multi_begin(hs, K, fn);
}

int all_values(pqa_handle* const* hs, int K) {
  for (int k = 0; k < K; ++k) {
    int rc = values_dev(hs[k]);
    if (rc) { hs[0]->err = hs[k]->err; return rc; }
  }
  return 0;
}

int all_rows(pqa_handle* const* hs, int K, int e, double* const* pts) {
  for (int k = 0; k < K; ++k) {
    int rc = rows_at(hs[k], e, pts[k]);
    if (rc) { hs[0]->err = hs[k]->err; return rc; }
  }
  return 0;
}

}  // namespace

extern "C" int pqa_add_weights(pqa_handle_t* const* hs, int K, const double* coeffs, double* sign, double* logabs, double* w) {
  if (!hs || K < 1 || !hs[0]) return -2;
  pqa_handle* h = hs[0];  // (errors are reported on the first handle)
  AddCoef C{};
  TRY(add_begin(hs, K, coeffs, "pqa_add_weights", C));
  const long W = h->W;
  StreamShare share(hs, K);
  OvlPtrs P{};
  TRY(multi_buffers(hs, K, P));
  TRY(ensure(h, h->b_add, (size_t)(K + 2) * W * sizeof(double)));
  double* d_s = (double*)h->b_add.p;
  double* d_l = d_s + W;
  double* d_w = d_l + W;
  TRY(all_values(hs, K));
  hipLaunchKernelGGL(k_add_weights, dim3((unsigned)((W + 255) / 256)), dim3(256), 0, h->stream, P, C, K, W, sign ? d_s : nullptr,
                     logabs ? d_l : nullptr, w ? d_w : nullptr);
  TRY(check_launch(h, "k_add_weights"));
  if (sign) TRY(copy_in(h, sign, d_s, (size_t)W * sizeof(double)));
  if (logabs) TRY(copy_in(h, logabs, d_l, (size_t)W * sizeof(double)));
  return copy_out(h, w, d_w, w ? (size_t)K * W * sizeof(double) : 0);
}

extern "C" int pqa_add_sweeps(pqa_handle_t* const* hs, int K, const double* coeffs, double tstep, int nsteps, const double* gauss,
                              const double* unif, double* acc) {
  if (!hs || K < 1 || !hs[0]) return -2;
  pqa_handle* h = hs[0];  // (errors are reported on the first handle)
  if (nsteps < 0) FAIL("pqa_add_sweeps: nsteps must not be negative");
  if (!gauss || !unif) FAIL("pqa_add_sweeps: gauss and unif must not be NULL");
  AddCoef C{};
  TRY(add_begin(hs, K, coeffs, "pqa_add_sweeps", C));
  const long W = h->W;
  const int N = h->N;
  StreamShare share(hs, K);
  OvlPtrs P{};
  TRY(multi_buffers(hs, K, P));
  // scratch on the first handle: one sweep's tapes (N W 3 + N W), the weights (K W), the old drift (3 W), acceptance counts (W),
  // per-sweep accepted fractions (nsteps)
  const size_t ng = (size_t)N * W * 3, nu = (size_t)N * W, nw = (size_t)K * W;
  TRY(ensure(h, h->b_add, (ng + nu + nw + 3 * (size_t)W + W + (size_t)std::max(nsteps, 1)) * sizeof(double)));
  double* d_g = (double*)h->b_add.p;
  double* d_u = d_g + ng;
  double* d_w = d_u + nu;
  double* d_grad = d_w + nw;
  double* d_acc = d_grad + 3 * (size_t)W;
  double* d_o = d_acc + W;
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
      TRY(all_values(hs, K));
      TRY(all_rows(hs, K, e, P.pts));
      hipLaunchKernelGGL(k_add_propose, dim3(gb), dim3(256), 0, st, P, C, K, W, tstep, (const double*)(d_g + (size_t)e * W * 3), d_w, d_grad);
      TRY(check_launch(h, "k_add_propose"));
      TRY(all_rows(hs, K, e, P.newpos));
      hipLaunchKernelGGL(k_add_decide, dim3(gb), dim3(256), 0, st, P, K, W, tstep, (const double*)(d_g + (size_t)e * W * 3),
                         (const double*)(d_u + (size_t)e * W), (const double*)d_w, (const double*)d_grad, d_acc);
      TRY(check_launch(h, "k_add_decide"));
      TRY(multi_update(hs, K, e, s));
    }
    hipLaunchKernelGGL(k_add_mean, dim3(1), dim3(256), 0, st, d_acc, W, (double)W * N, d_o + n);
    TRY(check_launch(h, "k_add_mean"));
  }
  return copy_out(h, acc, d_o, acc ? (size_t)nsteps * sizeof(double) : 0);
}

extern "C" int pqa_add_energy(pqa_handle_t* const* hs, int K, const double* coeffs, double threshold, const double* rot,
                              const double* unif, uint64_t seed, double* out) {
  if (!hs || K < 1 || !hs[0]) return -2;
  pqa_handle* h = hs[0];  // (errors are reported on the first handle)
  if (!out) FAIL("pqa_add_energy: out must not be NULL");
  AddCoef C{};
  TRY(add_begin(hs, K, coeffs, "pqa_add_energy", C));
  for (int k = 0; k < K; ++k)
    if (hs[k]->ecpb_on) FAIL("pqa_add_energy: the semi-local ECP integrator only (pqa_set_ecp_batched is on)");
  const long W = h->W;
  const int N = h->N;
  StreamShare share(hs, K);
  OvlPtrs P{};
  TRY(multi_buffers(hs, K, P));
  TRY(ensure(h, h->b_add, (size_t)(K + 6) * W * sizeof(double)));
  double* d_w = (double*)h->b_add.p;
  double* d_out = d_w + (size_t)K * W;
  hipStream_t st = h->stream;
  const unsigned gb = (unsigned)((W + 255) / 256);
  // every handle's own energy pass with the same draws: its six rows stay in its b_en
  AddRows E{};
  for (int k = 0; k < K; ++k) {
    int rc = energy_dev(hs[k], threshold, rot, unif, seed, 0u);
    if (rc) { h->err = hs[k]->err; return rc; }
    E.en[k] = (const double*)hs[k]->b_en.p;
  }
  TRY(all_values(hs, K));
  hipLaunchKernelGGL(k_add_weights, dim3(gb), dim3(256), 0, st, P, C, K, W, (double*)nullptr, (double*)nullptr, d_w);
  TRY(check_launch(h, "k_add_weights"));
  for (int e = 0; e < N; ++e) {
    hipLaunchKernelGGL(k_ovl_gather, dim3(gb), dim3(256), 0, st, P, K, N, e, W);
    TRY(check_launch(h, "k_ovl_gather"));
    TRY(all_rows(hs, K, e, P.pts));
    hipLaunchKernelGGL(k_add_grad2, dim3(gb), dim3(256), 0, st, P, K, W, (const double*)d_w, (int)(e == 0), d_out + 4 * (size_t)W);
    TRY(check_launch(h, "k_add_grad2"));
  }
  hipLaunchKernelGGL(k_add_combine, dim3(gb), dim3(256), 0, st, E, K, W, (const double*)d_w, h->ii_energy, d_out);
  TRY(check_launch(h, "k_add_combine"));
  return copy_out(h, out, d_out, (size_t)6 * W * sizeof(double));
}
