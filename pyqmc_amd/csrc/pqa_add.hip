// The superposition Psi = sum_k c_k Psi_k of K resident wave functions (AddWF, pyqmc/wf/addwf.py): its value and weights, Metropolis sweeps
// over |Psi|^2 (vmc_worker, pyqmc/method/mc.py:112-137) and its local energy, on the device with no host round trip of per-walker data.
// With w_k = c_k Psi_k / Psi (sum_k w_k = 1) at the current walkers, and v_k the ratio Psi_k(R') / Psi_k(R) of moving electron e:
//   Psi(R') / Psi(R)         = sum_k w_k v_k
//   rho_k                    = w_k v_k / sum_j w_j v_j                        (the weights at R')
//   grad_e Psi / Psi at R'   = sum_k rho_k grad_e Psi_k / Psi_k
//   E_L                      = sum_k w_k E_L,k                                (H is linear)
//
// pqa_add_sweeps is multi_sweeps of pqa_multi.hpp with
//   proposal   k_add_propose: w_k from the values, the drift sum_k rho_k g_k with AddWF.gradient_value's rules, limdrift
//   decision   k_add_decide: the new drift likewise, val = sum_k w_k val_k, t_prob |val|^2 against the uniform draw
//   after      k_ovl_fraction: the sweep's accepted fraction, the counts cleared
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
  multi_propose(P, K, w, tstep, gauss, g, grad);
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
  const double t_prob = multi_tprob(w, tstep, gauss, grad, ng);
  multi_accept(P, K, w, fabs(val) * fabs(val) * t_prob > unif[w], nacc);
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

// what the three entry points do after their own argument checks: the coefficients checked, the shared opening, the coefficients kept
int add_open(MultiCall& mc, const double* coeffs, AddCoef& C) {
  pqa_handle* h = mc.h;
  if (!coeffs) FAIL(std::string(mc.fn) + ": coeffs must not be NULL");
  TRY(mc.open());
  for (int k = 0; k < mc.K; ++k) C.c[k] = coeffs[k];
  return 0;
}

}  // namespace

extern "C" int pqa_add_weights(pqa_handle_t* const* hs, int K, const double* coeffs, double* sign, double* logabs, double* w) {
  MultiCall mc(hs, K, "pqa_add_weights", true);  // (it sizes the per-move scratch and clears dmc.old_valid, as it always has)
  pqa_handle* h = mc.h;
  if (!h) return -2;
  AddCoef C{};
  TRY(add_open(mc, coeffs, C));
  const long W = h->W;
  TRY(ensure(h, h->b_add, (size_t)(K + 2) * W * sizeof(double)));
  double* d_s = (double*)h->b_add.p;
  double* d_l = d_s + W;
  double* d_w = d_l + W;
  TRY(multi_values(hs, K));
  hipLaunchKernelGGL(k_add_weights, dim3((unsigned)((W + 255) / 256)), dim3(256), 0, h->stream, mc.P, C, K, W, sign ? d_s : nullptr,
                     logabs ? d_l : nullptr, w ? d_w : nullptr);
  TRY(check_launch(h, "k_add_weights"));
  if (sign) TRY(copy_in(h, sign, d_s, (size_t)W * sizeof(double)));
  if (logabs) TRY(copy_in(h, logabs, d_l, (size_t)W * sizeof(double)));
  return copy_out(h, w, d_w, w ? (size_t)K * W * sizeof(double) : 0);
}

extern "C" int pqa_add_sweeps(pqa_handle_t* const* hs, int K, const double* coeffs, double tstep, int nsteps, const double* gauss,
                              const double* unif, double* acc) {
  MultiCall mc(hs, K, "pqa_add_sweeps", true);
  pqa_handle* h = mc.h;
  if (!h) return -2;
  if (nsteps < 0) FAIL("pqa_add_sweeps: nsteps must not be negative");
  if (!gauss || !unif) FAIL("pqa_add_sweeps: gauss and unif must not be NULL");
  AddCoef C{};
  TRY(add_open(mc, coeffs, C));
  const long W = h->W;
  const OvlPtrs& P = mc.P;
  const dim3 gb((unsigned)((W + 255) / 256)), tb(256);
  hipStream_t st = h->stream;
  // scratch of its own: the weights (K W), the per-sweep accepted fractions (nsteps)
  const size_t nw = (size_t)K * W;
  SweepScratch sc{};
  TRY(multi_sweeps(
      mc, h->b_add, nw + nsteps, nsteps, gauss, unif, sc,
      [&](const double* g) {
        hipLaunchKernelGGL(k_add_propose, gb, tb, 0, st, P, C, K, W, tstep, g, sc.own, sc.grad);
        return check_launch(h, "k_add_propose");
      },
      [&](const double* g, const double* u) {
        hipLaunchKernelGGL(k_add_decide, gb, tb, 0, st, P, K, W, tstep, g, u, (const double*)sc.own, (const double*)sc.grad, sc.acc);
        return check_launch(h, "k_add_decide");
      },
      [&](int n) {
        hipLaunchKernelGGL((k_ovl_fraction<>), dim3(1), tb, 0, st, sc.acc, W, (double)W * h->N, sc.own + nw + n);
        return check_launch(h, "k_ovl_fraction");
      }));
  return copy_out(h, acc, sc.own + nw, acc ? (size_t)nsteps * sizeof(double) : 0);
}

extern "C" int pqa_add_energy(pqa_handle_t* const* hs, int K, const double* coeffs, double threshold, const double* rot,
                              const double* unif, uint64_t seed, double* out) {
  MultiCall mc(hs, K, "pqa_add_energy", true);
  pqa_handle* h = mc.h;
  if (!h) return -2;
  if (!out) FAIL("pqa_add_energy: out must not be NULL");
  AddCoef C{};
  TRY(add_open(mc, coeffs, C));
  for (int k = 0; k < K; ++k)
    if (hs[k]->ecpb_on) FAIL("pqa_add_energy: the semi-local ECP integrator only (pqa_set_ecp_batched is on)");
  const long W = h->W;
  const int N = h->N;
  const OvlPtrs& P = mc.P;
  TRY(ensure(h, h->b_add, (size_t)(K + 6) * W * sizeof(double)));
  double* d_w = (double*)h->b_add.p;
  double* d_out = d_w + (size_t)K * W;
  hipStream_t st = h->stream;
  const unsigned gb = (unsigned)((W + 255) / 256);
  // every handle's own energy pass with the same draws: its six rows stay in its b_en
  AddRows E{};
  TRY(multi_each(hs, K, [&](pqa_handle* g, int k) {
    TRY(energy_dev(g, threshold, rot, unif, seed, 0u));
    E.en[k] = (const double*)g->b_en.p;
    return 0;
  }));
  TRY(multi_values(hs, K));
  hipLaunchKernelGGL(k_add_weights, dim3(gb), dim3(256), 0, st, P, C, K, W, (double*)nullptr, (double*)nullptr, d_w);
  TRY(check_launch(h, "k_add_weights"));
  for (int e = 0; e < N; ++e) {
    hipLaunchKernelGGL(k_ovl_gather, dim3(gb), dim3(256), 0, st, P, K, N, e, W);
    TRY(check_launch(h, "k_ovl_gather"));
    TRY(multi_rows(hs, K, e, P.pts));
    hipLaunchKernelGGL(k_add_grad2, dim3(gb), dim3(256), 0, st, P, K, W, (const double*)d_w, (int)(e == 0), d_out + 4 * (size_t)W);
    TRY(check_launch(h, "k_add_grad2"));
  }
  hipLaunchKernelGGL(k_add_combine, dim3(gb), dim3(256), 0, st, E, K, W, (const double*)d_w, h->ii_energy, d_out);
  TRY(check_launch(h, "k_add_combine"));
  return copy_out(h, out, d_out, (size_t)6 * W * sizeof(double));
}
