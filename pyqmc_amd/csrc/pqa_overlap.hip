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
// and k_ovl_mean (the walker mean, a fixed-order tree: block_sum256).
#include "pqa_estim.hpp"

// the reference's arithmetic, operation by operation: no fused multiply-adds in this unit's own kernels
#pragma clang fp contract(off)

namespace {

constexpr int kMaxK = 8;

struct OvlPtrs {
  const double* x[kMaxK];     // js.x (W, N, 3) of every handle
  double* pts[kMaxK];         // b_pts: e's current position (W, 3)
  const double* out[kMaxK];   // b_out: the nine rows of pqa_wf_eval (9, W)
  double* newpos[kMaxK];      // b_newpos (W, 3)
  uint8_t* mask[kMaxK];       // b_mask (W)
  const double* sign[kMaxK];  // b_sign (W): Slater sign
  const double* lg[kMaxK];    // b_log (W): Slater log
  const double* ju[kMaxK];    // b_ju (W): Jastrow log
};

__device__ __forceinline__ double nan_to_num(double v) {
  if (v != v) return 0.0;
  if (v > DBL_MAX) return DBL_MAX;
  if (v < -DBL_MAX) return -DBL_MAX;
  return v;
}

__device__ __forceinline__ void limdrift1(double (&g)[3]) {  // mc.limdrift, cutoff 1
  const double tot = sqrt(g[0] * g[0] + g[1] * g[1] + g[2] * g[2]);
  if (tot > 1.0) for (int d = 0; d < 3; ++d) g[d] = g[d] / tot;
}

__global__ __launch_bounds__(256) void k_ovl_gather(OvlPtrs P, int K, int N, int e, long W) {
  const long w = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (w >= W) return;
  for (int k = 0; k < K; ++k)
    for (int d = 0; d < 3; ++d) P.pts[k][3 * w + d] = P.x[k][((size_t)w * N + e) * 3 + d];
}

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

// weights[i][j][w] = psi_i psi_j / rho (compute_weights): psi_k = phase_k exp(log_k - ref), rho = mean_k exp(2 (log_k - ref))
__global__ __launch_bounds__(256) void k_ovl_weights(OvlPtrs P, int K, long W, double* __restrict__ wts) {
  const long w = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (w >= W) return;
  double ph[kMaxK], lv[kMaxK], psi[kMaxK];
  double ref = -DBL_MAX;
  for (int k = 0; k < K; ++k) {
    ph[k] = nan_to_num(P.sign[k][w]);
    lv[k] = nan_to_num(P.lg[k][w] + P.ju[k][w]);
    ref = k ? fmax(ref, lv[k]) : lv[k];
  }
  double rho = 0.0;
  for (int k = 0; k < K; ++k) {
    const double t = nan_to_num(exp(2.0 * (lv[k] - ref)));
    rho = k ? rho + t : t;
    psi[k] = ph[k] * nan_to_num(exp(lv[k] - ref));
  }
  rho = rho / K;
  for (int i = 0; i < K; ++i)
    for (int j = 0; j < K; ++j) wts[((size_t)i * K + j) * W + w] = psi[i] * (psi[j] / rho);
}

// out[ij] = mean over walkers of wts[ij][.]: one block per (i, j), a fixed-order tree (the same bits on every call)
__global__ __launch_bounds__(256) void k_ovl_mean(const double* __restrict__ wts, long W, double* __restrict__ out) {
  __shared__ double part[256];
  const double* row = wts + (size_t)blockIdx.x * W;
  double a = 0.0;
  for (long w = threadIdx.x; w < W; w += 256) a += row[w];
  a = block_sum256(a, part);
  if (threadIdx.x == 0) out[blockIdx.x] = a / (double)W;
}

// every handle runs on the first handle's stream for the call's duration (launch_orb and the helpers launch on h->stream)
struct StreamShare {
  pqa_handle* const* hs;
  int K;
  hipStream_t own[kMaxK];
  StreamShare(pqa_handle* const* hs_, int K_) : hs(hs_), K(K_) {
    for (int k = 0; k < K; ++k) own[k] = hs[k]->stream;
    for (int k = 1; k < K; ++k) hs[k]->stream = hs[0]->stream;
  }
  ~StreamShare() {
    for (int k = 1; k < K; ++k) hs[k]->stream = own[k];
  }
};

int values_dev(pqa_handle* h) {  // pqa_wf_value's two parts, left on the device: b_sign / b_log (Slater), b_ju (Jastrow)
  TRY(slater_value_dev(h));
  hipLaunchKernelGGL((k_jastrow_value<>), dim3((unsigned)h->W), dim3(64), 0, h->stream, h->S, h->js, (double*)h->b_ju.p);
  return check_launch(h, "k_jastrow_value");
}

int rows_at(pqa_handle* h, int e, const double* pts) {  // pqa_wf_eval's chain (jmode 1) at pts (W, 3) -> b_out (9, W), orbital rows in b_motmp
  const int s = e >= h->nup;
  const long W = h->W;
  TRY(launch_orb(h, s, plain_points(pts, W), W, 5, (double*)h->b_motmp.p));
  hipLaunchKernelGGL(k_slater_eval<5>, dim3((unsigned)W), dim3(64), lds_det(h, 5), h->stream, h->S, h->st, e, (const double*)h->b_motmp.p, W, 1,
                     (const int*)nullptr, (double*)h->b_out.p);
  hipLaunchKernelGGL((k_jastrow_eval<>), dim3((unsigned)W), dim3(64), lds_j3(h), h->stream, h->S, h->js, e, pts, W, 1, (const int*)nullptr, 1, 1,
                     (double*)h->b_out.p + (size_t)5 * W);
  return check_launch(h, "k_slater_eval / k_jastrow_eval");
}

}  // namespace

extern "C" int pqa_overlap_sweeps(pqa_handle_t* const* hs, int K, double tstep, int nsteps, const double* gauss, const double* unif,
                                  double* overlap, double* weights, double* acc_ratio) {
  if (!hs || K < 1 || !hs[0]) return -2;
  pqa_handle* h = hs[0];  // (errors are reported on the first handle)
  if (K > kMaxK) FAIL("pqa_overlap_sweeps: at most 8 wave functions");
  if (nsteps < 0) FAIL("pqa_overlap_sweeps: nsteps must not be negative");
  if (!gauss || !unif || !overlap) FAIL("pqa_overlap_sweeps: gauss, unif and overlap must not be NULL");
  for (int k = 0; k < K; ++k) {
    pqa_handle* g = hs[k];
    if (!g) FAIL("pqa_overlap_sweeps: a NULL handle");
    for (int j = 0; j < k; ++j)
      if (hs[j] == g) FAIL("pqa_overlap_sweeps: the same handle twice");
    if (!g->has_slater || !g->has_j2 || g->has_j3 || g->cplx)
      FAIL("pqa_overlap_sweeps: every handle must be a real Slater x two-body-Jastrow product (others: the protocol route)");
    if (g->S.pbc || g->twist) FAIL("pqa_overlap_sweeps: open boundary conditions only (periodic handles: the protocol route)");
    if (g->W == 0) FAIL("pqa_overlap_sweeps: walkers not resident (call pqa_wf_recompute on every handle)");
    if (g->device != h->device) FAIL("pqa_overlap_sweeps: all handles must be on one device");
    if (g->W != h->W || g->N != h->N || g->nup != h->nup) FAIL("pqa_overlap_sweeps: all handles must have the same walkers and electrons");
  }
  HIPCHK(hipSetDevice(h->device));
  const long W = h->W;
  const int N = h->N;
  for (int k = 0; k < K; ++k) {
    pqa_handle* g = hs[k];
    g->dmc_old_valid = false;  // (as pqa_wf_update)
    TRY(sync_aos(g));
    int rc = jas_refresh(g);
    if (rc) { h->err = g->err; return rc; }
    g->saved_valid = false;
  }
  // every handle's queued work done before its stream is shared
  for (int k = 1; k < K; ++k) {
    hipError_t e = hipStreamSynchronize(hs[k]->stream);
    if (e != hipSuccess) FAIL(std::string("pqa_overlap_sweeps: ") + hipGetErrorString(e));
  }
  StreamShare share(hs, K);
  OvlPtrs P{};
  for (int k = 0; k < K; ++k) {
    pqa_handle* g = hs[k];
    const int nmo = std::max(g->nmo[0], g->nmo[1]);
    int rc = 0;
    if (!rc) rc = ensure(g, g->b_pts, (size_t)W * 3 * sizeof(double));
    if (!rc) rc = ensure(g, g->b_motmp, (size_t)W * 5 * nmo * sizeof(double));
    if (!rc) rc = ensure(g, g->b_out, (size_t)9 * W * sizeof(double));
    if (!rc) rc = ensure(g, g->b_newpos, (size_t)W * 3 * sizeof(double));
    if (!rc) rc = ensure(g, g->b_mask, (size_t)W);
    if (!rc) rc = ensure(g, g->b_flag, sizeof(int));
    if (rc) { h->err = g->err; return rc; }
    P.x[k] = g->js.x;
    P.pts[k] = (double*)g->b_pts.p;
    P.out[k] = (const double*)g->b_out.p;
    P.newpos[k] = (double*)g->b_newpos.p;
    P.mask[k] = (uint8_t*)g->b_mask.p;
    P.sign[k] = (const double*)g->b_sign.p;
    P.lg[k] = (const double*)g->b_log.p;
    P.ju[k] = (const double*)g->b_ju.p;
  }
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
  if (!h->pin_ovl) TRY(new_pinned(h, &h->pin_ovl, kMaxK, hipHostMallocDefault));
  if (!h->ovl_ev) TRY(new_event(h, &h->ovl_ev, hipEventDisableTiming));
  hipStream_t st = h->stream;
  HIPCHK(hipMemsetAsync(d_acc, 0, (size_t)W * sizeof(double), st));
  const unsigned gb = (unsigned)((W + 255) / 256);
  for (int n = 0; n < nsteps; ++n) {
    TRY(copy_in(h, d_g, gauss + (size_t)n * ng, ng * sizeof(double)));
    TRY(copy_in(h, d_u, unif + (size_t)n * nu, nu * sizeof(double)));
    for (int e = 0; e < N; ++e) {
      const int s = e >= h->nup;
      // slater.py:269-275 tests the spin's determinants before its update; nothing below changes them before that point
      for (int k = 0; k < K; ++k) {
        pqa_handle* g = hs[k];
        HIPCHK(hipMemsetAsync(g->b_flag.p, 0, sizeof(int), st));
        const long count = W * g->ndet_s[s];
        hipLaunchKernelGGL((k_has_zero<>), dim3((unsigned)((count + 255) / 256)), dim3(256), 0, st, (const double*)g->st.dlog[s], count,
                           (int*)g->b_flag.p);
        HIPCHK(hipMemcpyAsync(h->pin_ovl + k, g->b_flag.p, sizeof(int), hipMemcpyDeviceToHost, st));
      }
      HIPCHK(hipEventRecord(h->ovl_ev, st));
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
      HIPCHK(hipEventSynchronize(h->ovl_ev));  // (the proposal and decision stay queued while the host reads the flags)
      for (int k = 0; k < K; ++k) {
        pqa_handle* g = hs[k];
        const int nmo = g->nmo[s];
        const bool zero = h->pin_ovl[k] != 0;
        const uint8_t* dm = (const uint8_t*)g->b_mask.p;
        if (!zero)
          hipLaunchKernelGGL((k_sm_update<>), dim3((unsigned)W), dim3(64), lds_sm(g), st, g->S, g->st, e, (const double*)g->b_motmp.p, 5 * nmo, dm, 1);
        hipLaunchKernelGGL((k_jastrow_update<>), dim3((unsigned)W), dim3(64), 0, st, g->S, g->js, e, (const double*)g->b_newpos.p, dm);
        int rc = check_launch(g, "k_sm_update / k_jastrow_update");
        if (!rc && zero) rc = slater_rebuild(g);  // (the protocol's fallback: the Slater state rebuilt from the moved walkers)
        if (rc) { h->err = g->err; return rc; }
      }
    }
    for (int k = 0; k < K; ++k) {
      int rc = values_dev(hs[k]);
      if (rc) { h->err = hs[k]->err; return rc; }
    }
    hipLaunchKernelGGL(k_ovl_weights, dim3(gb), dim3(256), 0, st, P, K, W, d_w);
    hipLaunchKernelGGL(k_ovl_mean, dim3((unsigned)(K * K)), dim3(256), 0, st, (const double*)d_w, W, d_o + (size_t)n * K * K);
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
