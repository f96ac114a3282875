// Code shared by the units that drive K resident wave functions in one call (pqa_overlap: the mixture sum_k |Psi_k|^2; pqa_add: the
// superposition sum_k c_k Psi_k; pqa_mix: the estimators over the mixture); no other unit includes it.
//   MultiCall     what every entry does first: the handles checked (multi_validate), their states current, their streams shared for the
//                 call's duration, the pointer table OvlPtrs filled;
//   multi_each    the loop over the handles, a failure's message moved to the first handle (multi_values: values_dev, multi_rows: rows_at);
//   weights       compute_weights (sample_many.py:42-55) per walker (ovl_psi_rho, k_ovl_weights) and its walker mean (k_ovl_mean).
// multi_sweeps is the Metropolis sweep of pqa_overlap_sweeps and pqa_add_sweeps.  Per sweep the tapes are copied in; per electron e
// (spin s), all K handles' work ordered on the first handle's stream with no host round trip of its data:
//   has-zero   the vanished-determinant test of slater.py:269-275 on spin s of every handle (k_has_zero), its flags copied to pinned
//              host words behind an event the host waits on only before the updates: the work below is queued behind it (multi_flags)
//   values     per handle: sign and log of the Slater factor, the Jastrow exponent, left on the device (values_dev)
//   old rows   per handle: e's current position gathered (k_ovl_gather), launch_orb + k_slater_eval<5> + k_jastrow_eval (mode 1)
//              there (rows_at)
//   proposal   the entry's kernel: its drift from the rows, then multi_propose: x + gauss + tstep drift into every handle's b_newpos
//   new rows   per handle: rows_at the proposed position, the orbital rows in b_motmp (the saved rows of the update)
//   decision   the entry's kernel: its new drift and ratio, multi_tprob, multi_accept: the mask into every handle's b_mask, counted
//   update     per handle under the one mask: k_sm_update with the saved rows + k_jastrow_update; a handle whose spin-s determinants
//              had vanished instead gets k_jastrow_update and a rebuild of its Slater state from the moved walkers, the protocol's
//              fallback: Slater.recompute(configs) then the Jastrow update (multi_update)
// and after the sweep the entry's own step; k_ovl_fraction turns the counts into an accepted fraction.
#pragma once
#include "pqa_estim.hpp"

// the reference's arithmetic, operation by operation: no fused multiply-adds in what follows, here and in the including unit's own
// kernels (the handle's kernels, included above, keep theirs)
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

__device__ __forceinline__ void limdrift1(double (&g)[3]) {  // mc.limdrift, cutoff 1
  const double tot = sqrt(g[0] * g[0] + g[1] * g[1] + g[2] * g[2]);
  if (tot > 1.0) for (int d = 0; d < 3; ++d) g[d] = g[d] / tot;
}

// the drift g kept for the decision; the proposed position of walker w into every handle's b_newpos
__device__ __forceinline__ void multi_propose(const OvlPtrs& P, int K, long w, double tstep, const double* __restrict__ gauss,
                                              const double (&g)[3], double* __restrict__ grad) {
  for (int d = 0; d < 3; ++d) {
    grad[3 * w + d] = g[d];
    const double x = (P.pts[0][3 * w + d] + gauss[3 * w + d]) + g[d] * tstep;
    for (int k = 0; k < K; ++k) P.newpos[k][3 * w + d] = x;
  }
}

// the Metropolis factor of the move of walker w: the Gaussian draw forward, the draw plus both drifts backward
__device__ __forceinline__ double multi_tprob(long w, double tstep, const double* __restrict__ gauss, const double* __restrict__ grad,
                                              const double (&ng)[3]) {
  double gs[3], bs[3];
  for (int d = 0; d < 3; ++d) {
    gs[d] = gauss[3 * w + d];
    bs[d] = gs[d] + tstep * (grad[3 * w + d] + ng[d]);
  }
  const double forward = gs[0] * gs[0] + gs[1] * gs[1] + gs[2] * gs[2];
  const double backward = bs[0] * bs[0] + bs[1] * bs[1] + bs[2] * bs[2];
  return exp(1.0 / (2.0 * tstep) * (forward - backward));
}

// the decision of walker w into every handle's b_mask; the walker's accepted moves counted
__device__ __forceinline__ void multi_accept(const OvlPtrs& P, int K, long w, bool acc, double* __restrict__ nacc) {
  for (int k = 0; k < K; ++k) P.mask[k][w] = acc;
  nacc[w] += acc ? 1.0 : 0.0;
}

// compute_weights (sample_many.py:42-55) for walker w: psi[k] = phase_k exp(log_k - ref) with ref = max_k log_k; returns
// rho = mean_k exp(2 (log_k - ref)).  nan_to_num where the reference applies it.
__device__ __forceinline__ double ovl_psi_rho(const OvlPtrs& P, int K, long w, double (&psi)[kMaxK]) {
  double ph[kMaxK], lv[kMaxK];
  double ref = -DBL_MAX;
  for (int k = 0; k < K; ++k) {
    ph[k] = clamp_nan_to_num(P.sign[k][w]);
    lv[k] = clamp_nan_to_num(P.lg[k][w] + P.ju[k][w]);
    ref = k ? fmax(ref, lv[k]) : lv[k];
  }
  double rho = 0.0;
  for (int k = 0; k < K; ++k) {
    const double t = clamp_nan_to_num(exp(2.0 * (lv[k] - ref)));
    rho = k ? rho + t : t;
    psi[k] = ph[k] * clamp_nan_to_num(exp(lv[k] - ref));
  }
  return rho / K;
}

// weights[i][j][w] = psi_i psi_j / rho (compute_weights)
template <int PQA_UNIT = 0>  // (a template so that only the units that launch it compile it)
__global__ __launch_bounds__(256) void k_ovl_weights(OvlPtrs P, int K, long W, double* __restrict__ wts) {
  const long w = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (w >= W) return;
  double psi[kMaxK];
  const double rho = ovl_psi_rho(P, K, w, psi);
  for (int i = 0; i < K; ++i)
    for (int j = 0; j < K; ++j) wts[((size_t)i * K + j) * W + w] = psi[i] * (psi[j] / rho);
}

// out[ij] = mean over walkers of wts[ij][.]: one block per (i, j), a fixed-order tree (the same bits on every call)
template <int PQA_UNIT = 0>  // (a template so that only the units that launch it compile it)
__global__ __launch_bounds__(256) void k_ovl_mean(const double* __restrict__ wts, long W, double* __restrict__ out) {
  __shared__ double part[256];
  const double* row = wts + (size_t)blockIdx.x * W;
  double a = 0.0;
  for (long w = threadIdx.x; w < W; w += 256) a += row[w];
  a = block_sum256(a, part);
  if (threadIdx.x == 0) out[blockIdx.x] = a / (double)W;
}

// out[0] = sum_w nacc[w] / denom in a fixed order (one block); the counts cleared for the next sweep.  The counts are whole numbers, so
// the sum is exact in any order.
template <int PQA_UNIT = 0>  // (a template so that only the units that launch it compile it)
__global__ __launch_bounds__(256) void k_ovl_fraction(double* __restrict__ nacc, long W, double denom, double* __restrict__ out) {
  __shared__ double part[256];
  double a = 0.0;
  for (long w = threadIdx.x; w < W; w += 256) {
    a += nacc[w];
    nacc[w] = 0.0;
  }
  a = block_sum256(a, part);
  if (threadIdx.x == 0) out[0] = a / denom;
}

__global__ __launch_bounds__(256) void k_ovl_gather(OvlPtrs P, int K, int N, int e, long W) {
  const long w = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (w >= W) return;
  for (int k = 0; k < K; ++k)
    for (int d = 0; d < 3; ++d) P.pts[k][3 * w + d] = P.x[k][((size_t)w * N + e) * 3 + d];
}

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

// fn(handle, k) for every handle, up to the first failure; its message is reported on the first handle
template <class F>
int multi_each(pqa_handle* const* hs, int K, F fn) {
  for (int k = 0; k < K; ++k) {
    const int rc = fn(hs[k], k);
    if (rc) {
      if (k) hs[0]->err = hs[k]->err;
      return rc;
    }
  }
  return 0;
}

int multi_values(pqa_handle* const* hs, int K) {
  return multi_each(hs, K, [](pqa_handle* g, int) { return values_dev(g); });
}

int multi_rows(pqa_handle* const* hs, int K, int e, double* const* pts) {
  return multi_each(hs, K, [&](pqa_handle* g, int k) { return rows_at(g, e, pts[k]); });
}

// The handles a multi-handle call takes (fn: its name, for the messages); errors are reported on the first handle.
int multi_validate(pqa_handle* const* hs, int K, const char* fn) {
  pqa_handle* h = hs[0];
  const std::string f = std::string(fn) + ": ";
  if (K > kMaxK) FAIL(f + "at most 8 wave functions");
  for (int k = 0; k < K; ++k) {
    pqa_handle* g = hs[k];
    if (!g) FAIL(f + "a NULL handle");
    for (int j = 0; j < k; ++j)
      if (hs[j] == g) FAIL(f + "the same handle twice");
    if (!g->has_slater || !g->has_j2 || g->has_j3 || g->cplx)
      FAIL(f + "every handle must be a real Slater x two-body-Jastrow product (others: the protocol route)");
    if (g->S.pbc || g->twist) FAIL(f + "open boundary conditions only (periodic handles: the protocol route)");
    if (g->W == 0) FAIL(f + "walkers not resident (call pqa_wf_recompute on every handle)");
    if (g->device != h->device) FAIL(f + "all handles must be on one device");
    if (g->W != h->W || g->N != h->N || g->nup != h->nup) FAIL(f + "all handles must have the same walkers and electrons");
  }
  return 0;
}

// The opening of an entry.  The entry returns -2 when h is NULL (hs, K or the first handle missing), runs the argument checks that
// come before the handles' own, then open().  moves: the call moves walkers or evaluates rows (every entry but pqa_mix's two, which
// keep dmc.old_valid and grow no per-move scratch).
struct MultiCall {
  pqa_handle* const* hs;
  const int K;
  const char* fn;  // the entry's name, for the messages
  const bool moves;
  pqa_handle* h;  // the first handle: errors are reported on it
  OvlPtrs P{};
  hipStream_t own[kMaxK];
  bool shared = false;
  MultiCall(pqa_handle* const* hs_, int K_, const char* fn_, bool moves_)
      : hs(hs_), K(K_), fn(fn_), moves(moves_), h(hs_ && K_ >= 1 ? hs_[0] : nullptr) {}
  ~MultiCall() {
    for (int k = 1; shared && k < K; ++k) hs[k]->stream = own[k];
  }

  int open() {
    TRY(multi_validate(hs, K, fn));
    HIPCHK(hipSetDevice(h->device));
    // every handle's walker-major state current, its saved gradient_value rows dropped and its queued work done ...
    TRY(multi_each(hs, K, [&](pqa_handle* g, int) {
      if (moves) g->dmc.old_valid = false;  // (as pqa_wf_update)
      TRY(sync_aos(g));
      TRY(jas_refresh(g));
      g->saved_valid = false;
      return 0;
    }));
    for (int k = 1; k < K; ++k) {
      hipError_t e = hipStreamSynchronize(hs[k]->stream);
      if (e != hipSuccess) FAIL(std::string(fn) + ": " + hipGetErrorString(e));
    }
    // ... before it runs on the first handle's stream for the call's duration (launch_orb and the helpers launch on h->stream)
    for (int k = 0; k < K; ++k) own[k] = hs[k]->stream;
    for (int k = 1; k < K; ++k) hs[k]->stream = h->stream;
    shared = true;
    // every handle's per-move scratch sized and the pointer table filled
    const long W = h->W;
    TRY(multi_each(hs, K, [&](pqa_handle* g, int k) {
      if (moves) {
        const int nmo = std::max(g->nmo[0], g->nmo[1]);
        TRY(ensure(g, g->b_pts, (size_t)W * 3 * sizeof(double)));
        TRY(ensure(g, g->b_motmp, (size_t)W * 5 * nmo * sizeof(double)));
        TRY(ensure(g, g->b_out, (size_t)9 * W * sizeof(double)));
        TRY(ensure(g, g->b_newpos, (size_t)W * 3 * sizeof(double)));
        TRY(ensure(g, g->b_mask, (size_t)W));
        TRY(ensure(g, g->b_flag, sizeof(int)));
      }
      P.x[k] = g->js.x;
      P.pts[k] = (double*)g->b_pts.p;
      P.out[k] = (const double*)g->b_out.p;
      P.newpos[k] = (double*)g->b_newpos.p;
      P.mask[k] = (uint8_t*)g->b_mask.p;
      P.sign[k] = (const double*)g->b_sign.p;
      P.lg[k] = (const double*)g->b_log.p;
      P.ju[k] = (const double*)g->b_ju.p;
      return 0;
    }));
    // the first handle's pinned flag words and event
    if (moves && !h->pin_ovl) TRY(new_pinned(h, &h->pin_ovl, kMaxK, hipHostMallocDefault));
    if (moves && !h->ovl_ev) TRY(new_event(h, &h->ovl_ev, hipEventDisableTiming));
    return 0;
  }
};

// slater.py:269-275 tests the spin's determinants before its update; nothing a move does before its update changes them
int multi_flags(pqa_handle* const* hs, int K, int s) {
  pqa_handle* h = hs[0];
  hipStream_t st = h->stream;
  const long W = h->W;
  for (int k = 0; k < K; ++k) {
    pqa_handle* g = hs[k];
    HIPCHK(hipMemsetAsync(g->b_flag.p, 0, sizeof(int), st));
    const long count = W * g->ndet_s[s];
    hipLaunchKernelGGL((k_has_zero<>), dim3((unsigned)((count + 255) / 256)), dim3(256), 0, st, (const double*)g->st.dlog[s], count,
                       (int*)g->b_flag.p);
    HIPCHK(hipMemcpyAsync(h->pin_ovl + k, g->b_flag.p, sizeof(int), hipMemcpyDeviceToHost, st));
  }
  HIPCHK(hipEventRecord(h->ovl_ev, st));
  return 0;
}

// the updates of electron e (spin s) under every handle's b_mask, once the flags of multi_flags have arrived
int multi_update(pqa_handle* const* hs, int K, int e, int s) {
  pqa_handle* h = hs[0];
  hipStream_t st = h->stream;
  const long W = h->W;
  HIPCHK(hipEventSynchronize(h->ovl_ev));  // (the proposal and decision stay queued while the host reads the flags)
  return multi_each(hs, K, [&](pqa_handle* g, int k) {
    const bool zero = h->pin_ovl[k] != 0;
    const uint8_t* dm = (const uint8_t*)g->b_mask.p;
    if (!zero)
      hipLaunchKernelGGL((k_sm_update<>), dim3((unsigned)W), dim3(64), lds_sm(g), st, g->S, g->st, e, (const double*)g->b_motmp.p, 5 * g->nmo[s], dm, 1);
    hipLaunchKernelGGL((k_jastrow_update<>), dim3((unsigned)W), dim3(64), 0, st, g->S, g->js, e, (const double*)g->b_newpos.p, dm);
    TRY(check_launch(g, "k_sm_update / k_jastrow_update"));
    return zero ? slater_rebuild(g) : 0;  // (the protocol's fallback: the Slater state rebuilt from the moved walkers)
  });
}

// Scratch of a sweep call on the first handle: the old drift (W, 3), the walkers' accepted moves (W) and the entry's own `nown` doubles
struct SweepScratch {
  double *grad, *acc, *own;
};

// nsteps sweeps (see the head of this file) with the tapes gauss (nsteps, N, W, 3) and unif (nsteps, N, W).  The entry gives its scratch
// buffer and three steps that launch on the first handle's stream and return a status: propose(gauss of e), decide(gauss of e, unif
// of e), after(sweep).
template <class Propose, class Decide, class After>
int multi_sweeps(MultiCall& mc, DevBuf& buf, size_t nown, int nsteps, const double* gauss, const double* unif, SweepScratch& sc, Propose propose,
                 Decide decide, After after) {
  pqa_handle* h = mc.h;
  pqa_handle* const* hs = mc.hs;
  const int K = mc.K, N = h->N;
  const long W = h->W;
  const size_t ng = (size_t)N * W * 3, nu = (size_t)N * W;
  double *d_g, *d_u;  // one sweep's tapes
  auto layout = [&](Carver c) {
    d_g = c.take<double>(ng);
    d_u = c.take<double>(nu);
    sc.grad = c.take<double>(3 * (size_t)W);
    sc.acc = c.take<double>(W);
    sc.own = c.take<double>(nown);
    return c.size();
  };
  TRY(ensure(h, buf, layout(Carver())));
  layout(Carver(buf.p));
  hipStream_t st = h->stream;
  HIPCHK(hipMemsetAsync(sc.acc, 0, (size_t)W * sizeof(double), st));
  for (int n = 0; n < nsteps; ++n) {
    TRY(copy_in(h, d_g, gauss + (size_t)n * ng, ng * sizeof(double)));
    TRY(copy_in(h, d_u, unif + (size_t)n * nu, nu * sizeof(double)));
    for (int e = 0; e < N; ++e) {
      const int s = e >= h->nup;
      TRY(multi_flags(hs, K, s));
      hipLaunchKernelGGL(k_ovl_gather, dim3((unsigned)((W + 255) / 256)), dim3(256), 0, st, mc.P, K, N, e, W);
      TRY(check_launch(h, "k_has_zero / k_ovl_gather"));
      TRY(multi_values(hs, K));
      TRY(multi_rows(hs, K, e, mc.P.pts));
      TRY(propose((const double*)(d_g + (size_t)e * W * 3)));
      TRY(multi_rows(hs, K, e, mc.P.newpos));
      TRY(decide((const double*)(d_g + (size_t)e * W * 3), (const double*)(d_u + (size_t)e * W)));
      TRY(multi_update(hs, K, e, s));
    }
    TRY(after(n));
  }
  return 0;
}

}  // namespace
