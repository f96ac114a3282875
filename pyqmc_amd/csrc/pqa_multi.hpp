// Code shared by the units that drive K resident wave functions in one call (pqa_overlap: the mixture sum_k |Psi_k|^2; pqa_add: the
// superposition sum_k c_k Psi_k; pqa_mix: the estimators over the mixture); no other unit includes it.  Per electron both do the same around their own proposal and decision:
//   has-zero   the vanished-determinant test of slater.py:269-275 on spin s of every handle (k_has_zero), its flags copied to pinned
//              host words behind an event the host waits on only before the updates (multi_flags)
//   rows       per handle: e's current position gathered (k_ovl_gather), launch_orb + k_slater_eval<5> + k_jastrow_eval (mode 1) at
//              the old and at the proposed position (rows_at); each handle's value left on the device (values_dev)
//   weights    compute_weights (sample_many.py:42-55) per walker (ovl_psi_rho, k_ovl_weights) and its walker mean (k_ovl_mean)
//   update     per handle under the one mask: k_sm_update with the saved rows + k_jastrow_update; a handle whose spin-s determinants
//              had vanished instead gets k_jastrow_update and a rebuild of its Slater state from the moved walkers (multi_update)
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

// compute_weights (sample_many.py:42-55) for walker w: psi[k] = phase_k exp(log_k - ref) with ref = max_k log_k; returns
// rho = mean_k exp(2 (log_k - ref)).  nan_to_num where the reference applies it.
__device__ __forceinline__ double ovl_psi_rho(const OvlPtrs& P, int K, long w, double (&psi)[kMaxK]) {
  double ph[kMaxK], lv[kMaxK];
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

__global__ __launch_bounds__(256) void k_ovl_gather(OvlPtrs P, int K, int N, int e, long W) {
  const long w = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (w >= W) return;
  for (int k = 0; k < K; ++k)
    for (int d = 0; d < 3; ++d) P.pts[k][3 * w + d] = P.x[k][((size_t)w * N + e) * 3 + d];
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

// Every handle's walker-major state current and its queued work done, before its stream is shared (StreamShare follows this call).
int multi_begin(pqa_handle* const* hs, int K, const char* fn) {
  pqa_handle* h = hs[0];
  for (int k = 0; k < K; ++k) {
    pqa_handle* g = hs[k];
    g->dmc_old_valid = false;  // (as pqa_wf_update)
    TRY(sync_aos(g));
    int rc = jas_refresh(g);
    if (rc) { h->err = g->err; return rc; }
    g->saved_valid = false;
  }
  for (int k = 1; k < K; ++k) {
    hipError_t e = hipStreamSynchronize(hs[k]->stream);
    if (e != hipSuccess) FAIL(std::string(fn) + ": " + hipGetErrorString(e));
  }
  return 0;
}

// Every handle's per-move scratch sized and the pointer table filled; the first handle's pinned flag words and event created.
int multi_buffers(pqa_handle* const* hs, int K, OvlPtrs& P) {
  pqa_handle* h = hs[0];
  const long W = h->W;
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
  if (!h->pin_ovl) TRY(new_pinned(h, &h->pin_ovl, kMaxK, hipHostMallocDefault));
  if (!h->ovl_ev) TRY(new_event(h, &h->ovl_ev, hipEventDisableTiming));
  return 0;
}

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
  return 0;
}

}  // namespace
