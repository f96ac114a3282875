// pqa_tmb.hpp — the T-move candidates of a DMC step from the batched ECP integrator (EnergyAccumulator(use_old_ecp=False) ->
// jax_ecp.ECPAccumulator.nonlocal_tmoves, jax_ecp.py:110-135), for all electrons of the step at once.
//
// Front end of the T-move phase of pqa_dmc_steps when pqa_set_ecp_batched is on; it fills the lists the semi-local pair
// k_tm_count / k_tm_fill fills (TmBuf: cnt, off, pts, wgt, ptw; electron-major, spin-up first), and everything behind them — orbital
// rows, k_tm_ratio, k_tm_walker, the commit — is shared (pqa_dmc.hpp):
//   k_ecpb_fill in its T-move mode (pqa_ecpb.hpp; the selection, its tie rule and the uniform fallback are that kernel's) writes the dense
//   table [W][N][nsel] of positions and weights: nsel slots per (walker, electron), the deterministic selections ascending, then the
//   random ones;
//   k_tmb_count   cnt[e W + w] = slots whose weight is not exactly 0.0                      -> scan_ints
//   k_tmb_compact moves those slots to pts / wgt / ptw, in slot order within each (electron, walker).
// A slot of weight 0 has the amplitude ratio * 0 = 0: it is never the first crossing of the cumulative distribution, and with a finite
// ratio it adds nothing to the forward or the backward norm — the argument of pqa_dmc.hpp for the candidates of masked atoms.  Dropping them
// is what keeps the candidate count near the semi-local one: exp(-tau v_l / p) - 1 is exactly 0 wherever tau v_l / p < 2^-53, the far atoms.
// The candidates are left unfolded, as k_tm_fill leaves them: the orbital kernels and the Jastrow pair distances reduce every point
// themselves, and k_tm_walker folds the accepted one (TmBuf::nofold).
//
// Both kernels: one wave per walker, four walkers per block, lanes over the slots of one electron after the other.  A walker's part of
// the dense table is one contiguous run of N nsel doubles which the wave reads front to back (a thread per (electron, walker) would read
// 8 nsel bytes at a stride of 8 N nsel); the live slots of an (electron, walker) are found with one ballot per 64 slots, which also gives
// every live lane its rank, and are written next to each other.
#pragma once
#include "pqa_dmc.hpp"
#include "pqa_ecpb.hpp"

#define PQA_TMB_WB 4

// dw: [W][N][nsel] T-move weights.  grid = ceil(W / 4), block = 256.
template <int PQA_UNIT = 0>  // (a template so that only the units that launch it compile it)
static __global__ __launch_bounds__(64 * PQA_TMB_WB) void k_tmb_count(const double* __restrict__ dw, int nelec, int nsel, long W, int* __restrict__ cnt) {
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const long w = (long)blockIdx.x * PQA_TMB_WB + wv;
  if (w >= W) return;
  const double* t = dw + (size_t)w * nelec * nsel;
  for (int e = 0; e < nelec; ++e) {
    int c = 0;
    for (int s0 = 0; s0 < nsel; s0 += 64) {
      const int sl = s0 + lane;
      const bool live = sl < nsel && t[(size_t)e * nsel + sl] != 0.0;
      c += __popcll(__ballot(live));
    }
    if (lane == 0) cnt[(size_t)e * W + w] = c;
  }
}

// dpos: [W][N][nsel][3], dw: [W][N][nsel]; off: exclusive scan of cnt.  grid = ceil(W / 4), block = 256.
template <int PQA_UNIT = 0>  // (a template so that only the units that launch it compile it)
static __global__ __launch_bounds__(64 * PQA_TMB_WB) void k_tmb_compact(const double* __restrict__ dpos, const double* __restrict__ dw, int nelec, int nsel,
                                                                        long W, const long* __restrict__ off, double* __restrict__ pts,
                                                                        double* __restrict__ wgt, int* __restrict__ ptw) {
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const long w = (long)blockIdx.x * PQA_TMB_WB + wv;
  if (w >= W) return;
  const size_t t0 = (size_t)w * nelec * nsel;
  for (int e = 0; e < nelec; ++e) {
    long run = off[(size_t)e * W + w];
    if (off[(size_t)e * W + w + 1] == run) continue;  // (no live slot)
    for (int s0 = 0; s0 < nsel; s0 += 64) {
      const int sl = s0 + lane;
      const size_t i = t0 + (size_t)e * nsel + (sl < nsel ? sl : 0);
      const double wt = dw[i];
      const bool live = sl < nsel && wt != 0.0;
      const unsigned long long m = __ballot(live);
      if (live) {
        const long p = run + __popcll(m & ((1ull << lane) - 1ull));
        pts[3 * p] = dpos[3 * i]; pts[3 * p + 1] = dpos[3 * i + 1]; pts[3 * p + 2] = dpos[3 * i + 2];
        wgt[p] = wt;
        ptw[p] = (int)w;
      }
      run += __popcll(m);
    }
  }
}

using TmbFillKernel = void (*)(SysDev, JastrowState, EcpBuf, EcpbArgs, long);
static const TmbFillKernel tmb_fill_kernels[2] = {k_ecpb_fill<true>, k_ecpb_fill<false>};  // [PBC]

// The dense table of one step: every electron's nsel slots (positions into dpos, weights into dw).  rot: [N][necp][3][3] on the device;
// selu: [N][W][nsr] on the device or NULL -> Philox stream PQA_STREAM_TMSEL of (seed, step).
static inline void launch_tmb_table(pqa_handle* h, const double* rot, const double* selu, uint64_t seed, uint32_t step, double tau, double* dpos,
                                    double* dw) {
  EcpBuf E{};
  E.rot = rot; E.quad = h->d_quad; E.quadw = h->d_quadw; E.seed = seed; E.step = step;
  EcpbArgs A{};
  A.naip = h->d_ecpb_naip; A.qoff = h->d_ecpb_qoff; A.pstart = h->d_ecpb_pstart;
  A.npoints = h->ecpb_npoints; A.nsd = h->ecpb_nsd; A.nsr = h->ecpb_nsr; A.nsel = h->ecpb_nsel;
  A.e0 = 0; A.e1 = h->N; A.tau = tau; A.selu = selu; A.out_pos = dpos; A.out_w = dw; A.stream = PQA_STREAM_TMSEL;
  hipLaunchKernelGGL(tmb_fill_kernels[h->S.pbc ? 0 : 1], dim3((unsigned)((h->W + PQA_ECPB_WB - 1) / PQA_ECPB_WB)), dim3(64 * PQA_ECPB_WB), 0, h->stream,
                     h->S, h->js, E, A, h->W);
}
