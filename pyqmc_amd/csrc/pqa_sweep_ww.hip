// pyqmc_amd C ABI implementation (host side): the wave-per-walker electron sweep in one launch (pqa_ww.hpp) — eligibility, launch.
// A block is one wave, so the synchronisation INSIDE the device functions it calls (PQA_WSYNC, pqa_common.hpp) is the wave-level fence
// here: LDS operations of a wave execute in order, the fence keeps the compiler from moving them.
#define PQA_WSYNC() do { __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront"); __builtin_amdgcn_wave_barrier(); } while (0)
#define PQA_SYNC_NS pqa_sync_wave
#include "pqa_internal.hpp"
#include "pqa_ww.hpp"

static size_t ww_xoff(const pqa_handle* h) {  // doubles in front of the exchange area: what k_propose / k_accept keep in dynamic LDS
  const size_t b = std::max(std::max(lds_sm(h), lds_det(h, 5)), lds_j3(h));
  return (b + 7) / 8;
}
static bool ww_cstage(const pqa_handle* h) { return (size_t)h->nao * (h->nmo[0] + h->nmo[1]) * sizeof(double) <= 16 * 1024; }  // coefficient matrices in LDS
static size_t ww_lds(const pqa_handle* h) {
  return (ww_xoff(h) + PQA_WW_XCH + (size_t)5 * std::max(std::max(h->nmo[0], h->nmo[1]), 1) + (size_t)5 * h->nao +
          (ww_cstage(h) ? (size_t)h->nao * (h->nmo[0] + h->nmo[1]) : 0)) * sizeof(double);
}

bool ww_eligible(pqa_handle* h, long W) {
  if (h->ww.mode == 0 || h->cplx || h->S.pbc) return false;
  if (ww_lds(h) > 64 * 1024 || h->lmax > 5) return false;
  return h->ww.mode > 0 || W <= h->ww.max;
}

int sweep_ww(pqa_handle* h, const MoveBuf& mb) {
  using WwKernel = void (*)(SysDev, SlaterState, JastrowState, MoveBuf, int, int, int, int, long);
  static const WwKernel kernels[3] = {k_sweep_ww<2>, k_sweep_ww<3>, k_sweep_ww<5>};  // LMAX 2 | 3 | 5
  const long W = h->W;
  const dim3 grid((unsigned)W), block(64);
  hipLaunchKernelGGL(kernels[h->lmax <= 2 ? 0 : (h->lmax <= 3 ? 1 : 2)], grid, block, ww_lds(h), h->stream, h->S, h->st, h->js, mb, (int)h->has_slater,
                     (int)h->has_jastrow, (int)ww_xoff(h), (int)ww_cstage(h), W);
  return check_launch(h, "k_sweep_ww");
}
