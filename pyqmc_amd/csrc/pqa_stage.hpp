// Input staging shared by the per-electron protocol entries (pqa_capi.hip, pqa_gps.hip, pqa_geminal.hip); host code only.  An
// entry keeps its scope test, its launches and its copy_out; what every entry did by hand lives here once: the shared argument
// checks and the copies of the call's inputs into the handle's common per-call scratch (b_pts, b_widx, b_tves, b_newpos, b_mask).
// No entry keeps any of these buffers live across calls.  `fn` names the entry in every message; `W` is the walker count of the
// factor the entry works on (h->W, h->gps_W or h->gem_W).
#pragma once
#include "pqa_internal.hpp"

struct StagedPoints {
  const double* pts = nullptr;  // (P, 3) on the device
  const int* widx = nullptr;    // (nrow) on the device, nullptr: row r is walker r
  long P = 0;                   // nrow * npt; 0: nothing to do
};

// ints[0..n) of a host OR device array must lie in [0, bound): read through a host copy, as the header's pointer contract asks
inline int stage_check_ints(pqa_handle* h, const std::string& what, const int32_t* ints, int64_t n, long bound) {
  std::vector<int32_t> host((size_t)n);
  HIPCHK(hipMemcpy(host.data(), ints, (size_t)n * sizeof(int32_t), hipMemcpyDefault));
  for (int32_t v : host)
    if (v < 0 || v >= bound) FAIL(what + " out of range");
  return 0;
}

// Points (nrow, npt, 3) and the walker indices of their rows.  s->P == 0 on return: an empty call, nothing staged.
inline int stage_points(pqa_handle* h, const char* fn, long W, const double* pts, int64_t nrow, int npt, const int32_t* widx, StagedPoints* s) {
  *s = StagedPoints{};
  if (nrow <= 0 || npt <= 0) return 0;
  if (!pts) FAIL(std::string(fn) + ": pts is NULL");
  if (!widx && nrow != W) FAIL(std::string(fn) + ": nrow must equal the number of walkers when widx is NULL");
  const size_t P = (size_t)nrow * npt;
  TRY(ensure(h, h->b_pts, P * 3 * sizeof(double)));
  TRY(copy_in(h, h->b_pts.p, pts, P * 3 * sizeof(double)));  // (in flight while the indices are checked)
  s->pts = (const double*)h->b_pts.p;
  if (widx) {
    TRY(stage_check_ints(h, std::string(fn) + ": walker index", widx, nrow, W));
    TRY(ensure(h, h->b_widx, (size_t)nrow * sizeof(int)));
    TRY(copy_in(h, h->b_widx.p, widx, (size_t)nrow * sizeof(int)));
    s->widx = (const int*)h->b_widx.p;
  }
  s->P = (long)P;
  return 0;
}

// The inputs of an evaluation of electron e: mode 0 values at npt points per row, modes 1 and 2 derivatives at one point per row.
inline int stage_eval(pqa_handle* h, const char* fn, long W, int e, const double* pts, int64_t nrow, int npt, const int32_t* widx, int mode,
                      StagedPoints* s) {
  if (e < 0 || e >= h->N) FAIL(std::string(fn) + ": electron index out of range");
  if (mode < 0 || mode > 2 || (mode > 0 && npt != 1)) FAIL(std::string(fn) + ": bad mode / npt combination");
  return stage_points(h, fn, W, pts, nrow, npt, widx, s);
}

// The electron list of a testvalue_many call (ne >= 1) -> *des on the device.
inline int stage_electrons(pqa_handle* h, const char* fn, const int32_t* es, int ne, const int** des) {
  if (!es) FAIL(std::string(fn) + ": es is NULL");
  TRY(stage_check_ints(h, std::string(fn) + ": electron index", es, ne, h->N));
  TRY(ensure(h, h->b_tves, (size_t)ne * sizeof(int)));
  TRY(copy_in(h, h->b_tves.p, es, (size_t)ne * sizeof(int)));
  *des = (const int*)h->b_tves.p;
  return 0;
}

// The inputs of a move of electron e: new positions (W, 3) -> *dpos and the byte mask (W) -> *dmask (nullptr without a mask: every
// walker moves).  dpos == nullptr: the entry needs no positions in this call and epos is not read.
inline int stage_move(pqa_handle* h, const char* fn, long W, int e, const double* epos, const uint8_t* mask, const double** dpos,
                      const uint8_t** dmask) {
  *dmask = nullptr;
  if (e < 0 || e >= h->N) FAIL(std::string(fn) + ": electron index out of range");
  if (dpos) {
    if (!epos) FAIL(std::string(fn) + ": epos is NULL");
    TRY(ensure(h, h->b_newpos, (size_t)W * 3 * sizeof(double)));
    TRY(copy_in(h, h->b_newpos.p, epos, (size_t)W * 3 * sizeof(double)));
    *dpos = (const double*)h->b_newpos.p;
  }
  if (mask) {
    TRY(ensure(h, h->b_mask, (size_t)W));
    TRY(copy_in(h, h->b_mask.p, mask, (size_t)W));
    *dmask = (const uint8_t*)h->b_mask.p;
  }
  return 0;
}
