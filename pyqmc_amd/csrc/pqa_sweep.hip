// pyqmc_amd C ABI implementation (host side): layout conversions, the sweep routes, what the two propagation entries share (step_call_open,
// step_moves) and the fused VMC sweep (pqa_vmc_sweeps).
// See include/pyqmc_amd.h for the contract and pqa_internal.hpp for what the units share.
#include "pqa_sweep_launch.hpp"

void launch_step_real(pqa_handle* h, const LwState& L, const MoveBuf& mb, const StepArgs& a, int rowlen) {
  if (h->S.pbc) launch_step_lw<true, false>(h, L, mb, a, rowlen); else launch_step_lw<false, false>(h, L, mb, a, rowlen);
}
void launch_flush_real(pqa_handle* h, const LwState& L, int s, long W, long w0, long w1, int j_lo, int j_hi, int nq, int rowlen, int n_s) {
  launch_flush_lw<false>(h, L, s, W, w0, w1, j_lo, j_hi, nq, rowlen, n_s);
}

// energy of the resident walkers into device buffer b_en (6,W)
void transpose(pqa_handle* h, const double* in, double* out, long R, long C) {  // in [R][C] -> out [C][R]
  if (R <= 0 || C <= 0) return;
  hipLaunchKernelGGL((k_transpose<>), dim3((unsigned)((C + 31) / 32), (unsigned)((R + 31) / 32)), dim3(32, 8), 0, h->stream, in, out, R, C);
}

LwState lw_state(pqa_handle* h) {
  LwState L{};
  L.xt = (double*)h->b_xt.p;
  for (int s = 0; s < 2; ++s) {
    L.Tt[s] = (double*)h->b_Tt[s].p; L.rc[s] = (double*)h->b_rc[s].p; L.sel[s] = (uint8_t*)h->b_sel[s].p;
    L.dsign[s] = h->st.dsign[s]; L.dlog[s] = h->st.dlog[s];
  }
  L.auxt = (double*)h->b_auxt.p;
  return L;
}

// AoS (canonical, wave-per-walker kernels) -> SoA mirrors for the lane-per-walker kernels
int lw_from_aos(pqa_handle* h, bool with_cache) {
  const long W = h->W;
  const int nel[2] = {h->nup, h->ndn};
  TRY(ensure(h, h->b_xt, (size_t)W * h->N * 3 * sizeof(double)));
  TRY(ensure(h, h->b_auxt, (size_t)W * 8 * sizeof(double)));
  TRY(ensure(h, h->b_kpart, (size_t)W * h->N * 5 * sizeof(double)));
  transpose(h, h->js.x, (double*)h->b_xt.p, W, (long)h->N * 3);
  for (int s = 0; s < 2; ++s) {
    const size_t n = nel[s], cf = h->cplx ? 2 : 1;
    TRY(ensure(h, h->b_Tt[s], cf * W * n * n * sizeof(double)));
    const int row = 5 * h->nmo[s];
    TRY(ensure(h, h->b_rc[s], (size_t)2 * W * n * row * sizeof(double)));  // two slots per electron (pqa_lw.hpp)
    TRY(ensure(h, h->b_sel[s], (size_t)W * n));
    transpose(h, h->st.T[s], (double*)h->b_Tt[s].p, W, (long)(cf * n * n));
    if (n > 0 && row > 0) {
      // (without the cache: the caller knows the row cache and its selectors are live — the T-move phase of the DMC step)
      if (with_cache) hipLaunchKernelGGL((k_cache_to_rc<>), dim3((unsigned)W, (unsigned)n, (unsigned)((row + 255) / 256)), dim3(256), 0, h->stream,
                                         (const double*)h->st.cache[s], (double*)h->b_rc[s].p, (uint8_t*)h->b_sel[s].p, (int)n, row, W);
    }
  }
  return check_launch(h, "k_transpose");
}
// SoA -> AoS: coordinates and inverses (what the ECP kernels read); with_cache also the orbital cache
int lw_to_aos(pqa_handle* h, bool with_cache) {
  const long W = h->W;
  const int nel[2] = {h->nup, h->ndn};
  transpose(h, (const double*)h->b_xt.p, h->js.x, (long)h->N * 3, W);
  for (int s = 0; s < 2; ++s) {
    const long n = nel[s];
    transpose(h, (const double*)h->b_Tt[s].p, h->st.T[s], (h->cplx ? 2 : 1) * n * n, W);
    const int row = 5 * h->nmo[s];
    if (with_cache && n > 0 && row > 0)
      hipLaunchKernelGGL((k_cache_from_rc<>), dim3((unsigned)W, (unsigned)n, (unsigned)((row + 255) / 256)), dim3(256), 0, h->stream,
                         (const double*)h->b_rc[s].p, (const uint8_t*)h->b_sel[s].p, h->st.cache[s], (int)n, row, W);
  }
  return check_launch(h, "k_transpose");
}

// A fused call on the lane-per-walker kernels leaves the live state in the SoA planes and only marks the walker-major arrays
// stale: back-to-back fused calls (the blocks of a VMC run) then skip both layout conversions (~13 GB of traffic per call at
// 65536 walkers of the 64-electron system, 7 ms), and whoever needs the walker-major state — every protocol entry, the
// energy entry, branching — converts it back first.
int sync_aos(pqa_handle* h) {
  if (!h || !h->aos_stale) return 0;
  HIPCHK(hipSetDevice(h->device));
  h->aos_stale = false;
  return lw_to_aos(h, true);
}


// ---------------------------------------------------------------- one sweep over the electrons (shared by VMC and DMC)
// Geometry of the lane-per-walker kernels for W walkers.
LwCtx lw_geometry(const pqa_handle* h, long W) {
  LwCtx c;
  // thread groups per walker in k_step_lw.  Measured (tools/scratch/r3_step_abl*.sh, (H2O)8 step in ms at 4 / 8 / 16 groups):
  // 4096 walkers 6.38 / 5.15 / 4.67, 8192: 7.71 / 6.54 / 6.39, 16384: 10.7 / 9.8 / 11.1, 32768: 16.5 / 17.3 / 18.8, 65536: 30.8 / 32.7 / 37.3
  // 4 groups (a wave per group, k_step_lw's wide form) from 26624 walkers, 8 below, 16 below 16384 (re-measured at the end of round 4:
  // at 28672 walkers the wide form takes 13.1 ms per (H2O)8 step against 14.6 with 8 groups; at 24576 8 groups win 11.6 vs 12.2)
  c.Gm = 4;
  if ((long)4 * W < 1664L * 64) c.Gm = 8;
  if (c.Gm == 8 && (long)8 * W < 2048L * 64) c.Gm = 16;
  if (h->lw.gm > 0) c.Gm = std::min(h->lw.gm, 16);
  c.nmax = std::max(h->nup, h->ndn);
  // block size of the delayed Sherman-Morrison update: 4 from 16 electrons per spin (8 flushes at 32), 5 from 24 (7 flushes at 32:
  // 35.60 -> 35.32 ms per step of the 64-electron benchmark; 6 is slower again — the per-move commit touches KB rows)
  // small shards (every launch a latency chain, one block row per thread group): 8 — fewer flush launches and split step launches
  // ((H2O)8 at 4096 walkers: 4.08 ms per step with 5, 3.97 with 8, 3.94 with 11, 4.01 with 16; 8192: 5.97 / 5.80 / 5.90 / 6.00)
  const int kb = h->lw.kb < 0 ? (c.nmax >= 24 ? (W <= 8192 ? 8 : 5) : (c.nmax >= 16 ? 4 : 0)) : h->lw.kb;
  c.KB = (kb > 0) ? std::min(kb, std::max(c.nmax, 1)) : std::max(c.nmax, 1);  // KB = n: plain per-move update
  return c;
}
// ... and the state where the sweep works on it: walker-major, or (`lw`) the SoA planes with the sweep's scratch.
int lw_setup(pqa_handle* h, bool lw, LwCtx& c) {
  const long W = h->W;
  c = lw_geometry(h, W);
  if (!lw) TRY(sync_aos(h));
  if (lw) {
    if (!h->aos_stale) TRY(lw_from_aos(h));  // (stale walker-major arrays: the planes ARE the state)
    const size_t cf = h->cplx ? 2 : 1;
    TRY(ensure(h, h->b_rbuf, cf * c.KB * std::max(c.nmax, 1) * W * sizeof(double)));
    TRY(ensure(h, h->b_vbuf, cf * c.KB * std::max(c.nmax, 1) * W * sizeof(double)));
    TRY(ensure(h, h->b_act, (size_t)c.KB * W));
  }
  return 0;
}
// The next step's draws on the side stream, behind the sweep that has just been enqueued (the tape set of step + 1 was last read by the sweep
// of step - 1): they run beside this step's energy pass (k_tile_draws: 64 us of Philox + Box-Muller arithmetic at 65 536 walkers, next to
// memory- and latency-bound kernels) instead of in front of the next sweep.
int draws_ahead(pqa_handle* h, uint64_t seed, uint32_t next_step) {
  const long W = h->W;
  const size_t NW = (size_t)h->N * W;
  if (!h->draw.stream) {
    TRY(new_stream(h, &h->draw.stream));
    for (hipEvent_t& e : h->draw.ev) TRY(new_event(h, &e, hipEventDisableTiming));
  }
  DevBuf& bg = (next_step & 1) ? h->draw.b_gauss_b : h->b_gauss;
  DevBuf& bu = (next_step & 1) ? h->draw.b_unif_b : h->b_unif;
  TRY(ensure(h, bg, NW * 3 * sizeof(double)));
  TRY(ensure(h, bu, NW * sizeof(double)));
  HIPCHK(hipEventRecord(h->draw.ev[0], h->stream));
  HIPCHK(hipStreamWaitEvent(h->draw.stream, h->draw.ev[0], 0));
  hipLaunchKernelGGL((k_tile_draws<>), dim3((unsigned)((NW + 255) / 256)), dim3(256), 0, h->draw.stream, seed, next_step, h->N, W, (double*)bg.p, (double*)bu.p);
  HIPCHK(hipEventRecord(h->draw.ev[1], h->draw.stream));
  h->draw.ahead_valid = true; h->draw.ahead_step = next_step; h->draw.ahead_seed = seed; h->draw.ahead_W = W;
  return 0;
}

// Which kernels a sweep of W walkers runs on this handle.  Single-determinant handles (lw_eligible): the resident sweeps where the system
// is in their scope (one launch per sweep, state on chip; they read both tapes, so a call that brings one tape of the two takes the
// launches) — k_sweep_r8 (second generation, open-boundary real handles: pqa_res8.hpp) ahead of k_sweep_res (pqa_res.hpp) — else the
// launch-per-move sweep.  Every other handle: the wave-per-walker kernels, in one launch for small shards (pqa_ww.hpp).  A resident
// sweep's setup runs when the route first asks for it: res_setup never runs on a handle whose sweeps all go to k_sweep_r8.
static int sweep_route(pqa_handle* h, long W, bool tapes_ok, SweepRoute* route) {
  if (!lw_eligible(h)) { *route = ww_eligible(h, W) ? SweepRoute::ww : SweepRoute::ww_launches; return 0; }
  *route = SweepRoute::lw;
  if (!tapes_ok) return 0;
  bool use = false;
  TRY(r8_plan(h, &use));
  if (use) { *route = SweepRoute::r8; return 0; }
  TRY(res_plan(h, W, &use));
  if (use) *route = SweepRoute::res;
  return 0;
}

static bool N_ok(const pqa_handle* h) { return h->N <= 64 && h->natom <= 64 && std::max(h->nup, h->ndn) <= 64; }
// The lane-per-walker routes.  The sweep's draws first, if the call brought no tapes and the route reads them from memory.
static int sweep_electrons_fused(pqa_handle* h, const MoveBuf& mb_in, const LwCtx& lc, SweepRoute route) {
  const long W = h->W;
  MoveBuf mb = mb_in;
  const bool res = route != SweepRoute::lw;
  constexpr long draws_max = 16384;  // walker counts up to which a fused sweep draws its random numbers ahead (k_tile_draws)
  if (!mb.gauss && !mb.unif && (res || W <= draws_max)) {
    // small shards: the sweep's normals and uniforms drawn ahead by one launch from the same Philox streams (k_tile_draws) — in
    // k_step_lw the lead group's Box-Muller pairs are ~600 dependent instructions of every move's chain with one wave per SIMD
    const size_t NW = (size_t)h->N * W;
    // two tape sets, step s in set s & 1: pqa_vmc_sweeps draws step s + 1 on a side stream while step s's energy pass runs (draws_ahead)
    DevBuf& bg = (mb.step & 1) ? h->draw.b_gauss_b : h->b_gauss;
    DevBuf& bu = (mb.step & 1) ? h->draw.b_unif_b : h->b_unif;
    if (h->draw.ahead_valid && h->draw.ahead_step == mb.step && h->draw.ahead_seed == mb.seed && h->draw.ahead_W == W) {
      HIPCHK(hipStreamWaitEvent(h->stream, h->draw.ev[1], 0));
    } else {
      TRY(ensure(h, bg, NW * 3 * sizeof(double)));
      TRY(ensure(h, bu, NW * sizeof(double)));
      hipLaunchKernelGGL((k_tile_draws<>), dim3((unsigned)((NW + 255) / 256)), dim3(256), 0, h->stream, mb.seed, mb.step, h->N, W, (double*)bg.p, (double*)bu.p);
    }
    h->draw.ahead_valid = false;
    h->draw.on_device = true;
    mb.gauss = (const double*)bg.p; mb.unif = (const double*)bu.p;
  }
  if (route == SweepRoute::r8) return sweep_r8(h, mb);
  if (route == SweepRoute::res) return sweep_res(h, mb);
  const int N = h->N, KB = lc.KB, nmax = lc.nmax;
  const LwState L = lw_state(h);
  const int cfi = h->cplx ? 2 : 1, rowlen = cfi * nmax;  // doubles per inverse row
  // thread groups per walker (lc.Gm: ~4 waves per SIMD's worth of threads) and walkers per block: 256 threads at most, so more
  // than 4 groups narrow the block to 32 or 16 walkers — which is also what spreads a small shard over the chip
  int G = std::min(lc.Gm, 16);
  int NW = (G <= 4) ? 64 : 256 / G;
  // small shards (one 16-walker block per CU at most): 32 thread groups per walker — k_step_pre<.., 32>, 512 threads, two Jastrow
  // partners per thread: (H2O)8 step 3.93 -> 3.40 ms at 4096 walkers, 3.38 -> 2.88 at 1024; 64 groups (one partner per thread, 1024
  // threads) spill at the 128-register limit: 4.47 / 3.53 ms.
  if (W <= step_pre_max && N_ok(h) && step_pre_system_ok(h, rowlen) && KB <= 32 / 4) { G = 32; NW = 16; }  // (a block row per quartet of groups)

  auto step = [&](int e_acc, int e_prop) {
    StepArgs a{};
    a.e_acc = e_acc; a.e_prop = e_prop; a.has_jastrow = (int)h->has_jastrow; a.G = G; a.NW = NW; a.W = W; a.w0 = 0; a.w1 = W;
    a.j_skip = e_prop > 0 ? e_prop - 1 : -1;
    if (e_acc >= 0) {
      const int s = e_acc >= h->nup, n_s = s ? h->ndn : h->nup, i_s = e_acc - (s ? h->nup : 0);
      const int q = i_s % KB;
      a.j_lo = i_s - q; a.j_hi = std::min(a.j_lo + KB, n_s);
      a.Rbuf = (double*)h->b_rbuf.p + (size_t)q * cfi * n_s * W;
      a.Vbuf = (double*)h->b_vbuf.p + (size_t)q * cfi * n_s * W;
      a.act = (uint8_t*)h->b_act.p + (size_t)q * W;
    }
    if (h->cplx) launch_step_cx(h, L, mb, a, rowlen); else launch_step_real(h, L, mb, a, rowlen);
  };
  step(-1, 0);
  for (int e = 0; e < N; ++e) {
    const int s = e >= h->nup, n_s = s ? h->ndn : h->nup, i_s = e - (s ? h->nup : 0);
    const int q = i_s % KB, j_lo = i_s - q, j_hi = std::min(j_lo + KB, n_s);
    const bool block_done = (i_s == j_hi - 1);
    const bool need_flush = block_done && (j_hi - j_lo < n_s);
    // the next electron's inverse row is current after this move's commit unless it opens a new block of the SAME spin
    const bool fuse_next = (e + 1 < N) && !(need_flush && i_s + 1 < n_s);
    // ---- orbitals at the proposals: the rows go straight into the slot of electron i_s the walker is not using (accepting
    // flips the selector)
    TRY(launch_orb(h, s, plain_points(mb.newpos, W), W, 5, (double*)h->b_rc[s].p + (size_t)i_s * 2 * W * 5 * h->nmo[s],
                   (const unsigned char*)h->b_sel[s].p + (size_t)i_s * W, (long)W * 5 * h->nmo[s]));
    // ---- decide e, commit, propose e + 1
    hipEvent_t pe1 = nullptr;
    if (h->profile && (e % (4 * (int)prof_stride)) == 1) {  // sparsely sampled full (decide + propose) launches: an event pair costs ~2 us of stream time
      hipEvent_t pe0 = nullptr;
      TRY(prof_acquire(h, h->prof_part, pe0, pe1, fuse_next));  // (without fuse_next the pair is only created)
      if (fuse_next) HIPCHK(hipEventRecord(pe0, h->stream));
    }
    step(e, fuse_next ? e + 1 : -1);
    if (pe1) { HIPCHK(hipEventRecord(pe1, h->stream)); h->prof_part.launches += 1; }
    if (need_flush) {  // block finished: bring every other row of this spin up to date
      const int nq = j_hi - j_lo;
      hipEvent_t ce1 = nullptr;
      if (h->profile && ((j_lo / std::max(KB, 1)) % 4) == 0) {  // every 4th flush of a spin
        hipEvent_t ce0 = nullptr;
        TRY(prof_acquire(h, h->prof_commit, ce0, ce1));
        HIPCHK(hipEventRecord(ce0, h->stream));
      }
      if (h->cplx) launch_flush_cx(h, L, s, W, 0, W, j_lo, j_hi, nq, rowlen, n_s);
      else launch_flush_real(h, L, s, W, 0, W, j_lo, j_hi, nq, rowlen, n_s);
      if (ce1) { HIPCHK(hipEventRecord(ce1, h->stream)); h->prof_commit.launches += 1; }
    }
    if (!fuse_next && e + 1 < N) step(-1, e + 1);
  }
  return 0;
}

// the wave-per-walker kernels on the AoS state, launch by launch: k_propose -> orbitals at the proposals -> k_accept per move
static int sweep_ww_launches(pqa_handle* h, const MoveBuf& mb) {
  const long W = h->W;
  const size_t lds_acc = std::max(lds_sm(h), lds_det(h, 5));
  for (int e = 0; e < h->N; ++e) {
    const int s = e >= h->nup;
    const double* mo = (const double*)h->b_motmp.p;
    if (h->cplx) {
      hipLaunchKernelGGL(k_propose<true>, dim3((unsigned)W), dim3(64), 2 * lds_det(h, 5), h->stream, h->S, h->st, h->js, mb, e,
                         (int)h->has_slater, (int)h->has_jastrow, W);
      if (h->has_slater) TRY(launch_orb(h, s, plain_points(mb.newpos, W), W, 5, (double*)h->b_motmp.p));
      hipLaunchKernelGGL(k_accept<true>, dim3((unsigned)W), dim3(64), 2 * lds_acc, h->stream, h->S, h->st, h->js, mb, e,
                         (int)h->has_slater, (int)h->has_jastrow, mo, W);
      continue;
    }
    hipLaunchKernelGGL(k_propose<false>, dim3((unsigned)W), dim3(64), lds_det(h, 5), h->stream, h->S, h->st, h->js, mb, e,
                       (int)h->has_slater, (int)h->has_jastrow, W);
    if (h->has_slater) TRY(launch_orb(h, s, plain_points(mb.newpos, W), W, 5, (double*)h->b_motmp.p));
    hipLaunchKernelGGL(k_accept<false>, dim3((unsigned)W), dim3(64), lds_acc, h->stream, h->S, h->st, h->js, mb, e, (int)h->has_slater,
                       (int)h->has_jastrow, mo, W);
  }
  return 0;
}

// One proposal per electron, in index order, on the SoA state (the lane-per-walker routes above) or the AoS state with the
// wave-per-walker kernels (multi-determinant, three-body, large complex determinants); mb.dmc selects the DMC variant.
int sweep_electrons(pqa_handle* h, const MoveBuf& mb, const LwCtx& lc) {
  SweepRoute route;
  TRY(sweep_route(h, h->W, (mb.gauss != nullptr) == (mb.unif != nullptr), &route));
  if (h->route.debug && route != h->route.reported) {  // PQA_RES_DEBUG: the kernel a sweep runs, whenever it is not the last sweep's
    static const char* const names[] = {"k_sweep_r8", "k_sweep_res", "k_step_lw", "k_sweep_ww", "k_propose/k_accept"};
    fprintf(stderr, "[pqa] sweep route: %s\n", names[(int)route]);
    h->route.reported = route;
  }
  switch (route) {
    case SweepRoute::ww: return sweep_ww(h, mb);  // small shards: the whole sweep of a walker in one launch, one wave per walker (pqa_ww.hpp)
    case SweepRoute::ww_launches: return sweep_ww_launches(h, mb);
    default: return sweep_electrons_fused(h, mb, lc, route);
  }
}

int step_call_open(pqa_handle* h, StepCall& c, bool from_aos, const char* refused) {
  if (from_aos) TRY(sync_aos(h));
  HIPCHK(hipSetDevice(h->device));
  if (h->W == 0) FAIL("state not initialised (call pqa_wf_recompute)");
  if (c.nsteps <= 0) return 0;
  if (refused) FAIL(refused);
  const long W = c.W = h->W;
  const int N = c.N = h->N;
  h->saved_valid = false;
  const int nmo_max = std::max(std::max(h->nmo[0], h->nmo[1]), 1);
  TRY(ensure(h, h->b_newpos, (size_t)W * 3 * sizeof(double)));
  TRY(ensure(h, h->b_aux, (size_t)W * 8 * sizeof(double)));
  TRY(ensure(h, h->b_accept, (size_t)W));
  TRY(ensure(h, h->b_acccnt, (size_t)c.nsteps * c.nacc * sizeof(int)));
  TRY(ensure(h, h->b_motmp, (size_t)W * 5 * nmo_max * sizeof(double)));
  TRY(ensure(h, h->b_accw, (size_t)W * sizeof(int)));
  HIPCHK(hipMemsetAsync(h->b_acccnt.p, 0, (size_t)c.nsteps * c.nacc * sizeof(int), h->stream));
  HIPCHK(hipMemsetAsync(h->b_accw.p, 0, (size_t)W * sizeof(int), h->stream));
  if (h->S.pbc) {  // wrap counters of this call's accepted moves (pqa_get_wrap)
    TRY(ensure(h, h->b_dwrap, (size_t)W * 3 * sizeof(int)));
    TRY(ensure(h, h->b_wrap, (size_t)W * N * 3 * sizeof(int)));
    HIPCHK(hipMemsetAsync(h->b_wrap.p, 0, (size_t)W * N * 3 * sizeof(int), h->stream));
    h->wrap_W = W;
  }
  if (c.gauss) TRY(ensure(h, h->b_gauss, (size_t)N * W * 3 * sizeof(double)));
  if (c.unif) TRY(ensure(h, h->b_unif, (size_t)N * W * sizeof(double)));
  c.lw = lw_eligible(h);
  return lw_setup(h, c.lw, c.lc);
}
int step_moves(pqa_handle* h, const StepCall& c, int step, MoveBuf& mb) {
  const size_t NW = (size_t)c.N * c.W;
  mb = MoveBuf{};
  mb.newpos = (double*)h->b_newpos.p; mb.aux = (double*)h->b_aux.p; mb.accept = (uint8_t*)h->b_accept.p;
  mb.acc_w = (int*)h->b_accw.p; mb.seed = c.seed; mb.step = (uint32_t)step; mb.tstep = c.tstep;
  if (h->S.pbc && !h->twist) { mb.dwrap = (int*)h->b_dwrap.p; mb.wrap = (int*)h->b_wrap.p; }  // twisted handles keep the walkers unfolded
  if (c.gauss) TRY(copy_in(h, h->b_gauss.p, c.gauss + (size_t)step * NW * 3, NW * 3 * sizeof(double)));
  if (c.unif) TRY(copy_in(h, h->b_unif.p, c.unif + (size_t)step * NW, NW * sizeof(double)));
  mb.gauss = c.gauss ? (const double*)h->b_gauss.p : nullptr;
  mb.unif = c.unif ? (const double*)h->b_unif.p : nullptr;
  return 0;
}

extern "C" int pqa_vmc_sweeps(pqa_handle_t* h, double tstep, int nsteps, const double* gauss, const double* unif, double threshold,
                              const double* ecp_rot, const double* ecp_unif, uint64_t seed, double* acceptance,
                              double* energy_mean, uint8_t* accept_rec) {
  h->dmc.old_valid = false;  // (the state pqa_dmc_continue refers to is gone)
  StepCall call;
  call.nsteps = nsteps; call.tstep = tstep; call.seed = seed; call.gauss = gauss; call.unif = unif;
  const char* refused = "the ECP tapes of pqa_vmc_sweeps have the semi-local integrator's layout: with pqa_set_ecp_batched the draws come from the device streams (replay through pqa_energy)";
  TRY(step_call_open(h, call, false, h->ecpb_on && (ecp_rot || ecp_unif) ? refused : nullptr));
  if (nsteps <= 0) return 0;
  const long W = call.W;
  const bool lw = call.lw;
  const int N = call.N, nen = h->cplx ? 7 : 6;  // energy rows: complex determinants add Im(ecp) = Im(total)
  TRY(ensure(h, h->b_means, (size_t)nsteps * nen * sizeof(double)));
  if (accept_rec) TRY(ensure(h, h->b_accrec, (size_t)N * W));
  const size_t nrot = (size_t)N * std::max(h->necp, 1);
  h->draw.ahead_valid = false;
  for (int step = 0; step < nsteps; ++step) {
    MoveBuf mb;
    TRY(step_moves(h, call, step, mb));
    if (accept_rec) mb.accept_rec = (uint8_t*)h->b_accrec.p;
    h->r8.jsx_current = false;
    h->r8.xaos_next = energy_mean != nullptr && h->necp > 0;  // (consumed by sweep_r8 only)
    h->draw.on_device = false;
    TRY(sweep_electrons(h, mb, call.lc));
    h->r8.xaos_next = false;
    if (h->draw.on_device && energy_mean && step + 1 < nsteps && W >= 16384) TRY(draws_ahead(h, seed, (uint32_t)(step + 1)));
    // small shards: the accepted-move count, the energy rows and their means in one launch at the end of the step (three launches of ~5 us
    // otherwise — 2 % of the 50-determinant molecule's step at 2 048 walkers)
    const bool finish1 = energy_mean && W <= 16384;
    if (!finish1) hipLaunchKernelGGL((k_sum_reset_int<>), dim3(1), dim3(1024), 0, h->stream, (int*)h->b_accw.p, W, (int*)h->b_acccnt.p + step);
    TRY(check_launch(h, "k_propose/k_accept"));
    if (accept_rec) TRY(copy_in(h, accept_rec + (size_t)step * N * W, h->b_accrec.p, (size_t)N * W));
    if (energy_mean) {
      EnergyOpts eo;
      eo.soa_current = lw; eo.aos_T_needed = false; eo.assemble = !finish1;
      TRY(energy_dev(h, threshold, ecp_rot ? ecp_rot + (size_t)step * nrot * 9 : nullptr,
                     ecp_unif ? ecp_unif + (size_t)step * nrot * W : nullptr, seed, (uint32_t)step, eo));
      if (finish1)
        hipLaunchKernelGGL((k_energy_finish<>), dim3(nen + 1), dim3(256), 0, h->stream, (const double*)h->b_kc.p, h->en.d_ecp, h->ii_energy, W,
                           (double*)h->b_en.p, (double*)h->b_means.p + (size_t)step * nen, nen, (int*)h->b_accw.p, (int*)h->b_acccnt.p + step);
      else
        hipLaunchKernelGGL((k_row_means<>), dim3(nen), dim3(256), 0, h->stream, (const double*)h->b_en.p, W, (double*)h->b_means.p + (size_t)step * nen);
      TRY(check_launch(h, "k_row_means"));
    }
  }
  h->aos_stale = lw;  // converted back on demand (sync_aos)
  h->jas_stale = h->has_j2;
  std::vector<int> cnt(nsteps);
  TRY(copy_out(h, cnt.data(), h->b_acccnt.p, (size_t)nsteps * sizeof(int)));
  if (acceptance) {
    std::vector<double> acc(nsteps);
    for (int i = 0; i < nsteps; ++i) acc[i] = (double)cnt[i] / ((double)W * N);
    HIPCHK(hipMemcpy(acceptance, acc.data(), nsteps * sizeof(double), hipMemcpyDefault));
  }
  if (energy_mean) HIPCHK(hipMemcpy(energy_mean, h->b_means.p, (size_t)nsteps * nen * sizeof(double), hipMemcpyDefault));
  return 0;
}
