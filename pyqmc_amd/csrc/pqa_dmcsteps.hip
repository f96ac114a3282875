// pyqmc_amd C ABI implementation (host side): the fused DMC step loop (pqa_dmc_steps: dmc_draws, dmc_scratch, tmove_phase) and the T-move
// entry (pqa_tmoves).
// See include/pyqmc_amd.h for the contract and pqa_internal.hpp for what the units share.
#include "pqa_carver.hpp"
#include "pqa_internal.hpp"
#include "pqa_tmb.hpp"
int scan_ints(pqa_handle* h, const int* c, long* o, long n, long Wm, long* marks) {
  const long nt = (n + 1023) / 1024;
  TRY(ensure(h, h->b_tmtile, (size_t)(nt + 1) * sizeof(long)));
  long* tile = (long*)h->b_tmtile.p;
  hipLaunchKernelGGL((k_scan_local<>), dim3((unsigned)nt), dim3(1024), 0, h->stream, c, o, n, tile);
  hipLaunchKernelGGL((k_scan_tiles<>), dim3(1), dim3(1024), 0, h->stream, tile, nt);
  hipLaunchKernelGGL((k_scan_add<>), dim3((unsigned)nt), dim3(1024), 0, h->stream, o, n, (const long*)tile, nt, Wm, marks);
  return check_launch(h, "k_scan_local/tiles/add");
}

// ---------------------------------------------------------------- fused DMC propagation
DmcDraws dmc_draws(const pqa_handle* h) {
  DmcDraws d{};
  const int necp = h->necp;
  d.batched = necp > 0 && h->ecpb_on;
  d.nsel = d.batched ? h->ecpb_nsel : 0; d.nsr = d.batched ? h->ecpb_nsr : 0;
  d.selu = d.batched && d.nsel < h->ecpb_npoints && d.nsr > 0;
  d.tmoves = necp > 0 && (d.batched ? d.nsel > 0 : h->dmc.tm_P > 0);
  d.nrot = (size_t)h->N * std::max(necp, 1);
  d.nu = d.batched ? (d.selu ? d.nsr : 0) : necp;
  return d;
}
// The scratch of one call in dmc.b_call; B: the T-move buffers (pqa_dmc.hpp), the pointers a call fixes filled in here.  The T-move pieces are
// empty (NULL) on a handle without T-moves, pass or tabpos / tabwgt on the other integrator's, tmu without tapes.  Every piece starts on a 256-byte
// boundary, as the allocation of its own that it used to be did.
struct DmcScratch {
  double *w, *r2, *out;     // [W] weights; [2][W] sum over electrons of |gauss + drift|^2, accepted and proposed; [nsteps][navg] step averages
  TmBuf B;
  long* marks;              // [N + 1] a scan's value at the first (electron, walker) of every electron
  double *tabpos, *tabwgt;  // [N][W][nsel][3], [N][W][nsel] the dense table of a step (batched integrator)
  double *uold, *tmu;       // [N][W] U_e of every electron at its position (k_tm_uold); this step's tm_u1 [N][W], tm_u2 [N][W], tm_unif [N W nu]
};
static size_t dmc_scratch(Carver c, const pqa_handle* h, const StepCall& call, const DmcDraws& d, bool tapes, DmcScratch& s) {
  auto piece = [&c](auto*& p, size_t n) { p = n ? c.take<std::remove_reference_t<decltype(*p)>>(n) : nullptr; c.off = (c.off + 255) & ~(size_t)255; };
  const size_t W = (size_t)call.W, NW = d.tmoves ? (size_t)call.N * W : 0, nkw = (std::max(h->necp, 1) + 63) / 64;
  piece(s.w, W);
  piece(s.r2, 2 * W);
  piece(s.out, (size_t)call.nsteps * (h->cplx ? 8 : 7));
  piece(s.B.cnt, NW);
  piece(s.B.off, NW ? NW + 1 : 0);
  piece(s.B.pass, d.batched ? 0 : NW * nkw);
  piece(s.tabpos, NW * d.nsel * 3);
  piece(s.tabwgt, NW * d.nsel);
  piece(s.B.acc, NW);
  piece(s.B.acc_off, NW ? NW + 1 : 0);
  piece(s.marks, NW ? (size_t)call.N + 1 : 0);
  piece(s.B.acc_idx, NW);
  piece(s.B.acc_pos, NW * 3);
  piece(s.uold, NW);
  piece(s.tmu, tapes ? (2 + d.nu) * NW : 0);
  if (s.tmu) { s.B.u1 = s.tmu; s.B.u2 = s.tmu + NW; s.B.unif = d.nu ? s.tmu + 2 * NW : nullptr; }
  return c.size();
}

// ---- the T-move phase of a step (dmc.py:157-175)
// Front end: the candidates of every (electron, walker), electron-major — counts B.cnt, their scan B.off, eoff the first candidate of every
// electron, and the lists B.pts / B.wgt / B.ptw.  Semi-local integrator: k_tm_count / k_tm_fill.  Batched: every electron's selected
// points (k_ecpb_fill, T-move mode), then the slots that carry a weight (pqa_tmb.hpp).
static int tm_candidates(pqa_handle* h, const StepCall& call, const DmcDraws& d, DmcScratch& s, bool tapes, std::vector<long>& eoff) {
  TmBuf& B = s.B;
  const long W = call.W;
  const int N = call.N;
  const dim3 gw256((unsigned)((W + 255) / 256)), gtmb((unsigned)((W + PQA_TMB_WB - 1) / PQA_TMB_WB));
  if (d.batched) {
    launch_tmb_table(h, B.rot, (tapes && d.selu) ? B.unif : nullptr, call.seed, B.step, call.tstep, s.tabpos, s.tabwgt);
    hipLaunchKernelGGL((k_tmb_count<>), gtmb, dim3(64 * PQA_TMB_WB), 0, h->stream, (const double*)s.tabwgt, N, d.nsel, W, B.cnt);
    TRY(check_launch(h, "k_ecpb_fill/k_tmb_count"));
  } else {
    hipLaunchKernelGGL((k_tm_count<>), dim3(gw256.x, (unsigned)N), dim3(256), 0, h->stream, h->S, h->js, B, W);
    TRY(check_launch(h, "k_tm_count"));
  }
  TRY(scan_ints(h, (const int*)B.cnt, B.off, (long)N * W, W, s.marks));
  TRY(copy_out(h, eoff.data(), s.marks, eoff.size() * sizeof(long)));
  const long tot = eoff[N];
  if (tot == 0) return 0;
  TRY(ensure(h, h->b_tpos, (size_t)tot * 3 * sizeof(double)));
  TRY(ensure(h, h->b_twgt, (size_t)tot * sizeof(double)));
  TRY(ensure(h, h->dmc.b_amp, (size_t)tot * 2 * sizeof(double)));
  TRY(ensure(h, h->dmc.b_ptw, (size_t)tot * sizeof(int)));
  B.pts = (double*)h->b_tpos.p; B.wgt = (double*)h->b_twgt.p; B.amp = (double*)h->dmc.b_amp.p; B.rat = B.amp + tot;
  B.ptw = (int*)h->dmc.b_ptw.p;
  if (d.batched) {
    hipLaunchKernelGGL((k_tmb_compact<>), gtmb, dim3(64 * PQA_TMB_WB), 0, h->stream, (const double*)s.tabpos, (const double*)s.tabwgt, N, d.nsel, W,
                       (const long*)B.off, B.pts, B.wgt, B.ptw);
    return check_launch(h, "k_tmb_compact");
  }
  hipLaunchKernelGGL((k_tm_fill<>), dim3((unsigned)W, (unsigned)N), dim3(64), 0, h->stream, h->S, h->js, B, W);
  return check_launch(h, "k_tm_fill");
}
// Back end, the same for both integrators: orbital rows at the candidates, their ratios, one heat-bath choice per (electron, walker) in electron
// order (k_tm_walker), and the accepted moves' orbital rows into the cache.  eoff comes in as the candidates' marks; *accepted: moves made.
static int tm_moves(pqa_handle* h, const StepCall& call, const DmcScratch& s, int step, std::vector<long>& eoff, long* accepted) {
  const TmBuf& B = s.B;
  const long W = call.W;
  const int N = call.N, nmo_max = std::max(std::max(h->nmo[0], h->nmo[1]), 1);
  const bool lw = call.lw;
  const size_t NW = (size_t)N * W;
  const dim3 gw256((unsigned)((W + 255) / 256));
  const long tot = eoff[N], tot_up = eoff[h->nup];
  const long cnt_s[2] = {tot_up, tot - tot_up}, base_s[2] = {0, tot_up};
  if (h->has_slater)
    for (int sp = 0; sp < 2; ++sp) {
      if (cnt_s[sp] == 0) continue;
      TRY(ensure(h, h->b_emo[sp], (size_t)cnt_s[sp] * nmo_max * sizeof(double)));
      TRY(launch_orb(h, sp, plain_points(B.pts + 3 * base_s[sp], cnt_s[sp]), cnt_s[sp], 1, (double*)h->b_emo[sp].p));
    }
  // ratios of all candidates against the state before the first T-move: one thread per candidate (k_tm_ratio)
  const bool pre = h->ndet == 1 && !h->has_j3 && !h->cplx;
  // U_e of every electron at its current position: from the second step of a call on, the energy evaluation that closed the
  // previous step left exactly that ([N][W], k_kinetic_lw) — the walkers have not moved since
  const double* d_uold = nullptr;
  if (pre && h->has_jastrow) {
    if (lw && step > 0 && h->has_j2 && !h->has_j3) d_uold = (const double*)h->b_kpart.p + (size_t)4 * NW;
    else {
      hipLaunchKernelGGL((k_tm_uold<>), dim3(gw256.x, (unsigned)N), dim3(256), 0, h->stream, h->S, h->js, B, W, s.uold);
      d_uold = s.uold;
    }
  }
  if (pre)
    for (int sp = 0; sp < 2; ++sp) {
      if (cnt_s[sp] == 0) continue;
      const dim3 g((unsigned)((cnt_s[sp] + 255) / 256));
      hipLaunchKernelGGL((k_tm_ratio<>), g, dim3(256), 0, h->stream, h->S, h->st, h->js, B, sp, (int)h->has_slater, (int)h->has_jastrow,
                         (const double*)h->b_emo[sp].p, base_s[sp], cnt_s[sp], W, d_uold);
    }
  const size_t lds_tm = std::max(lds_sm(h), lds_det(h, 1));
  if (h->cplx) hipLaunchKernelGGL(k_tm_walker<true>, dim3((unsigned)W), dim3(64), 2 * lds_tm, h->stream, h->S, h->st, h->js, B, (int)h->has_slater,
                                  (int)h->has_jastrow, (const double*)h->b_emo[0].p, (const double*)h->b_emo[1].p, tot_up, W, 0);
  else hipLaunchKernelGGL(k_tm_walker<false>, dim3((unsigned)W), dim3(64), lds_tm, h->stream, h->S, h->st, h->js, B, (int)h->has_slater,
                          (int)h->has_jastrow, (const double*)h->b_emo[0].p, (const double*)h->b_emo[1].p, tot_up, W, pre ? 1 : 0);
  TRY(check_launch(h, "k_tm_walker"));
  TRY(scan_ints(h, (const int*)B.acc, B.acc_off, (long)NW, W, s.marks));
  hipLaunchKernelGGL((k_tm_gather<>), dim3((unsigned)((NW + 255) / 256)), dim3(256), 0, h->stream, B, (const double*)h->js.x, N, W);
  TRY(check_launch(h, "k_tm_gather"));
  TRY(copy_out(h, eoff.data(), s.marks, eoff.size() * sizeof(long)));
  const long nacc[2] = {eoff[N], eoff[h->nup]};
  *accepted = nacc[0];
  if (!h->has_slater) return 0;
  // gradient / Laplacian rows of the moved electrons, one launch per spin
  const long na_s[2] = {nacc[1], nacc[0] - nacc[1]}, a0_s[2] = {0, nacc[1]};
  for (int sp = 0; sp < 2; ++sp) {
    if (na_s[sp] == 0) continue;
    TRY(ensure(h, h->b_emo[sp], (size_t)na_s[sp] * 5 * nmo_max * sizeof(double)));
    TRY(launch_orb(h, sp, plain_points(B.acc_pos + 3 * a0_s[sp], na_s[sp]), na_s[sp], 5, (double*)h->b_emo[sp].p));
    hipLaunchKernelGGL((k_tm_cache<>), dim3((unsigned)na_s[sp]), dim3(64), 0, h->stream, h->S, h->st, (const int*)(B.acc_idx + a0_s[sp]),
                       (const double*)h->b_emo[sp].p, sp, W, lw ? (double*)h->b_rc[sp].p : (double*)nullptr, lw ? (const uint8_t*)h->b_sel[sp].p : (const uint8_t*)nullptr);
  }
  return check_launch(h, "k_tm_cache");
}
// This step's rotations and uniforms (the tapes' slices, or k_gen_rot and the kernels' own Philox streams), the candidates, the moves.
static int tmove_phase(pqa_handle* h, const StepCall& call, const DmcDraws& d, DmcScratch& s, int step, const pqa_dmc_tapes_t* tp, long* accepted) {
  TmBuf& B = s.B;
  const size_t NW = (size_t)call.N * call.W, nrot = d.nrot;
  B.step = (uint32_t)step; B.pts = B.wgt = B.amp = B.rat = nullptr; B.ptw = nullptr;  // (the lists: sized by this step's candidates)
  if (tp) {
    TRY(copy_in(h, h->b_rot.p, tp->tm_rot + (size_t)step * nrot * 9, nrot * 9 * sizeof(double)));
    TRY(copy_in(h, s.tmu, tp->tm_u1 + (size_t)step * NW, NW * sizeof(double)));
    TRY(copy_in(h, s.tmu + NW, tp->tm_u2 + (size_t)step * NW, NW * sizeof(double)));
    TRY(copy_in(h, s.tmu + 2 * NW, tp->tm_unif + (size_t)step * NW * d.nu, NW * d.nu * sizeof(double)));
  } else {
    hipLaunchKernelGGL((k_gen_rot<>), dim3((unsigned)((nrot + 63) / 64)), dim3(64), 0, h->stream, (int)nrot, call.seed ^ 0x9E3779B97F4A7C15ull,
                       (uint32_t)step, (double*)h->b_rot.p);
    TRY(check_launch(h, "k_gen_rot"));
  }
  B.rot = (const double*)h->b_rot.p;
  HIPCHK(hipMemsetAsync(B.acc, 0, NW * sizeof(int), h->stream));
  std::vector<long> eoff((size_t)call.N + 1);
  TRY(tm_candidates(h, call, d, s, tp != nullptr, eoff));
  return eoff[call.N] > 0 ? tm_moves(h, call, s, step, eoff, accepted) : 0;
}
// What pqa_dmc_steps refuses about its arguments (nullptr: nothing).
static const char* dmc_refused(const pqa_handle* h, const DmcDraws& d, const pqa_dmc_tapes_t* tp, bool null_argument) {
  if (null_argument) return "pqa_dmc_steps: weights / step_avg / step_acc must not be NULL";
  if (!tp) return nullptr;
  if (!tp->gauss || !tp->unif) return "pqa_dmc_steps: a tape set needs gauss and unif";
  if (h->necp > 0 && (!tp->ecp_rot || (d.nu > 0 && !tp->ecp_unif))) return "pqa_dmc_steps: a tape set needs ecp_rot and ecp_unif for ECP systems";
  if (d.tmoves && (!tp->tm_rot || (d.nu > 0 && !tp->tm_unif) || !tp->tm_u1 || !tp->tm_u2)) return "pqa_dmc_steps: a tape set needs the four T-move tapes";
  return nullptr;
}

// nsteps steps of dmc_propagate (pyqmc/method/dmc.py:123-221) without leaving the device: T-moves, drift-diffusion with
// fixed-node rejection, local energy, weight update, weighted step averages.  Walker-per-wave kernels (the AoS state).
extern "C" int pqa_dmc_steps(pqa_handle_t* h, double tstep, int nsteps, double branchcut, double e_trial, double e_est, double threshold,
                             double* weights, const pqa_dmc_tapes_t* tp, uint64_t seed, double* step_avg, double* step_acc) {
  const DmcDraws d = dmc_draws(h);
  StepCall call;
  call.nsteps = nsteps; call.nacc = 2; call.tstep = tstep; call.seed = seed;
  if (tp) { call.gauss = tp->gauss; call.unif = tp->unif; }  // (a tape set always brings both)
  TRY(step_call_open(h, call, true, dmc_refused(h, d, tp, !weights || !step_avg || !step_acc)));
  if (nsteps <= 0) return 0;
  const int navg = h->cplx ? 8 : 7;  // numbers per step in step_avg (complex: + the weighted mean of Im ecp = Im total)
  const long W = call.W;
  const int N = call.N, necp = h->necp;
  const bool lw = call.lw;
  DmcScratch s{};
  TRY(ensure(h, h->dmc.b_call, dmc_scratch(Carver(), h, call, d, tp != nullptr, s)));
  dmc_scratch(Carver(h->dmc.b_call.p), h, call, d, tp != nullptr, s);
  TRY(ensure(h, h->dmc.b_old, (size_t)2 * W * sizeof(double)));
  if (d.tmoves) TRY(ensure(h, h->b_rot, d.nrot * 9 * sizeof(double)));
  HIPCHK(hipMemsetAsync(s.r2, 0, (size_t)2 * W * sizeof(double), h->stream));
  TRY(copy_in(h, s.w, weights, (size_t)W * sizeof(double)));
  const dim3 gw256((unsigned)((W + 255) / 256));
  double* eold = (double*)h->dmc.b_old.p;
  std::vector<long> tm_accepted((size_t)nsteps, 0);
  // the tapes of energy evaluation i (0: the starting configuration): rotations (N, necp, 3, 3) and N W nu uniforms
  auto ecp_rot = [&](int i) { return (tp && necp) ? tp->ecp_rot + (size_t)i * d.nrot * 9 : nullptr; };
  auto ecp_unif = [&](int i) { return (tp && d.nu > 0) ? tp->ecp_unif + (size_t)i * N * W * d.nu : nullptr; };
  // energy of the starting configuration (dmc.py:146-149) — or, after pqa_dmc_continue, the energies the previous call's last step
  // left in eold / v2old: what the reference itself carries from step to step (dmc.py:148-149, :199-200)
  const bool cont = h->dmc.cont;
  h->dmc.cont = false;
  if (cont && !(h->dmc.old_valid && h->dmc.old_W == W)) FAIL("pqa_dmc_continue: no previous pqa_dmc_steps call on the resident walkers' state");
  if (!cont) {
    TRY(energy_dev(h, threshold, ecp_rot(0), ecp_unif(0), seed, 0u));
    hipLaunchKernelGGL((k_dmc_keep<>), gw256, dim3(256), 0, h->stream, (const double*)h->b_en.p, eold, eold + W, W);
  }
  s.B.quad = h->d_quad; s.B.seed = seed; s.B.tau = tstep; s.B.threshold = threshold; s.B.nofold = h->twist ? 1 : 0;
  for (int step = 0; step < nsteps; ++step) {
    if (d.tmoves) TRY(tmove_phase(h, call, d, s, step, tp, &tm_accepted[step]));
    MoveBuf mb;
    TRY(step_moves(h, call, step, mb));
    mb.dmc = 1; mb.r2_acc = s.r2; mb.r2_prop = s.r2 + W;
    if (lw && d.tmoves) TRY(lw_from_aos(h, false));  // the T-moves worked on the AoS coordinates and inverses
    TRY(sweep_electrons(h, mb, call.lc));
    hipLaunchKernelGGL((k_sum_reset_int<>), dim3(1), dim3(1024), 0, h->stream, (int*)h->b_accw.p, W, (int*)h->b_acccnt.p + 2 * step);
    TRY(check_launch(h, "k_propose/k_accept (dmc)"));
    EnergyOpts eo;
    eo.soa_current = lw;  // (aos_T_needed: the next step's T-moves)
    TRY(energy_dev(h, threshold, ecp_rot(step + 1), ecp_unif(step + 1), seed, (uint32_t)(step + 1), eo));
    hipLaunchKernelGGL((k_dmc_weights<>), gw256, dim3(256), 0, h->stream, (const double*)h->b_en.p, eold, eold + W, s.r2, s.r2 + W, s.w, tstep, branchcut,
                       e_trial, e_est, N, W);
    hipLaunchKernelGGL((k_dmc_averages<>), dim3(1), dim3(1024), 0, h->stream, (const double*)h->b_en.p, (const double*)s.w, W,
                       s.out + (size_t)step * navg, h->cplx ? 7 : 6);
    TRY(check_launch(h, "k_dmc_weights/k_dmc_averages"));
  }
  if (lw) TRY(lw_to_aos(h, true));
  h->jas_stale = h->has_j2;
  std::vector<int> cnt((size_t)nsteps * 2);
  TRY(copy_in(h, step_avg, s.out, (size_t)nsteps * navg * sizeof(double)));
  TRY(copy_in(h, weights, s.w, (size_t)W * sizeof(double)));
  TRY(copy_out(h, cnt.data(), h->b_acccnt.p, cnt.size() * sizeof(int)));
  for (int i = 0; i < nsteps; ++i) {
    step_acc[2 * i] = (double)cnt[2 * i] / ((double)W * N);
    step_acc[2 * i + 1] = (double)tm_accepted[i] / ((double)W * N);
  }
  h->dmc.old_valid = true; h->dmc.old_W = W;
  return 0;
}

extern "C" int pqa_dmc_continue(pqa_handle_t* h, int on) {
  h->dmc.cont = on != 0;
  return 0;
}

extern "C" int pqa_dmc_can_continue(pqa_handle_t* h) { return (h->dmc.old_valid && h->dmc.old_W == h->W) ? 1 : 0; }

extern "C" int pqa_tmove_npoints(pqa_handle_t* h) { return h->dmc.tm_P; }

extern "C" int pqa_tmoves(pqa_handle_t* h, int e, double tau, double threshold, const double* rot, const double* unif,
                          double* ratio, double* weight, double* pos) {
  TRY(sync_aos(h));
  HIPCHK(hipSetDevice(h->device));
  if (h->cplx && ratio) FAIL("pqa_tmoves: complex orbitals — pass ratio = NULL (positions and weights only) and take the ratios from pqa_wf_testvalue");
  if (h->W == 0) FAIL("state not initialised (call recompute)");
  if (e < 0 || e >= h->N) FAIL("electron index out of range");
  const long W = h->W;
  const int P = h->dmc.tm_P, s = e >= h->nup;
  if (P == 0) return 0;
  if (!rot || !unif) FAIL("pqa_tmoves needs the rotation and mask-uniform tapes");
  h->saved_valid = false;
  const size_t np = (size_t)W * P;
  TRY(ensure(h, h->b_rot, (size_t)h->necp * 9 * sizeof(double)));
  TRY(ensure(h, h->b_eunif, (size_t)h->necp * W * sizeof(double)));
  TRY(ensure(h, h->b_tpos, np * 3 * sizeof(double)));
  TRY(ensure(h, h->b_twgt, np * sizeof(double)));
  TRY(ensure(h, h->b_tlive, np));
  TRY(ensure(h, h->b_trat, np * sizeof(double)));
  TRY(copy_in(h, h->b_rot.p, rot, (size_t)h->necp * 9 * sizeof(double)));
  TRY(copy_in(h, h->b_eunif.p, unif, (size_t)h->necp * W * sizeof(double)));
  hipLaunchKernelGGL((k_tmove_points<>), dim3((unsigned)W), dim3(64), 0, h->stream, h->S, h->js, e, tau, threshold,
                     (const double*)h->b_rot.p, (const double*)h->b_eunif.p, (const double*)h->d_quad, (const int*)h->dmc.d_ptk,
                     (const int*)h->dmc.d_pti, P, W, (double*)h->b_tpos.p, (double*)h->b_twgt.p, (uint8_t*)h->b_tlive.p);
  TRY(check_launch(h, "k_tmove_points"));
  if (!ratio) {  // candidate positions and weights only (dead candidates carry weight 0)
    TRY(copy_in(h, weight, h->b_twgt.p, np * sizeof(double)));
    return copy_out(h, pos, h->b_tpos.p, np * 3 * sizeof(double));
  }
  if (h->has_slater) {
    TRY(ensure(h, h->b_motmp, np * std::max(h->nmo[s], 1) * sizeof(double)));
    TRY(launch_orb(h, s, plain_points((const double*)h->b_tpos.p, (long)np), (long)np, 1, (double*)h->b_motmp.p));
  }
  hipLaunchKernelGGL((k_tmove_ratio<>), dim3((unsigned)W), dim3(64), lds_det(h, 1), h->stream, h->S, h->st, h->js, e, (int)h->has_slater,
                     (int)h->has_jastrow, (const double*)h->b_motmp.p, (const double*)h->b_tpos.p, (const uint8_t*)h->b_tlive.p, P,
                     (double*)h->b_trat.p);
  TRY(check_launch(h, "k_tmove_ratio"));
  TRY(copy_in(h, ratio, h->b_trat.p, np * sizeof(double)));
  TRY(copy_in(h, weight, h->b_twgt.p, np * sizeof(double)));
  return copy_out(h, pos, h->b_tpos.p, np * 3 * sizeof(double));
}

// ---------------------------------------------------------------- measurement
