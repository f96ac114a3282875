// Host-side internals shared by every translation unit of libpyqmc_amd.so (the UNITS of __graft_entry__.py): the handle, the
// error macros, the helpers through which the handle allocates and records what it owns, and the functions one unit calls in
// another.  pqa_create.hip builds and destroys the handle, pqa_capi.hip holds the protocol entry points and the walker state,
// pqa_orb*.hip / pqa_sweep*.hip / pqa_res*.hip / pqa_energy.hip / pqa_dmcsteps.hip the fused paths, the remaining units one
// estimator each.  The device code lives in the kernel headers; every kernel has internal linkage, so a unit only compiles what
// it launches.
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <array>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "../../include/pyqmc_amd.h"
#include "pqa_ao.hpp"
#include "pqa_common.hpp"
#include "pqa_cslater.hpp"
#include "pqa_dmc.hpp"
#include "pqa_energy.hpp"
#include "pqa_ecp.hpp"
#include "pqa_ecpb.hpp"
#include "pqa_jastrow.hpp"
#include "pqa_lw.hpp"
#include "pqa_slater.hpp"
#include "pqa_res.hpp"
#include "pqa_res8_tab.hpp"
#include "pqa_dm.hpp"
#include "pqa_vmc.hpp"

struct DevBuf {
  void* p = nullptr;
  size_t cap = 0;
};

// launch profiler: a pool of event pairs around sampled launches (prof_acquire), their elapsed time summed on demand (prof_drain)
struct ProfSet {
  std::vector<std::pair<hipEvent_t, hipEvent_t>> ev;
  size_t used = 0;
  long launches = 0;
  double ms = 0.0;
};

struct ChunkHost {
  std::vector<int> nk, row0;
  std::vector<int> shell_kb, shell_chunk;  // per shell: first tile row inside its chunk, chunk index
  std::vector<int> cw_off[3], cw_shell[3];  // shell lists per (chunk, lane group) for 4, 8 and 16 groups
  int rows_pad = 0;
};

// which kernels a sweep over the electrons runs (sweep_route, pqa_sweep.hip)
enum class SweepRoute { none = -1, r8, res, lw, ww, ww_launches };

struct pqa_handle {
  int device = 0;
  hipStream_t stream = nullptr;
  std::string err;
  // What the handle allocates it records here (ensure, upload_table, new_event, new_stream, new_pinned below), and pqa_destroy
  // frees the records: nothing is freed by name.  streams[0] is `stream`.
  std::vector<void*> owned;   // table allocations
  std::vector<DevBuf*> bufs;  // the DevBuf fields that hold an allocation
  std::vector<hipEvent_t> events;
  std::vector<hipStream_t> streams;
  std::vector<void*> pinned;
  // host copies needed after create
  int natom = 0, nup = 0, ndn = 0, N = 0, nao = 0, nshell = 0;
  int nmo[2] = {0, 0}, nt[2] = {1, 1}, ndet = 1, ndet_s[2] = {1, 1};
  int na = 0, nb = 0, necp = 0;
  bool aos_stale = false;  // the lane-per-walker planes hold the live state; the walker-major arrays are converted back on demand (sync_aos)
  int pbc_maxcls = PQA_PRE_NCUT;  // most distinct shell cut-offs any atom has (picks the pre-pass instantiation)
  int pbc_nw = 2;  // words per (atom, point) of the sorted image lists k_pbc_prepass writes (4 entries each)
  bool orb_general = false;  // PQA_ORB_GENERAL=1: big open handles evaluate orbitals by k_ao + k_mo_rows instead of the windowed k_orb (A/B, tests)
  bool invert_attr = false;  // k_build_invert's dynamic-LDS limit raised (n > 90)
  bool big = false;         // more than 64 electrons or orbitals of a spin: general orbital path, wave-per-walker kernels (pqa_create)
  bool pbc_high_l = false;  // a periodic cell with g / h shells: orbitals through k_ao<.., 5> + k_mo_rows (pqa_orb_pbc.hip)
  bool twist = false;  // twisted boundary conditions: complex lattice-summed AOs, unfolded positions (include/pyqmc_amd.h)
  bool cplx = false;  // complex orbitals: mo_* hold [Re C | Im C], see pqa_cslater.hpp
  bool has_slater = false, has_jastrow = false;  // has_jastrow: any Jastrow factor (two- and/or three-body)
  bool has_j2 = false, has_j3 = false;
  int na3 = 0, nb3 = 0;
  double* d_c3 = nullptr;
  DevBuf b_j3u;
  double ii_energy = 0.0;
  EwaldDev ew{};  // periodic Coulomb tables (pqa_set_ewald)
  bool ew_set = false;
  std::vector<int> shell_l, shell_np, shell_ao;
  int lmax = 0;  // highest l of the basis (picks the LMAX instantiation of the sweeps)
  std::vector<int> rt_shells;  // [nshell][2] host copy of SysDev::shell_rt (radial tables of the contracted shells)
  double rt_err = 0.0;         // largest table error found at create, relative to sum |c| a^k
  std::vector<int> shell_cost;  // phase-1 cost model of a shell (shell_costs): balances the lane groups of the orbital kernels
  SysDev S{};
  ChunkHost chunks[2];  // [0]: KC=16 (5 components), [1]: KC=32 (value only)
  ChunkTab tab[2]{};
  const unsigned char* out_sel = nullptr;  // two-slot output of the NEXT orbital launch (ChunkTab::out_sel; set by launch_orb)
  long out_slot_stride = 0;
  int orb_col0 = 0;  // first orbital column of the NEXT k_orb launch (ChunkTab::col0; set by launch_orb for handles with > 64 orbitals)
  double* d_mo[2] = {nullptr, nullptr};       // [nao][nmo]
  double* d_cpad[2][2] = {{nullptr, nullptr}, {nullptr, nullptr}};  // [tab][spin]
  double *d_acoeff = nullptr, *d_bcoeff = nullptr, *d_detcoeff = nullptr, *d_quad = nullptr, *d_quadw = nullptr;
  int *d_ecp_naip = nullptr, *d_ecp_qoff = nullptr;  // per-atom quadrature rule (pqa_set_ecp_naip)
  int ecp_naip = 0;                                  // 0: the reference's default, 6 or 12 by channel count
  std::vector<int> ecp_nch;                          // channels (incl. local) of every ECP atom
  // batched ECP integrator (pqa_set_ecp_batched, pqa_ecpb.hpp): per-atom point counts, table size, selections, slots per electron
  int ecpb_on = 0, ecpb_npoints = 0, ecpb_nsd = 0, ecpb_nsr = 0, ecpb_nsel = 0;
  int *d_ecpb_naip = nullptr, *d_ecpb_qoff = nullptr, *d_ecpb_pstart = nullptr;
  double *d_aq = nullptr, *d_bq = nullptr;  // merged Pade numerators (jas_merge_tables); jas_merge: PQA_JAS_MERGE=0 keeps the function-by-function route (A/B)
  int jas_merge = 1;
  // walker state
  long W = 0;
  SlaterState st{};
  JastrowState js{};
  DevBuf b_x, b_T[2], b_dsign[2], b_dlog[2], b_cache[2], b_aval, b_bval;
  DevBuf b_alt_x, b_alt_T[2], b_alt_dsign[2], b_alt_dlog[2], b_alt_cache[2], b_alt_aval, b_alt_bval, b_alt_j3u, b_rsidx;  // pqa_resample's other halves
  // scratch
  DevBuf b_pts, b_motmp, b_out, b_widx, b_mask, b_ao, b_flag, b_newpos, b_aux, b_accept, b_accrec, b_acccnt, b_accw, b_dwrap, b_wrap, b_epass, b_eptw[2], b_econ[2], b_eu0[2], b_tves, b_pgdet, b_pbcd0, b_pbcmask, b_pbcth;
  int* d_colmap[2] = {nullptr, nullptr};  // [ndet_s][nmo_s] column of an orbital in a unique determinant, or -1
  int jas_fold_allowed = 1;  // PQA_JAS_FOLD=0: Voronoi reduction in every periodic Jastrow pair (A/B, bitwise check)
  int ecp_nchan = 0, ecp_nterm = 0;
  long wrap_W = 0;
  DevBuf b_gauss, b_unif, b_kc, b_en, b_means, b_sign, b_log, b_ju;
  // value-only orbitals of each spin at a walker chunk of points: pqa_s2 (at the other spin's electrons), pqa_symmetry (at the
  // spin's transformed electrons)
  DevBuf b_orbphi[2];
  DevBuf b_s2out;  // pqa_s2 (pqa_s2.hip): outputs
  DevBuf b_tbpts;  // pqa_tbdm_sweep (pqa_tbdm.hip): the auxiliary points of a walker chunk, gathered from the evaluator handle
  DevBuf b_j3dm;   // k_j3_moves (pqa_j3dm.hpp): the three-body differences of a walker chunk
  // pqa_symmetry (pqa_symmetry.hip), per walker chunk: transformed coordinates, determinant ratios (sign, log) of each spin; the
  // ratios of every operator
  DevBuf b_symx, b_symdet[2], b_symout;
  // pqa_sq (pqa_sq.hip): q vectors and their integer coordinates, per-walker values of a walker chunk, the mean mode's row partials and
  // running sums
  DevBuf b_sqq, b_sqout, b_sqpart, b_sqacc;
  // pqa_ewald2d (pqa_ewald2d.hip): the call's tables, per-walker values of a walker chunk, the mean mode's partial sums
  DevBuf b_e2tab, b_e2out, b_e2acc;
  // Gaussian-process Jastrow factor (pqa_gps.hip), a state of its own beside the walker state above: support points (nsup, 2, 3)
  // followed by alpha (nsup); the unit's own walkers (gps_W, N, 3), e [gps_W][N][2 nsup] and S [gps_W][2 nsup].  Per-call inputs and
  // outputs go through the common scratch above (pqa_stage.hpp, b_out).  gps_nsup == 0: pqa_gps_set has not run; gps_W == 0: no recompute yet
  DevBuf b_gps_par, b_gps_x, b_gps_e, b_gps_s;
  int gps_nsup = 0;
  double gps_f = 0.0;
  long gps_W = 0;
  // AO-pair (geminal) Jastrow factor (pqa_geminal.hip), a state of its own as the one above: the symmetric G (nao, nao); the unit's
  // own walkers (gem_W, N, 3), their AO values A [gem_W][N][nao] and sums T [gem_W][nao]; the value plane a mode-1 evaluation kept
  // for the update that follows it; per-call scratch of its own: AO planes, the rows h = (T - a_e) G (inputs and outputs go through the
  // common scratch above: pqa_stage.hpp, b_pts for gcoeff, b_out).  gem_set: pqa_geminal_set has run; gem_W == 0: no recompute yet
  DevBuf b_gem_g, b_gem_x, b_gem_a, b_gem_t, b_gem_saved, b_gem_ao, b_gem_h;
  bool gem_set = false, gem_saved_valid = false;
  int gem_saved_e = -1;
  long gem_W = 0;
  // pqa_overlap_sweeps (pqa_overlap.hip), on the first handle of the call: one sweep's tapes, the old-position drift, acceptance counts,
  // the (K, K, W) weights and the per-sweep overlaps; pinned words the vanished-determinant flags of all K handles come back in
  DevBuf b_ovl;
  int* pin_ovl = nullptr;
  hipEvent_t ovl_ev = nullptr;                  // pqa_overlap_sweeps / pqa_add_sweeps: the flags of an electron move have reached pin_ovl
  // pqa_add_* (pqa_add.hip), on the first handle of the call: one sweep's tapes, the (K, W) weights, the old-position drift, acceptance
  // counts and per-sweep fractions; or the weights and the six combined energy rows
  DevBuf b_add;
  // pqa_sr_moments / pqa_sr_moments_orb (pqa_sr.hip): the running moments, energy means, weights, a walker chunk's gathered matrix and
  // scales, the slices' partial tiles, the column description and the orbital columns' inverse map
  DevBuf b_sr;
  // pqa_obdm_sweeps (pqa_obdm.hip), on the evaluator's handle in the mean mode: a walker chunk's panels T, B and norm terms, the slices'
  // partial tiles, the running sums and their scaled copy
  DevBuf b_obdm;
  hipEvent_t tb_ev[2] = {nullptr, nullptr};     // pqa_tbdm_sweep / pqa_obdm_sweeps: a chunk's ratios produced / consumed
  hipEvent_t tune_ev[2] = {nullptr, nullptr};   // periodic k_orb: timing of the tile-size trials (tp_tune)
  DevBuf b_tpos, b_twgt, b_tlive, b_trat;  // pqa_tmoves: candidates of one electron; the first two also the candidate lists of a DMC step
  DevBuf b_tmtile, b_tmmarks;  // scan_ints: tile sums; the marks of the energy pass's scans
  // DMC (pqa_dmc_steps, pqa_dmcsteps.hip).  cont (pqa_dmc_continue): the next call starts from the energies its predecessor's last step left in
  // b_old [2][W] (local energy, |v|^2), which therefore outlives the call; old_valid / old_W: the resident state is still the one that call
  // ended with.  tm_P, d_ptk, d_pti: T-move points of the semi-local integrator over all ECP atoms, their atom and index in the atom's rule.
  // b_call: every piece whose size the call's W, N, nsteps, necp and nsel fix, laid out by dmc_scratch (pqa_dmcsteps.hip).  Sized by a step's
  // candidate count, with ensure's regrowth headroom: b_amp [2][ncand] ratio x weight and ratio, b_ptw [ncand] walker of a candidate (positions
  // and weights: b_tpos, b_twgt; orbital rows: b_emo).
  struct {
    bool cont = false, old_valid = false;
    long old_W = 0;
    int tm_P = 0, *d_ptk = nullptr, *d_pti = nullptr;
    DevBuf b_old, b_call, b_amp, b_ptw;
  } dmc;
  DevBuf b_xt, b_Tt[2], b_rc[2], b_sel[2], b_auxt, b_kpart, b_rbuf, b_vbuf, b_act;  // lane-per-walker SoA mirrors (pqa_lw.hpp)
  // launch-per-move sweep on those planes (k_step_lw / k_step_pre, pqa_lw.hpp).  mode (PQA_LW): 1 lane-per-walker fused sweeps for
  // single-determinant handles, 0 the wave-per-walker kernels.  kb (PQA_LW_KB), electrons per Sherman-Morrison block: -1 automatic (4 for
  // >= 16 electrons per spin), 0 = update every row on every move.  Blocking is bitwise identical and cuts the inverse's HBM traffic ~3x;
  // it pays since k_flush_lw stages the block's update vectors in LDS (1.26 -> 0.27 ms per flush at 65536 walkers): commit + flush
  // 15.5 -> 8.4 ms per step.  gm (PQA_LW_GM): thread groups of the move kernels, 0 = automatic.  step_pre (PQA_STEP_PRE): 0 = k_step_lw
  // for small shards too (A/B, bitwise check)
  struct { int mode = 1, kb = -1, gm = 0, step_pre = 1; } lw;
  DevBuf b_rot, b_eunif, b_elocal, b_ecnt, b_eoff, b_epts[2], b_ewgt[2], b_epte[2], b_emo[2], b_ecp;
  DevBuf b_erat[2];  // Slater ratios of the ECP points, per spin (k_ecp_orbcol: the route that keeps no orbital rows in b_emo)
  int orb_tp = 0;  // 0 = automatic
  struct TpTune { float ms[2] = {1e30f, 1e30f}; int n[2] = {0, 0}; int choice = 0; };  // periodic k_orb: [0] 32-point, [1] 64-point tiles
  TpTune tp_tune[2][48];  // per chunk table (5 / 1 components) and log2 bucket of the point count
  WideTab wide[2]{};  // lane-group shell lists of the whole-K small-launch kernel (k_orb_wide), per chunk table (64 groups; periodic: 32)
  std::vector<const void*> wide_attr;  // kernels whose dynamic-LDS limit has been raised
  int orb_ws = -1;  // -1 automatic; 1 wave-specialised orbital kernel; 0 phase-alternating k_orb (PQA_ORB_WS)
  // The route of the last sweep that PQA_RES_DEBUG reported (sweep_route, pqa_sweep.hip; debug: the variable was set at create)
  struct { bool debug = false; SweepRoute reported = SweepRoute::none; } route;
  // resident sweep (pqa_res.hpp / pqa_res.hip): the whole electron sweep of 16 walkers in one block, one launch per sweep.
  // mode (PQA_RES): -1 automatic (by shard size, res_plan), 0 never, 1 whenever the system is in scope.  ready / ok: res_setup has run /
  // accepted the system.  dense: the tile holds the AOs in their own order (rows padded to x4 only, res_rows4) and the contraction
  // reads d_cres — for bases whose chunk-padded rows do not fit one LDS tile (the 2x2x2 diamond cell: 208 AOs, 224 padded rows)
  struct { int mode = -1; bool ready = false, ok = false, dense = false; ResTab tab{}; size_t lds = 0; } res;
  // dense coefficient copy [res_rows_alloc(res_rows4)][ldc] of each spin in AO order, for k_sweep_res's dense mode and k_sweep_r8
  // (cres_upload: allocated by the first setup that needs it, refreshed by set_mo)
  double* d_cres[2] = {nullptr, nullptr};
  int pbc_mincls = 0;
  bool pbc_lists_ok = false;
  // second generation of the resident sweep for open-boundary real handles (pqa_res8.hpp / pqa_res8.hip): 8 walkers per 256-thread block, two
  // blocks per CU, wave-uniform AO phase.  mode (PQA_R8): -1 automatic (r8_plan), 0 never (k_sweep_res / the launches), 1 whenever in
  // scope.  util: filled atom slots of the work items.  xaos_next: the next k_sweep_r8 launch also writes the walker-major coordinates
  // (js.x); jsx_current: ... and did: energy_dev skips its transpose of the coordinate planes
  struct { int mode = -1; bool ready = false, ok = false; R8Tab tab{}; size_t lds = 0; double util = 0.0; bool xaos_next = false, jsx_current = false; } r8;
  // wave-per-walker sweep in one launch (pqa_ww.hpp).  mode (PQA_WW): -1 by shard size (up to max walkers), 0 off, 1 always.  50-determinant
  // water molecule, VMC step with energy, launches -> one launch: 0.722 -> 0.663 ms at 1 024 walkers, 0.884 -> 0.801 at 2 048, 1.428 -> 1.382 at 4 096, 2.25 -> 2.38 at 8 192
  struct { int mode = -1; long max = 4096; } ww;
  // energy pass (energy_dev, pqa_energy.hip).  The five switches, read by energy_plan alone: ecp_wave (PQA_ECP_WAVE=1) wave-per-walker ECP
  // accumulation; ecp_point_lw (PQA_ECP_POINT_LW=0) k_ecp_point on the planes instead of k_ecp_point_lw; ecp_acc_waves (PQA_ECP_ACC_WAVES) 1 / 4
  // waves per walker in k_ecp_accum / k_kinetic_coulomb (0: 4 while walkers x electrons <= 32768); ecp_lds (PQA_ECP_LDS=0) first-generation
  // k_ecp_count / k_ecp_fill; ecp_defer (PQA_ECP_DEFER=0) point totals read back in every evaluation (all A/B, tests).  stream / ev: the side
  // stream the kinetic pass of a small shard runs on beside the ECP passes, with its fork, coordinates and hand-over events.  W: walkers of
  // the evaluation whose per-walker rows b_en holds (pqa_energy_last); d_ecp: its ECP row(s) (nullptr: no ECP).  pin_tot: pinned,
  // device-visible host words the scan kernel writes the point totals to.  Point totals may stay on the device (small shards): hint / hint_valid
  // are the totals of the last evaluation that read them (every 16th of evals does) and pick the launch sizes in between.  last_*: the
  // lists the last evaluation left — points per spin (-1: on the device, then last_dev points at them), their sum (pqa_last_ecp_points),
  // segments per walker (EcpBuf::nseg).  ecp_route_reported / route_reported: what PQA_RES_DEBUG last printed (1: k_ecp_orbcol, 0: rows)
  struct {
    int ecp_wave = 0, ecp_point_lw = 1, ecp_acc_waves = 0, ecp_lds = 1, ecp_defer = 1;
    hipStream_t stream = nullptr;
    hipEvent_t ev[3] = {nullptr, nullptr, nullptr};
    long W = 0;
    const double* d_ecp = nullptr;
    long* pin_tot = nullptr;
    bool hint_valid = false;
    long hint[2] = {0, 0}, evals = 0;
    long last_tot[2] = {0, 0}, last_points = 0;
    const long* last_dev[2] = {nullptr, nullptr};
    int last_nseg = 1;
    int ecp_route_reported = -1;
    std::string route_reported;
  } en;
  // the NEXT step's sweep draws (k_tile_draws) generated beside the energy pass of the current step: second tape set, its stream and events
  // (ahead_*: the step, seed and walker count the set was drawn for; on_device: the last sweep took its draws from k_tile_draws)
  struct {
    DevBuf b_gauss_b, b_unif_b;
    hipStream_t stream = nullptr;
    hipEvent_t ev[2] = {nullptr, nullptr};
    bool ahead_valid = false, on_device = false;
    uint32_t ahead_step = 0;
    uint64_t ahead_seed = 0;
    long ahead_W = 0;
  } draw;
  long orb_p_hint = 0;  // launch_orb: points the next launch is expected to work on when its P is an upper bound (0: P)
  // density-matrix sampling (pqa_dm.hpp): per slot the auxiliary walkers (position, orbital row, density), the kept samples
  // and the orbitals at the configurations' electrons; accumulators of the estimator in dm_val / dm_norm
  struct DmSlot { DevBuf pos, row, f, newpos, keep_pos, keep_row, keep_f, cfg; long n = 0, ncfg = 0; int nkeep = 0, spin = 0; };
  DmSlot dm[2];
  DevBuf dm_val, dm_norm[2], dm_tmp, dm_ijkl, dm_assign[2], dm_ratio, dm_acc;
  long dm_nconf = 0, dm_nval = 0;
  int dm_cx = 0;
  bool tile_attr_set = false;
  bool saved_valid = false;
  bool jas_stale = false;  // fused sweeps move x without patching avalues/bvalues
  int saved_e = -1;
  // measurement
  hipEvent_t ev0 = nullptr, ev1 = nullptr;
  bool profile = false;
  ProfSet prof_orb;     // orbital launches (launch_orb) and the resident sweeps' launches
  ProfSet prof_commit;  // Sherman-Morrison commit launches of the fused sweep
  ProfSet prof_part;    // partial-sum launches (k_move_part_lw) of the fused sweep
  unsigned prof_tick = 0;  // the orbital set's event pairs bracket every prof_stride-th eligible launch
  double prof_pc = 0.0;    // point-components of the orbital set's launches
};
// profiling: event pairs bracket a 1-in-prof_stride sample of the eligible launches (an event pair costs ~2 us of stream time)
static constexpr unsigned prof_stride = 4;

#define HIPCHK(call)                                                                                     \
  do {                                                                                                   \
    hipError_t e_ = (call);                                                                              \
    if (e_ != hipSuccess) {                                                                              \
      char buf_[512];                                                                                    \
      snprintf(buf_, sizeof buf_, "%s failed: %s (%s:%d)", #call, hipGetErrorString(e_), __FILE__, __LINE__); \
      h->err = buf_;                                                                                     \
      return -1;                                                                                         \
    }                                                                                                    \
  } while (0)
#define FAIL(msg)      \
  do {                 \
    h->err = (msg);    \
    return -2;         \
  } while (0)
#define TRY(x)          \
  do {                  \
    int rc_ = (x);      \
    if (rc_) return rc_; \
  } while (0)

static inline int ensure(pqa_handle* h, DevBuf& b, size_t bytes) {
  if (bytes <= b.cap && b.p) return 0;
  // A buffer that has to GROW holds data-dependent sizes (ECP / T-move point lists: ~38 points per walker +- sqrt(N)
  // from step to step).  Exact-size regrowth made every new maximum a hipFree + hipMalloc pair, i.e. a device
  // synchronisation and milliseconds of driver time in the first dozens of steps (the first timed steps on a fresh box
  // ran 15 % slow); 25 % headroom on regrowth ends that after the second step.  First allocations stay exact.
  const bool regrow = b.p != nullptr;
  if (b.p) HIPCHK(hipFree(b.p));
  b.p = nullptr;
  b.cap = 0;
  size_t want = std::max<size_t>(regrow ? bytes + bytes / 4 : bytes, 256);
  HIPCHK(hipMalloc(&b.p, want));
  b.cap = want;
  if (!regrow) h->bufs.push_back(&b);  // (std::swap of two recorded buffers keeps both records valid: pqa_resample)
  return 0;
}

template <class T>
static int upload_table(pqa_handle* h, const T* src, size_t n, T** dst) {
  *dst = nullptr;
  if (n == 0) n = 1;
  void* p = nullptr;
  HIPCHK(hipMalloc(&p, n * sizeof(T)));
  h->owned.push_back(p);
  if (src) HIPCHK(hipMemcpy(p, src, n * sizeof(T), hipMemcpyHostToDevice));
  else HIPCHK(hipMemset(p, 0, n * sizeof(T)));
  *dst = (T*)p;
  return 0;
}

// event / non-blocking stream / pinned host words of the handle, recorded for pqa_destroy
static inline int new_event(pqa_handle* h, hipEvent_t* e, unsigned flags = hipEventDefault) {
  HIPCHK(hipEventCreateWithFlags(e, flags));
  h->events.push_back(*e);
  return 0;
}
static inline int new_stream(pqa_handle* h, hipStream_t* s) {
  HIPCHK(hipStreamCreateWithFlags(s, hipStreamNonBlocking));
  h->streams.push_back(*s);
  return 0;
}
template <class T>
static int new_pinned(pqa_handle* h, T** p, size_t n, unsigned flags) {
  HIPCHK(hipHostMalloc((void**)p, n * sizeof(T), flags));
  h->pinned.push_back(*p);
  return 0;
}

// The next event pair of a profiler set, created if the pool has none left.  take = false only makes sure the pair exists.
static inline int prof_acquire(pqa_handle* h, ProfSet& p, hipEvent_t& e0, hipEvent_t& e1, bool take = true) {
  if (p.used == p.ev.size()) {
    hipEvent_t a, b;
    TRY(new_event(h, &a));
    TRY(new_event(h, &b));
    p.ev.emplace_back(a, b);
  }
  if (take) {
    e0 = p.ev[p.used].first;
    e1 = p.ev[p.used].second;
    ++p.used;
  }
  return 0;
}
// elapsed time of the pairs used since the last drain, added to the set's total (the stream has been synchronised)
static inline int prof_drain(pqa_handle* h, ProfSet& p) {
  for (size_t i = 0; i < p.used; ++i) {
    float ms = 0.f;
    HIPCHK(hipEventElapsedTime(&ms, p.ev[i].first, p.ev[i].second));
    p.ms += ms;
  }
  p.used = 0;
  return 0;
}

static inline int copy_in(pqa_handle* h, void* dst, const void* src, size_t bytes) {
  if (bytes == 0) return 0;
  HIPCHK(hipMemcpyAsync(dst, src, bytes, hipMemcpyDefault, h->stream));
  return 0;
}
static inline int copy_out(pqa_handle* h, void* dst, const void* src, size_t bytes) {
  if (bytes) HIPCHK(hipMemcpyAsync(dst, src, bytes, hipMemcpyDefault, h->stream));
  HIPCHK(hipStreamSynchronize(h->stream));
  return 0;
}
static inline int check_launch(pqa_handle* h, const char* what) {
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) {
    h->err = std::string(what) + " launch failed: " + hipGetErrorString(e);
    return -1;
  }
  return 0;
}

static inline size_t lds_j3(const pqa_handle* h) {  // bytes needed by kernels that call jas_eval with the three-body term
  return h->has_j3 ? ((size_t)h->S.j3_off + (size_t)h->natom * (3 + 6 * h->na3 * h->nb3)) * sizeof(double) : 0;
}
static inline size_t lds_sm(const pqa_handle* h) {
  const size_t n = std::max(h->nup, h->ndn);
  if (n > PQA_MAXN_FAST) return std::max((3 * n + 64) * sizeof(double), lds_j3(h));  // sm_update_wave works on the inverse in place there
  return std::max((n * (n + 1) + 2 * n + 64 + n) * sizeof(double), lds_j3(h));
}
static inline size_t lds_det(const pqa_handle* h, int ncomp) {
  return std::max((size_t)std::max(h->ndet_s[0], h->ndet_s[1]) * ncomp * sizeof(double), lds_j3(h));
}

struct LwCtx {
  int Gm = 1, KB = 1, nmax = 1;
};
// the lane-per-walker fused sweep (pqa_lw.hpp) covers the handle: one determinant, no three-body Jastrow, complex ones up to 32 per spin
static inline bool lw_eligible(const pqa_handle* h) {
  return h->lw.mode != 0 && h->has_slater && h->ndet == 1 && !h->has_j3 && (!h->cplx || std::max(h->nup, h->ndn) <= 32);
}

// ---- functions defined in one unit and called from others
// pqa_orb.hip: out[p][ncomp][nmo_spin]; out_sel / slot_stride: two-slot output (ChunkTab::out_sel), else plain rows
int launch_orb(pqa_handle* h, int spin, PointAddr pa, long P, int ncomp, double* out, const unsigned char* out_sel = nullptr, long slot_stride = 0);
PointAddr plain_points(const double* base, long P);
// pqa_orb_pbc.hip: AO planes out[ncomp][P][nao] at arbitrary points, thread per point (test entry, parameter gradients, the general
// periodic path); ncomp 1, 4 or 5
int launch_ao(pqa_handle* h, PointAddr pa, long P, int ncomp, double* out);
// pqa_sweep.hip
void transpose(pqa_handle* h, const double* in, double* out, long R, long C);  // in [R][C] -> out [C][R]
LwState lw_state(pqa_handle* h);
int lw_from_aos(pqa_handle* h, bool with_cache = true);
int lw_to_aos(pqa_handle* h, bool with_cache);
int sync_aos(pqa_handle* h);
LwCtx lw_geometry(const pqa_handle* h, long W);  // launch geometry of the lane-per-walker kernels: pure
int lw_setup(pqa_handle* h, bool lw, LwCtx& c);  // the geometry, the state in the layout the sweep works on, and (lw) its scratch
// One call of a propagation entry (pqa_vmc_sweeps, pqa_dmc_steps).  The entry fills in what it was called with: nsteps, tstep, seed, the sweep
// tapes it brought (host, [nsteps][N][W][3] / [nsteps][N][W]; NULL: device draws) and nacc, the acceptance counts it keeps per step (DMC: 2).
// step_call_open does what both do before their first step: the walker-major state first if from_aos (DMC: the starting energy and the first
// T-moves read it), the device, the W check, the entry's own refusal (raised where the entries raised it: after the W check, and not for
// nsteps <= 0, where the caller returns 0), saved_valid, the per-move scratch, the zeroed counts and wrap counters, the tape buffers, lw_setup.
// step_moves fills one step's MoveBuf and copies that step's tapes in; it holds the rule that twisted handles get no wrap pointers.
struct StepCall {
  int nsteps = 0, nacc = 1, N = 0;
  long W = 0;
  double tstep = 0.0;
  uint64_t seed = 0;
  const double *gauss = nullptr, *unif = nullptr;
  bool lw = false;  // lw_eligible; lc: lw_setup's geometry
  LwCtx lc;
};
int step_call_open(pqa_handle* h, StepCall& c, bool from_aos, const char* refused);
int step_moves(pqa_handle* h, const StepCall& c, int step, MoveBuf& mb);
int sweep_electrons(pqa_handle* h, const MoveBuf& mb, const LwCtx& lc);
void launch_step_real(pqa_handle* h, const LwState& L, const MoveBuf& mb, const StepArgs& a, int rowlen);
void launch_flush_real(pqa_handle* h, const LwState& L, int s, long W, long w0, long w1, int j_lo, int j_hi, int nq, int rowlen, int n_s);
// pqa_sweep_cx.hip
void launch_step_cx(pqa_handle* h, const LwState& L, const MoveBuf& mb, const StepArgs& a, int rowlen);
void launch_flush_cx(pqa_handle* h, const LwState& L, int s, long W, long w0, long w1, int j_lo, int j_hi, int nq, int rowlen, int n_s);
// the one-launch sweeps.  *_plan: whether the sweep takes this handle (and shard size) — the setup runs on first use, once per handle; out of
// scope leaves *use false and returns 0, a device error returns its code with h->err set
static inline int res_rows4(const pqa_handle* h) { return ((h->twist ? 2 : 1) * h->nao + 3) & ~3; }  // rows of a dense tile: the AOs (twisted: real, then imaginary parts) padded to x4
static inline int res_rows_alloc(int rows4) { return rows4 + 96; }  // rows of the dense coefficient copies d_cres: zero beyond the basis (k_sweep_r8 contracts six k-steps per trip in every wave)
// pqa_res.hip
int res_plan(pqa_handle* h, long W, bool* use);
int sweep_res(pqa_handle* h, const MoveBuf& mb);
int cres_upload(pqa_handle* h, int s, const double* mo_host);  // d_cres[s]: refreshed from set_mo's mo_host, or (nullptr) made from d_mo[s]
int unique_primitives(pqa_handle* h, std::vector<double>& pe_u, std::vector<double>& pc_u, std::vector<int>& q0_u);
int sweep_launch_begin(pqa_handle* h, const MoveBuf& mb, hipEvent_t* e1);  // tapes check and profiling bracket of a one-launch sweep
// pqa_res8.hip
int r8_plan(pqa_handle* h, bool* use);
int sweep_r8(pqa_handle* h, const MoveBuf& mb);
// pqa_sweep_ww.hip
bool ww_eligible(pqa_handle* h, long W);
int sweep_ww(pqa_handle* h, const MoveBuf& mb);
// pqa_energy.hip
// What a caller tells energy_dev about its evaluation.  soa_current: the lane-per-walker planes hold the live state (a fused sweep just ran);
// aos_T_needed: the caller works on the walker-major inverses next (the DMC step's T-moves); assemble = false: the rows of b_en are left to
// the caller (k_energy_finish, from b_kc and en.d_ecp); slater_only: the Slater factor's energy terms alone (the correlated evaluations add
// every set's Jastrow themselves); host_totals: the ECP point totals are read on the host in this evaluation (en.last_tot >= 0 afterwards)
struct EnergyOpts { bool soa_current = false, aos_T_needed = true, assemble = true, slater_only = false, host_totals = false; };
int energy_dev(pqa_handle* h, double threshold, const double* rot, const double* unif, uint64_t seed, uint32_t step, const EnergyOpts& o = {});
// pqa_dmcsteps.hip
// What a DMC call draws besides its sweeps' normals and uniforms (pqa_dmc_tapes_t), by the handle's ECP integrator; read by the tape
// check and scratch of pqa_dmc_steps, its per-step staging and pqa_philox_dmc_tapes.  batched (pqa_set_ecp_batched): the energy passes and
// the T-move tables come from that integrator, nsel slots per electron; selu: its selection drops points, so its nsr selection uniforms
// per (electron, walker) exist.  tmoves: a step makes T-moves.  nrot: rotations of one energy evaluation or one step's T-moves, N x
// max(necp, 1).  nu: uniforms per (electron, walker) of one evaluation or one step's T-moves — the necp mask uniforms, layout (N, necp, W),
// or the batched integrator's nsr where selu, layout (N, W, nsr): ecp_unif / tm_unif advance by N W nu doubles, and neither exists where nu = 0.
struct DmcDraws { bool batched, selu, tmoves; int nsel, nsr, nu; size_t nrot; };
DmcDraws dmc_draws(const pqa_handle* h);
int scan_ints(pqa_handle* h, const int* c, long* o, long n, long Wm, long* marks);
// pqa_create.hip
int set_mo(pqa_handle* h, int s, const double* mo_host);  // orbital coefficients of a spin: d_mo, the padded copies, the resident sweep's
int set_c3(pqa_handle* h, const double* c);               // three-body coefficients, symmetrised
int jas_merge_tables(pqa_handle* h);                      // merged Pade numerators, after every change of acoeff / bcoeff
int ecp_quadrature_offset(int naip);                      // first row of a quadrature rule in d_quad (-1: no such rule)
// pqa_capi.hip
int jas_refresh(pqa_handle* h);       // basis sums a fused sweep left stale, recomputed
int slater_rebuild(pqa_handle* h);    // orbital cache, inverses and determinants of both spins from js.x
int slater_value_dev(pqa_handle* h);  // sign / log of the Slater factor -> b_sign / b_log

// Raises kernel fn's dynamic-LDS limit to the 160 KiB of a CU, once per handle.
inline int raise_lds_limit(pqa_handle* h, const void* fn) {
  if (std::find(h->wide_attr.begin(), h->wide_attr.end(), fn) != h->wide_attr.end()) return 0;
  HIPCHK(hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024));
  h->wide_attr.push_back(fn);
  return 0;
}

// d log Psi / d det_coeff of the resident walkers -> b_pgdet (W, ndet), complex handles (re, im) interleaved; the sign (complex: phase)
// and log of the determinant expansion it divides by -> b_sign, b_log.  On h's stream.
template <int PQA_UNIT = 0>  // (a template so that only the units that call it compile the kernels)
inline int pgrad_det_dev(pqa_handle* h) {
  const long W = h->W;
  TRY(slater_value_dev(h));
  TRY(ensure(h, h->b_pgdet, (size_t)(h->cplx ? 2 : 1) * W * h->ndet * sizeof(double)));
  const dim3 gd((unsigned)((W * h->ndet + 255) / 256));
  if (h->cplx)
    hipLaunchKernelGGL((k_pgrad_det_c<PQA_UNIT>), gd, dim3(256), 0, h->stream, h->S, h->st, (const double*)h->b_sign.p, (const double*)h->b_log.p, W,
                       (double*)h->b_pgdet.p);
  else
    hipLaunchKernelGGL((k_pgrad_det<PQA_UNIT>), gd, dim3(256), 0, h->stream, h->S, h->st, (const double*)h->b_sign.p, (const double*)h->b_log.p, W,
                       (double*)h->b_pgdet.p);
  return check_launch(h, "k_pgrad_det");
}

// d log Psi / d ccoeff of the resident walkers -> b_out (W, natom, na3, na3, nb3, 3): k_j3_pgrad, one wave per walker with the a / b
// value tables of that walker in LDS.  On h's stream.
template <int PQA_UNIT = 0>  // (a template so that only the units that call it compile the kernel)
inline int j3_pgrad_dev(pqa_handle* h) {
  const size_t lds = ((size_t)h->N * h->natom * h->na3 + (size_t)h->N * (h->N - 1) / 2 * h->nb3) * sizeof(double);
  if (lds > 150 * 1024) FAIL("three-body parameter gradient: the a/b value tables of one walker do not fit LDS");
  TRY(ensure(h, h->b_out, (size_t)h->W * h->natom * h->na3 * h->na3 * h->nb3 * 3 * sizeof(double)));
  if (lds > 64 * 1024) TRY(raise_lds_limit(h, reinterpret_cast<const void*>(k_j3_pgrad<PQA_UNIT>)));
  hipLaunchKernelGGL((k_j3_pgrad<PQA_UNIT>), dim3((unsigned)h->W), dim3(64), lds, h->stream, h->S, h->js, (double*)h->b_out.p);
  return check_launch(h, "k_j3_pgrad");
}
// accumulators of the density-matrix estimators: shapes recorded on the first sweep, checked on the others; buffers sized
int dm_prepare(pqa_handle* h, long nconf, long nval, int cx, int first, long nnorm_a, long nnorm_b);
