// pyqmc_amd C ABI implementation (host side): local energy on the device (kinetic, Coulomb / Ewald, ECP), pqa_energy, pqa_set_ewald, pqa_get_wrap.
// See include/pyqmc_amd.h for the contract and pqa_internal.hpp for what the units share.
//
// energy_dev decides the routes of an evaluation once (energy_plan -> EnergyPlan) and runs its stages from the plan:
// kinetic -> Ewald -> ECP lists -> ECP orbitals -> ECP accumulation -> assemble.
#include "pqa_internal.hpp"
#include "pqa_ecp_orbcol.hpp"

namespace {

// ---------------------------------------------------------------- the plan
struct EnergyPlan {
  long W = 0;
  bool soa = false;                              // the lane-per-walker planes hold the live state
  bool has_jastrow = false, has_j2 = false;      // the Jastrow terms the kernels include (none of a slater_only evaluation)
  bool rot_tape = false, unif_tape = false;      // the caller's ECP rotations / uniforms (else: generated from seed and step)
  enum Kinetic { kin_lw, kin_coulomb } kinetic = kin_coulomb;
  bool kin_quad = false;                         // k_kinetic_lw: quad-cooperative row reads
  int waves = 1;                                 // waves per walker of k_kinetic_coulomb and k_ecp_accum (1 or 4)
  // what the ECP passes' walker-major input needs after a sweep: nothing (no ECP, or no sweep), the coordinates (k_sweep_r8 wrote them /
  // a transpose), or the whole walker-major state (lw_to_aos)
  enum Coords { coords_none, coords_sweep, coords_transpose, coords_state } coords = coords_none;
  bool soa_T = false;                            // the inverses stay in the planes
  bool ewald_planes = false;                     // k_ewald reads the coordinate planes
  bool ecp = false;
  enum Lists { lists_none, lists_batched, lists_lds, lists_first } lists = lists_none;
  long nseg = 1;                                 // segments per walker of the point lists (EcpBuf::nseg)
  size_t tab_b = 0;                              // LDS bytes of the second-generation list passes' tables
  long pmax = 0;                                 // quadrature points of one electron over all ECP atoms, at most
  bool scan_small = true;                        // k_scan_small2 (one block) instead of the device-wide scan_ints
  bool fill_ue = false;                          // the fill pass takes U_e from k_kinetic_lw's output
  enum Orbitals { orb_none, orb_column, orb_rows } orbitals = orb_none;
  enum Points { pts_none, pts_point_lw, pts_point, pts_accum } points = pts_none;
  // the two decisions that read the evaluation counter and the last totals read back (not part of the reported route)
  bool defer = false;                            // the point totals stay on the device: no host synchronisation inside this evaluation
  bool side = false;                             // the kinetic / Coulomb / Ewald passes run on the side stream beside the ECP passes
  bool assemble = true;
};

// Every route decision of an evaluation, each predicate once.  Reads the handle, writes nothing.
EnergyPlan energy_plan(const pqa_handle* h, long W, const EnergyOpts& o, bool rot_tape, bool unif_tape) {
  EnergyPlan P;
  P.W = W; P.soa = o.soa_current; P.assemble = o.assemble; P.rot_tape = rot_tape; P.unif_tape = unif_tape;
  P.has_jastrow = h->has_jastrow && !o.slater_only;
  P.has_j2 = h->has_j2 && !o.slater_only;
  P.ecp = h->necp > 0;
  const bool batched = h->ecpb_on != 0, cx = h->cplx, pbc = h->S.pbc != 0;
  const bool small = W * h->N <= 32768;  // launches too small to fill the chip with one wave per walker
  // thread per quadrature point and an ordered per-walker sum, or the wave-per-walker accumulation (several determinants, three-body factor)
  const bool thread_pt = h->ndet == 1 && !h->has_j3 && h->en.ecp_wave == 0;
  const bool pt_lw = P.soa && h->en.ecp_point_lw && thread_pt;  // ... on the planes: k_ecp_point_lw

  P.kinetic = P.soa ? EnergyPlan::kin_lw : EnergyPlan::kin_coulomb;
  P.kin_quad = P.soa && !cx && W >= 16384 && (W & 3) == 0;  // large shards, real determinants
  // four waves per walker while the launch is too small to fill the chip with one (measured after the three-body / determinant-pass fixes: C4
  // +7 % at 2048 walkers, even at 4096, -7 % at 8192; the 32-electron twisted cell +1 % at 1024, -1.5 % at 2048, -6 % at 8192)
  P.waves = (h->en.ecp_acc_waves == 4 || (h->en.ecp_acc_waves == 0 && small)) ? 4 : 1;
  // the ECP kernels read walker-major coordinates; the inverse only when the wave-per-walker accumulation runs (or the caller works on the
  // walker-major state next: the DMC step's T-moves) — the thread-per-point kernels take the planes
  P.soa_T = P.soa && !o.aos_T_needed && (!cx || h->en.ecp_point_lw) && thread_pt;
  if (P.soa && P.ecp) P.coords = !P.soa_T ? EnergyPlan::coords_state : h->r8.jsx_current ? EnergyPlan::coords_sweep : EnergyPlan::coords_transpose;
  P.ewald_planes = P.soa && !P.ecp;  // (with ECPs the coordinates were just transposed back)
  P.fill_ue = P.soa && P.has_j2;
  if (P.ecp) {
    // second-generation list passes (pqa_ecp.hpp): tables in LDS, four walkers per block
    P.tab_b = ecp_tab_bytes(h->necp, h->ecp_nchan, h->ecp_nterm);
    const bool lds = h->en.ecp_lds && h->necp <= 64 && (long)h->necp * ((h->N + 63) / 64) <= 64 && P.tab_b <= 32768;
    P.lists = batched ? EnergyPlan::lists_batched : lds ? EnergyPlan::lists_lds : EnergyPlan::lists_first;
    // (atom-major lists where the orbital kernel gains from them: periodic cells, whose per-lane image walks then have similar
    // lengths within a tile — 2x2x2 diamond VMC +3 % at 32768 walkers; open systems gain nothing and pay a longer scan and sum)
    P.nseg = (P.lists == EnergyPlan::lists_lds && pbc) ? h->necp : 1;
    P.scan_small = P.nseg * W <= 16384;
    // complex determinants off the planes: wave-per-walker accumulation in complex arithmetic
    P.points = (cx && !pt_lw) || !thread_pt ? EnergyPlan::pts_accum : pt_lw ? EnergyPlan::pts_point_lw : EnergyPlan::pts_point;
    // k_ecp_orbcol (one Slater ratio per quadrature point from the inverse column, pqa_ecp_orbcol.hpp) exactly where k_ecp_point_lw reads
    // the planes of a real, open-boundary handle with the semi-local integrator, and the kernel's tables and the columns of PQA_OC_R runs
    // fit a block's LDS (then two blocks fit a CU).  Everything else keeps the orbital rows of launch_orb and the dot product.
    const bool column = pt_lw && h->has_slater && !batched && !pbc && h->S.nL <= 0 && !cx && h->nshell <= PQA_WS_MAXSH &&
                        (int)h->S.nprim <= PQA_WS_MAXP &&
                        PQA_OC_STATIC_LDS + ecp_orbcol_lds(h->S.nao, std::max(h->nup, h->ndn)) <= (size_t)64 * 1024;
    P.orbitals = column ? EnergyPlan::orb_column : h->has_slater ? EnergyPlan::orb_rows : EnergyPlan::orb_none;
    // Small shards: no device -> host round trip for the totals (two copies and the host's wake-up: ~80 us of a 0.3 - 0.8 ms step).  The
    // lists are sized for every point of every ECP atom, the orbital launch and the per-point pass cover that bound and their blocks beyond
    // the device-side count leave at once (PointAddr::count, EcpBuf::ptot; k_ecp_accum / k_ecp_sum read the list offsets from the device
    // anyway); the kernel choice follows the totals of the last evaluation that did read them (every 16th does).
    P.pmax = (long)h->necp * std::max(h->S.ecp_naip_max, 1);
    P.defer = !batched && !o.host_totals && h->en.ecp_defer != 0 && !pbc && h->en.hint_valid && (h->en.evals % 16) != 0 &&
              (W * (long)h->N * P.pmax) * (long)(64 + 8 * std::max(h->nmo[0], h->nmo[1])) <= (long)256 << 20;
    // After a sweep, shards whose ECP passes read their point totals back: the host waits for the counting passes while the kinetic pass
    // runs beside them on the side stream, and has the rest of the evaluation enqueued before the device gets there (the read-back was an
    // idle gap of ~50 us).  Walker-major evaluations of small shards: the kinetic / Coulomb pass beside the ECP passes — both are a few
    // thousand latency-bound waves (50-determinant water molecule, 2 048 walkers: 125 us and 245 us one after the other)
    P.side = P.soa ? (!batched && W <= 16384 && !P.defer) : small;
  }
  return P;
}

// The route as PQA_RES_DEBUG reports it: the plan's fields that depend on neither the evaluation counter nor the point totals.
std::string energy_route_text(const pqa_handle* h, const EnergyPlan& P) {
  const std::string cx = h->cplx ? "complex " : "", x = P.waves == 4 ? " x4" : " x1";
  std::string kin = P.kinetic == EnergyPlan::kin_lw ? std::string(h->S.pbc ? "periodic " : "") + cx + "lw" + (P.kin_quad ? " quad" : "") : cx + "coulomb" + x;
  static const char* const lists[] = {"none", "batched", "lds", "first"};
  static const char* const orbitals[] = {"none", "column", "rows"};
  std::string li = lists[P.lists], pt = "none";
  if (P.nseg > 1) li += " nseg=" + std::to_string(P.nseg);
  if (P.points == EnergyPlan::pts_point_lw) pt = cx + "point_lw";
  if (P.points == EnergyPlan::pts_point) pt = P.soa_T ? "point on planes" : "point walker-major";
  if (P.points == EnergyPlan::pts_accum) pt = cx + "accum" + x;
  return "kinetic=" + kin + " lists=" + li + " orbitals=" + orbitals[P.orbitals] + " points=" + pt;
}

// ---------------------------------------------------------------- the side stream
// fork(): the launches that follow (they go to h->stream) run on en.stream, behind what the caller's stream holds so far.  Between
// main_begin() and main_end() they go to the caller's stream again, and the side stream waits for them.  hand_over() ends the side stream's
// part: the launches go on in the caller's stream, which join() makes wait for the side stream.  h->stream is restored on every exit.
struct SideStream {
  pqa_handle* h;
  hipStream_t main = nullptr;
  bool forked = false, handed = false;
  explicit SideStream(pqa_handle* h_) : h(h_) {}
  SideStream(const SideStream&) = delete;
  ~SideStream() { if (forked) h->stream = main; }
  int fork() {
    if (!h->en.stream) {
      TRY(new_stream(h, &h->en.stream));
      for (hipEvent_t& e : h->en.ev) TRY(new_event(h, &e, hipEventDisableTiming));
    }
    HIPCHK(hipEventRecord(h->en.ev[0], h->stream));
    HIPCHK(hipStreamWaitEvent(h->en.stream, h->en.ev[0], 0));
    main = h->stream; forked = true;
    h->stream = h->en.stream;
    return 0;
  }
  void main_begin() { if (forked) h->stream = main; }
  int main_end() {
    if (!forked) return 0;
    HIPCHK(hipEventRecord(h->en.ev[2], h->stream));
    HIPCHK(hipStreamWaitEvent(h->en.stream, h->en.ev[2], 0));
    h->stream = h->en.stream;
    return 0;
  }
  int hand_over() {
    if (!forked) return 0;
    HIPCHK(hipEventRecord(h->en.ev[1], h->stream));
    h->stream = main;
    forked = false; handed = true;
    return 0;
  }
  int join() {
    if (handed) HIPCHK(hipStreamWaitEvent(h->stream, h->en.ev[1], 0));
    return 0;
  }
};

// One evaluation: the plan, the caller's arguments, and what the ECP stages hand to each other.
struct EnergyRun {
  pqa_handle* h;
  const EnergyPlan& P;
  SideStream& side;
  double threshold;
  const double *rot, *unif;
  uint64_t seed;
  uint32_t step;
  EcpBuf B{};
  EcpbArgs A{};
  long tot[2] = {0, 0};                          // points of each spin's list (defer: their upper bound)
  const long* cnt_dev[2] = {nullptr, nullptr};   // the device-side totals
};

// ---------------------------------------------------------------- kernel tables
// One typed table per kernel family, indexed by its template flags; an instantiation is named once.  Every table lists `true` before
// `false` and four waves before one, hence ix(): the compiler emits kernels in the order the unit names them, this is the order it always
// had, and the unit's device code stays what it was byte for byte.  For the same reason each table stands in front
// of the stage that launches from it, and k_ecp_accum has its complex half in front of the thread-per-point families and its real half behind.
constexpr int ix(bool flag) { return flag ? 0 : 1; }

using KineticLwKernel = void (*)(SysDev, LwState, int, long, double*);
const KineticLwKernel kinetic_lw_kernels[2][2][2] = {  // [CX][PBC][QUAD]; no quad-cooperative complex kernel
    {{nullptr, k_kinetic_lw<true, true>}, {nullptr, k_kinetic_lw<false, true>}},
    {{k_kinetic_lw<true, false, true>, k_kinetic_lw<true>}, {k_kinetic_lw<false, false, true>, k_kinetic_lw<false>}}};

int kinetic_lw(pqa_handle* h, const EnergyPlan& P) {
  const long W = P.W;
  const dim3 gk((unsigned)((((W + 63) / 64 + 7) / 8) * 8 * h->N)), bk(64);  // see k_kinetic_lw
  hipLaunchKernelGGL(kinetic_lw_kernels[ix(h->cplx)][ix(h->S.pbc)][ix(P.kin_quad)], gk, bk, 0, h->stream, h->S, lw_state(h), (int)P.has_jastrow, W,
                     (double*)h->b_kpart.p);
  hipLaunchKernelGGL((k_kinetic_reduce<>), dim3((unsigned)((W + 255) / 256)), dim3(256), 0, h->stream, (const double*)h->b_kpart.p,
                     h->N, W, (double*)h->b_kc.p);
  return check_launch(h, "k_kinetic_lw");
}

using KineticCoulombKernel = void (*)(SysDev, SlaterState, JastrowState, int, int, long, double*, int);
const KineticCoulombKernel kinetic_coulomb_kernels[2][2] = {  // [CX][waves]
    {k_kinetic_coulomb<true, 4>, k_kinetic_coulomb<true, 1>}, {k_kinetic_coulomb<false, 4>, k_kinetic_coulomb<false, 1>}};

int kinetic_coulomb(pqa_handle* h, const EnergyPlan& P) {
  const size_t st = (size_t)(h->cplx ? 2 : 1) * lds_det(h, 5);
  hipLaunchKernelGGL(kinetic_coulomb_kernels[ix(h->cplx)][ix(P.waves == 4)], dim3((unsigned)P.W), dim3(64 * P.waves), P.waves * st, h->stream,
                     h->S, h->st, h->js, (int)h->has_slater, (int)P.has_jastrow, P.W, (double*)h->b_kc.p, (int)(st / sizeof(double)));
  return check_launch(h, "k_kinetic_coulomb");
}

// ---------------------------------------------------------------- the stages
int stage_kinetic(pqa_handle* h, const EnergyPlan& P, SideStream& side) {
  if (P.side) TRY(side.fork());
  if (P.kinetic == EnergyPlan::kin_coulomb) return kinetic_coulomb(h, P);
  TRY(kinetic_lw(h, P));
  if (P.coords == EnergyPlan::coords_none) return 0;
  side.main_begin();  // (the ECP passes' input: in their stream; the Ewald pass on the side stream reads the walker-major coordinates too)
  if (P.coords == EnergyPlan::coords_transpose) { transpose(h, (const double*)h->b_xt.p, h->js.x, (long)h->N * 3, P.W); TRY(check_launch(h, "k_transpose")); }
  if (P.coords == EnergyPlan::coords_state) TRY(lw_to_aos(h, false));
  return side.main_end();
}

int stage_ewald(pqa_handle* h, const EnergyPlan& P) {
  if (!h->S.pbc) return 0;
  if (!h->ew_set) FAIL("periodic Coulomb energy needs the Ewald tables (pqa_set_ewald)");
  const long W = P.W;
  const bool soa = P.ewald_planes;
  const double* x = soa ? (const double*)h->b_xt.p : h->js.x;
  const size_t lds_ew = ((size_t)h->N * 3 + (h->ew.gn ? (size_t)h->N * 3 * (h->ew.nmax + 1) * 2 : 0)) * sizeof(double);
  hipLaunchKernelGGL((k_ewald<>), dim3((unsigned)W), dim3(PQA_EWALD_T), lds_ew, h->stream, h->S, h->ew, x,
                     soa ? 1L : (long)h->N * 3, soa ? 3 * W : 3L, soa ? W : 1L, W, (double*)h->b_kc.p);
  return check_launch(h, "k_ewald");
}

// rotations and uniforms of the quadrature: the caller's tapes, or generated
int ecp_draws(EnergyRun& R) {
  pqa_handle* h = R.h;
  const size_t nrot = (size_t)h->N * h->necp;
  TRY(ensure(h, h->b_rot, nrot * 9 * sizeof(double)));
  if (R.P.rot_tape) TRY(copy_in(h, h->b_rot.p, R.rot, nrot * 9 * sizeof(double)));
  else {
    hipLaunchKernelGGL((k_gen_rot<>), dim3((unsigned)((nrot + 63) / 64)), dim3(64), 0, h->stream, (int)nrot, R.seed, R.step, (double*)h->b_rot.p);
    TRY(check_launch(h, "k_gen_rot"));
  }
  R.B.rot = (const double*)h->b_rot.p;
  if (R.P.unif_tape && R.P.lists != EnergyPlan::lists_batched) {
    TRY(ensure(h, h->b_eunif, nrot * R.P.W * sizeof(double)));
    TRY(copy_in(h, h->b_eunif.p, R.unif, nrot * R.P.W * sizeof(double)));
    R.B.unif = (const double*)h->b_eunif.p;
  }
  return 0;
}

using EcpListTKernel = void (*)(SysDev, JastrowState, EcpBuf, int, int, long);  // second generation: tables in LDS
using EcpListKernel = void (*)(SysDev, JastrowState, EcpBuf, long);
const EcpListTKernel ecp_count_t_kernels[2] = {k_ecp_count_t<true>, k_ecp_count_t<false>};  // [PBC]
const EcpListKernel ecp_count_kernels[2] = {k_ecp_count<true>, k_ecp_count<false>};         // [PBC]

// counting pass, scan of the two spins' counts, and the totals: left on the device (defer) or read back
int ecp_count(EnergyRun& R) {
  pqa_handle* h = R.h;
  const EnergyPlan& P = R.P;
  EcpBuf& B = R.B;
  const long W = P.W, nsw = P.nseg * W;
  if (P.lists == EnergyPlan::lists_lds)
    hipLaunchKernelGGL(ecp_count_t_kernels[ix(h->S.pbc)], dim3((unsigned)((W + PQA_ECP_WB - 1) / PQA_ECP_WB)), dim3(64 * PQA_ECP_WB), P.tab_b, h->stream,
                       h->S, h->js, B, h->ecp_nchan, h->ecp_nterm, W);
  else
    hipLaunchKernelGGL(ecp_count_kernels[ix(h->S.pbc)], dim3((unsigned)W), dim3(64), 0, h->stream, h->S, h->js, B, W);
  // small shards: one launch; otherwise device-wide scans of the two spins' point counts (one block took 0.26 ms at 65536 walkers)
  // (both totals land in the handle's pinned, device-visible host words: one stream synchronisation is the whole read-back)
  if (!h->en.pin_tot) TRY(new_pinned(h, &h->en.pin_tot, 4, hipHostMallocMapped));
  if (P.scan_small)
    hipLaunchKernelGGL((k_scan_small2<>), dim3(1), dim3(1024), 0, h->stream, (const int*)B.cnt, B.off, (const int*)B.cnt + nsw, B.off + (nsw + 1), nsw, h->en.pin_tot);
  else {
    TRY(ensure(h, h->b_tmmarks, 4 * sizeof(long)));
    TRY(scan_ints(h, (const int*)B.cnt, B.off, nsw, nsw, (long*)h->b_tmmarks.p));
    TRY(scan_ints(h, (const int*)B.cnt + nsw, B.off + (nsw + 1), nsw, nsw, (long*)h->b_tmmarks.p + 2));
  }
  TRY(check_launch(h, P.lists == EnergyPlan::lists_lds ? "k_ecp_count_t/k_scan_small2" : "k_ecp_count/k_scan_small2"));
  if (P.defer) {  // the lists' upper bound: every point of every ECP atom
    R.tot[0] = W * (long)h->nup * P.pmax; R.tot[1] = W * (long)h->ndn * P.pmax;
  } else {
    if (P.scan_small) {
      HIPCHK(hipStreamSynchronize(h->stream));
      R.tot[0] = h->en.pin_tot[0]; R.tot[1] = h->en.pin_tot[1];
    } else {  // (marks[1], marks[3] of the two scans: one copy)
      long mk[4];
      TRY(copy_out(h, mk, h->b_tmmarks.p, 4 * sizeof(long)));
      R.tot[0] = mk[1]; R.tot[1] = mk[3];
    }
    h->en.hint[0] = R.tot[0]; h->en.hint[1] = R.tot[1]; h->en.hint_valid = true;
  }
  ++h->en.evals;
  R.cnt_dev[0] = B.off + nsw; R.cnt_dev[1] = B.off + (nsw + 1) + nsw;
  B.ptot[0] = P.defer ? R.cnt_dev[0] : nullptr; B.ptot[1] = P.defer ? R.cnt_dev[1] : nullptr;
  return 0;
}

using EcpbFillKernel = void (*)(SysDev, JastrowState, EcpBuf, EcpbArgs, long);
const EcpbFillKernel ecpb_fill_kernels[2] = {k_ecpb_fill<true>, k_ecpb_fill<false>};  // [PBC]
const EcpListTKernel ecp_fill_t_kernels[2][2] = {{k_ecp_fill_t<true, true>, k_ecp_fill_t<false, true>}, {k_ecp_fill_t<true, false>, k_ecp_fill_t<false, false>}};  // [UE][PBC]
const EcpListKernel ecp_fill_kernels[2] = {k_ecp_fill<true>, k_ecp_fill<false>};  // [PBC]

void launch_ecpb_fill(pqa_handle* h, const EcpBuf& B, const EcpbArgs& A, long W) {
  hipLaunchKernelGGL(ecpb_fill_kernels[ix(h->S.pbc)], dim3((unsigned)((W + PQA_ECPB_WB - 1) / PQA_ECPB_WB)), dim3(64 * PQA_ECPB_WB), 0, h->stream, h->S, h->js, B, A, W);
}

// ECP lists: the draws, the local channels, and per spin the quadrature points that passed the stochastic mask with their weights
int stage_ecp_lists(EnergyRun& R) {
  pqa_handle* h = R.h;
  const EnergyPlan& P = R.P;
  EcpBuf& B = R.B;
  EcpbArgs& A = R.A;
  const long W = P.W, nsw = P.nseg * W;
  const bool batched = P.lists == EnergyPlan::lists_batched;
  TRY(ecp_draws(R));
  B.quad = h->d_quad; B.quadw = h->d_quadw; B.seed = R.seed; B.step = R.step; B.threshold = R.threshold;
  TRY(ensure(h, h->b_elocal, W * sizeof(double)));
  B.nseg = (int)P.nseg;
  TRY(ensure(h, h->b_ecnt, 2 * nsw * sizeof(int)));
  TRY(ensure(h, h->b_eoff, 2 * (nsw + 1) * sizeof(long)));
  TRY(ensure(h, h->b_ecp, (h->cplx ? 2 : 1) * W * sizeof(double)));
  TRY(ensure(h, h->b_epass, (size_t)W * h->necp * ((h->N + 63) / 64) * sizeof(unsigned long long)));
  B.local = (double*)h->b_elocal.p; B.cnt = (int*)h->b_ecnt.p; B.off = (long*)h->b_eoff.p;
  B.passbits = (unsigned long long*)h->b_epass.p;
  B.has_j2 = P.has_j2 ? 1 : 0;
  B.ue = P.fill_ue ? (const double*)h->b_kpart.p + (size_t)4 * h->N * W : nullptr;  // k_kinetic_lw left U_e there
  if (batched) {  // every (walker, electron) has ecpb_nsel slots: no counting pass, no scan (pqa_ecpb.hpp)
    A.naip = h->d_ecpb_naip; A.qoff = h->d_ecpb_qoff; A.pstart = h->d_ecpb_pstart;
    A.npoints = h->ecpb_npoints; A.nsd = h->ecpb_nsd; A.nsr = h->ecpb_nsr; A.nsel = h->ecpb_nsel;
    A.e0 = 0; A.e1 = h->N; A.tau = 0.0;
    if (P.unif_tape && A.nsel < A.npoints) {  // here: the (N, W, nselect_random) selection uniforms
      const size_t nb = (size_t)h->N * W * A.nsr * sizeof(double);
      TRY(ensure(h, h->b_eunif, nb));
      TRY(copy_in(h, h->b_eunif.p, R.unif, nb));
      A.selu = (const double*)h->b_eunif.p;
    }
    R.tot[0] = W * (long)h->nup * A.nsel; R.tot[1] = W * (long)h->ndn * A.nsel;
  } else
    TRY(ecp_count(R));
  h->en.last_points = P.defer ? -1 : R.tot[0] + R.tot[1];
  h->en.last_nseg = B.nseg;
  for (int s = 0; s < 2; ++s) {
    h->en.last_tot[s] = P.defer ? -1 : R.tot[s];
    h->en.last_dev[s] = P.defer ? R.cnt_dev[s] : nullptr;
    const size_t n = (size_t)std::max<long>(R.tot[s], 1);
    TRY(ensure(h, h->b_epts[s], n * 3 * sizeof(double)));
    TRY(ensure(h, h->b_ewgt[s], n * sizeof(double)));
    TRY(ensure(h, h->b_epte[s], n * sizeof(int)));
    TRY(ensure(h, h->b_eptw[s], n * sizeof(int)));
    TRY(ensure(h, h->b_econ[s], (h->cplx ? 2 : 1) * n * sizeof(double)));
    TRY(ensure(h, h->b_eu0[s], n * sizeof(double)));
    B.ptw[s] = (int*)h->b_eptw[s].p;
    B.u0[s] = (double*)h->b_eu0[s].p;
    if (P.orbitals == EnergyPlan::orb_column) TRY(ensure(h, h->b_erat[s], n * sizeof(double)));  // (no orbital rows on this route)
    else TRY(ensure(h, h->b_emo[s], n * std::max(h->nmo[s], 1) * sizeof(double)));
    B.pts[s] = (double*)h->b_epts[s].p; B.wgt[s] = (double*)h->b_ewgt[s].p; B.pte[s] = (int*)h->b_epte[s].p;
  }
  if (batched) {  // (also with no point at all: the local channels and the list offsets come from this launch)
    launch_ecpb_fill(h, B, A, W);
    TRY(check_launch(h, "k_ecpb_fill"));
  }
  if (P.soa) TRY(R.side.join());  // (the fill pass reads U_e from the kinetic pass's output)
  if (batched || R.tot[0] + R.tot[1] <= 0) return 0;
  if (P.lists == EnergyPlan::lists_lds)
    hipLaunchKernelGGL(ecp_fill_t_kernels[ix(P.fill_ue)][ix(h->S.pbc)], dim3((unsigned)((W + PQA_ECP_WB - 1) / PQA_ECP_WB)), dim3(64 * PQA_ECP_WB), P.tab_b,
                       h->stream, h->S, h->js, B, h->ecp_nchan, h->ecp_nterm, W);
  else
    hipLaunchKernelGGL(ecp_fill_kernels[ix(h->S.pbc)], dim3((unsigned)W), dim3(64), 0, h->stream, h->S, h->js, B, W);
  return check_launch(h, P.lists == EnergyPlan::lists_lds ? "k_ecp_fill_t" : "k_ecp_fill");
}

// ECP orbitals: what the Slater ratio of every point needs — the ratio itself from the inverse column, or the point's orbital row
int stage_ecp_orbitals(EnergyRun& R) {
  pqa_handle* h = R.h;
  const EnergyPlan& P = R.P;
  if (R.tot[0] + R.tot[1] <= 0 || P.orbitals == EnergyPlan::orb_none) return 0;
  for (int s = 0; s < 2; ++s) {
    PointAddr pa = plain_points(R.B.pts[s], R.tot[s]);
    if (P.defer) pa.count = R.cnt_dev[s];
    if (P.orbitals == EnergyPlan::orb_column) {
      if (R.tot[s] <= 0 || h->nmo[s] == 0) continue;  // (a spin without a point: no launch)
      hipLaunchKernelGGL((k_ecp_orbcol), dim3((unsigned)((R.tot[s] + 63) / 64)), dim3(256), ecp_orbcol_lds(h->S.nao, s ? h->ndn : h->nup), h->stream,
                         h->S, lw_state(h), h->tab[1], s, pa, R.tot[s], (const int*)R.B.pte[s], (const int*)R.B.ptw[s], P.W, (double*)h->b_erat[s].p);
    } else {
      if (P.defer) h->orb_p_hint = std::max<long>(h->en.hint[s], 1);
      const int rc = launch_orb(h, s, pa, R.tot[s], 1, (double*)h->b_emo[s].p);
      h->orb_p_hint = 0;
      if (rc != 0) return rc;
    }
  }
  return P.orbitals == EnergyPlan::orb_column ? check_launch(h, "k_ecp_orbcol") : 0;
}

using EcpAccumKernel = void (*)(SysDev, SlaterState, JastrowState, EcpBuf, int, int, const double*, const double*, long, double*, int);
using EcpPointLwKernel = void (*)(SysDev, LwState, EcpBuf, int, int, int, const double*, long, long, double*, const double*, long, double*, const double*, const double*);
using EcpPointKernel = void (*)(SysDev, SlaterState, JastrowState, EcpBuf, int, int, int, const double*, long, double*, const double*, long, long, long);
const EcpAccumKernel ecp_accum_cx_kernels[2][2] = {  // [PBC][waves], complex arithmetic
    {k_ecp_accum<true, true, 4>, k_ecp_accum<true, true, 1>}, {k_ecp_accum<false, true, 4>, k_ecp_accum<false, true, 1>}};
const EcpPointLwKernel ecp_point_lw_kernels[2][2] = {  // [CX][PBC]
    {k_ecp_point_lw<true, true>, k_ecp_point_lw<false, true>}, {k_ecp_point_lw<true, false>, k_ecp_point_lw<false, false>}};
const EcpPointKernel ecp_point_kernels[2] = {k_ecp_point<true>, k_ecp_point<false>};  // [PBC]

// thread per point, then an ordered per-walker sum
int ecp_points(EnergyRun& R) {
  pqa_handle* h = R.h;
  const EnergyPlan& P = R.P;
  const EcpBuf& B = R.B;
  const long W = P.W;
  const long* tot = R.tot;
  const bool lw = P.points == EnergyPlan::pts_point_lw, column = P.orbitals == EnergyPlan::orb_column;
  // small shards: the two spin channels of k_ecp_point_lw in one launch (two launches of ~11 us for a few thousand points each)
  const bool both = lw && tot[0] > 0 && tot[1] > 0 && std::max(h->en.hint[0], h->en.hint[1]) <= 262144 && h->en.hint_valid;
  for (int s = 0; s < 2; ++s) {
    if (tot[s] <= 0 || (both && s == 1)) continue;  // (a spin without a point: no launch)
    const int o = both ? 1 : s;  // the spin that rides along in a two-spin launch (none: the spin itself, with no points)
    const long n = both ? std::max(tot[0], tot[1]) : tot[s];
    const dim3 g((unsigned)((n + 255) / 256), both ? 2 : 1);
    if (lw)
      hipLaunchKernelGGL(ecp_point_lw_kernels[ix(h->cplx)][ix(h->S.pbc)], g, dim3(256), 0, h->stream, h->S, lw_state(h), B, s, (int)h->has_slater,
                         (int)P.has_jastrow, (const double*)h->b_emo[s].p, tot[s], W, (double*)h->b_econ[s].p,
                         both ? (const double*)h->b_emo[o].p : nullptr, both ? tot[o] : 0L, both ? (double*)h->b_econ[o].p : nullptr,
                         column ? (const double*)h->b_erat[s].p : nullptr, both && column ? (const double*)h->b_erat[o].p : nullptr);
    else {
      // (the planes are the live state whenever this evaluation follows a lane-per-walker sweep, also where the walker-major copy
      // was refreshed for the caller's next step — the DMC loop's T-moves)
      const long n_s = s ? h->ndn : h->nup;
      const double* Tb = P.soa_T ? (const double*)h->b_Tt[s].p : (const double*)h->st.T[s];
      hipLaunchKernelGGL(ecp_point_kernels[ix(h->S.pbc)], g, dim3(256), 0, h->stream, h->S, h->st, h->js, B, s, (int)h->has_slater, (int)P.has_jastrow,
                         (const double*)h->b_emo[s].p, tot[s], (double*)h->b_econ[s].p, Tb, P.soa_T ? 1 : n_s * n_s, P.soa_T ? n_s * W : n_s,
                         P.soa_T ? W : 1);
    }
  }
  const bool cx = lw && h->cplx;  // (complex contributions: the imaginary parts behind the real ones)
  hipLaunchKernelGGL((k_ecp_sum<>), dim3((unsigned)((W + 255) / 256)), dim3(256), 0, h->stream, B, (const double*)h->b_econ[0].p,
                     (const double*)h->b_econ[1].p, W, (double*)h->b_ecp.p, cx ? std::max<long>(tot[0], 1) : 0L, cx ? std::max<long>(tot[1], 1) : 0L);
  return check_launch(h, lw ? "k_ecp_point_lw/k_ecp_sum" : "k_ecp_point/k_ecp_sum");
}

const EcpAccumKernel ecp_accum_kernels[2][2] = {  // [PBC][waves], real
    {k_ecp_accum<true, false, 4>, k_ecp_accum<true, false, 1>}, {k_ecp_accum<false, false, 4>, k_ecp_accum<false, false, 1>}};

// wave-per-walker accumulation (complex determinants off the planes, several determinants, three-body factor): P.waves waves share a walker's points
int ecp_accum(EnergyRun& R) {
  pqa_handle* h = R.h;
  const EnergyPlan& P = R.P;
  const size_t st = (size_t)(h->cplx ? 2 : 1) * lds_det(h, 1);
  const EcpAccumKernel k = (h->cplx ? ecp_accum_cx_kernels : ecp_accum_kernels)[ix(h->S.pbc)][ix(P.waves == 4)];
  hipLaunchKernelGGL(k, dim3((unsigned)P.W), dim3(64 * P.waves), P.waves * st, h->stream, h->S, h->st, h->js, R.B, (int)h->has_slater, (int)P.has_jastrow,
                     (const double*)h->b_emo[0].p, (const double*)h->b_emo[1].p, P.W, (double*)h->b_ecp.p, (int)(st / sizeof(double)));
  return check_launch(h, "k_ecp_accum");
}

int stage_ecp_accumulate(EnergyRun& R) { return R.P.points == EnergyPlan::pts_accum ? ecp_accum(R) : ecp_points(R); }

}  // namespace

int energy_dev(pqa_handle* h, double threshold, const double* rot, const double* unif, uint64_t seed, uint32_t step, const EnergyOpts& o) {
  const long W = h->W;
  struct JsxOnce { pqa_handle* h; ~JsxOnce() { h->r8.jsx_current = false; } } jsx_once{h};  // (valid for the evaluation that follows the sweep only)
  if (!o.soa_current) h->r8.jsx_current = false;
  const EnergyPlan P = energy_plan(h, W, o, rot != nullptr, unif != nullptr);
  if (h->route.debug) {  // PQA_RES_DEBUG: the routes of this evaluation, whenever they are not the last one's
    const int column = P.orbitals == EnergyPlan::orb_column;
    if (P.ecp && column != h->en.ecp_route_reported) {
      fprintf(stderr, "[pqa] ecp route: %s\n", column ? "k_ecp_orbcol" : "k_orb rows + dot product");
      h->en.ecp_route_reported = column;
    }
    const std::string route = energy_route_text(h, P);
    if (route != h->en.route_reported) {
      fprintf(stderr, "[pqa] energy route: %s\n", route.c_str());
      h->en.route_reported = route;
    }
  }
  SideStream side(h);  // (launches go to h->stream: restored on every exit)
  TRY(ensure(h, h->b_kc, (size_t)4 * W * sizeof(double)));
  TRY(ensure(h, h->b_en, (size_t)(h->cplx ? 7 : 6) * W * sizeof(double)));
  h->en.W = W;  // (pqa_energy_last: the rows this evaluation, or its caller's k_energy_finish, leaves in b_en)
  TRY(stage_kinetic(h, P, side));
  TRY(stage_ewald(h, P));
  TRY(side.hand_over());  // the ECP passes go on in the caller's stream; the assembly waits for the side stream
  h->en.last_points = 0;
  const double* d_ecp = nullptr;
  if (P.ecp) {
    EnergyRun R{h, P, side, threshold, rot, unif, seed, step};
    TRY(stage_ecp_lists(R));
    TRY(stage_ecp_orbitals(R));
    TRY(stage_ecp_accumulate(R));
    d_ecp = (const double*)h->b_ecp.p;
  }
  TRY(side.join());
  h->en.d_ecp = d_ecp;
  if (!P.assemble) return 0;  // (the caller finishes: k_energy_finish)
  hipLaunchKernelGGL((k_energy_assemble<>), dim3((unsigned)((W + 255) / 256)), dim3(256), 0, h->stream, (const double*)h->b_kc.p, d_ecp,
                     h->ii_energy, W, (double*)h->b_en.p, (int)h->cplx);
  return check_launch(h, "k_energy_assemble");
}

// ---------------------------------------------------------------- batched ECP integrator (jax_ecp.py)
extern "C" int pqa_set_ecp_batched(pqa_handle_t* h, int32_t enable, const int32_t* naip, int32_t nsd, int32_t nsr) {
  HIPCHK(hipSetDevice(h->device));
  if (!enable) { h->ecpb_on = 0; return 0; }
  if (h->necp == 0) { h->ecpb_on = 0; return 0; }  // nothing to integrate
  if (h->necp > 64) FAIL("the batched ECP integrator holds one ECP atom per lane: at most 64 ECP atoms");
  if (!naip || nsd < 0 || nsr < 0) FAIL("bad arguments");
  std::vector<int> na((size_t)h->necp), qo((size_t)h->necp), ps((size_t)h->necp);
  int np = 0;
  for (int k = 0; k < h->necp; ++k) {
    static const int offs[][2] = {{6, 0}, {12, 6}, {18, 18}, {26, 36}, {32, 62}, {50, 94}};
    int off = naip[k] == 0 ? 0 : -1;
    for (auto& o : offs) if (o[0] == naip[k]) off = o[1];
    if (off < 0) FAIL("naip must be 0 or one of 6, 12, 18, 26, 32, 50 for every atom (eval_ecp.py:266-267)");
    if (naip[k] > 0 && h->ecp_nch[k] < 2) FAIL("quadrature points on an atom without a non-local channel");
    na[k] = naip[k]; qo[k] = off; ps[k] = np; np += naip[k];
  }
  HIPCHK(hipStreamSynchronize(h->stream));
  if (!h->d_ecpb_naip) {
    TRY(upload_table(h, na.data(), na.size(), &h->d_ecpb_naip));
    TRY(upload_table(h, qo.data(), qo.size(), &h->d_ecpb_qoff));
    TRY(upload_table(h, ps.data(), ps.size(), &h->d_ecpb_pstart));
  } else {
    HIPCHK(hipMemcpy(h->d_ecpb_naip, na.data(), na.size() * sizeof(int), hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(h->d_ecpb_qoff, qo.data(), qo.size() * sizeof(int), hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(h->d_ecpb_pstart, ps.data(), ps.size() * sizeof(int), hipMemcpyHostToDevice));
  }
  h->ecpb_npoints = np; h->ecpb_nsd = nsd; h->ecpb_nsr = nsr;
  h->ecpb_nsel = (nsd + nsr >= np) ? np : nsd + nsr;  // jax_ecp.py:236-237: nothing is dropped
  if (h->ecpb_nsel < np && nsd + nsr > PQA_ECPB_MAXSEL) FAIL("more than 256 selected points per electron");
  h->ecpb_on = 1;
  return 0;
}

extern "C" int pqa_ecp_batched_nselected(pqa_handle_t* h) { return h->ecpb_on ? h->ecpb_nsel : 0; }

extern "C" int pqa_ecp_batched_moves(pqa_handle_t* h, int e, double tau, const double* rot, const double* unif, uint64_t seed,
                                     double* weight, double* pos) {
  TRY(sync_aos(h));
  HIPCHK(hipSetDevice(h->device));
  if (h->W == 0) FAIL("state not initialised (call pqa_wf_recompute)");
  if (!h->ecpb_on) FAIL("pqa_set_ecp_batched first");
  if (e < 0 || e >= h->N || !(tau > 0.0) || !rot) FAIL("bad arguments");
  const long W = h->W;
  const int nsel = h->ecpb_nsel;
  if (nsel == 0) return 0;
  // the kernel indexes the rotations by (electron, atom): place this electron's necp matrices at its row
  const size_t nrot = (size_t)h->N * h->necp;
  TRY(ensure(h, h->b_rot, nrot * 9 * sizeof(double)));
  TRY(copy_in(h, (double*)h->b_rot.p + (size_t)e * h->necp * 9, rot, (size_t)h->necp * 9 * sizeof(double)));
  EcpBuf B{};
  B.rot = (const double*)h->b_rot.p; B.quad = h->d_quad; B.quadw = h->d_quadw; B.seed = seed; B.step = 0x7d0u;
  EcpbArgs A{};
  A.naip = h->d_ecpb_naip; A.qoff = h->d_ecpb_qoff; A.pstart = h->d_ecpb_pstart;
  A.npoints = h->ecpb_npoints; A.nsd = h->ecpb_nsd; A.nsr = h->ecpb_nsr; A.nsel = nsel;
  A.e0 = e; A.e1 = e + 1; A.tau = tau;
  if (unif && nsel < A.npoints) {
    const size_t nb = (size_t)h->N * W * A.nsr * sizeof(double);  // (indexed by (electron, walker, draw) like the energy pass)
    TRY(ensure(h, h->b_eunif, nb));
    TRY(copy_in(h, (double*)h->b_eunif.p + (size_t)e * W * A.nsr, unif, (size_t)W * A.nsr * sizeof(double)));
    A.selu = (const double*)h->b_eunif.p;
  }
  TRY(ensure(h, h->b_epts[0], (size_t)W * nsel * 3 * sizeof(double)));
  TRY(ensure(h, h->b_ewgt[0], (size_t)W * nsel * sizeof(double)));
  A.out_pos = (double*)h->b_epts[0].p; A.out_w = (double*)h->b_ewgt[0].p;
  launch_ecpb_fill(h, B, A, W);
  TRY(check_launch(h, "k_ecpb_fill"));
  TRY(copy_in(h, weight, A.out_w, (size_t)W * nsel * sizeof(double)));
  return copy_out(h, pos, A.out_pos, (size_t)W * nsel * 3 * sizeof(double));
}

extern "C" int pqa_set_ewald(pqa_handle_t* h, double alpha, int32_t ng, const double* gpoints, const double* gweight,
                             const double* ion_cos, const double* ion_sin, double ee_const, double ei_const, double ii,
                             const int32_t* gidx, const double* recip) {
  HIPCHK(hipSetDevice(h->device));
  if (!h->S.pbc) FAIL("Ewald tables on an open-boundary handle");
  if (ng < 0 || !(alpha > 0.0)) FAIL("bad Ewald parameters");
  HIPCHK(hipStreamSynchronize(h->stream));
  double* d;
  TRY(upload_table(h, gpoints, (size_t)ng * 3, &d)); h->ew.g = d;
  TRY(upload_table(h, gweight, (size_t)ng, &d)); h->ew.gweight = d;
  TRY(upload_table(h, ion_cos, (size_t)ng, &d)); h->ew.ion_cos = d;
  TRY(upload_table(h, ion_sin, (size_t)ng, &d)); h->ew.ion_sin = d;
  h->ew.ng = ng; h->ew.alpha = alpha; h->ew.ee_const = ee_const; h->ew.ei_const = ei_const;
  h->ew.gn = nullptr; h->ew.nmax = 0;
  if (gidx && recip && ng > 0) {
    std::vector<int> gi((size_t)ng * 3);
    HIPCHK(hipMemcpy(gi.data(), gidx, gi.size() * sizeof(int), hipMemcpyDefault));
    int nmax = 0;
    for (int v : gi) nmax = std::max(nmax, std::abs(v));
    const size_t lds = ((size_t)h->N * 3 + (size_t)h->N * 3 * (nmax + 1) * 2) * sizeof(double);
    if (lds <= 64 * 1024) {  // otherwise stay with the direct sincos form
      int* dgi;
      TRY(upload_table(h, gi.data(), gi.size(), &dgi));
      h->ew.gn = dgi; h->ew.nmax = nmax;
      HIPCHK(hipMemcpy(h->ew.recip, recip, 9 * sizeof(double), hipMemcpyDefault));
    }
  }
  h->ii_energy = ii;
  h->ew_set = true;
  return 0;
}

extern "C" int pqa_get_wrap(pqa_handle_t* h, int32_t* wrap) {
  HIPCHK(hipSetDevice(h->device));
  if (!h->S.pbc) FAIL("open-boundary handle has no wrap counters");
  if (h->wrap_W != h->W || h->W == 0) FAIL("no fused sweep has run on the resident walkers");
  return copy_out(h, wrap, h->b_wrap.p, (size_t)h->W * h->N * 3 * sizeof(int));
}

extern "C" int pqa_energy(pqa_handle_t* h, double threshold, const double* rot, const double* unif, uint64_t seed, double* out) {
  TRY(sync_aos(h));
  HIPCHK(hipSetDevice(h->device));
  if (h->W == 0) FAIL("state not initialised (call pqa_wf_recompute)");
  h->saved_valid = false;
  TRY(energy_dev(h, threshold, rot, unif, seed, 0u));
  return copy_out(h, out, h->b_en.p, (size_t)(h->cplx ? 7 : 6) * h->W * sizeof(double));
}

extern "C" int pqa_energy_last(pqa_handle_t* h, double* out) {
  HIPCHK(hipSetDevice(h->device));
  if (h->W == 0 || h->en.W != h->W) FAIL("no energy evaluation has run on the resident walkers");
  return copy_out(h, out, h->b_en.p, (size_t)(h->cplx ? 7 : 6) * h->W * sizeof(double));
}

