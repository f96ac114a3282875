// pyqmc_amd C ABI implementation (host side): the resident electron sweep (pqa_res.hpp) — tables, eligibility, launch.
// Chosen by sweep_route (pqa_sweep.hip) in place of the per-move launches of the lane-per-walker sweep.
#include "pqa_internal.hpp"

// Every instantiation of the kernel, [plain | PBC | PBC + CX][LMAX 2 | 3; the complex row 3 | 2][DMC]: the table drives the dynamic-LDS
// attribute (res_setup) and the launch (res_kernel, sweep_res).  (s, p, d shells: 25 running sums of a shell's lattice sum in registers;
// with f shells 35.)  The complex row lists LMAX 3 first because the compiler emits the kernels in the order the unit names them: this is
// the order it always has, and the unit's device code stays what it was byte for byte.
using ResKernel = void (*)(SysDev, LwState, MoveBuf, ChunkTab, ResTab, int, long, long, long);
static const ResKernel res_kernels[3][2][2] = {
    {{k_sweep_res<false, 2>, k_sweep_res<true, 2>}, {k_sweep_res<false, 3>, k_sweep_res<true, 3>}},
    {{k_sweep_res<false, 2, true>, k_sweep_res<true, 2, true>}, {k_sweep_res<false, 3, true>, k_sweep_res<true, 3, true>}},
    {{k_sweep_res<false, 3, true, true>, k_sweep_res<true, 3, true, true>}, {k_sweep_res<false, 2, true, true>, k_sweep_res<true, 2, true, true>}}};
static ResKernel res_kernel(const pqa_handle* h, bool dmc) {
  const int variant = h->cplx ? 2 : (h->S.pbc ? 1 : 0);
  return res_kernels[variant][(h->lmax > 2) != (variant == 2)][dmc];
}

// Dense coefficient copy d_cres[s] [res_rows_alloc(rows4)][ldc] of spin s in AO order (rows beyond nao and columns beyond nmo zero).
// mo_host: set_mo's new coefficients — refreshes the copy if a setup has made one; nullptr (the setups): allocated on first use and
// filled from d_mo[s].
int cres_upload(pqa_handle* h, int s, const double* mo_host) {
  if (h->nmo[s] == 0 || (mo_host && !h->d_cres[s])) return 0;
  const int ldc = 16 * h->nt[s], nmo = h->nmo[s];
  std::vector<double> pad((size_t)res_rows_alloc(res_rows4(h)) * ldc, 0.0), mo;  // (zero rows behind the basis: k_sweep_r8's K split)
  if (!mo_host) {
    mo.resize((size_t)h->nao * nmo);
    HIPCHK(hipMemcpy(mo.data(), h->d_mo[s], mo.size() * sizeof(double), hipMemcpyDeviceToHost));
    mo_host = mo.data();
    if (!h->d_cres[s]) TRY(upload_table<double>(h, nullptr, pad.size(), &h->d_cres[s]));
  }
  for (int a = 0; a < h->nao; ++a)
    for (int j = 0; j < nmo; ++j) pad[(size_t)a * ldc + j] = mo_host[(size_t)a * nmo + j];
  if (h->twist) {  // rows nao .. 2 nao: the imaginary AO parts, (i AO_im)(C_re + i C_im) = AO_im (-C_im + i C_re), columns [re | im] (upload_cpad)
    const int nr = nmo / 2;
    for (int a = 0; a < h->nao; ++a)
      for (int j = 0; j < nr; ++j) {
        pad[(size_t)(h->nao + a) * ldc + j] = -mo_host[(size_t)a * nmo + nr + j];
        pad[(size_t)(h->nao + a) * ldc + nr + j] = mo_host[(size_t)a * nmo + j];
      }
  }
  HIPCHK(hipStreamSynchronize(h->stream));
  HIPCHK(hipMemcpy(h->d_cres[s], pad.data(), pad.size() * sizeof(double), hipMemcpyHostToDevice));
  return 0;
}

// Primitives: shells with the same (exponent, coefficient) sequence — the same shell of every atom of a species — share one LDS copy.
// pe_u / pc_u: the distinct sequences; q0_u[shell]: where the shell's sequence starts in them.
int unique_primitives(pqa_handle* h, std::vector<double>& pe_u, std::vector<double>& pc_u, std::vector<int>& q0_u) {
  std::vector<double> pe((size_t)h->S.nprim), pc((size_t)h->S.nprim);
  std::vector<int> po((size_t)h->nshell + 1);
  HIPCHK(hipMemcpy(pe.data(), h->S.prim_exp, pe.size() * sizeof(double), hipMemcpyDeviceToHost));
  HIPCHK(hipMemcpy(pc.data(), h->S.prim_coef, pc.size() * sizeof(double), hipMemcpyDeviceToHost));
  HIPCHK(hipMemcpy(po.data(), h->S.shell_prim_off, po.size() * sizeof(int), hipMemcpyDeviceToHost));
  q0_u.assign((size_t)h->nshell, 0);
  for (int sh = 0; sh < h->nshell; ++sh) {
    const int n = po[sh + 1] - po[sh];
    int found = -1;
    for (int prev = 0; prev < sh && found < 0; ++prev)
      if (po[prev + 1] - po[prev] == n && std::equal(pe.begin() + po[sh], pe.begin() + po[sh + 1], pe.begin() + po[prev]) &&
          std::equal(pc.begin() + po[sh], pc.begin() + po[sh + 1], pc.begin() + po[prev])) found = q0_u[prev];
    if (found < 0) { found = (int)pe_u.size(); pe_u.insert(pe_u.end(), pe.begin() + po[sh], pe.begin() + po[sh + 1]); pc_u.insert(pc_u.end(), pc.begin() + po[sh], pc.begin() + po[sh + 1]); }
    q0_u[sh] = found;
  }
  return 0;
}

// Passes over the padded coefficient rows of the 16-row chunk table (h->chunks[0]: the coefficient matrices cpad[0] are shared
// with k_orb), shell lists per (pass, lane group), LDS budget.  Once per handle (res_plan); returns 0 and leaves res.ok = false when the system is
// outside the kernel's scope, an error code (h->err set) when the device refuses a copy, an allocation or the LDS attribute.
static int res_setup(pqa_handle* h) {
  h->res.ok = false;
  if (h->res.mode == 0) return 0;
  if (!h->has_slater || h->ndet != 1 || h->has_j3) return 0;
  // complex determinants: periodic cells (twisted or not), 16 electrons and 16 orbitals per spin — a row of the inverse is 32 doubles
  if (h->cplx && (!h->S.pbc || h->nup > 16 || h->ndn > 16)) return 0;
  if (h->twist && !h->cplx) return 0;
  if (h->S.pbc && (h->S.nL <= 0 || h->pbc_high_l || !h->pbc_lists_ok)) return 0;  // periodic: lattice-summed orbitals, l <= 3
  if (h->nup > 32 || h->ndn > 32 || h->nmo[0] > 32 || h->nmo[1] > 32 || h->N > 64 || h->N < 1 || h->natom > 64) return 0;
  if (h->lmax > 3) return 0;
  const ChunkHost& c = h->chunks[0];
  const int nch = (int)c.nk.size();
  if (nch == 0) return 0;
  std::vector<double> pe_u, pc_u;
  std::vector<int> q0_u;
  TRY(unique_primitives(h, pe_u, pc_u, q0_u));
  const int nprim_u = (int)pe_u.size();
  int rows_cap = 1 << 30;
  size_t part_rn = 0;
  for (int s = 0; s < 2; ++s) {
    if ((s ? h->ndn : h->nup) == 0) continue;
    const int nt = h->nt[s];
    if (nt < 1 || nt > 2) return 0;
    rows_cap = std::min(rows_cap, 4 * PQA_RES_MAXKS * (8 / nt));
    part_rn = std::max(part_rn, (size_t)(8 / nt) * 16 * res_ps(nt) + (size_t)16 * PQA_RES_RS);
  }
  // periodic: the image lists take what is left beside a one-pass tile — up to 32 entries per (point, atom), at least 10
  int icap = 0;
  size_t pbc_b = 0;
  auto pick_icap = [&](size_t rest) {  // largest capacity whose lists fit `rest` bytes (0: none)
    for (int cand = 32; cand >= 10; --cand)
      if (res_lds_pbc(h->natom, h->S.nL, cand, h->nshell, h->twist) + 8 <= rest) return cand;
    return 0;
  };
  if (h->S.pbc) {
    const size_t f0 = res_lds_fixed(h->nshell, nprim_u, h->natom, h->na, h->nshell, PQA_RES_MAXPASS);
    const size_t tile = (size_t)80 * c.rows_pad * sizeof(double), budget0 = (size_t)160 * 1024 - 256;
    icap = f0 + tile < budget0 ? pick_icap(budget0 - f0 - tile) : 0;
    if (icap == 0) icap = 10;
    pbc_b = res_lds_pbc(h->natom, h->S.nL, icap, h->nshell, h->twist) + 8;
  }
  const size_t fixed = res_lds_fixed(h->nshell, nprim_u, h->natom, h->na, h->nshell, PQA_RES_MAXPASS) + pbc_b;
  const size_t budget = 160 * 1024 - 256;
  if (fixed + part_rn * sizeof(double) > budget) return 0;
  const size_t avail = (budget - fixed) / sizeof(double);
  // one pass if the whole basis fits (the partials then reuse the tile's memory); otherwise the tile shares the region with them
  const int rows_all = c.rows_pad;
  // (twisted cells: dense rows only — the real rows of the whole basis, then the imaginary rows)
  const bool one = !h->twist && rows_all <= rows_cap && (size_t)80 * rows_all <= avail;
  // dense mode: the chunk padding (16-row chunks: 224 rows for the 208 AOs of the 2x2x2 diamond cell) is what keeps the basis out of one
  // tile, and the AOs in their own order (padded to x4) fit
  const int rows4 = res_rows4(h);
  const size_t fixed1 = res_lds_fixed(h->nshell, nprim_u, h->natom, h->na, h->nshell, 1);
  bool dense = false;
  if (!one && rows4 <= rows_cap) {
    const size_t tile = std::max((size_t)80 * rows4, part_rn) * sizeof(double) + 8;
    if (!h->S.pbc) dense = fixed1 + tile <= budget;
    else if (fixed1 + tile < budget) {
      const int cand = pick_icap(budget - fixed1 - tile);
      if (cand > 0) { dense = true; icap = cand; pbc_b = res_lds_pbc(h->natom, h->S.nL, cand, h->nshell, h->twist) + 8; }
    }
  }
  if (h->twist && !dense) return 0;
  const int kt_cap = (one || dense) ? (dense ? rows4 : rows_all) : std::min(rows_cap, (int)(((avail - part_rn) / 80) & ~(size_t)3));
  if (kt_cap < 20) return 0;
  ResTab RT{};
  h->res.dense = dense;
  if (dense)
    for (int s = 0; s < 2; ++s) TRY(cres_upload(h, s, nullptr));
  int ch = 0, kt = 0;
  std::vector<int> pass_of_chunk((size_t)nch, 0);
  if (dense) {
    RT.npass = 1; RT.pass_row0[0] = 0; kt = rows4; ch = nch;
  }
  while (ch < nch) {  // greedy: consecutive chunks while their padded rows fit the tile
    if (RT.npass == PQA_RES_MAXPASS) return 0;
    const int base = c.row0[ch];
    int end = ch;
    while (end < nch && c.row0[end] + ((c.nk[end] + 3) & ~3) - base <= kt_cap) ++end;
    if (end == ch) return 0;
    for (int q = ch; q < end; ++q) pass_of_chunk[q] = RT.npass;
    RT.pass_row0[RT.npass] = base;
    kt = std::max(kt, c.row0[end - 1] + ((c.nk[end - 1] + 3) & ~3) - base);
    ch = end;
    ++RT.npass;
  }
  RT.pass_row0[RT.npass] = dense ? rows4 : c.rows_pad;
  RT.kt = kt;
  RT.part_off = (RT.npass == 1) ? 0 : 80 * kt;
  RT.region = (RT.npass == 1) ? (int)std::max((size_t)80 * kt, part_rn) : (int)((size_t)80 * kt + part_rn);
  // shell lists: per pass the shells by descending phase-1 cost, dealt to the 32 lane groups in snake order — neighbours in cost
  // (the same kind of shell) land in neighbouring groups, i.e. in one wave, and the groups' totals stay balanced
  std::vector<int> off(1, 0), list, srow((size_t)h->nshell, 0);
  for (int sh = 0; sh < h->nshell; ++sh) srow[sh] = dense ? h->shell_ao[sh] : c.row0[c.shell_chunk[sh]] + c.shell_kb[sh];
  for (int p = 0; p < RT.npass; ++p) {
    std::vector<int> mem;
    for (int sh = 0; sh < h->nshell; ++sh)
      if (pass_of_chunk[c.shell_chunk[sh]] == p) mem.push_back(sh);
    std::stable_sort(mem.begin(), mem.end(), [&](int a, int b) {
      if (h->shell_cost[a] != h->shell_cost[b]) return h->shell_cost[a] > h->shell_cost[b];
      return h->shell_l[a] > h->shell_l[b];
    });
    std::vector<std::vector<int>> grp(PQA_RES_G);
    for (size_t k = 0; k < mem.size(); ++k) {
      const int round = (int)(k / PQA_RES_G), pos = (int)(k % PQA_RES_G);
      grp[(round & 1) ? PQA_RES_G - 1 - pos : pos].push_back(mem[k]);
    }
    for (int g = 0; g < PQA_RES_G; ++g) {
      for (int sh : grp[g]) list.push_back(sh);
      off.push_back((int)list.size());
    }
  }
  RT.nlist = (int)list.size();
  int* tmp_i = nullptr;
  TRY(upload_table(h, off.data(), off.size(), &tmp_i)); RT.grp_off = tmp_i;
  TRY(upload_table(h, list.data(), list.size(), &tmp_i)); RT.grp_shell = tmp_i;
  TRY(upload_table(h, srow.data(), srow.size(), &tmp_i)); RT.shell_row = tmp_i;
  TRY(upload_table(h, q0_u.data(), q0_u.size(), &tmp_i)); RT.shell_q0 = tmp_i;
  double* tmp_d = nullptr;
  TRY(upload_table(h, pe_u.data(), pe_u.size(), &tmp_d)); RT.prim_exp_u = tmp_d;
  TRY(upload_table(h, pc_u.data(), pc_u.size(), &tmp_d)); RT.prim_coef_u = tmp_d;
  RT.nprim_u = nprim_u;
  h->res.lds = (size_t)RT.region * sizeof(double) + res_lds_fixed(h->nshell, nprim_u, h->natom, h->na, RT.nlist, RT.npass);
  h->res.lds = (h->res.lds + 7) & ~(size_t)7;
  RT.pbc_off = (int)h->res.lds; RT.icap = icap;
  RT.twist = h->twist ? 1 : 0; RT.im_off = h->nao;
  if (const char* e = getenv("PQA_RES_ICAP")) RT.icap = std::max(1, std::min(icap, atoi(e)));  // (tests: short lists, the pairs that overflow walk the masks)
  h->res.lds += pbc_b;
  if (h->res.lds > 160 * 1024) return 0;
  for (const auto& variant : res_kernels)
    for (const auto& lm : variant)
      for (ResKernel k : lm) HIPCHK(hipFuncSetAttribute((const void*)k, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024));
  if (const char* dbg = getenv("PQA_RES_DEBUG"); dbg && atoi(dbg) > 1) {  // the lane groups' shell lists with the cost model's figures
    for (int g = 0; g < PQA_RES_G * RT.npass; ++g) {
      fprintf(stderr, "[pqa_res] group %2d:", g);
      for (int k = off[g]; k < off[g + 1]; ++k) fprintf(stderr, " sh %d (l %d, np %d, cost %d)", list[k], h->shell_l[list[k]], h->shell_np[list[k]], h->shell_cost[list[k]]);
      fprintf(stderr, "\n");
    }
  }
  if (getenv("PQA_RES_DEBUG")) fprintf(stderr, "[pqa_res] passes %d, tile rows %d (padded basis %d), LDS %zu B, image-list capacity %d\n", RT.npass, RT.kt, c.rows_pad, h->res.lds, RT.icap);
  h->res.tab = RT;
  h->res.ok = true;
  return 0;
}

static bool res_auto(const pqa_handle* h, long W) {
  // automatic: measured against the launch-per-move sweep (gpurun_out/res_scan.jsonl, round 5; sweep only): (H2O)8 1.66x at 512
  // walkers, 1.88x at 4096, 1.38x at 16384, 1.06x at 32768, 1.02x at 49152, 0.97x at 65536; H2O (8 electrons: a walker's 32 lanes
  // are mostly idle) 1.2x up to 4096 walkers, 0.49x at 16384.  One round of blocks (16 walkers per CU) always wins.
  // periodic cells (lattice-summed AO phase in the block, round 5; 2x2x2 diamond cell, sweep alone, launches -> resident): 4.10 -> 2.71 ms at
  // 2048 walkers, 4.43 -> 2.74 at 4096, 7.56 -> 5.48 at 8192, 12.5 -> 10.9 at 16384, 17.2 -> 16.4 at 24576, even at 32768
  // (after the image lists were dealt to several threads per pair and the lattice sums went to ds_add_f64: DMC step 13.6 -> 12.1 ms at 4096,
  // 43.3 -> 41.4 at 16384, 82.8 -> 82.1 at 32768)
  // complex determinants (twisted 8-atom cell, VMC step with energy, launches -> resident): 4.29 -> 2.90 ms at 4096 walkers, 6.69 -> 5.33 at 8192,
  // 8.57 -> 7.76 at 12288, 10.8 -> 10.2 at 16384
  // (with the instantiation for bases without f shells: 15.3 -> 14.5 ms at 24 576 walkers, 19.7 -> 19.3 at 32 768)
  if (h->cplx) return W <= 32768;
  if (h->S.pbc) return W <= 32768;
  return W <= 4096 || (std::max(h->nup, h->ndn) >= 16 && W <= 49152);
}
int res_plan(pqa_handle* h, long W, bool* use) {
  *use = false;
  if (!h->res.ready) { TRY(res_setup(h)); h->res.ready = true; }  // (a setup that failed is tried, and fails, again)
  *use = h->res.ok && (h->res.mode > 0 || res_auto(h, W));
  return 0;
}

// What a one-launch sweep does in front of its launch: both tapes are there; under the profiler the launch is bracketed (one launch per
// sweep: every one) — *e1 is the closing event the caller records behind the launch, nullptr without the profiler.
int sweep_launch_begin(pqa_handle* h, const MoveBuf& mb, hipEvent_t* e1) {
  *e1 = nullptr;
  if (!mb.gauss || !mb.unif) FAIL("resident sweep: the random-number tapes are missing");
  if (!h->profile) return 0;
  hipEvent_t e0 = nullptr;
  TRY(prof_acquire(h, h->prof_orb, e0, *e1));
  HIPCHK(hipEventRecord(e0, h->stream));
  h->prof_orb.launches += 1;
  h->prof_pc += (double)h->W * h->N * 5;  // point-components of this launch (as launch_orb counts them)
  return 0;
}

// One sweep over all electrons of walkers [0, W): a single launch.  mb carries both tapes (the caller drew them if there were none).
int sweep_res(pqa_handle* h, const MoveBuf& mb) {
  hipEvent_t e1 = nullptr;
  TRY(sweep_launch_begin(h, mb, &e1));
  const long W = h->W;
  const LwState L = lw_state(h);
  ChunkTab Tc = h->tab[0];
  if (h->res.dense) { Tc.cpad[0] = h->d_cres[0]; Tc.cpad[1] = h->d_cres[1]; }
  const dim3 grid((unsigned)((W + PQA_RES_NW - 1) / PQA_RES_NW)), block(PQA_RES_NT);
  hipLaunchKernelGGL(res_kernel(h, mb.dmc != 0), grid, block, h->res.lds, h->stream, h->S, L, mb, Tc, h->res.tab, (int)h->has_jastrow, W, 0L, W);
  if (e1) HIPCHK(hipEventRecord(e1, h->stream));
  return check_launch(h, "k_sweep_res");
}
