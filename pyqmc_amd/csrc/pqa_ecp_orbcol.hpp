// Slater ratios of the ECP quadrature points from the inverse COLUMN, without molecular-orbital rows.
//
// The semi-local ECP term needs one number per quadrature point r' of electron e: ratio = sum_k phi_occ[k](r') T[k][e].  k_orb<1> evaluates all
// nmo orbital values of every point (an nao x nmo fp64 MFMA contraction per point behind a K-chunked LDS tile), writes them out, and
// k_ecp_point_lw reads them back for the dot product.  Contracted the other way round, the points of one (walker, electron) pair — a RUN of 6
// to 50 consecutive entries of the point list — share
//     V[mu] = sum_k C[mu][occ[k]] T[k][e],        ratio(r') = sum_mu AO_mu(r') V[mu],
// so the nao x n product is paid once per run and a point costs its AO values and one multiply-add per AO: no tile, no chunks, no rows in HBM.
//
// Block = 256 threads, 64 consecutive points of one spin's list, lane = point (the launch shape of k_orb<.., TP = 64>).
//   prologue   the basis tables go to LDS (as k_orb's LDSTAB path); run heads by ballot, run index = prefix popcount; the runs' inverse columns
//              go to LDS; thread = AO row mu forms V[run][mu] for up to PQA_OC_R runs, k = 0 .. n-1 in that order (fused multiply-adds)
//   main loop  wave wv takes the shells k_orb's 64-point lists give lane group wv (all chunks: the lists are balanced by cost) and every AO value
//              feeds acc = fma(value, V[run(lane)][mu], acc)
//   epilogue   the four waves' partial sums meet in LDS; lane p of wave 0 adds them in wave order 0, 1, 2, 3 and stores ratio[p]
// Every order is fixed and a block's composition depends on the point list alone: two evaluations give the same bits, with the point totals read
// back or left on the device (PointAddr::count).  More than PQA_OC_R runs in a block (rules of fewer than four points: none today): further
// passes over the block's runs, each lane keeping the sum of the pass its run belongs to.
#pragma once
#include "pqa_ao.hpp"
#include "pqa_ecp.hpp"

#define PQA_OC_R 16  // runs whose V columns a block holds at a time (64 points of 6-point rules: 12 runs at most)
// LDS of a block: the static tables below + dynamic [PQA_OC_R][nao | 1] (V: an odd stride, so lanes of different runs read different banks)
// + [n rounded up to PQA_OC_KC][PQA_OC_R] (the runs' inverse columns, zero beyond n)
#define PQA_OC_KC 32  // coefficients of its AO row a thread holds in registers at a time
#define PQA_OC_STATIC_LDS ((size_t)PQA_WS_MAXSH * (3 * sizeof(double) + 6 * sizeof(int)) + (size_t)PQA_WS_MAXP * 2 * sizeof(double) + 4 * 64 * sizeof(double) + 2 * 64 * sizeof(int))
__host__ __device__ inline size_t ecp_orbcol_lds(int nao, int n) { return (size_t)PQA_OC_R * ((size_t)(nao | 1) + (size_t)((n + PQA_OC_KC - 1) / PQA_OC_KC * PQA_OC_KC)) * sizeof(double); }

// ratio[p] for the points p < P (or < *pa.count) of spin s; pte / ptw: the points' electron and walker (EcpBuf); T from the resident planes.
// grid = ceil(P / 64), block = 256, dynamic LDS = ecp_orbcol_lds(nao, n_s); needs nshell <= PQA_WS_MAXSH and nprim <= PQA_WS_MAXP.
static __global__ __launch_bounds__(256) void k_ecp_orbcol(SysDev S, LwState L, ChunkTab T, int s, PointAddr pa, long P, const int* __restrict__ pte,
                                                    const int* __restrict__ ptw, long W, double* __restrict__ ratio) {
  P = point_count(pa, P);
  const long p0 = (long)blockIdx.x * 64;
  if (p0 >= P) return;
  extern __shared__ __align__(16) double oc_lds[];
  __shared__ double sh_xyz[PQA_WS_MAXSH][3];
  __shared__ int sh_meta[PQA_WS_MAXSH][6];  // l, nprim, first primitive, first AO row, radial table offset (-1: none) and intervals
  __shared__ double pr_exp[PQA_WS_MAXP], pr_coef[PQA_WS_MAXP];
  __shared__ double part[4][64];
  __shared__ int run_i[64], run_w[64];  // the block's runs: row of the spin's inverse, walker
  const int tid = threadIdx.x, lane = tid & 63, wv = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int n = s ? S.ndn : S.nup, nmo = S.nmo[s], nao = S.nao, vs = nao | 1, nk = (n + PQA_OC_KC - 1) / PQA_OC_KC * PQA_OC_KC;
  const int* __restrict__ occ = S.det_occ[s];
  const bool ident = S.occ_ident[s] != 0;
  const double* __restrict__ Cs = S.mo[s];
  // PQA_OC_KC coefficients of AO row mu from column k0 on, zero beyond the row's n: all loads of a call are in flight together
  double c[PQA_OC_KC];
  auto load_row = [&](int mu, int k0) {
    const double* __restrict__ crow = Cs + (size_t)mu * nmo;
    if (ident && (nmo & 3) == 0 && k0 + PQA_OC_KC <= n) {
#pragma unroll
      for (int u = 0; u < PQA_OC_KC; u += 4) {
        const double4 q = *reinterpret_cast<const double4*>(crow + k0 + u);
        c[u] = q.x; c[u + 1] = q.y; c[u + 2] = q.z; c[u + 3] = q.w;
      }
    } else {
#pragma unroll
      for (int u = 0; u < PQA_OC_KC; ++u) {
        const int k = k0 + u;
        c[u] = (k < n) ? crow[ident ? k : occ[k]] : 0.0;
      }
    }
  };
  // the first (in every system that fits one pass of 256 rows and PQA_OC_KC columns: the only) piece of this thread's row is requested
  // now, so that its round trip runs under the staging of the tables and the gather of the inverse columns
  bool have_c = tid < nao;
  if (have_c) load_row(tid, 0);
  const bool c_stays = nao <= 256 && n <= PQA_OC_KC;
  for (int sh = tid; sh < S.nshell; sh += 256) {
    const int ia = S.shell_atom[sh];
    sh_xyz[sh][0] = S.atom_xyz[3 * ia]; sh_xyz[sh][1] = S.atom_xyz[3 * ia + 1]; sh_xyz[sh][2] = S.atom_xyz[3 * ia + 2];
    sh_meta[sh][0] = S.shell_l[sh];
    sh_meta[sh][1] = S.shell_prim_off[sh + 1] - S.shell_prim_off[sh];
    sh_meta[sh][2] = S.shell_prim_off[sh];
    sh_meta[sh][3] = S.shell_ao_off[sh];
    sh_meta[sh][4] = S.shell_rt[2 * sh]; sh_meta[sh][5] = S.shell_rt[2 * sh + 1];
  }
  for (int p = tid; p < S.nprim; p += 256) { pr_exp[p] = S.prim_exp[p]; pr_coef[p] = S.prim_coef[p]; }
  const long pmine = (p0 + lane < P) ? p0 + lane : P - 1;  // (lanes past the list repeat its last point: no new run, nothing stored)
  double px, py, pz;
  load_point(pa, pmine, px, py, pz);
  const int e = pte[pmine], w = ptw[pmine];
  // runs: maximal stretches of consecutive points of the block with equal (walker, electron)
  const int e_prev = __shfl_up(e, 1, 64), w_prev = __shfl_up(w, 1, 64);
  const bool head = lane == 0 || e != e_prev || w != w_prev;
  const unsigned long long heads = __ballot(head);
  const int run = __popcll(heads & (~0ull >> (63 - lane))) - 1, nrun = __popcll(heads);
  if (wv == 0 && head) { run_i[run] = e - s * S.nup; run_w[run] = w; }
  double* V = oc_lds;                             // [PQA_OC_R][vs]
  double* tc = oc_lds + (size_t)PQA_OC_R * vs;    // [nk][PQA_OC_R]
  const double* __restrict__ Tt = L.Tt[s];
  const int* __restrict__ cw_off = T.cw_off[0];
  const int* __restrict__ cw_shell = T.cw_shell[0];
  double acc = 0.0;
  for (int r0 = 0; r0 < nrun; r0 += PQA_OC_R) {
    const int nr = (nrun - r0 < PQA_OC_R) ? nrun - r0 : PQA_OC_R;
    __syncthreads();  // tables and runs staged (a further pass: the last pass's V has been read)
    for (int idx = tid; idx < nk * PQA_OC_R; idx += 256) {
      const int k = idx / PQA_OC_R, r = idx % PQA_OC_R;
      tc[idx] = (r < nr && k < n) ? Tt[((size_t)run_i[r0 + r] * n + k) * W + run_w[r0 + r]] : 0.0;
    }
    __syncthreads();
    for (int mu = tid; mu < nao; mu += 256) {  // the row's coefficients from registers for every run; the columns by broadcast reads, four runs each
      double v[PQA_OC_R];
#pragma unroll
      for (int r = 0; r < PQA_OC_R; ++r) v[r] = 0.0;
      for (int k0 = 0; k0 < nk; k0 += PQA_OC_KC) {
        if (!(have_c && mu == tid && k0 == 0)) load_row(mu, k0);
        if (!c_stays) have_c = false;
#pragma unroll
        for (int g = 0; g < PQA_OC_R; g += 4) {
          if (g < nr) {
#pragma unroll
            for (int u = 0; u < PQA_OC_KC; ++u) {
              const double4 t = *reinterpret_cast<const double4*>(tc + (k0 + u) * PQA_OC_R + g);
              v[g] = fma(c[u], t.x, v[g]); v[g + 1] = fma(c[u], t.y, v[g + 1]); v[g + 2] = fma(c[u], t.z, v[g + 2]); v[g + 3] = fma(c[u], t.w, v[g + 3]);
            }
          }
        }
      }
#pragma unroll
      for (int g = 0; g < PQA_OC_R; g += 4)
        if (g < nr) { V[g * vs + mu] = v[g]; V[(g + 1) * vs + mu] = v[g + 1]; V[(g + 2) * vs + mu] = v[g + 2]; V[(g + 3) * vs + mu] = v[g + 3]; }
    }
    __syncthreads();
    const bool mine = run >= r0 && run < r0 + nr;
    const double* __restrict__ Vr = V + (mine ? run - r0 : 0) * vs;
    double a = 0.0;
    for (int ch = 0; ch < T.nchunk; ++ch) {
      const int s_end = cw_off[ch * 4 + wv + 1];
      for (int si = cw_off[ch * 4 + wv]; si < s_end; ++si) {
        const int sh = cw_shell[si];
        // (the shell is the same for the whole wave: scalar control flow in the angular switch and the primitive loop)
        const int l_ = __builtin_amdgcn_readfirstlane(sh_meta[sh][0]), np_ = __builtin_amdgcn_readfirstlane(sh_meta[sh][1]);
        const int q0 = __builtin_amdgcn_readfirstlane(sh_meta[sh][2]), row = __builtin_amdgcn_readfirstlane(sh_meta[sh][3]);
        const int rt_ = __builtin_amdgcn_readfirstlane(sh_meta[sh][4]), rn_ = __builtin_amdgcn_readfirstlane(sh_meta[sh][5]);
        const double x = px - sh_xyz[sh][0], y = py - sh_xyz[sh][1], z = pz - sh_xyz[sh][2];
        auto to_sum = [&](int m, double v, double, double, double, double) { a = fma(v, Vr[row + m], a); };
        if (rt_ >= 0) shell_eval_tab(l_, x, y, z, S.rtab + rt_, rn_, to_sum);  // contracted shell: the radial sum from its table
        else shell_eval<1>(l_, x, y, z, pr_exp + q0, pr_coef + q0, np_, to_sum);
      }
    }
    if (mine) acc = a;
  }
  part[wv][lane] = acc;
  __syncthreads();
  if (wv == 0 && p0 + lane < P) ratio[p0 + lane] = ((part[0][lane] + part[1][lane]) + part[2][lane]) + part[3][lane];
}
