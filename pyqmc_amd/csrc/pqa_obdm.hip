// One-body density matrix (OBDMAccumulator, pyqmc/observables/obdm.py:139-193) from the resident state: every auxiliary sweep of one
// evaluation in one call, read-only on the wave function's handle, contracted on the orbital evaluator's handle without a trip
// through the host.
//
// For walker w and sweep s let r' be the auxiliary walker assign[s][w] of kept sample s of the evaluator's slot, F = f(r') / norb,
// and e run over the listed electrons es:
//
//   b[w][i]    = phi_i(r') / F                                                   (the slot's kept rows and densities)
//   R[w][e]    = Psi(r_e -> r') / Psi = (sum_D w_D v_D(r')[e] / sum_D w_D) exp(A_e(r'))
//   v_D(q)[e]  = sum_k phi^s_{occ_D[k]}(q) T^s_D[e][k]                           (the single-move ratio; T the electron-major inverse)
//   A_e(q)     = U(e -> q) - U                                                   (two-body Jastrow factor, as k_tbdm_pairs forms it)
//   t[w][j]    = sum_e R[w][e] phi_j(r_e)
//   value[w]  += b[w] (x) t[w],   norm[w][i] += phi_i(r')^2 / F
//
// The estimator is a rank-one update per walker and sweep, so its walker mean is a thin product, value_mean = B^T T / W with the
// (W, norb) panels B and T: k_obdm_mean runs it on v_mfma_f64_16x16x4_f64 with the walkers as the k dimension, and no per-walker
// (norb, norb) matrix exists in that mode.  The per-walker mode hands the ratios to k_obdm_acc (pqa_dm.hpp) on the device, after
// which the evaluator holds exactly what pqa_obdm_accumulate leaves.
//
// Every sum has a fixed order that does not depend on the walker chunk: a slice of the mean product is kSlice consecutive walkers
// counted from walker 0 (chunks hold whole slices), a slice's partial tile is one MFMA chain, and k_obdm_reduce adds the partial tiles
// to the running sums one after the other in slice order, sweep after sweep.
//
// Complex and twisted handles, complex evaluators (pqa_obdm_sweeps_c; the same host driver, obdm_sweeps, with DmEntry::cx set):
//
//   b[w][j]  = phi_j(r') / F,  F = sum_i |phi_i(r')|^2 / norb                     (complex / real)
//   R[w][e]  = (sum_D w_D v_D(r')[e] / sum_D w_D) exp(A_e(r'))                     (complex; A_e real)
//   w_D      = c_D phase_up,D phase_dn,D exp(log_up,D + log_dn,D - ref)            (complex: dsign holds unit phases, pqa_cslater.hpp)
//   t[w][k]  = conj( sum_e R[w][e] phi_k(r_e) )
//   value[w] += b[w] (x) t[w],   norm[w][j] += |phi_j(r')|^2 / F                   (no further conjugation; the norm is real)
//
// k_obdm_rt_c forms R from the interleaved complex inverse (or, for a real handle, the real one with imaginary parts exactly 0) and
// writes PLANAR panels Tr, Ti, Br, Bi and the real Nn; k_obdm_mean_c runs value_mean = B^T T / W as real products,
//   Re = Br^T Tr - Bi^T Ti,   Im = Br^T Ti + Bi^T Tr,
// two accumulators per wave and two (real evaluator: Bi = 0) or four MFMAs per k-step; a slice's partials are 2 norb^2 + norb doubles
// [Re | Im | norm], reduced by k_obdm_reduce like the real ones, and k_obdm_out_c scales and interleaves them.  A twisted handle keeps
// its walkers unfolded, so k_obdm_epts hands the evaluator the true positions and its orbital kernel puts the wrap phase on
// phi_k(r_e); the wave function's own orbital launch folds r' and derives the phase there.  The per-walker mode hands the interleaved
// ratios to k_obdm_acc with rc = 1.  Slices, chunks and the order of every sum are those of the real entries.
#include "pqa_estim.hpp"
#include "pqa_j3dm.hpp"

namespace {

constexpr int kSlice = 64;  // walkers per slice of the mean product: 16 k-steps of the 16x16x4 MFMA
constexpr uint32_t kStreamAssign = 0x4f42u;  // Philox counter word of the assignment draws

// xe[(w ne + t)][3] = coordinates of listed electron es[t] of resident walker w
__global__ __launch_bounds__(256) void k_obdm_epts(const double* __restrict__ x, const int* __restrict__ es, int ne, int N, long W,
                                                   double* __restrict__ xe) {
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  if (i >= W * ne) return;
  const long w = i / ne;
  const int t = (int)(i - w * ne);
  const double* p = x + ((size_t)w * N + es[t]) * 3;
  xe[3 * i] = p[0]; xe[3 * i + 1] = p[1]; xe[3 * i + 2] = p[2];
}

// pts[wl][3] = pos[assign[w0 + wl]] for the wc walkers of a chunk.  draw: the assignment is drawn here, floor(u naux) with u from
// Philox keyed by (seed; walker, sweep), and stored.
__global__ __launch_bounds__(256) void k_obdm_gather(const double* __restrict__ pos, int* __restrict__ assign, long w0, long wc, int draw,
                                                     uint64_t seed, uint32_t sweep, long naux, double* __restrict__ pts) {
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  if (i >= wc) return;
  const long w = w0 + i;
  int a;
  if (draw) {
    const Philox ph = philox(seed, (uint32_t)w, sweep, PQA_STREAM_ACCEPT, kStreamAssign);
    const long k = (long)(u01(ph.c[0], ph.c[1]) * (double)naux);
    a = (int)(k < naux ? k : naux - 1);
    assign[w] = a;
  } else a = assign[w];
  const double* p = pos + 3 * (size_t)a;
  pts[3 * i] = p[0]; pts[3 * i + 1] = p[1]; pts[3 * i + 2] = p[2];
}

// v[d n + i] = sum_k phi[occ_d[k]] T_d[i][k] for every unique determinant d of spin s and electron i (k_tbdm_pairs' product with
// one right-hand side): GS = 2^m >= min(n, 64) lanes share a row of the inverse, a butterfly over the group adds the partial sums.
__device__ __forceinline__ void inverse_rows(const SysDev& S, const SlaterState& st, int s, long w, const double* __restrict__ phi, double* v) {
  const int lane = threadIdx.x, n = s ? S.ndn : S.nup, D = S.ndet_s[s];
  int GS = 1;
  while (GS < n && GS < 64) GS <<= 1;
  const int per = 64 / GS, g = lane / GS, j = lane & (GS - 1);
  const double* Tw = st.T[s] + (size_t)w * D * n * n;
  for (int r0 = 0; r0 < D * n; r0 += per) {
    const int r = r0 + g;
    const bool act = r < D * n;
    double p = 0.0;
    if (act) {
      const int* occ = S.det_occ[s] + (size_t)(r / n) * n;
      for (int k = j; k < n; k += GS) p += phi[occ[k]] * Tw[(size_t)r * n + k];
    }
    for (int off = 1; off < GS; off <<= 1) p += __shfl_xor(p, off, 64);
    if (act && j == 0) v[r] = p;
  }
}

// One wave per walker of the chunk.  phi_up / phi_dn [wc][nmo_s]: the wave function's orbitals at the walkers' r' (a spin without a
// listed electron: not read); pts [wc][3]; es [ne]; cfg [W][ne][norb]: the evaluator's orbitals at the listed electrons; rows / f: the
// kept sample's orbital rows [naux][norb] and densities; assign [W].  Outputs (each may be NULL): R [wc][ne], the panels T, B, Nn
// [wc][norb] (t, b and the norm term of the walker).
// Dynamic LDS (doubles): 3 N coordinates, 2 ne (Jastrow differences, ratios), ndet weights (several determinants), the v tables
// ndet_up nup + ndet_dn ndn.
// J3 (pqa_obdm_sweeps_j3 on a three-body handle): A3 [wc][ne], the three-body differences k_j3_moves left, join the exponent.
template <bool PBC, bool J3 = false>
__global__ __launch_bounds__(64) void k_obdm_rt(SysDev S, SlaterState st, JastrowState js, const double* __restrict__ phi_up,
                                                const double* __restrict__ phi_dn, const double* __restrict__ pts,
                                                const int* __restrict__ es, int ne, long w0, int jas, int spins,
                                                const double* __restrict__ cfg, const double* __restrict__ rows,
                                                const double* __restrict__ f, const int* __restrict__ assign, int norb,
                                                double* __restrict__ R, double* __restrict__ T, double* __restrict__ B,
                                                double* __restrict__ Nn, const double* __restrict__ A3) {
  extern __shared__ double lds[];
  const int N = S.nelec, lane = threadIdx.x, D = S.ndet;
  const long wl = blockIdx.x, w = w0 + wl;
  double* xs = lds;                     // [N][3]
  double* A = lds + 3 * N;              // [ne]
  double* Rl = A + ne;                  // [ne]
  double* wd = Rl + ne;                 // [D] (D > 1)
  double* vu = wd + (D > 1 ? D : 0);    // [ndet_up][nup]
  double* vd = vu + (size_t)S.ndet_s[0] * S.nup;  // [ndet_dn][ndn]
  const double* xw = js.x + (size_t)w * N * 3;
  for (int q = lane; q < 3 * N; q += 64) xs[q] = xw[q];
  const double qx = pts[3 * wl], qy = pts[3 * wl + 1], qz = pts[3 * wl + 2];
  __syncthreads();
  if (jas) {
    const double irb = 1.0 / S.rcut_b, ira = 1.0 / S.rcut_a;
    for (int t = lane; t < ne; t += 64) {  // a lane owns a listed electron
      const int e = es[t], se = e >= S.nup;
      const double ex = xs[3 * e], ey = xs[3 * e + 1], ez = xs[3 * e + 2];
      double un = 0.0, uo = 0.0;
      for (int j = 0; j < N; ++j) {
        if (j == e) continue;
        const int col = se + (j >= S.nup);
        const double jx = xs[3 * j], jy = xs[3 * j + 1], jz = xs[3 * j + 2];
        un += pair_u<PBC>(S, qx - jx, qy - jy, qz - jz, col, irb);
        uo += pair_u<PBC>(S, ex - jx, ey - jy, ez - jz, col, irb);
      }
      un += ion_u<PBC>(S, qx, qy, qz, se, ira);
      uo += ion_u<PBC>(S, ex, ey, ez, se, ira);
      A[t] = un - uo;
    }
  }
  double den = 1.0;
  if (D > 1) {  // determinant weights relative to the largest |determinant|
    const double ref = det_ref(S, st, w);
    double t = 0.0;
    for (int Dd = lane; Dd < D; Dd += 64) {
      const double x = det_weight(S, st, w, Dd, ref);
      wd[Dd] = x;
      t += x;
    }
    den = wave_sum(t);
  }
  if (spins & 1) inverse_rows(S, st, 0, w, phi_up + (size_t)wl * S.nmo[0], vu);
  if (spins & 2) inverse_rows(S, st, 1, w, phi_dn + (size_t)wl * S.nmo[1], vd);
  __syncthreads();
  for (int t = lane; t < ne; t += 64) {
    const int e = es[t], s = e >= S.nup, i = e - s * S.nup, n = s ? S.ndn : S.nup;
    const double* v = s ? vd : vu;
    double ratio;
    if (D > 1) {
      ratio = 0.0;
      for (int Dd = 0; Dd < D; ++Dd) ratio += wd[Dd] * v[(size_t)S.det_map[s * D + Dd] * n + i];
      ratio /= den;
    } else ratio = v[i];
    if (J3) ratio *= exp((jas ? A[t] : 0.0) + A3[(size_t)wl * ne + t]);
    else if (jas) ratio *= exp(A[t]);
    Rl[t] = ratio;
    if (R) R[(size_t)wl * ne + t] = ratio;
  }
  if (!T) return;
  __syncthreads();
  const int a = assign[w];
  const double* brow = rows + (size_t)a * norb;
  const double F = f[a] / norb;
  const double* cw = cfg + (size_t)w * ne * norb;
  for (int j = lane; j < norb; j += 64) {
    double s = 0.0;
    for (int t = 0; t < ne; ++t) s += Rl[t] * cw[(size_t)t * norb + j];
    const double b = brow[j];
    T[(size_t)wl * norb + j] = s;
    B[(size_t)wl * norb + j] = b / F;
    Nn[(size_t)wl * norb + j] = (b * b) / F;
  }
}

// inverse_rows in complex arithmetic: v[d n + i] as (re, im) pairs.  hc: the handle is complex (phi [re block | im block] of
// S.nmo[s] / 2 orbitals each, T interleaved); else the real tables are read and the imaginary parts are exactly 0.  The butterfly adds
// both planes.
__device__ __forceinline__ void inverse_rows_c(const SysDev& S, const SlaterState& st, int s, long w, int hc, const double* __restrict__ phi,
                                               double* v) {
  const int lane = threadIdx.x, n = s ? S.ndn : S.nup, D = S.ndet_s[s], nmo = S.nmo[s] / 2;
  int GS = 1;
  while (GS < n && GS < 64) GS <<= 1;
  const int per = 64 / GS, g = lane / GS, j = lane & (GS - 1);
  const double* Tw = st.T[s] + (size_t)w * D * n * n * (hc ? 2 : 1);
  for (int r0 = 0; r0 < D * n; r0 += per) {
    const int r = r0 + g;
    const bool act = r < D * n;
    cx p = {0.0, 0.0};
    if (act) {
      const int* occ = S.det_occ[s] + (size_t)(r / n) * n;
      if (hc) {
        const double* Tr = Tw + (size_t)r * n * 2;
        for (int k = j; k < n; k += GS) p = cadd(p, cmul(cx{phi[occ[k]], phi[nmo + occ[k]]}, cx{Tr[2 * k], Tr[2 * k + 1]}));
      } else
        for (int k = j; k < n; k += GS) p.r += phi[occ[k]] * Tw[(size_t)r * n + k];
    }
    for (int off = 1; off < GS; off <<= 1) {
      p.r += __shfl_xor(p.r, off, 64);
      p.i += __shfl_xor(p.i, off, 64);
    }
    if (act && j == 0) { v[2 * r] = p.r; v[2 * r + 1] = p.i; }
  }
}

// k_obdm_rt for complex / twisted handles and complex evaluators: one wave per walker of the chunk, arguments as there, with
// hc: the wave function's handle is complex (phi rows [wc][S.nmo[s]] = [re block | im block], T and dsign interleaved), oc: the
// evaluator is (cfg [W][ne][2 norb], rows [naux][2 norb]; else [.][norb]).  Outputs (each may be NULL): R [wc][ne] interleaved
// complex, the planar panels Tr, Ti (t = conj(sum_e R_e phi(r_e))), Br, Bi (b; Bi only with oc) and Nn, each [wc][norb].
// Dynamic LDS (doubles): 3 N coordinates, ne Jastrow differences, 2 ne ratios, 2 ndet weights (several determinants), the v tables
// 2 (ndet_up nup + ndet_dn ndn).
template <bool PBC>
__global__ __launch_bounds__(64) void k_obdm_rt_c(SysDev S, SlaterState st, JastrowState js, const double* __restrict__ phi_up,
                                                  const double* __restrict__ phi_dn, const double* __restrict__ pts,
                                                  const int* __restrict__ es, int ne, long w0, int jas, int spins, int hc, int oc,
                                                  const double* __restrict__ cfg, const double* __restrict__ rows,
                                                  const double* __restrict__ f, const int* __restrict__ assign, int norb,
                                                  double* __restrict__ R, double* __restrict__ Tr, double* __restrict__ Ti,
                                                  double* __restrict__ Br, double* __restrict__ Bi, double* __restrict__ Nn) {
  extern __shared__ double lds[];
  const int N = S.nelec, lane = threadIdx.x, D = S.ndet;
  const long wl = blockIdx.x, w = w0 + wl;
  double* xs = lds;                         // [N][3]
  double* A = lds + 3 * N;                  // [ne]
  double* Rl = A + ne;                      // [ne][2]
  double* wd = Rl + 2 * ne;                 // [D][2] (D > 1)
  double* vu = wd + (D > 1 ? 2 * D : 0);    // [ndet_up][nup][2]
  double* vd = vu + (size_t)2 * S.ndet_s[0] * S.nup;  // [ndet_dn][ndn][2]
  const double* xw = js.x + (size_t)w * N * 3;
  for (int q = lane; q < 3 * N; q += 64) xs[q] = xw[q];
  const double qx = pts[3 * wl], qy = pts[3 * wl + 1], qz = pts[3 * wl + 2];
  __syncthreads();
  if (jas) {
    const double irb = 1.0 / S.rcut_b, ira = 1.0 / S.rcut_a;
    for (int t = lane; t < ne; t += 64) {  // a lane owns a listed electron
      const int e = es[t], se = e >= S.nup;
      const double ex = xs[3 * e], ey = xs[3 * e + 1], ez = xs[3 * e + 2];
      double un = 0.0, uo = 0.0;
      for (int j = 0; j < N; ++j) {
        if (j == e) continue;
        const int col = se + (j >= S.nup);
        const double jx = xs[3 * j], jy = xs[3 * j + 1], jz = xs[3 * j + 2];
        un += pair_u<PBC>(S, qx - jx, qy - jy, qz - jz, col, irb);
        uo += pair_u<PBC>(S, ex - jx, ey - jy, ez - jz, col, irb);
      }
      un += ion_u<PBC>(S, qx, qy, qz, se, ira);
      uo += ion_u<PBC>(S, ex, ey, ez, se, ira);
      A[t] = un - uo;
    }
  }
  cx den = {1.0, 0.0};
  if (D > 1) {  // determinant weights relative to the largest |determinant|
    const double ref = det_ref(S, st, w);
    cx t = {0.0, 0.0};
    for (int Dd = lane; Dd < D; Dd += 64) {
      const cx x = hc ? det_weight_c(S, st, w, Dd, ref) : cx{det_weight(S, st, w, Dd, ref), 0.0};
      wd[2 * Dd] = x.r; wd[2 * Dd + 1] = x.i;
      t = cadd(t, x);
    }
    den = wave_sum_cx(t);
  }
  if (spins & 1) inverse_rows_c(S, st, 0, w, hc, phi_up + (size_t)wl * S.nmo[0], vu);
  if (spins & 2) inverse_rows_c(S, st, 1, w, hc, phi_dn + (size_t)wl * S.nmo[1], vd);
  __syncthreads();
  for (int t = lane; t < ne; t += 64) {
    const int e = es[t], s = e >= S.nup, i = e - s * S.nup, n = s ? S.ndn : S.nup;
    const double* v = s ? vd : vu;
    cx ratio;
    if (D > 1) {
      ratio = {0.0, 0.0};
      for (int Dd = 0; Dd < D; ++Dd) {
        const size_t o = (size_t)S.det_map[s * D + Dd] * n + i;
        ratio = cadd(ratio, cmul(cx{wd[2 * Dd], wd[2 * Dd + 1]}, cx{v[2 * o], v[2 * o + 1]}));
      }
      ratio = cdiv(ratio, den);
    } else ratio = {v[2 * i], v[2 * i + 1]};
    if (jas) ratio = cscale(ratio, exp(A[t]));
    Rl[2 * t] = ratio.r; Rl[2 * t + 1] = ratio.i;
    if (R) { R[2 * ((size_t)wl * ne + t)] = ratio.r; R[2 * ((size_t)wl * ne + t) + 1] = ratio.i; }
  }
  if (!Tr) return;
  __syncthreads();
  const int a = assign[w], nmo2 = oc ? 2 * norb : norb;
  const double* brow = rows + (size_t)a * nmo2;
  const double F = f[a] / norb;
  const double* cw = cfg + (size_t)w * ne * nmo2;
  for (int j = lane; j < norb; j += 64) {
    cx s = {0.0, 0.0};
    for (int t = 0; t < ne; ++t)
      s = cadd(s, cmul(cx{Rl[2 * t], Rl[2 * t + 1]}, cx{cw[(size_t)t * nmo2 + j], oc ? cw[(size_t)t * nmo2 + norb + j] : 0.0}));
    const size_t o = (size_t)wl * norb + j;
    Tr[o] = s.r;
    Ti[o] = -s.i;
    const double br = brow[j];
    Br[o] = br / F;
    if (oc) {
      const double bi = brow[norb + j];
      Bi[o] = bi / F;
      Nn[o] = (br * br + bi * bi) / F;
    } else Nn[o] = (br * br) / F;
  }
}

// Partial tiles of B^T T and partial column sums of Nn for the slices of a chunk: one wave per 16 x 16 tile (p0, q0) and slice of
// kSlice walkers.  part [slice][P P + P]: the tile's entries, and from the waves of the q0 = 0 tiles the norm columns p0 .. p0 + 15
// summed walker after walker.  WT: walker r of the chunk carries the weight wts[r], applied to the B operand as it is loaded and to
// the norm term as it is added (a weight of 1 leaves every bit as the unweighted instance has it).
template <bool WT>
__global__ __launch_bounds__(64) void k_obdm_mean(const double* __restrict__ B, const double* __restrict__ T, const double* __restrict__ Nn,
                                                  const double* __restrict__ wts, long wc, int P, double* __restrict__ part) {
  const int lane = threadIdx.x, i16 = lane & 15, kq = lane >> 4;
  const int p0 = blockIdx.x * 16, q0 = blockIdx.y * 16;
  const long sl = blockIdx.z, n_lo = sl * kSlice, n_hi = (n_lo + kSlice < wc) ? n_lo + kSlice : wc;
  double* out = part + (size_t)sl * ((size_t)P * P + P);
  const bool pin = p0 + i16 < P, qin = q0 + i16 < P;
  d4 acc = {0.0, 0.0, 0.0, 0.0};
  for (long r = n_lo; r < n_hi; r += 4) {
    const long rr = r + kq;
    double a = (pin && rr < n_hi) ? B[rr * P + p0 + i16] : 0.0;
    if (WT) a *= rr < n_hi ? wts[rr] : 0.0;
    const double b = (qin && rr < n_hi) ? T[rr * P + q0 + i16] : 0.0;
    acc = __builtin_amdgcn_mfma_f64_16x16x4f64(a, b, acc, 0, 0, 0);
  }
#pragma unroll
  for (int r = 0; r < 4; ++r) {  // lane holds D[row = kq + 4 r][col = i16]
    const int p = p0 + kq + 4 * r, q = q0 + i16;
    if (p < P && q < P) out[(size_t)p * P + q] = acc[r];
  }
  if (q0 == 0 && kq == 0 && pin) {
    double s = 0.0;
    for (long r = n_lo; r < n_hi; ++r) s += WT ? wts[r] * Nn[r * P + p0 + i16] : Nn[r * P + p0 + i16];
    out[(size_t)P * P + p0 + i16] = s;
  }
}

// k_obdm_mean for the planar complex panels: the same wave per tile and slice and the same operand mapping, two accumulators
// (Re = Br^T Tr - Bi^T Ti, Im = Br^T Ti + Bi^T Tr).  BI = false (real evaluator, Bi not read): two MFMAs per k-step, else four.
// part [slice][2 P P + P]: the tile's real parts, its imaginary parts, the norm columns.  The weight multiplies both B operands.
template <bool WT, bool BI>
__global__ __launch_bounds__(64) void k_obdm_mean_c(const double* __restrict__ Br, const double* __restrict__ Bi, const double* __restrict__ Tr,
                                                    const double* __restrict__ Ti, const double* __restrict__ Nn,
                                                    const double* __restrict__ wts, long wc, int P, double* __restrict__ part) {
  const int lane = threadIdx.x, i16 = lane & 15, kq = lane >> 4;
  const int p0 = blockIdx.x * 16, q0 = blockIdx.y * 16;
  const long sl = blockIdx.z, n_lo = sl * kSlice, n_hi = (n_lo + kSlice < wc) ? n_lo + kSlice : wc;
  const size_t PP = (size_t)P * P;
  double* out = part + (size_t)sl * (2 * PP + P);
  const bool pin = p0 + i16 < P, qin = q0 + i16 < P;
  d4 re = {0.0, 0.0, 0.0, 0.0}, im = {0.0, 0.0, 0.0, 0.0};
  for (long r = n_lo; r < n_hi; r += 4) {
    const long rr = r + kq;
    const bool in = rr < n_hi;
    const double wt = WT ? (in ? wts[rr] : 0.0) : 1.0;
    double ar = (pin && in) ? Br[rr * P + p0 + i16] : 0.0;
    if (WT) ar *= wt;
    const double tr = (qin && in) ? Tr[rr * P + q0 + i16] : 0.0;
    const double ti = (qin && in) ? Ti[rr * P + q0 + i16] : 0.0;
    re = __builtin_amdgcn_mfma_f64_16x16x4f64(ar, tr, re, 0, 0, 0);
    im = __builtin_amdgcn_mfma_f64_16x16x4f64(ar, ti, im, 0, 0, 0);
    if (BI) {
      double ai = (pin && in) ? Bi[rr * P + p0 + i16] : 0.0;
      if (WT) ai *= wt;
      re = __builtin_amdgcn_mfma_f64_16x16x4f64(-ai, ti, re, 0, 0, 0);
      im = __builtin_amdgcn_mfma_f64_16x16x4f64(ai, tr, im, 0, 0, 0);
    }
  }
#pragma unroll
  for (int r = 0; r < 4; ++r) {  // lane holds D[row = kq + 4 r][col = i16]
    const int p = p0 + kq + 4 * r, q = q0 + i16;
    if (p < P && q < P) { out[(size_t)p * P + q] = re[r]; out[PP + (size_t)p * P + q] = im[r]; }
  }
  if (q0 == 0 && kq == 0 && pin) {
    double s = 0.0;
    for (long r = n_lo; r < n_hi; ++r) s += WT ? wts[r] * Nn[r * P + p0 + i16] : Nn[r * P + p0 + i16];
    out[2 * PP + p0 + i16] = s;
  }
}

// The final scale of the complex mean: out [P P interleaved complex | P real] = fac [Re | Im | norm] of sums, fac = scale
// (wsum == NULL) or 1 / (mult wsum[0]).
__global__ __launch_bounds__(256) void k_obdm_out_c(const double* __restrict__ sums, long PP, int P, const double* __restrict__ wsum, double mult,
                                                    double scale, double* __restrict__ out) {
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  if (i >= PP + P) return;
  const double fac = wsum ? 1.0 / (mult * wsum[0]) : scale;
  if (i < PP) { out[2 * i] = fac * sums[i]; out[2 * i + 1] = fac * sums[PP + i]; }
  else out[PP + i] = fac * sums[PP + i];
}

// sums[i] (+)= part[0][i] + part[1][i] + ... one after the other (start != 0: from zero)
__global__ __launch_bounds__(256) void k_obdm_reduce(const double* __restrict__ part, long n, long nslice, int start, double* __restrict__ sums) {
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  double s = start ? 0.0 : sums[i];
  for (long sl = 0; sl < nslice; ++sl) s += part[(size_t)sl * n + i];
  sums[i] = s;
}

// out[i] = in[i] / (mult wsum[0]): the final scale of the weighted mean
__global__ __launch_bounds__(256) void k_obdm_wscale(const double* __restrict__ in, long n, const double* __restrict__ wsum, double mult,
                                                     double* __restrict__ out) {
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  if (i < n) out[i] = (1.0 / (mult * wsum[0])) * in[i];
}


// Scope of the entries that read wf's resident walkers for the evaluator ev (the pqa_obdm_sweeps and pqa_dm_points_resident entries):
// dm_pair_scope, a slot, the listed electrons distinct.  spins: bit 0 / 1 set when an up / down electron is listed.
int resident_scope(pqa_handle* h, pqa_handle* ev, const DmEntry& en, int slot, const int32_t* es, int ne, int* spins_out) {
  TRY(dm_pair_scope(h, ev, en));
  const std::string fn = en.name;
  if (slot < 0 || slot > 1) FAIL(fn + ": slot must be 0 or 1");
  if (!es || ne < 1) FAIL(fn + ": no electron listed (use the protocol route)");
  int spins = 0;
  std::vector<char> seen((size_t)h->N, 0);
  for (int t = 0; t < ne; ++t) {
    if (es[t] < 0 || es[t] >= h->N) FAIL(fn + ": electron index out of range (use the protocol route)");
    if (seen[es[t]]) FAIL(fn + ": an electron is listed twice (use the protocol route)");
    seen[es[t]] = 1;
    spins |= es[t] >= h->nup ? 2 : 1;
  }
  *spins_out = spins;
  return 0;
}

// ev's orbitals of the slot's spin at the listed electrons of wf's resident walkers, into the slot's rows (what pqa_dm_points leaves
// from a host array): the coordinates are gathered on wf's stream after ev's queued work, which may still read b_pts, and the
// orbitals run on ev's own stream; tb_ev[1] is recorded on ev's stream behind them.  The caller has passed resident_scope.
int resident_points(pqa_handle* h, pqa_handle* ev, int slot, const int32_t* es, int ne) {
  auto& d = ev->dm[slot];
  const long W = h->W;
  const int norb = ev->nmo[d.spin];
  TRY(on_ev(h, ev, ensure(ev, ev->b_pts, (size_t)W * ne * 3 * sizeof(double))));
  TRY(on_ev(h, ev, ensure(ev, d.cfg, (size_t)W * ne * norb * sizeof(double))));
  TRY(ensure(h, h->b_tves, (size_t)ne * sizeof(int)));
  if (!h->tb_ev[0])
    for (hipEvent_t& e : h->tb_ev) TRY(new_event(h, &e, hipEventDisableTiming));
  const hipEvent_t produced = h->tb_ev[0], consumed = h->tb_ev[1];
  TpTuneGuard tune_ev(ev);
  ev->saved_valid = false;
  d.ncfg = W * ne;
  HIPCHK(hipEventRecord(consumed, ev->stream));
  HIPCHK(hipStreamWaitEvent(h->stream, consumed, 0));
  TRY(copy_in(h, h->b_tves.p, es, (size_t)ne * sizeof(int)));
  hipLaunchKernelGGL(k_obdm_epts, dim3((unsigned)((W * ne + 255) / 256)), dim3(256), 0, h->stream, (const double*)h->js.x,
                     (const int*)h->b_tves.p, ne, h->N, W, (double*)ev->b_pts.p);
  TRY(check_launch(h, "k_obdm_epts"));
  HIPCHK(hipEventRecord(produced, h->stream));
  HIPCHK(hipStreamWaitEvent(ev->stream, produced, 0));
  TRY(on_ev(h, ev, launch_orb(ev, d.spin, plain_points((const double*)ev->b_pts.p, W * ne), W * ne, 1, (double*)d.cfg.p)));
  HIPCHK(hipEventRecord(consumed, ev->stream));
  return 0;
}

// The kernel variants of a call: the real ones of a kind share a signature, the complex ones have their own.
decltype(&k_obdm_rt<false, false>) obdm_rt_kernel(bool pbc, bool j3) {
  return pbc ? (j3 ? k_obdm_rt<true, true> : k_obdm_rt<true, false>) : (j3 ? k_obdm_rt<false, true> : k_obdm_rt<false, false>);
}
decltype(&k_obdm_rt_c<false>) obdm_rt_c_kernel(bool pbc) { return pbc ? k_obdm_rt_c<true> : k_obdm_rt_c<false>; }
decltype(&k_obdm_mean<false>) obdm_mean_kernel(bool wt) { return wt ? k_obdm_mean<true> : k_obdm_mean<false>; }
decltype(&k_obdm_mean_c<false, false>) obdm_mean_c_kernel(bool wt, bool bi) {
  return wt ? (bi ? k_obdm_mean_c<true, true> : k_obdm_mean_c<true, false>) : (bi ? k_obdm_mean_c<false, true> : k_obdm_mean_c<false, false>);
}

// pqa_obdm_sweeps (weights == NULL), pqa_obdm_sweeps_w (the mean mode with the walker weights `weights`), pqa_obdm_sweeps_c and
// pqa_obdm_sweeps_j3 (either)
int obdm_sweeps(pqa_handle* h, pqa_handle* ev, const DmEntry& en, int slot, const int32_t* es, int ne, int nsweeps, const int32_t* assign,
                uint64_t seed, int mean, int first, int64_t chunk, double* ratio, int32_t* assign_out, double* value_mean, double* norm_mean,
                const double* weights) {
  const std::string fn = en.name;
  const bool cx = en.cx;
  int spins = 0;
  TRY(resident_scope(h, ev, en, slot, es, ne, &spins));
  const bool j3 = en.j3 && h->has_j3;  // (the three-body differences are formed and added)
  const long W = h->W;
  const int N = h->N;
  auto& d = ev->dm[slot];
  if (nsweeps < 1 || nsweeps > d.nkeep) FAIL(fn + ": more sweeps than pqa_dm_walk kept samples (use the protocol route)");
  if (d.n <= 0) FAIL(fn + ": no auxiliary walkers (call pqa_dm_walk)");
  if (mean && (!value_mean || !norm_mean)) FAIL(fn + ": the mean mode needs value_mean and norm_mean");
  if (!mean && !first && ev->dm_nconf != W)
    FAIL(fn + ": the wave function holds another number of walkers than the accumulators were started with (use the protocol route)");
  if (mean && !first) FAIL(fn + ": the mean mode starts its sums in every call (first must be set)");
  if (assign)
    for (size_t i = 0; i < (size_t)nsweeps * W; ++i)
      if (assign[i] < 0 || assign[i] >= d.n) FAIL(fn + ": assignment outside the auxiliary walkers");
  if (weights) TRY(check_weights(h, fn.c_str(), weights, W));
  // nmo2: the doubles of an orbital row of the evaluator ([re block | im block] when it is complex), norb: its orbitals
  const int hc = h->cplx ? 1 : 0, oc = ev->cplx ? 1 : 0, nmo2 = ev->nmo[d.spin], norb = oc ? nmo2 / 2 : nmo2;
  if (norb <= 0) FAIL(fn + ": the evaluator has no orbitals of the walk's spin");
  const int D = h->ndet, cz = cx ? 2 : 1;  // (cz: doubles per ratio, weight and inverse-row entry)
  const size_t lds = ((size_t)3 * N + (1 + (size_t)cz) * ne + (D > 1 ? cz * D : 0) + cz * ((size_t)h->ndet_s[0] * h->nup + (size_t)h->ndet_s[1] * h->ndn)) * sizeof(double);
  if (lds > 160 * 1024) FAIL(fn + ": more determinants than one LDS block holds (use the protocol route)");
  const auto rt = obdm_rt_kernel(h->S.pbc, j3);
  const auto rt_c = obdm_rt_c_kernel(h->S.pbc);
  const auto mean_r = obdm_mean_kernel(weights != nullptr);
  const auto mean_c = obdm_mean_c_kernel(weights != nullptr, oc != 0);
  if (lds > 64 * 1024) TRY(raise_lds_limit(h, cx ? (const void*)rt_c : (const void*)rt));
  // scratch per walker: the point, the orbital rows of the spins present, and the ratios (per-walker mode) or the three panels and
  // the walker's share of a slice's partial tile (mean mode)
  const int nm0 = (spins & 1) ? h->nmo[0] : 0, nm1 = (spins & 2) ? h->nmo[1] : 0;
  const size_t npart = (size_t)cz * norb * norb + norb;  // doubles of a slice's partials, and of the running sums
  const int npanel = cx ? 5 : 3;                           // T, B, Nn / Tr, Ti, Br, Bi, Nn
  const bool need_R = !mean || ratio;
  size_t lds_j3 = 0;
  if (j3) TRY(j3_moves_lds<false>(h, fn, ne, &lds_j3));
  const size_t per_walker = (3 + (size_t)nm0 + nm1 + (j3 ? ne : 0) + (need_R ? cz * ne : 0) + (mean ? npanel * (size_t)norb + (npart + kSlice - 1) / kSlice : 0)) * sizeof(double);
  long Wc = chunk > 0 ? std::min<long>(W, chunk) : walker_chunk(W, per_walker);
  if (mean && Wc < W) Wc = std::max<long>(kSlice, Wc - Wc % kSlice);  // (whole slices: the slices do not depend on the chunk)
  const long nsl_max = (std::min(Wc, W) + kSlice - 1) / kSlice;
  TRY(on_ev(h, ev, ensure(ev, ev->dm_assign[0], (size_t)nsweeps * W * sizeof(int))));
  if (assign) TRY(on_ev(h, ev, copy_in(ev, ev->dm_assign[0].p, assign, (size_t)nsweeps * W * sizeof(int))));
  if (need_R) TRY(on_ev(h, ev, ensure(ev, ev->dm_ratio, (size_t)Wc * ne * cz * sizeof(double))));
  // (weighted: the W weights and their sum behind the mean mode's scratch)
  if (mean) TRY(on_ev(h, ev, ensure(ev, ev->b_obdm, ((size_t)npanel * Wc * norb + (size_t)(nsl_max + 2) * npart + (weights ? (size_t)W + 1 : 0)) * sizeof(double))));
  else TRY(on_ev(h, ev, dm_prepare(ev, W, (long)norb * norb, cx ? 1 : 0, first, norb, 0)));
  TRY(ensure(h, h->b_tbpts, (size_t)3 * Wc * sizeof(double)));
  if (j3) TRY(ensure(h, h->b_j3dm, (size_t)Wc * ne * sizeof(double)));
  if (nm0) TRY(ensure(h, h->b_orbphi[0], (size_t)Wc * nm0 * sizeof(double)));
  if (nm1) TRY(ensure(h, h->b_orbphi[1], (size_t)Wc * nm1 * sizeof(double)));
  TpTuneGuard tune(h), tune_ev(ev);
  int* d_assign = (int*)ev->dm_assign[0].p;
  double* d_pts = (double*)h->b_tbpts.p;
  double* d_R = need_R ? (double*)ev->dm_ratio.p : nullptr;
  double *d_T = nullptr, *d_B = nullptr, *d_N = nullptr, *d_part = nullptr, *d_sums = nullptr, *d_out = nullptr, *d_wts = nullptr, *d_wsum = nullptr;
  double *d_Ti = nullptr, *d_Bi = nullptr;  // (the complex entry's imaginary panels)
  if (mean) {
    const size_t pan = (size_t)Wc * norb;
    d_T = (double*)ev->b_obdm.p;
    d_B = d_T + pan;
    d_N = d_B + pan;
    if (cx) { d_Ti = d_N + pan; d_Bi = d_Ti + pan; }
    d_part = (double*)ev->b_obdm.p + npanel * pan;
    d_sums = d_part + (size_t)nsl_max * npart;
    d_out = d_sums + npart;
    if (weights) { d_wts = d_out + npart; d_wsum = d_wts + W; }
  }
  TRY(resident_points(h, ev, slot, es, ne));
  const int* d_es = (const int*)h->b_tves.p;  // (allocated and filled by resident_points)
  const hipEvent_t produced = h->tb_ev[0], consumed = h->tb_ev[1];
  if (weights) {
    TRY(on_ev(h, ev, copy_in(ev, d_wts, weights, (size_t)W * sizeof(double))));
    hipLaunchKernelGGL((k_wsum<>), dim3(1), dim3(256), 0, ev->stream, (const double*)d_wts, W, d_wsum);
    TRY(on_ev(h, ev, check_launch(ev, "k_wsum")));
  }
  for (int s = 0; s < nsweeps; ++s) {
    const double* keep_pos = (const double*)d.keep_pos.p + (size_t)s * d.n * 3;
    const double* keep_row = (const double*)d.keep_row.p + (size_t)s * d.n * nmo2;
    const double* keep_f = (const double*)d.keep_f.p + (size_t)s * d.n;
    int* asg = d_assign + (size_t)s * W;
    for (long w0 = 0; w0 < W; w0 += Wc) {
      const long wc = std::min(Wc, W - w0);
      HIPCHK(hipStreamWaitEvent(h->stream, consumed, 0));  // (the previous chunk's ratios / panels have been contracted)
      hipLaunchKernelGGL(k_obdm_gather, dim3((unsigned)((wc + 255) / 256)), dim3(256), 0, h->stream, keep_pos, asg, w0, wc, assign ? 0 : 1,
                         seed, (uint32_t)s, d.n, d_pts);
      TRY(check_launch(h, "k_obdm_gather"));
      if (nm0) TRY(launch_orb(h, 0, plain_points(d_pts, wc), wc, 1, (double*)h->b_orbphi[0].p));
      if (nm1) TRY(launch_orb(h, 1, plain_points(d_pts, wc), wc, 1, (double*)h->b_orbphi[1].p));
      if (j3) TRY(launch_j3_moves<false>(h, lds_j3, (const double*)d_pts, d_es, ne, w0, wc, 0, 0, spins, (double*)h->b_j3dm.p));
      if (cx)
        hipLaunchKernelGGL(rt_c, dim3((unsigned)wc), dim3(64), lds, h->stream, h->S, h->st, h->js, (const double*)h->b_orbphi[0].p,
                           (const double*)h->b_orbphi[1].p, (const double*)d_pts, d_es, ne, w0, (int)h->has_j2, spins, hc, oc,
                           (const double*)d.cfg.p, keep_row, keep_f, (const int*)asg, norb, d_R, d_T, d_Ti, d_B, d_Bi, d_N);
      else
        hipLaunchKernelGGL(rt, dim3((unsigned)wc), dim3(64), lds, h->stream, h->S, h->st, h->js, (const double*)h->b_orbphi[0].p,
                           (const double*)h->b_orbphi[1].p, (const double*)d_pts, d_es, ne, w0, (int)h->has_j2, spins, (const double*)d.cfg.p,
                           keep_row, keep_f, (const int*)asg, norb, d_R, d_T, d_B, d_N, j3 ? (const double*)h->b_j3dm.p : (const double*)nullptr);
      TRY(check_launch(h, "k_obdm_rt"));
      if (ratio)
        HIPCHK(hipMemcpyAsync(ratio + ((size_t)s * W + w0) * ne * cz, d_R, (size_t)wc * ne * cz * sizeof(double), hipMemcpyDefault, h->stream));
      HIPCHK(hipEventRecord(produced, h->stream));
      HIPCHK(hipStreamWaitEvent(ev->stream, produced, 0));
      if (mean) {
        const long nsl = (wc + kSlice - 1) / kSlice;
        const unsigned tiles = (unsigned)((norb + 15) / 16);
        const dim3 grid(tiles, tiles, (unsigned)nsl);
        const double* wts = weights ? (const double*)d_wts + w0 : (const double*)nullptr;
        if (cx)
          hipLaunchKernelGGL(mean_c, grid, dim3(64), 0, ev->stream, (const double*)d_B, (const double*)d_Bi, (const double*)d_T, (const double*)d_Ti,
                             (const double*)d_N, wts, wc, norb, d_part);
        else
          hipLaunchKernelGGL(mean_r, grid, dim3(64), 0, ev->stream, (const double*)d_B, (const double*)d_T, (const double*)d_N, wts, wc, norb, d_part);
        hipLaunchKernelGGL(k_obdm_reduce, dim3((unsigned)((npart + 255) / 256)), dim3(256), 0, ev->stream, (const double*)d_part, (long)npart,
                           nsl, (int)(s == 0 && w0 == 0), d_sums);
        TRY(on_ev(h, ev, check_launch(ev, "k_obdm_mean")));
      } else {
        hipLaunchKernelGGL((k_obdm_acc<>), dim3((unsigned)wc), dim3(256), (size_t)2 * norb * sizeof(double), ev->stream, keep_row, keep_f,
                           (const int*)asg + w0, (const double*)d.cfg.p + (size_t)w0 * ne * nmo2, (const double*)d_R, cx ? 1 : 0, oc, ne, norb,
                           (int)(first && s == 0), (double*)ev->dm_val.p + (size_t)w0 * norb * norb * cz, (double*)ev->dm_norm[0].p + (size_t)w0 * norb);
        TRY(on_ev(h, ev, check_launch(ev, "k_obdm_acc")));
      }
      HIPCHK(hipEventRecord(consumed, ev->stream));
    }
  }
  if (ratio) HIPCHK(hipStreamSynchronize(h->stream));  // (the caller's array is complete on return)
  if (mean) {
    if (cx)
      hipLaunchKernelGGL(k_obdm_out_c, dim3((unsigned)((npart + 255) / 256)), dim3(256), 0, ev->stream, (const double*)d_sums, (long)norb * norb, norb,
                         (const double*)d_wsum, (double)nsweeps, 1.0 / ((double)W * nsweeps), d_out);
    else if (weights)
      hipLaunchKernelGGL(k_obdm_wscale, dim3((unsigned)((npart + 255) / 256)), dim3(256), 0, ev->stream, (const double*)d_sums, (long)npart,
                         (const double*)d_wsum, (double)nsweeps, d_out);
    else
      hipLaunchKernelGGL((k_scale_copy<>), dim3((unsigned)((npart + 255) / 256)), dim3(256), 0, ev->stream, (const double*)d_sums, (long)npart,
                         1.0 / ((double)W * nsweeps), d_out);
    TRY(on_ev(h, ev, check_launch(ev, "k_scale_copy")));
    HIPCHK(hipMemcpyAsync(value_mean, d_out, (size_t)cz * norb * norb * sizeof(double), hipMemcpyDefault, ev->stream));
    HIPCHK(hipMemcpyAsync(norm_mean, d_out + (size_t)cz * norb * norb, (size_t)norb * sizeof(double), hipMemcpyDefault, ev->stream));
  }
  if (assign_out) HIPCHK(hipMemcpyAsync(assign_out, d_assign, (size_t)nsweeps * W * sizeof(int), hipMemcpyDefault, ev->stream));
  if (mean || assign_out) HIPCHK(hipStreamSynchronize(ev->stream));
  return 0;
}

}  // namespace

extern "C" int pqa_obdm_sweeps(pqa_handle_t* h, pqa_handle_t* ev, int slot, const int32_t* es, int ne, int nsweeps, const int32_t* assign,
                               uint64_t seed, int mean, int first, int64_t chunk, double* ratio, int32_t* assign_out, double* value_mean,
                               double* norm_mean) {
  return obdm_sweeps(h, ev, DmEntry{"pqa_obdm_sweeps", false}, slot, es, ne, nsweeps, assign, seed, mean, first, chunk, ratio, assign_out,
                     value_mean, norm_mean, nullptr);
}

// The mean mode with walker weights: value_mean = sum_s sum_w w_w b_s[w] (x) t_s[w] / (nsweeps sum_w w_w), norm_mean likewise.
extern "C" int pqa_obdm_sweeps_w(pqa_handle_t* h, pqa_handle_t* ev, int slot, const int32_t* es, int ne, int nsweeps, const int32_t* assign,
                                 uint64_t seed, int64_t chunk, const double* weights, int32_t* assign_out, double* value_mean,
                                 double* norm_mean) {
  if (!h) return -2;
  if (!weights) FAIL("pqa_obdm_sweeps_w: weights is NULL");
  return obdm_sweeps(h, ev, DmEntry{"pqa_obdm_sweeps_w", false}, slot, es, ne, nsweeps, assign, seed, 1, 1, chunk, nullptr, assign_out,
                     value_mean, norm_mean, weights);
}

// pqa_obdm_sweeps for complex and twisted wave-function handles and complex evaluators (real ones are taken too): ratio (nsweeps, W, ne)
// and value_mean (norb, norb) are interleaved complex, norm_mean is real.  weights != NULL: the weighted mean (mean mode only).
extern "C" int pqa_obdm_sweeps_c(pqa_handle_t* h, pqa_handle_t* ev, int slot, const int32_t* es, int ne, int nsweeps, const int32_t* assign,
                                 uint64_t seed, int mean, int first, int64_t chunk, const double* weights, double* ratio, int32_t* assign_out,
                                 double* value_mean, double* norm_mean) {
  if (!h) return -2;
  if (weights && !mean) FAIL("pqa_obdm_sweeps_c: walker weights need the mean mode");
  return obdm_sweeps(h, ev, DmEntry{"pqa_obdm_sweeps_c", true}, slot, es, ne, nsweeps, assign, seed, mean, first, chunk, ratio, assign_out,
                     value_mean, norm_mean, weights);
}

// pqa_obdm_sweeps_c's parameter list for real handles with a three-body Jastrow factor (handles without one are taken too and give the
// bits of pqa_obdm_sweeps / pqa_obdm_sweeps_w): ratio and value_mean are real.  weights != NULL: the weighted mean (mean mode only).
extern "C" int pqa_obdm_sweeps_j3(pqa_handle_t* h, pqa_handle_t* ev, int slot, const int32_t* es, int ne, int nsweeps, const int32_t* assign,
                                  uint64_t seed, int mean, int first, int64_t chunk, const double* weights, double* ratio, int32_t* assign_out,
                                  double* value_mean, double* norm_mean) {
  if (!h) return -2;
  if (weights && !mean) FAIL("pqa_obdm_sweeps_j3: walker weights need the mean mode");
  return obdm_sweeps(h, ev, DmEntry{"pqa_obdm_sweeps_j3", false, true}, slot, es, ne, nsweeps, assign, seed, mean, first, chunk, ratio,
                     assign_out, value_mean, norm_mean, weights);
}

// pqa_dm_points with the listed electrons' coordinates gathered from wf's resident walkers, device to device, in the scope of the entry
static int dm_points_resident(pqa_handle* h, pqa_handle* ev, const DmEntry& en, int slot, const int32_t* es, int ne) {
  const std::string fn = en.name;
  int spins = 0;
  TRY(resident_scope(h, ev, en, slot, es, ne, &spins));
  if (ev->dm[slot].n <= 0) FAIL(fn + ": no auxiliary walkers in the slot (call pqa_dm_walk: it names the slot's spin)");
  if (ev->nmo[ev->dm[slot].spin] <= 0) FAIL(fn + ": the evaluator has no orbitals of the walk's spin");
  return resident_points(h, ev, slot, es, ne);
}

extern "C" int pqa_dm_points_resident(pqa_handle_t* h, pqa_handle_t* ev, int slot, const int32_t* es, int ne) {
  return dm_points_resident(h, ev, DmEntry{"pqa_dm_points_resident", false}, slot, es, ne);
}

// pqa_dm_points_resident for complex and twisted handles and complex evaluators (pqa_obdm_sweeps_c's scope: a twisted evaluator needs
// a twisted wf, whose walkers are unfolded, so that the evaluator's orbital kernel puts the wrap phase on phi_k(r_e))
extern "C" int pqa_dm_points_resident_c(pqa_handle_t* h, pqa_handle_t* ev, int slot, const int32_t* es, int ne) {
  return dm_points_resident(h, ev, DmEntry{"pqa_dm_points_resident_c", true}, slot, es, ne);
}

// pqa_dm_points_resident in the scope of pqa_obdm_sweeps_j3 / pqa_tbdm_sweep_j3 (a three-body factor admitted)
extern "C" int pqa_dm_points_resident_j3(pqa_handle_t* h, pqa_handle_t* ev, int slot, const int32_t* es, int ne) {
  return dm_points_resident(h, ev, DmEntry{"pqa_dm_points_resident_j3", false, true}, slot, es, ne);
}

// Weighted walker mean of one of ev's per-walker accumulators (pqa_dm_fetch's `which`), times scale
extern "C" int pqa_dm_fetch_w(pqa_handle_t* h, int which, int ncol, double scale, const double* weights, double* out) {
  if (!h) return -2;
  HIPCHK(hipSetDevice(h->device));
  if (h->dm_nconf <= 0) FAIL("pqa_dm_fetch_w: nothing accumulated");
  if (!out) FAIL("pqa_dm_fetch_w: out is NULL");
  const long rows = h->dm_nconf;
  const double* src;
  long cols;
  if (which == 0) {
    src = (const double*)h->dm_val.p;
    cols = h->dm_nval * (h->dm_cx ? 2 : 1);
    if (ncol != cols) FAIL("pqa_dm_fetch_w: ncol does not match the accumulated value");
  } else if (which == 1 || which == 2) {
    src = (const double*)h->dm_norm[which - 1].p;
    cols = ncol;
    if (cols < 1 || (size_t)rows * cols * sizeof(double) > h->dm_norm[which - 1].cap) FAIL("pqa_dm_fetch_w: ncol exceeds the accumulated norm");
  } else FAIL("pqa_dm_fetch_w: which must be 0, 1 or 2");
  TRY(check_weights(h, "pqa_dm_fetch_w", weights, rows));
  const long nsl = wcol_slices(rows);
  // scratch: [means (cols) | partials (nsl, cols) | weights (rows) | their sum]
  TRY(ensure(h, h->dm_tmp, ((size_t)cols * (nsl + 1) + rows + 1) * sizeof(double)));
  double* d_acc = (double*)h->dm_tmp.p;
  double* d_part = d_acc + cols;
  double* d_wts = d_part + (size_t)nsl * cols;
  double* d_wsum = d_wts + rows;
  TRY(copy_in(h, d_wts, weights, (size_t)rows * sizeof(double)));
  hipLaunchKernelGGL((k_wsum<>), dim3(1), dim3(256), 0, h->stream, (const double*)d_wts, rows, d_wsum);
  TRY(check_launch(h, "k_wsum"));
  TRY(wcol_means_dev<>(h, src, d_wts, rows, cols, 1, 1, 1, scale, d_wsum, d_part, d_acc));
  return copy_out(h, out, d_acc, (size_t)cols * sizeof(double));
}

// Bytes the evaluator holds for the fused one-body estimator: scratch = the mean mode's panels, partial tiles and sums plus the
// ratios of a walker chunk; per_walker = the per-walker accumulators (value and norms) the mean mode never allocates.
extern "C" int pqa_obdm_bytes(pqa_handle_t* ev, int64_t* scratch, int64_t* per_walker) {
  if (!ev) return -2;
  if (scratch) *scratch = (int64_t)(ev->b_obdm.cap + ev->dm_ratio.cap);
  if (per_walker) *per_walker = (int64_t)(ev->dm_val.cap + ev->dm_norm[0].cap + ev->dm_norm[1].cap);
  return 0;
}
