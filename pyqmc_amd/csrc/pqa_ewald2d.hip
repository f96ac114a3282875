// Coulomb energy of the resident walkers in a slab geometry: periodic along the first two lattice vectors, open along the third
// (Yeh and Berkowitz, J. Chem. Phys. 111, 3155; pyqmc/observables/ewald2d.py:162-304).  Read-only on the handle.
//
// Per pair with minimal-image displacement d = (dx, dy, z) (min_image, pqa_common.hpp: all three lattice vectors, as the
// reference's MinimalImageDistance), s = alpha |z|, a_k = k / 2 alpha:
//   real    sum_L erfc(alpha |d + L|) / |d + L|                       over the in-plane displacements L (any nlatvec)
//   charge  -(2 pi / A) [|z| erf(s) + exp(-s^2) / (alpha sqrt(pi))]
//   recip   2 sum_k cos(k.d) W(k, z),   W = (pi / (A k)) [e^{kz} erfc(a_k + alpha z) + e^{-kz} erfc(a_k - alpha z)].
// W is even in z and evaluated in the scaled form, in which nothing overflows (the reference's e^{kz} erfc(.) is inf * 0 once
// k |z| > 709): with t+ = a_k + s, t- = a_k - s and e^{+-k|z|} erfc(t+-) = exp(-a_k^2 - s^2) erfcx(t+-),
//   t- >= 0:  W = p_k E [erfcx(t+) + erfcx(t-)]
//   t- <  0:  W = p_k E [erfcx(t+) - erfcx(-t-)] + q_k exp(-k |z|)           (erfcx(t) = 2 exp(t^2) - erfcx(-t))
// p_k = (pi / (A k)) exp(-a_k^2) and q_k = 2 pi / (A k) from the host, E = exp(-s^2) once per pair.  Where p_k E < 1e-20 the erfcx
// bracket (at most 2) is dropped: the dropped part of a term is below 2e-20 relative to 1.
//
// erfcx(t), t >= 0: the piecewise polynomials of pqa_erfc_tab.hpp on [0, 6.5) (2.2e-15 relative), beyond them the asymptotic
// series (1 / (t sqrt(pi))) sum_n (-1)^n (2n - 1)!! / (2 t^2)^n with ten terms.  Successive terms fall by (2n + 1) / (2 t^2), i.e. by
// 84.5 / (2n + 1) at t = 6.5, so the eleventh is 1e-11 there; every use multiplies erfcx(t) by exp(-a_k^2 - s^2) <= exp(-t^2 / 2)
// <= 6.7e-10, which puts the truncation below 1e-20 relative to 1.
//
// cos(k.d): every k is an integer combination n0 b0 + n1 b1 of the two in-plane reciprocal rows and k.a_i is a multiple of 2 pi for
// all three lattice vectors, so cos(k.d) = Re[e^{i k.r_i} conj(e^{i k.r_j})] whatever the image.  The powers 0..nmax of the two base
// phases e^{i b_a.r} of every electron and ion go to LDS once per walker (the recurrence of k_ewald's gidx path): a (pair, k) term
// costs four 16-byte LDS reads and two complex products, no sincos.
//
// k_ewald2d: one block of 256 threads per walker.  Lanes run over the items (electron pairs, then electron-ion pairs), the
// inner loop over k (wave-uniform tables through the scalar cache).  Fixed-order block sums (block_sum256): ee = pairs + N self,
// ei = -sum q_I pairs.  Mean mode (k_ewald2d_fold): thread t adds the walkers w = t mod 256 in ascending order, carried across the
// walker chunks, and the 256 partial sums are added in a fixed order after the last chunk: no atomics, and the bits do not
// depend on the chunk size.
#include "pqa_erfc_tab.hpp"
#include "pqa_estim.hpp"

namespace {

constexpr int kE2Threads = 256;
constexpr size_t kE2LdsStatic = 8 << 10;              // bound of the kernel's static LDS (erfcx table, reduction)
constexpr size_t kE2LdsMax = (160 << 10) - kE2LdsStatic;

struct E2Args {
  int N, nion, nk, M, nlat;  // electrons, ions, k vectors, powers per base phase, in-plane displacements
  double alpha, c0, self_ee;  // c0 = 2 pi / A; self_ee: the self constant of a unit charge
  const double* kt;           // [nk][4]: k, k / 2 alpha, p_k, q_k
  const int* kn;              // [nk][2]: integer coordinates in the basis recip
  const double* lat;          // [nlat][3]
  const double* ion_xyz;      // [nion][3]
  const double* ion_q;        // [nion]
  double recip[6];            // rows b_0, b_1
};

__global__ __launch_bounds__(kE2Threads) void k_ewald2d(SysDev S, E2Args A, const double* __restrict__ x, long sw, long se, long sc,
                                                        long w0, long wc, double* __restrict__ out) {
  extern __shared__ __align__(16) double lds[];  // (the phase tables are read 16 bytes at a time)
  __shared__ double etab[PQA_ERFC_N][PQA_ERFC_DEG + 1];
  __shared__ double red[kE2Threads];
  const int tid = threadIdx.x, N = A.N, P = A.N + A.nion, M = A.M;
  const long wl = blockIdx.x, w = w0 + wl;
  double* xyz = lds;                                                         // [P][3]: electrons, then ions, folded into the cell
  double2* ph = reinterpret_cast<double2*>(lds + ((3 * P + 1) & ~1));        // [P][2][M]
  for (int k = tid; k < PQA_ERFC_N * (PQA_ERFC_DEG + 1); k += kE2Threads)
    etab[k / (PQA_ERFC_DEG + 1)][k % (PQA_ERFC_DEG + 1)] = PQA_ERFC_TAB[k / (PQA_ERFC_DEG + 1)][k % (PQA_ERFC_DEG + 1)];
  for (int p = tid; p < P; p += kE2Threads) {
    double px, py, pz;
    if (p < N) {
      const double* xp = x + w * sw + (long)p * se;
      px = xp[0]; py = xp[sc]; pz = xp[2 * sc];
    } else {
      px = A.ion_xyz[3 * (p - N)]; py = A.ion_xyz[3 * (p - N) + 1]; pz = A.ion_xyz[3 * (p - N) + 2];
    }
    fold_cell(S, px, py, pz);
    xyz[3 * p] = px; xyz[3 * p + 1] = py; xyz[3 * p + 2] = pz;
  }
  __syncthreads();
  for (int q = tid; q < 2 * P; q += kE2Threads) {
    const int p = q >> 1, a = q & 1;
    double sn, cs;
    sincos(A.recip[3 * a] * xyz[3 * p] + A.recip[3 * a + 1] * xyz[3 * p + 1] + A.recip[3 * a + 2] * xyz[3 * p + 2], &sn, &cs);
    double2* t = ph + (size_t)q * M;
    double cr = 1.0, ci = 0.0;
    for (int m = 0; m < M; ++m) {
      t[m] = make_double2(cr, ci);
      const double nr = cr * cs - ci * sn;
      ci = cr * sn + ci * cs;
      cr = nr;
    }
  }
  __syncthreads();

  auto erfcx_tab = [&](double t) {  // 0 <= t < PQA_ERFC_XMAX
    const int i = min((int)(t * (1.0 / PQA_ERFC_H)), PQA_ERFC_N - 1);
    const double u = 2.0 * (t - i * PQA_ERFC_H) * (1.0 / PQA_ERFC_H) - 1.0;
    const double* c = etab[i];
    double p = c[PQA_ERFC_DEG];
#pragma unroll
    for (int k = PQA_ERFC_DEG - 1; k >= 0; --k) p = p * u + c[k];
    return p;
  };
  auto erfcx_pos = [&](double t) {  // t >= 0
    if (t < PQA_ERFC_XMAX) return erfcx_tab(t);
    const double u = 0.5 / (t * t);
    double s = 1.0 - 19.0 * u;
#pragma unroll
    for (int c = 17; c >= 1; c -= 2) s = 1.0 - c * u * s;
    return s * 0.56418958354775628695 / t;  // 1 / sqrt(pi)
  };

  const double a2 = A.alpha * A.alpha;
  auto pair = [&](int pi, int pj) {
    double dx = xyz[3 * pi] - xyz[3 * pj], dy = xyz[3 * pi + 1] - xyz[3 * pj + 1], dz = xyz[3 * pi + 2] - xyz[3 * pj + 2];
    min_image(S, dx, dy, dz);
    double acc = 0.0;
    for (int l = 0; l < A.nlat; ++l) {
      const double rx = dx + A.lat[3 * l], ry = dy + A.lat[3 * l + 1], rz = dz + A.lat[3 * l + 2];
      const double r2 = rx * rx + ry * ry + rz * rz, hr2 = 0.5 * r2;
      if (a2 * r2 > 40.0) continue;  // erfc(x) / r < 4e-19 for x^2 > 40 (as k_ewald)
      double ir = __builtin_amdgcn_rsq(r2);
      ir = ir * fma(-hr2 * ir, ir, 1.5);
      ir = ir * fma(-hr2 * ir, ir, 1.5);
      acc += (r2 > 0.0) ? erfcx_tab(A.alpha * (r2 * ir)) * exp(-a2 * r2) * ir : __builtin_inf();  // coincident particles: erfc(0) / 0
    }
    const double az = fabs(dz), s = A.alpha * az, E = exp(-s * s);
    const double erf_s = s < PQA_ERFC_XMAX ? 1.0 - E * erfcx_tab(s) : 1.0;  // (1 - erf(6.5) = 4e-20)
    acc -= A.c0 * (az * erf_s + E * 0.56418958354775628695 / A.alpha);
    const double2 *ti = ph + (size_t)pi * 2 * M, *tj = ph + (size_t)pj * 2 * M;
    double rs = 0.0;
    for (int k = 0; k < A.nk; ++k) {
      const int n0 = A.kn[2 * k], n1 = A.kn[2 * k + 1];
      const int m0 = abs(n0), m1 = M + abs(n1);
      const double f0 = n0 < 0 ? -1.0 : 1.0, f1 = n1 < 0 ? -1.0 : 1.0;
      const double2 ai = ti[m0], bi = ti[m1], aj = tj[m0], bj = tj[m1];
      const double aiy = f0 * ai.y, biy = f1 * bi.y, ajy = f0 * aj.y, bjy = f1 * bj.y;
      const double eir = ai.x * bi.x - aiy * biy, eii = ai.x * biy + aiy * bi.x;
      const double ejr = aj.x * bj.x - ajy * bjy, eji = aj.x * bjy + ajy * bj.x;
      const double cs = eir * ejr + eii * eji;
      const double kk = A.kt[4 * k], ak = A.kt[4 * k + 1], pe = A.kt[4 * k + 2] * E;
      const double tm = ak - s;
      double wgt = 0.0;
      if (pe > 1e-20) {
        const double ep = erfcx_pos(ak + s), em = erfcx_pos(fabs(tm));
        wgt = pe * (tm < 0.0 ? ep - em : ep + em);
      }
      if (tm < 0.0) wgt += A.kt[4 * k + 3] * exp(-kk * az);
      rs += cs * wgt;
    }
    return acc + 2.0 * rs;
  };

  const int npair = N * (N - 1) / 2, nitem = npair + N * A.nion;
  double ee = 0.0, ei = 0.0;
  for (int it = tid; it < nitem; it += kE2Threads) {
    int pi, pj;
    if (it < npair) {  // pair it -> (i < j), row-major upper triangle
      int i = 0, rem = it;
      while (rem >= N - 1 - i) { rem -= N - 1 - i; ++i; }
      pi = i; pj = i + 1 + rem;
    } else {
      pi = (it - npair) / A.nion; pj = N + (it - npair) % A.nion;
    }
    const double v = pair(pi, pj);
    if (it < npair) ee += v;
    else ei -= A.ion_q[pj - N] * v;
  }
  ee = block_sum256(ee, red);
  ei = block_sum256(ei, red);
  if (tid == 0) { out[wl] = ee + N * A.self_ee; out[wc + wl] = ei; }
}

// mean mode: part[z][t] = (first chunk ? 0 : part[z][t]) + the chunk's values v ([2][wc]) of the walkers w = t mod 256, ascending; after
// the last chunk acc[z] = (sum_t part[z][t], fixed order) / W
__global__ __launch_bounds__(kE2Threads) void k_ewald2d_fold(const double* __restrict__ v, long w0, long wc, int first, int last, double W,
                                                             double* __restrict__ part, double* __restrict__ acc) {
  __shared__ double red[kE2Threads];
  const int t = threadIdx.x;
  for (int z = 0; z < 2; ++z) {
    double s = first ? 0.0 : part[z * kE2Threads + t];
    long wl = (t - w0 % kE2Threads + kE2Threads) % kE2Threads;  // first walker of the chunk that is t mod 256
    for (; wl < wc; wl += kE2Threads) s += v[z * wc + wl];
    part[z * kE2Threads + t] = s;
    if (last) {
      const double r = block_sum256(s, red);
      if (t == 0) acc[z] = r / W;
    }
  }
}

}  // namespace

extern "C" int pqa_ewald2d(pqa_handle_t* h, const pqa_ewald2d_t* tab, int mean, double* ee, double* ei) {
  HIPCHK(hipSetDevice(h->device));
  if (h->W == 0) FAIL("pqa_ewald2d: state not initialised (call recompute)");
  if (!h->S.pbc) FAIL("pqa_ewald2d: open-boundary handle (the slab sum needs a periodic cell)");
  if (!tab || !ee || !ei) FAIL("pqa_ewald2d: tab / ee / ei is NULL");
  if (tab->nk < 0 || tab->nlat < 1 || !tab->lat || (tab->nk > 0 && (!tab->kn || !tab->knorm || !tab->kpref)))
    FAIL("pqa_ewald2d: incomplete tables (nk >= 0 with kn / knorm / kpref, nlat >= 1 with lat)");
  if (!(tab->alpha > 0.0) || !(tab->area > 0.0)) FAIL("pqa_ewald2d: alpha and area must be positive");
  if (tab->nion < 0 || (tab->nion > 0 && (!tab->ion_xyz || !tab->ion_charge))) FAIL("pqa_ewald2d: nion > 0 needs ion_xyz and ion_charge");
  const long W = h->W;
  const int N = h->N, nk = tab->nk, nlat = tab->nlat;
  const bool own = tab->nion == 0;  // the handle's ions
  const int nion = own ? h->natom : tab->nion;
  // the live coordinates, in place: the sweep's planes [N*3][W] when the walker-major arrays are stale, else js.x [W][N][3]
  const bool planes = h->aos_stale;
  const double* x = planes ? (const double*)h->b_xt.p : h->js.x;
  const long sw = planes ? 1L : 3L * N, se = planes ? 3L * W : 3L, sc = planes ? W : 1L;

  int nmax = 0;
  for (long k = 0; k < 2L * nk; ++k) nmax = std::max(nmax, std::abs(tab->kn[k]));
  E2Args A{};
  A.N = N; A.nion = nion; A.nk = nk; A.M = nmax + 1; A.nlat = nlat;
  A.alpha = tab->alpha; A.c0 = 2.0 * M_PI / tab->area; A.self_ee = tab->self_const;
  for (int k = 0; k < 6; ++k) A.recip[k] = tab->recip[k];
  const int P = N + nion;
  const size_t lds = ((size_t)((3 * P + 1) & ~1) + (size_t)P * 2 * A.M * 2) * sizeof(double);
  if (lds > kE2LdsMax) FAIL("pqa_ewald2d: the phase tables of the electrons and ions do not fit the LDS");
  if (lds + kE2LdsStatic > 64 * 1024) TRY(raise_lds_limit(h, (const void*)k_ewald2d));

  // tables: kt [nk][4], lat [nlat][3], ion_xyz [nion][3], ion_q [nion] (doubles), then kn [nk][2] (ints)
  const size_t nd = (size_t)4 * nk + 3 * nlat + (own ? 0 : 4 * (size_t)nion);
  std::vector<double> host(std::max<size_t>(nd, 1));
  for (int k = 0; k < nk; ++k) {
    const double kk = tab->knorm[k];
    if (!(kk > 0.0)) FAIL("pqa_ewald2d: k vectors must have a positive norm");
    host[4 * k] = kk; host[4 * k + 1] = kk / (2.0 * tab->alpha); host[4 * k + 2] = tab->kpref[k]; host[4 * k + 3] = 2.0 * M_PI / (tab->area * kk);
  }
  std::copy(tab->lat, tab->lat + 3 * nlat, host.begin() + 4 * nk);
  if (!own) {
    std::copy(tab->ion_xyz, tab->ion_xyz + 3 * nion, host.begin() + 4 * nk + 3 * nlat);
    std::copy(tab->ion_charge, tab->ion_charge + nion, host.begin() + 4 * nk + 3 * nlat + 3 * nion);
  }
  TRY(ensure(h, h->b_e2tab, nd * sizeof(double) + (size_t)2 * nk * sizeof(int) + 16));
  double* d_tab = (double*)h->b_e2tab.p;
  int* d_kn = (int*)(d_tab + nd);
  TRY(copy_in(h, d_tab, host.data(), nd * sizeof(double)));
  TRY(copy_in(h, d_kn, tab->kn, (size_t)2 * nk * sizeof(int)));
  A.kt = d_tab; A.kn = d_kn; A.lat = d_tab + 4 * nk;
  A.ion_xyz = own ? h->S.atom_xyz : A.lat + 3 * nlat;
  A.ion_q = own ? h->S.atom_charge : A.ion_xyz + 3 * nion;

  const long Wc = tab->walker_chunk > 0 ? std::min<long>(W, tab->walker_chunk) : walker_chunk(W, 2 * sizeof(double));
  TRY(ensure(h, h->b_e2out, (size_t)2 * Wc * sizeof(double)));
  double* d_out = (double*)h->b_e2out.p;
  if (mean) TRY(ensure(h, h->b_e2acc, (size_t)(2 * kE2Threads + 2) * sizeof(double)));
  for (long w0 = 0; w0 < W; w0 += Wc) {
    const long wc = std::min(Wc, W - w0);
    hipLaunchKernelGGL(k_ewald2d, dim3((unsigned)wc), dim3(kE2Threads), lds, h->stream, h->S, A, x, sw, se, sc, w0, wc, d_out);
    TRY(check_launch(h, "k_ewald2d"));
    if (!mean) {
      TRY(copy_out(h, ee + w0, d_out, (size_t)wc * sizeof(double)));
      TRY(copy_out(h, ei + w0, d_out + wc, (size_t)wc * sizeof(double)));
      continue;
    }
    double* part = (double*)h->b_e2acc.p;
    hipLaunchKernelGGL(k_ewald2d_fold, dim3(1), dim3(kE2Threads), 0, h->stream, (const double*)d_out, w0, wc, (int)(w0 == 0),
                       (int)(w0 + wc == W), (double)W, part, part + 2 * kE2Threads);
    TRY(check_launch(h, "k_ewald2d_fold"));
  }
  if (!mean) return 0;
  const double* acc = (const double*)h->b_e2acc.p + 2 * kE2Threads;
  TRY(copy_out(h, ee, acc, sizeof(double)));
  return copy_out(h, ei, acc + 1, sizeof(double));
}
