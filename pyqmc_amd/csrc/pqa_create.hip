// Construction and destruction of the handle (host side): the tables a system is packed into, in stages (create_impl), and the
// teardown that frees what the handle recorded.  See include/pyqmc_amd.h for the contract.
#include "pqa_internal.hpp"

static thread_local std::string g_create_error;

// determinant of a row-major 3 x 3 matrix, and its inverse by cofactors: inv[r][c] = cof(c, r) / det
static double det3(const double* a) { return a[0] * (a[4] * a[8] - a[5] * a[7]) - a[1] * (a[3] * a[8] - a[5] * a[6]) + a[2] * (a[3] * a[7] - a[4] * a[6]); }
static void inv3(const double* a, double det, double* v) {
  const double id = 1.0 / det;
  v[0] = (a[4] * a[8] - a[5] * a[7]) * id; v[1] = (a[2] * a[7] - a[1] * a[8]) * id; v[2] = (a[1] * a[5] - a[2] * a[4]) * id;
  v[3] = (a[5] * a[6] - a[3] * a[8]) * id; v[4] = (a[0] * a[8] - a[2] * a[6]) * id; v[5] = (a[2] * a[3] - a[0] * a[5]) * id;
  v[6] = (a[3] * a[7] - a[4] * a[6]) * id; v[7] = (a[1] * a[6] - a[0] * a[7]) * id; v[8] = (a[0] * a[4] - a[1] * a[3]) * id;
}

// ---------------------------------------------------------------- membership masks (k_pbc_prepass)
// The reference's image-membership rule asks, for candidate image j of an atom, whether member[class][b + img_n[j]] is set,
// b being the membership base of the (point, atom) pair (pbc_ctx_base).  Tabulated here for every base in an extended grid
// (side + 2 E per axis, E = side >= every |img_n|) as a 128-bit mask over the candidates, so that the pre-pass replaces ~10
// four-load tests per thread by one 16-byte look-up.  315 KB per atom class for M = 4.
static int member_masks(pqa_handle* h, const pqa_system_t* sys, PbcDev& P) {
  P.memb_mask = nullptr;
  P.memb_E = 0;
  const int side = 2 * sys->member_M + 1, E = side, T = side + 2 * E, nc = sys->n_member_class, nj = std::min(sys->nL, 128);
  if ((size_t)nc * T * T * T * 16 > ((size_t)64 << 20)) return 0;  // (absurdly large rule: candidate-by-candidate tests)
  std::vector<unsigned char> mem((size_t)nc * side * side * side);
  std::vector<int> imgn((size_t)sys->nL * 3);
  HIPCHK(hipMemcpy(mem.data(), sys->member, mem.size(), hipMemcpyDefault));
  HIPCHK(hipMemcpy(imgn.data(), sys->img_n, imgn.size() * sizeof(int), hipMemcpyDefault));
  for (int j = 0; j < nj; ++j)
    for (int c = 0; c < 3; ++c)
      if (std::abs(imgn[3 * j + c]) > E) return 0;  // a base outside the grid could still reach a member: no table
  std::vector<unsigned long long> mask((size_t)nc * T * T * T * 2, 0ull);
  for (int cl = 0; cl < nc; ++cl)
    for (int i0 = 0; i0 < T; ++i0)
      for (int i1 = 0; i1 < T; ++i1)
        for (int i2 = 0; i2 < T; ++i2) {
          unsigned long long* m = &mask[2 * ((((size_t)cl * T + i0) * T + i1) * T + i2)];
          for (int j = 0; j < nj; ++j) {
            const int n0 = i0 - E + imgn[3 * j], n1 = i1 - E + imgn[3 * j + 1], n2 = i2 - E + imgn[3 * j + 2];
            if (n0 < 0 || n0 >= side || n1 < 0 || n1 >= side || n2 < 0 || n2 >= side) continue;
            if (mem[(((size_t)cl * side + n0) * side + n1) * side + n2]) m[j >> 6] |= 1ull << (j & 63);
          }
        }
  unsigned long long* d = nullptr;
  TRY(upload_table(h, mask.data(), mask.size(), &d));
  P.memb_mask = d;
  P.memb_E = E;
  return 0;
}

// ---------------------------------------------------------------- near-candidate masks (k_pbc_prepass)
// The pre-pass folds point - atom into the cell-centred parallelepiped and then needs the lattice vectors L_j with
// |d - L_j|^2 <= atom_cut.  The candidate list (num_Ls[atom] vectors, 79 in the 2x2x2 diamond cell) is what ANY point of the
// cell may need; a given point needs about a sixth of it.  Tabulated here, for every sub-cell of a G^3 grid over the fractional
// coordinates [-1/2, 1/2)^3, the candidates whose distance to the sub-cell's centre is at most sqrt(atom_cut) + the sub-cell's
// half diagonal (padded): a superset of what any point inside it can admit.  16 bytes per (atom, sub-cell).
static int near_masks(pqa_handle* h, const pqa_system_t* sys, const std::vector<int>& nl, const std::vector<double>& ac, PbcDev& P) {
  P.near_mask = nullptr;
  P.near_G = 0;
  int G = (size_t)h->natom * 16 * 16 * 16 * 16 <= ((size_t)2 << 20) ? 16 : 8;  // (the table should stay in an XCD's L2)
  if (const char* e = getenv("PQA_PRE_GRID")) G = std::max(0, std::min(16, atoi(e)));
  while (G > 1 && (size_t)h->natom * G * G * G * 16 > ((size_t)64 << 20)) G /= 2;
  if (G < 2) return 0;
  const int nj = std::min(sys->nL, 128);
  std::vector<double> ls((size_t)nj * 3);
  HIPCHK(hipMemcpy(ls.data(), sys->Ls, ls.size() * sizeof(double), hipMemcpyDefault));
  const double* a = sys->lattice;
  const double hw = 0.5 / G + 1e-6;  // half width of a sub-cell in fractional coordinates, padded for the rounding of the fold
  double rho = 0.0;
  for (int sg = 0; sg < 4; ++sg) {   // half of the longest body diagonal
    const double s1 = (sg & 1) ? -hw : hw, s2 = (sg & 2) ? -hw : hw;
    double d2 = 0.0;
    for (int c = 0; c < 3; ++c) { const double v = hw * a[c] + s1 * a[3 + c] + s2 * a[6 + c]; d2 += v * v; }
    rho = std::max(rho, std::sqrt(d2));
  }
  std::vector<unsigned long long> mask((size_t)h->natom * G * G * G * 2, 0ull);
  for (int ia = 0; ia < h->natom; ++ia) {
    const double reach = std::sqrt(std::max(ac[ia], 0.0)) * (1.0 + 1e-9) + rho + 1e-9;
    const int n = std::min(nl[ia], nj);
    for (int g0 = 0; g0 < G; ++g0)
      for (int g1 = 0; g1 < G; ++g1)
        for (int g2 = 0; g2 < G; ++g2) {
          const double f[3] = {(g0 + 0.5) / G - 0.5, (g1 + 0.5) / G - 0.5, (g2 + 0.5) / G - 0.5};
          double ctr[3];
          for (int c = 0; c < 3; ++c) ctr[c] = f[0] * a[c] + f[1] * a[3 + c] + f[2] * a[6 + c];
          unsigned long long* m = &mask[2 * ((((size_t)ia * G + g0) * G + g1) * G + g2)];
          for (int j = 0; j < n; ++j) {
            const double dx = ctr[0] - ls[3 * j], dy = ctr[1] - ls[3 * j + 1], dz = ctr[2] - ls[3 * j + 2];
            if (dx * dx + dy * dy + dz * dz <= reach * reach) m[j >> 6] |= 1ull << (j & 63);
          }
        }
  }
  unsigned long long* d = nullptr;
  TRY(upload_table(h, mask.data(), mask.size(), &d));
  P.near_mask = d;
  P.near_G = G;
  return 0;
}

// ---------------------------------------------------------------- Voronoi-relevant lattice vectors (min_image)
// v is relevant iff v/2 is strictly closer to 0 (and v) than to every other lattice point.  Candidates: coefficients in
// {-2..2}^3 (all relevant vectors of any cell that is not absurdly skewed), tested against the points with coefficients in
// {-4..4}^3.  One of each +- pair; three-dimensional lattices have at most 7 pairs.
static int voronoi_vectors(const double* a, PbcDev& P) {
  P.nvor = 0;
  for (int q = 0; q < 7; ++q) { P.vor[q][0] = P.vor[q][1] = P.vor[q][2] = 0.0; P.vorh[q] = 1.0; }  // padding: never violated
  auto vec = [&](int i, int j, int k, double* v) {
    for (int c = 0; c < 3; ++c) v[c] = i * a[c] + j * a[3 + c] + k * a[6 + c];
  };
  for (int i = -2; i <= 2; ++i)
    for (int j = -2; j <= 2; ++j)
      for (int k = -2; k <= 2; ++k) {
        if (i < 0 || (i == 0 && (j < 0 || (j == 0 && k <= 0)))) continue;  // one of each pair, not the origin
        double v[3];
        vec(i, j, k, v);
        const double half = 0.5 * std::sqrt(v[0] * v[0] + v[1] * v[1] + v[2] * v[2]);
        bool relevant = true;
        for (int p = -4; p <= 4 && relevant; ++p)
          for (int q = -4; q <= 4 && relevant; ++q)
            for (int r = -4; r <= 4; ++r) {
              if ((p == 0 && q == 0 && r == 0) || (p == i && q == j && r == k)) continue;
              double u[3];
              vec(p, q, r, u);
              const double d = std::sqrt((0.5 * v[0] - u[0]) * (0.5 * v[0] - u[0]) + (0.5 * v[1] - u[1]) * (0.5 * v[1] - u[1]) +
                                         (0.5 * v[2] - u[2]) * (0.5 * v[2] - u[2]));
              if (d <= half * (1.0 + 1e-9)) { relevant = false; break; }
            }
        if (!relevant) continue;
        if (P.nvor >= 7) return 1;
        for (int c = 0; c < 3; ++c) P.vor[P.nvor][c] = v[c];
        P.vorh[P.nvor] = 2.0 * half * half;  // |v|^2 / 2
        ++P.nvor;
      }
  return P.nvor >= 3 ? 0 : 1;
}

// ---------------------------------------------------------------- phase-1 cost model of the shells
// One evaluation of a shell costs a radial part per primitive and an angular part / tile stores per function.  An open
// system evaluates every shell once per point.  A periodic one evaluates it once per image inside the SHELL's cut-off — the
// wave walks max-over-lanes of that count, about 1.4 x the mean V_sphere(shell_cut) / V_cell plus one — and from the second
// (farther) image on only the primitives that survive the screening at half the shortest lattice vector are evaluated.
// Packing the lane groups with the per-evaluation cost alone gave a group holding two diffuse p shells (13 images each in
// the 2x2x2 diamond cell) 2.3 x the average load, and a barrier ends every chunk.
// Radial tables of the contracted shells (SysDev::rtab, radial_tab in pqa_ao.hpp): per distinct (exponent, coefficient) sequence of at least
// PQA_RT_MINP primitives the sum R(x) = sum_p c_p exp(-a_p x) as degree-9 polynomials on the intervals y = x + 2^-7 in
// 2^(o-7) [1 + j/8, 1 + (j+1)/8), o = 0 .. until every primitive is below exp(-46).  Chebyshev interpolation at the 10 nodes of every interval
// in long double, converted to powers of the local variable u in [-1, 1]; the largest error found at 33 points per interval (in the device's
// arithmetic: double Horner) is kept in h->rt_err, relative to sum_p |c_p| (1e-15 for cc-pVDZ-shaped contractions; pqa_debug_radtab_err, and
// the device tests compare the orbitals with the primitive sums).  Open systems only (the lattice sums keep their exponentials), value-only
// orbital kernel only; PQA_RADTAB=0 turns it off.
static int build_radial_tables(pqa_handle* h, const pqa_system_t* sys, SysDev& S) {
  std::vector<int> rt((size_t)2 * sys->nshell, -1);
  std::vector<double> tab;
  h->rt_err = 0.0;
  const char* env = getenv("PQA_RADTAB");
  const bool on = !(env && atoi(env) == 0) && sys->pbc == 0;
  std::vector<double> pe_((size_t)std::max(sys->nprim, 1)), pc_((size_t)std::max(sys->nprim, 1));
  std::vector<int> po_((size_t)sys->nshell + 1);
  HIPCHK(hipMemcpy(pe_.data(), sys->prim_exp, (size_t)sys->nprim * sizeof(double), hipMemcpyDefault));
  HIPCHK(hipMemcpy(pc_.data(), sys->prim_coef, (size_t)sys->nprim * sizeof(double), hipMemcpyDefault));
  HIPCHK(hipMemcpy(po_.data(), sys->shell_prim_off, po_.size() * sizeof(int), hipMemcpyDefault));
  const double* prim_exp = pe_.data();
  const double* prim_coef = pc_.data();
  const int* shell_prim_off = po_.data();
  if (on) {
    constexpr int n = PQA_RT_DEG + 1;
    long double nodes[n], Tm[n][n];  // Chebyshev nodes; T_q(u) in powers of u
    const long double pi = acosl(-1.0L);
    for (int k = 0; k < n; ++k) nodes[k] = cosl(pi * (k + 0.5L) / n);
    for (int q = 0; q < n; ++q)
      for (int d = 0; d < n; ++d) Tm[q][d] = 0.0L;
    Tm[0][0] = 1.0L; Tm[1][1] = 1.0L;
    for (int q = 2; q < n; ++q)
      for (int d = 0; d < n; ++d) Tm[q][d] = (d > 0 ? 2.0L * Tm[q - 1][d - 1] : 0.0L) - Tm[q - 2][d];
    for (int sh = 0; sh < sys->nshell; ++sh) {
      const int p0 = shell_prim_off[sh], np = shell_prim_off[sh + 1] - p0;
      if (np < PQA_RT_MINP) continue;
      int same = -1;
      for (int prev = 0; prev < sh && same < 0; ++prev) {
        const int q0 = shell_prim_off[prev];
        if (shell_prim_off[prev + 1] - q0 == np && rt[2 * prev] >= 0 && std::equal(prim_exp + p0, prim_exp + p0 + np, prim_exp + q0) &&
            std::equal(prim_coef + p0, prim_coef + p0 + np, prim_coef + q0)) same = prev;
      }
      if (same >= 0) { rt[2 * sh] = rt[2 * same]; rt[2 * sh + 1] = rt[2 * same + 1]; continue; }
      double amin = prim_exp[p0];
      for (int p = 0; p < np; ++p) amin = std::min(amin, prim_exp[p0 + p]);
      if (!(amin > 0.0)) continue;
      const int noct = std::max(1, (int)std::ceil(std::log2((46.0 / amin + PQA_RT_X0) / PQA_RT_X0)));
      if (noct > 40) continue;
      const int nint = noct * PQA_RT_NSUB;
      const size_t tab0 = tab.size();
      double err_sh = 0.0;
      rt[2 * sh] = (int)tab.size(); rt[2 * sh + 1] = nint;
      long double scale = 0.0L;
      for (int p = 0; p < np; ++p) scale += fabsl((long double)prim_coef[p0 + p]);
      auto F = [&](long double x) {
        long double f = 0.0L;
        for (int p = 0; p < np; ++p) f += (long double)prim_coef[p0 + p] * expl(-(long double)prim_exp[p0 + p] * x);
        return f;
      };
      for (int o = 0; o < noct; ++o)
        for (int j = 0; j < PQA_RT_NSUB; ++j) {
          const long double ylo = (long double)PQA_RT_X0 * ldexpl(1.0L, o) * (1.0L + (long double)j / PQA_RT_NSUB);
          const long double yhi = (long double)PQA_RT_X0 * ldexpl(1.0L, o) * (1.0L + (long double)(j + 1) / PQA_RT_NSUB);
          const long double xc = 0.5L * (ylo + yhi) - (long double)PQA_RT_X0, hw = 0.5L * (yhi - ylo);
          {
            long double fv[n], cc[n], mono[n];
            for (int q = 0; q < n; ++q) fv[q] = F(xc + hw * nodes[q]);
            for (int q = 0; q < n; ++q) {
              long double sum = 0.0L;
              for (int m = 0; m < n; ++m) sum += fv[m] * cosl(q * pi * (m + 0.5L) / n);
              cc[q] = (q == 0 ? 1.0L : 2.0L) * sum / n;
            }
            for (int d = 0; d < n; ++d) { mono[d] = 0.0L; for (int q = 0; q < n; ++q) mono[d] += cc[q] * Tm[q][d]; }
            double m64[n];
            for (int d = 0; d < n; ++d) { m64[d] = (double)mono[d]; tab.push_back(m64[d]); }
            for (int t = 0; t <= 32; ++t) {  // the table against the sums, in the arithmetic the device uses (double Horner)
              const double u = -1.0 + t / 16.0;
              double pv = m64[n - 1];
              for (int d = n - 2; d >= 0; --d) pv = std::fma(pv, u, m64[d]);
              const long double ex = F(xc + hw * (long double)u);
              err_sh = std::max(err_sh, (double)(fabsl((long double)pv - ex) / scale));
            }
          }
        }
      // A table is kept only if it reproduces the primitive sum to rounding everywhere: the tight primitives of all-electron sets (exponent
      // 11 720 in cc-pVDZ oxygen: e^{-a x} falls by e^-11 across the first interval) are beyond a degree-9 fit — 1e-5 of sum |c| — and such
      // shells keep their exponentials.
      if (err_sh > PQA_RT_MAXERR) { tab.resize(tab0); rt[2 * sh] = -1; rt[2 * sh + 1] = 0; }
      else h->rt_err = std::max(h->rt_err, err_sh);
    }
  }
  double* td = nullptr; int* ti = nullptr;
  TRY(upload_table(h, tab.data(), tab.size(), &td)); S.rtab = td;
  TRY(upload_table(h, rt.data(), rt.size(), &ti)); S.shell_rt = ti;
  h->rt_shells.assign(rt.begin(), rt.end());
  if (getenv("PQA_RES_DEBUG")) fprintf(stderr, "[pqa] radial tables: %zu doubles, largest error %.2e of sum |c|\n", tab.size(), h->rt_err);
  return 0;
}

static void shell_costs(pqa_handle* h, const pqa_system_t* sys) {
  const int tw = h->twist ? 2 : 1;
  h->shell_cost.assign((size_t)h->nshell, 0);
  std::vector<double> scut, pexp;
  double vol = 0.0, half2 = 0.0;
  if (sys->pbc && sys->nL > 0 && sys->shell_cut) {
    scut.resize((size_t)h->nshell);
    hipMemcpy(scut.data(), sys->shell_cut, scut.size() * sizeof(double), hipMemcpyDefault);
    pexp.resize((size_t)sys->nprim);
    hipMemcpy(pexp.data(), sys->prim_exp, pexp.size() * sizeof(double), hipMemcpyDefault);
    const double* a = sys->lattice;
    vol = fabs(det3(a));
    half2 = 1e300;
    for (int i = 0; i < 3; ++i) half2 = std::min(half2, 0.25 * (a[3 * i] * a[3 * i] + a[3 * i + 1] * a[3 * i + 1] + a[3 * i + 2] * a[3 * i + 2]));
  }
  std::vector<int> poff((size_t)h->nshell + 1);
  hipMemcpy(poff.data(), sys->shell_prim_off, poff.size() * sizeof(int), hipMemcpyDefault);
  for (int s = 0; s < h->nshell; ++s) {
    const int ang = 25 * tw * (2 * h->shell_l[s] + 1) + 40;
    if (scut.empty() || !(vol > 0.0)) { h->shell_cost[s] = 45 * h->shell_np[s] + ang; continue; }
    const double mean = 4.18879020478639 * scut[s] * std::sqrt(scut[s]) / vol;
    const double iters = std::max(1.0, 1.4 * mean + 1.0);
    int far = 0;  // primitives still evaluated beyond the nearest image
    for (int q = poff[s]; q < poff[s + 1]; ++q) far += (pexp[q] * half2 <= 50.0) ? 1 : 0;
    h->shell_cost[s] = (int)((45 * h->shell_np[s] + ang + 30) + (iters - 1.0) * (45 * far + ang + 30));
  }
}

// ---------------------------------------------------------------- chunk tables for k_orb
static void build_chunks(const pqa_handle* h, int KC, ChunkHost& c) {
  c = ChunkHost();
  for (int g = 0; g < 3; ++g) c.cw_off[g].push_back(0);
  // twisted cells: a shell's complex lattice sum occupies 2 (2l+1) tile rows, real parts then imaginary parts, in ONE
  // chunk, so that a single walk over the images fills both (evaluating the parts as two separate shells doubled the
  // exp work).  shell_kb / shell_chunk keep an entry sh + nshell for the imaginary rows (coefficient upload).
  const int nsx = h->nshell, tw = h->twist ? 2 : 1;
  c.shell_kb.assign((size_t)tw * h->nshell, 0);
  c.shell_chunk.assign((size_t)tw * h->nshell, 0);
  // phase-1 cost of a shell: radial part per primitive + angular part / tile stores per function
  auto cost = [&](int s) { return h->shell_cost[s]; };
  auto nfun = [&](int s) { return tw * (2 * h->shell_l[s] + 1); };
  int nao = 0;
  for (int s = 0; s < nsx; ++s) nao += nfun(s);
  // Longest-processing-time packing over (chunk, group) slots under the chunk's row capacity; if a shell does not
  // fit anywhere a chunk is added.  4 groups per chunk (64-point tiles) is the layout that is balanced; the
  // 8-group lists (32-point tiles) are a second LPT inside each chunk.
  std::vector<int> order((size_t)nsx);
  for (int s = 0; s < nsx; ++s) order[s] = s;
  std::stable_sort(order.begin(), order.end(), [&](int a, int b) { return cost(a) > cost(b); });
  int nchunk = std::max((nao + KC - 1) / KC, 1);
  std::vector<std::vector<int>> load;
  std::vector<int> rows;
  std::vector<std::vector<std::vector<int>>> slot;  // [chunk][group] -> shells
  for (;;) {
    load.assign((size_t)nchunk, std::vector<int>(4, 0));
    rows.assign((size_t)nchunk, 0);
    slot.assign((size_t)nchunk, std::vector<std::vector<int>>(4));
    bool ok = true;
    for (int s : order) {
      int bc = -1, bg = -1;
      for (int ch = 0; ch < nchunk; ++ch) {
        if (rows[ch] + nfun(s) > KC) continue;
        for (int g = 0; g < 4; ++g)
          if (bc < 0 || load[ch][g] < load[bc][bg]) { bc = ch; bg = g; }
      }
      if (bc < 0) { ok = false; break; }
      slot[bc][bg].push_back(s);
      load[bc][bg] += cost(s);
      rows[bc] += nfun(s);
    }
    if (ok) break;
    ++nchunk;
  }
  int row0 = 0;
  for (int ch = 0; ch < nchunk; ++ch) {
    if (rows[ch] == 0) continue;  // (possible after a capacity retry)
    const int ci = (int)c.nk.size();
    c.nk.push_back(rows[ch]);
    c.row0.push_back(row0);
    row0 += (rows[ch] + 3) & ~3;
    int kb = 0;
    std::vector<int> members;
    for (int g = 0; g < 4; ++g)
      for (int s : slot[ch][g]) {
        c.shell_kb[s] = kb; c.shell_chunk[s] = ci;
        if (tw == 2) { c.shell_kb[s + h->nshell] = kb + nfun(s) / 2; c.shell_chunk[s + h->nshell] = ci; }
        kb += nfun(s);
        members.push_back(s);
      }
    for (int g = 0; g < 4; ++g) {
      for (int s : slot[ch][g]) c.cw_shell[0].push_back(s);
      c.cw_off[0].push_back((int)c.cw_shell[0].size());
    }
    std::stable_sort(members.begin(), members.end(), [&](int a, int b) { return cost(a) > cost(b); });
    std::vector<std::vector<int>> l8(8);
    std::vector<int> load8(8, 0);
    for (int s : members) {
      int best = 0;
      for (int q = 1; q < 8; ++q)
        if (load8[q] < load8[best]) best = q;
      l8[best].push_back(s);
      load8[best] += cost(s);
    }
    for (int q = 0; q < 8; ++q) {
      for (int s : l8[q]) c.cw_shell[1].push_back(s);
      c.cw_off[1].push_back((int)c.cw_shell[1].size());
    }
    std::vector<std::vector<int>> l16(16);  // 16-point tiles: 16 lane groups
    std::vector<int> load16(16, 0);
    for (int s : members) {
      int best = 0;
      for (int q = 1; q < 16; ++q)
        if (load16[q] < load16[best]) best = q;
      l16[best].push_back(s);
      load16[best] += cost(s);
    }
    for (int q = 0; q < 16; ++q) {
      for (int s : l16[q]) c.cw_shell[2].push_back(s);
      c.cw_off[2].push_back((int)c.cw_shell[2].size());
    }
  }
  c.rows_pad = row0;
}

// zero-padded coefficient matrix for one chunk table / spin
static int upload_cpad(pqa_handle* h, int t, int s, const double* mo_host) {
  const ChunkHost& c = h->chunks[t];
  const int ldc = 16 * h->nt[s], nmo = h->nmo[s];
  std::vector<double> pad((size_t)std::max(c.rows_pad, 1) * ldc, 0.0);
  for (int sh = 0; sh < h->nshell; ++sh)  // tile row (chunk, shell_kb + m)  <-  AO shell_ao[sh] + m
    for (int m = 0; m < 2 * h->shell_l[sh] + 1; ++m)
      for (int j = 0; j < nmo; ++j)
        pad[(size_t)(c.row0[c.shell_chunk[sh]] + c.shell_kb[sh] + m) * ldc + j] = mo_host[(size_t)(h->shell_ao[sh] + m) * nmo + j];
  if (h->twist) {  // rows of the imaginary AO parts: (i AO_im)(C_re + i C_im) = AO_im (-C_im + i C_re), columns [re | im]
    const int nr = nmo / 2;
    for (int sh = 0; sh < h->nshell; ++sh) {
      const int sx = sh + h->nshell;
      for (int m = 0; m < 2 * h->shell_l[sh] + 1; ++m)
        for (int j = 0; j < nr; ++j) {
          const double* src = mo_host + (size_t)(h->shell_ao[sh] + m) * nmo;
          double* dst = pad.data() + (size_t)(c.row0[c.shell_chunk[sx]] + c.shell_kb[sx] + m) * ldc;
          dst[j] = -src[nr + j];
          dst[nr + j] = src[j];
        }
    }
  }
  HIPCHK(hipMemcpy(h->d_cpad[t][s], pad.data(), pad.size() * sizeof(double), hipMemcpyHostToDevice));
  return 0;
}

int set_mo(pqa_handle* h, int s, const double* mo_host) {
  if (h->nmo[s] == 0 || !mo_host) return 0;  // an empty spin channel (fully polarised systems): nothing to upload
  HIPCHK(hipMemcpy(h->d_mo[s], mo_host, (size_t)h->nao * std::max(h->nmo[s], 1) * sizeof(double), hipMemcpyHostToDevice));
  for (int t = 0; t < 2; ++t) TRY(upload_cpad(h, t, s, mo_host));
  TRY(cres_upload(h, s, mo_host));  // (the resident sweep's dense coefficient copy, if it keeps one)
  return 0;
}

// ---------------------------------------------------------------- create / destroy
extern "C" int pqa_device_count(void) {
  int n = 0;
  if (hipGetDeviceCount(&n) != hipSuccess) return 0;
  return n;
}

extern "C" const char* pqa_last_error(const pqa_handle_t* h) { return h ? h->err.c_str() : g_create_error.c_str(); }

// ccoeff (natom,na3,na3,nb3,3) -> C = (c + c^T_kl)/2 (three_body_jastrow.py:94-96)
int set_c3(pqa_handle* h, const double* c) {
  const int A = h->natom, na = h->na3, nb = h->nb3;
  std::vector<double> sym((size_t)A * na * na * nb * 3);
  for (int I = 0; I < A; ++I)
    for (int k = 0; k < na; ++k)
      for (int l = 0; l < na; ++l)
        for (int m = 0; m < nb * 3; ++m) {
          const size_t a = (((size_t)I * na + k) * na + l) * nb * 3 + m, b = (((size_t)I * na + l) * na + k) * nb * 3 + m;
          sym[a] = 0.5 * (c[a] + c[b]);
        }
  HIPCHK(hipMemcpy(h->d_c3, sym.data(), sym.size() * sizeof(double), hipMemcpyHostToDevice));
  return 0;
}

// The reference's quadrature grids (eval_ecp.py:278-336, generate_quadrature_grids), every rule in the reference's point order.
// Octahedral families from the 27 points of {-1,0,1}^3 (x slowest, z fastest: numpy's mgrid order) by their count of non-zero
// coordinates: OA (1, the axes), OB (2, / sqrt 2), OC (3, / sqrt 3), OD = the three cyclic column rolls of (+-1, +-1, +-3) / sqrt 11.
// Icosahedral families from polar angles: A the poles, B the ten points at atan 2 / pi - atan 2, C the twenty at c_1, c_2.
int ecp_quadrature_offset(int naip) {
  switch (naip) { case 6: return 0; case 12: return 6; case 18: return 18; case 26: return 36; case 32: return 62; case 50: return 94; default: return -1; }
}
static void ecp_quadrature_tables(std::vector<double>& quad, std::vector<double>& quadw) {
  std::vector<std::array<double, 3>> O[4], I[3];
  for (int x = -1; x <= 1; ++x)
    for (int y = -1; y <= 1; ++y)
      for (int z = -1; z <= 1; ++z) {
        const int nz = (x != 0) + (y != 0) + (z != 0);
        if (nz == 0) continue;
        const double sc = nz == 1 ? 1.0 : std::sqrt((double)nz);
        O[nz - 1].push_back({x / sc, y / sc, z / sc});
      }
  {
    const double f = std::sqrt(3.0 / 11.0);
    std::vector<std::array<double, 3>> d1;
    for (auto& p : O[2]) d1.push_back({p[0] * f, p[1] * f, p[2] * f * 3.0});
    for (int roll = 0; roll < 3; ++roll)  // np.roll(d1, roll, axis=1): column j moves to column (j + roll) % 3
      for (auto& p : d1) {
        std::array<double, 3> q;
        for (int j = 0; j < 3; ++j) q[(j + roll) % 3] = p[j];
        O[3].push_back(q);
      }
  }
  {
    const double pi = std::acos(-1.0), b1 = std::atan(2.0), s5 = std::sqrt(5.0);
    const double c1 = std::acos((2.0 + s5) / std::sqrt(15.0 + 6.0 * s5)), c2 = std::acos(1.0 / std::sqrt(15.0 + 6.0 * s5));
    auto sph = [](double t, double p) { return std::array<double, 3>{std::sin(t) * std::cos(p), std::sin(t) * std::sin(p), std::cos(t)}; };
    I[0].push_back(sph(0.0, 0.0)); I[0].push_back(sph(pi, 0.0));
    for (int k = 0; k < 10; ++k) I[1].push_back(sph(k % 2 == 0 ? b1 : pi - b1, k * pi / 5.0));
    for (int k = 0; k < 10; ++k) I[2].push_back(sph(k % 2 == 0 ? pi - c1 : c1, k * pi / 5.0));
    for (int k = 0; k < 10; ++k) I[2].push_back(sph(k % 2 == 0 ? pi - c2 : c2, k * pi / 5.0));
  }
  auto emit = [&](const std::vector<std::array<double, 3>>* fam, int nfam, const double* w) {
    for (int f = 0; f < nfam; ++f)
      for (auto& p : fam[f]) { quad.insert(quad.end(), p.begin(), p.end()); quadw.push_back(w[f]); }
  };
  const double w6[] = {1.0 / 6}, w12[] = {1.0 / 12, 1.0 / 12}, w18[] = {1.0 / 30, 1.0 / 15}, w26[] = {1.0 / 21, 4.0 / 105, 27.0 / 840};
  const double w32[] = {5.0 / 168, 5.0 / 168, 27.0 / 840}, w50[] = {4.0 / 315, 64.0 / 2835, 27.0 / 1280, 14641.0 / 725760};
  emit(O, 1, w6); emit(I, 2, w12); emit(O, 2, w18); emit(O, 3, w26); emit(I, 3, w32); emit(O, 4, w50);
}

// ---- create_impl's stages, in the order they run
// switches of the environment, then the system's sizes and kinds and the limits they must respect
static int create_switches(pqa_handle* h, const pqa_system_t* sys) {
  // Environment switches.  Each pins one of two routes that the handle otherwise picks from the system and the shard size, so that
  // a test can compare them (results agree up to summation order, bitwise where the test says so).  Read here unless noted;
  // the last column names the tests/test_gpu_*.py files that set the switch:
  //   PQA_RES 0|1           resident sweeps off / forced (default: res_plan, r8_plan)                     fullsize, parity, pbc
  //   PQA_R8 0|1            k_sweep_r8 off / forced for open-boundary real handles                          fullsize, parity
  //   PQA_WW 0|1            one-launch wave-per-walker sweep off / forced (default: up to ww.max walkers)   fullsize
  //   PQA_LW 0              wave-per-walker kernels instead of the lane-per-walker fused sweep              parity, pbc
  //   PQA_LW_KB k           electrons per Sherman-Morrison block (0: every row on every move)               parity; bench.py reads it
  //   PQA_LW_GM g           thread groups per walker of the move kernels (0: automatic)                     jastrow_merge
  //   PQA_STEP_PRE 0        k_step_lw for small shards too, instead of k_step_pre                           parity, fullsize, jastrow_merge
  //   PQA_ECP_LDS 0         first-generation ECP list passes (k_ecp_count / k_ecp_fill)                     parity
  //   PQA_ECP_POINT_LW 0    k_ecp_point on the planes instead of k_ecp_point_lw                             parity, pbc
  //   PQA_ECP_WAVE 1        wave-per-walker ECP accumulation                                                parity
  //   PQA_ECP_ACC_WAVES 1|4 waves per walker of k_ecp_accum / k_kinetic_coulomb                             parity
  //   PQA_ECP_DEFER 0       ECP point totals read back at every evaluation                                  parity
  //   PQA_ORB_TP 16|32|64   point tile of k_orb (periodic: pins the automatic choice)                       pbc
  //   PQA_ORB_WS 0|1        phase-alternating / wave-specialised k_orb                                      parity
  //   PQA_ORB_GENERAL 1     orbitals beyond 64 per spin by k_ao + k_mo_rows instead of the windowed k_orb   parity
  //   PQA_JAS_MERGE 0       Pade functions one by one instead of the merged rational function               jastrow_merge
  //   PQA_JAS_FOLD 0        Voronoi reduction in every periodic Jastrow pair                                pbc
  //   PQA_RADTAB 0          primitive sums instead of radial tables (build_radial_tables)                   parity
  //   PQA_PRE_GRID g        sub-cells per axis of the pre-pass candidate masks (0: all tested; near_masks)  pbc
  //   PQA_PRE_NCUT n        at least n shell cut-off classes in the pre-pass instantiation (below)          pbc
  //   PQA_PBC_NW n          words per (point, atom) pre-pass image list (below; 1: direct tests)            pbc
  //   PQA_RES_ICAP n        shorter image lists in the periodic resident sweep (pqa_res.hip)                fullsize
  // Diagnostics: PQA_RES_DEBUG 1|2 prints the resident sweeps' tile / LDS plans (pqa_res.hip, pqa_res8.hip), the radial-table fit
  // error and, whenever a handle's sweep takes another route than its last one, "[pqa] sweep route: <kernel>" (sweep_electrons); PQA_R8_STAGGER and PQA_R8_ABL set fields of k_sweep_r8's table (pqa_res8.hip; PQA_R8_ABL: timing builds only).
  const struct { const char* name; int* field; } sw[] = {
      {"PQA_ORB_TP", &h->orb_tp}, {"PQA_LW", &h->lw.mode}, {"PQA_RES", &h->res.mode}, {"PQA_R8", &h->r8.mode}, {"PQA_WW", &h->ww.mode},
      {"PQA_ECP_DEFER", &h->en.ecp_defer}, {"PQA_ORB_WS", &h->orb_ws}, {"PQA_LW_KB", &h->lw.kb}, {"PQA_LW_GM", &h->lw.gm},
      {"PQA_ECP_WAVE", &h->en.ecp_wave}, {"PQA_ECP_POINT_LW", &h->en.ecp_point_lw}, {"PQA_ECP_LDS", &h->en.ecp_lds}, {"PQA_JAS_FOLD", &h->jas_fold_allowed},
      {"PQA_ECP_ACC_WAVES", &h->en.ecp_acc_waves}, {"PQA_STEP_PRE", &h->lw.step_pre}, {"PQA_JAS_MERGE", &h->jas_merge}};
  for (const auto& w : sw)
    if (const char* e = getenv(w.name)) *w.field = atoi(e);
  h->route.debug = getenv("PQA_RES_DEBUG") != nullptr;
  h->natom = sys->natom; h->nup = sys->nelec_up; h->ndn = sys->nelec_dn; h->N = h->nup + h->ndn;
  h->nao = sys->nao; h->nshell = sys->nshell;
  h->has_slater = sys->has_slater != 0;
  h->cplx = h->has_slater && sys->complex_orbitals != 0;
  h->twist = sys->twisted != 0;
  if (h->twist && !(h->cplx && sys->pbc && sys->nL > 0)) FAIL("twisted boundary conditions need pbc, complex_orbitals and the periodic orbital tables");
  if (h->cplx && ((sys->nmo_up | sys->nmo_dn) & 1)) FAIL("complex orbitals: nmo_up / nmo_dn count the real columns [Re C | Im C] and must be even");
  h->has_j2 = sys->na > 0 || sys->nb > 0;
  h->has_j3 = sys->na3 > 0 && sys->nb3 > 0;
  h->has_jastrow = h->has_j2 || h->has_j3;
  h->na = sys->na; h->nb = sys->nb; h->necp = sys->necp; h->na3 = h->has_j3 ? sys->na3 : 0; h->nb3 = h->has_j3 ? sys->nb3 : 0;
  if (h->na > PQA_MAXBAS || h->nb > PQA_MAXBAS) FAIL("more than 16 two-body Jastrow basis functions per kind");
  if (h->na3 > PQA_MAXBAS3 || h->nb3 > PQA_MAXBAS3) FAIL("more than 8 three-body Jastrow basis functions per kind");
  if (h->nup > PQA_MAXN || h->ndn > PQA_MAXN) FAIL("more than 128 electrons per spin channel are not supported");
  // More than 64 electrons or orbitals of a spin (slater.py:155-260 takes any number): the handle runs on the kernels that are
  // general in n — orbitals by the thread-per-point evaluator + k_mo_rows, determinants by the wave-per-walker kernels with two
  // columns per lane (k_build_invert, slater_ratios, sm_update_wave on the inverse in place), no lane-per-walker planes.
  h->big = h->nup > PQA_MAXN_FAST || h->ndn > PQA_MAXN_FAST || (sys->has_slater && (sys->nmo_up > PQA_MAXN_FAST || sys->nmo_dn > PQA_MAXN_FAST));
  if (h->big && h->twist) FAIL("twisted cells: at most 64 electrons and 64 orbitals per spin channel (the general orbital path evaluates real AOs)");
  if (h->big && h->cplx && !(sys->pbc && sys->nL > 0)) FAIL("complex orbitals beyond 64 per spin: periodic handles only");
  if (h->big) h->lw.mode = 0;
  if (const char* e = getenv("PQA_ORB_GENERAL")) h->orb_general = atoi(e) != 0;
  return 0;
}

// cell (lattice, its inverse, Voronoi vectors, whether Jastrow pairs may skip the reduction) and atoms
static int create_lattice(pqa_handle* h, const pqa_system_t* sys, PbcDev& P) {
  SysDev& S = h->S;
  S.natom = h->natom; S.nup = h->nup; S.ndn = h->ndn; S.nelec = h->N;
  S.pbc = sys->pbc;
  if (S.pbc < 0 || S.pbc > 2) FAIL("pbc must be 0 (open), 1 (orthogonal cell) or 2 (general cell)");
  if (S.pbc) {
    const double* a = sys->lattice;
    const double det = det3(a);
    if (!(fabs(det) > 1e-12)) FAIL("singular lattice");
    for (int i = 0; i < 9; ++i) P.lat[i] = a[i];
    if (S.pbc == 2 && voronoi_vectors(a, P)) FAIL("could not determine the Voronoi-relevant vectors of the lattice");
    inv3(a, det, P.linv);
    {  // inradius of {frac in [-1/2, 1/2)^3}: the face frac_c = 1/2 is 1 / (2 |column c of linv|) away from the origin
      double rho = 1e300;
      for (int c = 0; c < 3; ++c) rho = std::min(rho, 0.5 / sqrt(P.linv[c] * P.linv[c] + P.linv[3 + c] * P.linv[3 + c] + P.linv[6 + c] * P.linv[6 + c]));
      double rmax = 0.0;
      if (sys->na > 0) rmax = std::max(rmax, sys->rcut_a);
      if (sys->nb > 0) rmax = std::max(rmax, sys->rcut_b);
      if (sys->na3 > 0 && sys->nb3 > 0) rmax = std::max(rmax, std::max(sys->rcut_a3, sys->rcut_b3));
      P.jas_fold = (h->jas_fold_allowed && rmax <= rho * (1.0 + 1e-12)) ? 1 : 0;
    }
  }
  double* tmp_d;
  TRY(upload_table(h, sys->atom_xyz, (size_t)h->natom * 3, &tmp_d)); S.atom_xyz = tmp_d;
  TRY(upload_table(h, sys->atom_charge, (size_t)h->natom, &tmp_d)); S.atom_charge = tmp_d;
  for (int i = 0; i < h->natom; ++i)
    for (int j = i + 1; j < h->natom; ++j) {
      double d2 = 0;
      for (int k = 0; k < 3; ++k) { const double d = sys->atom_xyz[3 * i + k] - sys->atom_xyz[3 * j + k]; d2 += d * d; }
      h->ii_energy += sys->atom_charge[i] * sys->atom_charge[j] / std::sqrt(d2);
    }
  return 0;
}

// basis tables of the orbitals and, for a cell, the lattice-sum tables: image lists, cut-off classes, masks, twist phases, membership
static int create_orbital_tables(pqa_handle* h, const pqa_system_t* sys, PbcDev& P) {
  SysDev& S = h->S;
  double* tmp_d; int* tmp_i;
  S.nshell = sys->nshell; S.nprim = sys->nprim; S.nao = sys->nao;
  for (int s = 0; s < sys->nshell; ++s) {
    if (sys->shell_l[s] < 0 || sys->shell_l[s] > 5) FAIL("shells up to h (l <= 5, as numba/gto.py:107-118) are implemented");
    if (sys->nL > 0 && sys->shell_l[s] > 3) {
      if (h->twist) FAIL("twisted cells: shells up to f (l <= 3); g and h shells are implemented for open systems and untwisted cells");
      h->pbc_high_l = true;  // the general (thread-per-point) orbital path, pqa_orb_pbc.hip
    }
    h->shell_l.push_back(sys->shell_l[s]);
    h->lmax = std::max(h->lmax, sys->shell_l[s]);
    h->shell_np.push_back(sys->shell_prim_off[s + 1] - sys->shell_prim_off[s]);
    h->shell_ao.push_back(sys->shell_ao_off[s]);
  }
  TRY(upload_table(h, sys->shell_atom, (size_t)sys->nshell, &tmp_i)); S.shell_atom = tmp_i;
  TRY(upload_table(h, sys->shell_l, (size_t)sys->nshell, &tmp_i)); S.shell_l = tmp_i;
  TRY(upload_table(h, sys->shell_prim_off, (size_t)sys->nshell + 1, &tmp_i)); S.shell_prim_off = tmp_i;
  TRY(upload_table(h, sys->shell_ao_off, (size_t)sys->nshell, &tmp_i)); S.shell_ao_off = tmp_i;
  TRY(upload_table(h, sys->prim_exp, (size_t)sys->nprim, &tmp_d)); S.prim_exp = tmp_d;
  TRY(upload_table(h, sys->prim_coef, (size_t)sys->nprim, &tmp_d)); S.prim_coef = tmp_d;
  TRY(build_radial_tables(h, sys, S));
  S.nL = 0;
  if (S.pbc) {
    if (sys->nL <= 0 || !sys->Ls || !sys->num_Ls || !sys->atom_cut || !sys->shell_cut) FAIL("periodic orbitals need the lattice-sum tables (Ls, num_Ls, atom_cut, shell_cut)");
    std::vector<int> nl((size_t)h->natom);
    HIPCHK(hipMemcpy(nl.data(), sys->num_Ls, nl.size() * sizeof(int), hipMemcpyDefault));
    for (int v : nl)
      if (v < 1 || v > sys->nL) FAIL("num_Ls out of range");
    S.nL = sys->nL;
    TRY(upload_table(h, sys->Ls, (size_t)sys->nL * 3, &tmp_d)); P.Ls = tmp_d;
    TRY(upload_table(h, sys->num_Ls, (size_t)h->natom, &tmp_i)); P.num_Ls = tmp_i;
    TRY(upload_table(h, sys->atom_cut, (size_t)h->natom, &tmp_d)); P.atom_cut = tmp_d;
    TRY(upload_table(h, sys->shell_cut, (size_t)sys->nshell, &tmp_d)); P.shell_cut = tmp_d;
    {  // distinct shell cut-offs per atom, ascending: the classes k_pbc_prepass orders an atom's images by
      std::vector<double> sc((size_t)sys->nshell), cc((size_t)h->natom * PQA_MAXCLS, 0.0);
      std::vector<int> sa((size_t)sys->nshell), nc((size_t)h->natom, 0);
      HIPCHK(hipMemcpy(sc.data(), sys->shell_cut, sc.size() * sizeof(double), hipMemcpyDefault));
      HIPCHK(hipMemcpy(sa.data(), sys->shell_atom, sa.size() * sizeof(int), hipMemcpyDefault));
      for (int a = 0; a < h->natom; ++a) {
        std::vector<double> u;
        for (int q = 0; q < sys->nshell; ++q)
          if (sa[q] == a) u.push_back(sc[q]);
        std::sort(u.begin(), u.end());
        u.erase(std::unique(u.begin(), u.end()), u.end());
        if ((int)u.size() > PQA_MAXCLS) continue;  // nc = 0: this atom's images are tested directly
        nc[a] = (int)u.size();
        for (size_t q = 0; q < u.size(); ++q) cc[(size_t)a * PQA_MAXCLS + q] = u[q];
      }
      TRY(upload_table(h, cc.data(), cc.size(), &tmp_d)); P.cls_cut = tmp_d;
      TRY(upload_table(h, nc.data(), nc.size(), &tmp_i)); P.ncls = tmp_i;
      h->pbc_maxcls = *std::max_element(nc.begin(), nc.end());
      h->pbc_mincls = *std::min_element(nc.begin(), nc.end());
      if (const char* e = getenv("PQA_PRE_NCUT")) h->pbc_maxcls = std::max(h->pbc_maxcls, atoi(e));  // (tests: the ten-class instantiation)
    }
    {  // capacity of the per-(atom, point) image lists: the lattice points inside a sphere of the largest atom cut-off number
       // V_sphere / V_cell on average; 1.5 x that + 8 with room for a terminator (lanes beyond it test images directly)
      std::vector<double> ac((size_t)h->natom);
      HIPCHK(hipMemcpy(ac.data(), sys->atom_cut, ac.size() * sizeof(double), hipMemcpyDefault));
      const double* a = sys->lattice;
      const double vol = fabs(det3(a));
      const double r2 = *std::max_element(ac.begin(), ac.end());
      const double mean = 4.18879020478639 * r2 * std::sqrt(r2) / std::max(vol, 1e-12);
      const int cap = (int)std::min(127.0, std::ceil(1.5 * mean + 8.0));
      h->pbc_nw = cap / 4 + 1;
      if (const char* e = getenv("PQA_PBC_NW")) h->pbc_nw = std::max(1, std::min(32, atoi(e)));
      TRY(near_masks(h, sys, nl, ac, P));
    }
    P.twist = h->twist ? 1 : 0;
    if (h->twist) {
      std::vector<double> ls((size_t)sys->nL * 3), ph((size_t)sys->nL * 2);
      HIPCHK(hipMemcpy(ls.data(), sys->Ls, ls.size() * sizeof(double), hipMemcpyDefault));
      for (int j = 0; j < sys->nL; ++j) {
        const double a = sys->twist_k[0] * ls[3 * j] + sys->twist_k[1] * ls[3 * j + 1] + sys->twist_k[2] * ls[3 * j + 2];
        ph[2 * j] = std::cos(a); ph[2 * j + 1] = std::sin(a);
      }
      TRY(upload_table(h, ph.data(), ph.size(), &tmp_d)); P.img_phase = tmp_d;
      for (int a = 0; a < 3; ++a)
        P.ktl[a] = sys->twist_k[0] * sys->lattice[3 * a] + sys->twist_k[1] * sys->lattice[3 * a + 1] + sys->twist_k[2] * sys->lattice[3 * a + 2];
    }
    P.member = nullptr;
    if (sys->member) {
      if (!sys->img_n || !sys->atom_n || !sys->member_class || sys->member_M < 0 || sys->n_member_class < 1) FAIL("incomplete image-membership tables");
      const double* a = sys->lattice_prim;
      const double det = det3(a);
      if (!(fabs(det) > 1e-12)) FAIL("singular primitive lattice");
      inv3(a, det, P.lprim_inv);
      const size_t side = 2 * (size_t)sys->member_M + 1;
      unsigned char* tmp_b;
      TRY(upload_table(h, sys->member, (size_t)sys->n_member_class * side * side * side, &tmp_b)); P.member = tmp_b;
      TRY(upload_table(h, sys->member_class, (size_t)h->natom, &tmp_i)); P.member_class = tmp_i;
      TRY(upload_table(h, sys->img_n, (size_t)sys->nL * 3, &tmp_i)); P.img_n = tmp_i;
      TRY(upload_table(h, sys->atom_n, (size_t)h->natom * 3, &tmp_i)); P.atom_n = tmp_i;
      P.member_M = sys->member_M;
      TRY(member_masks(h, sys, P));
      for (int i = 0; i < 9; ++i) {  // supercell matrix = lattice . inv(lattice_prim), must be integer
        double v_ = 0.0;
        for (int k = 0; k < 3; ++k) v_ += sys->lattice[3 * (i / 3) + k] * P.lprim_inv[3 * k + (i % 3)];
        P.supercell[i] = (int)lround(v_);
        if (fabs(v_ - P.supercell[i]) > 1e-6) FAIL("lattice is not an integer multiple of lattice_prim");
      }
    }
  }
  return 0;
}

// determinants (occupations, column maps, coefficients), the shells' chunk tables and the padded orbital coefficients
static int create_determinants(pqa_handle* h, const pqa_system_t* sys) {
  SysDev& S = h->S;
  int* tmp_i;
  h->nmo[0] = sys->nmo_up; h->nmo[1] = sys->nmo_dn;
  h->ndet = sys->ndet; h->ndet_s[0] = sys->ndet_up; h->ndet_s[1] = sys->ndet_dn;
  S.ndet = h->ndet;
  const int* occ_src[2] = {sys->det_occ_up, sys->det_occ_dn};
  const double* mo_src[2] = {sys->mo_up, sys->mo_dn};
  const int nel[2] = {h->nup, h->ndn};
  shell_costs(h, sys);
  build_chunks(h, 16, h->chunks[0]);
  build_chunks(h, 32, h->chunks[1]);
  for (int s = 0; s < 2; ++s) {
    if (h->nmo[s] > (h->cplx ? 2 : 1) * PQA_MAXN) FAIL("more than 128 orbitals per spin are not supported");
    const int nt = (h->nmo[s] + 15) / 16;
    h->nt[s] = nt <= 1 ? 1 : (nt == 2 ? 2 : (nt <= 4 ? 4 : (nt <= 8 ? 8 : 16)));  // (8: padded coefficient rows of 128 columns, contracted in two windows of four tiles; periodic big handles through k_mo_rows)
    S.nmo[s] = h->nmo[s]; S.ndet_s[s] = h->ndet_s[s];
    TRY(upload_table(h, occ_src[s], (size_t)h->ndet_s[s] * nel[s], &tmp_i)); S.det_occ[s] = tmp_i;
    {
      std::vector<int> oc((size_t)std::max(nel[s], 1));
      if (nel[s] > 0) HIPCHK(hipMemcpy(oc.data(), occ_src[s], (size_t)nel[s] * sizeof(int), hipMemcpyDefault));
      S.occ_ident[s] = 1;
      for (int k = 0; k < nel[s]; ++k) S.occ_ident[s] &= (oc[k] == k) ? 1 : 0;
    }
    {
      std::vector<int> occ_h((size_t)h->ndet_s[s] * nel[s]), cm((size_t)h->ndet_s[s] * std::max(h->nmo[s], 1), -1);
      if (!occ_h.empty()) HIPCHK(hipMemcpy(occ_h.data(), occ_src[s], occ_h.size() * sizeof(int), hipMemcpyDefault));
      for (int u = 0; u < h->ndet_s[s]; ++u)
        for (int k = 0; k < nel[s]; ++k) {
          const int m = occ_h[(size_t)u * nel[s] + k];
          if (m < 0 || m >= h->nmo[s]) FAIL("determinant occupation outside the orbital range");
          cm[(size_t)u * h->nmo[s] + m] = k;
        }
      TRY(upload_table(h, cm.data(), cm.size(), &h->d_colmap[s]));
    }
    TRY(upload_table<double>(h, nullptr, (size_t)h->nao * std::max(h->nmo[s], 1), &h->d_mo[s])); S.mo[s] = h->d_mo[s];
    for (int t = 0; t < 2; ++t)
      TRY(upload_table<double>(h, nullptr, (size_t)(std::max(h->chunks[t].rows_pad, 1) + 32) * 16 * h->nt[s], &h->d_cpad[t][s]));
    if (h->nmo[s] > 0) TRY(set_mo(h, s, mo_src[s]));
  }
  TRY(upload_table(h, sys->det_coeff, (size_t)h->ndet, &h->d_detcoeff)); S.det_coeff = h->d_detcoeff;
  TRY(upload_table(h, sys->det_map, (size_t)2 * h->ndet, &tmp_i)); S.det_map = tmp_i;
  for (int t = 0; t < 2; ++t) {
    const ChunkHost& c = h->chunks[t];
    ChunkTab& T = h->tab[t];
    T.nchunk = (int)c.nk.size();
    TRY(upload_table(h, c.nk.data(), c.nk.size(), &tmp_i)); T.chunk_nk = tmp_i;
    TRY(upload_table(h, c.shell_kb.data(), c.shell_kb.size(), &tmp_i)); T.shell_kb = tmp_i;
    TRY(upload_table(h, c.row0.data(), c.row0.size(), &tmp_i)); T.chunk_row0 = tmp_i;
    for (int g = 0; g < 3; ++g) {
      TRY(upload_table(h, c.cw_off[g].data(), c.cw_off[g].size(), &tmp_i)); T.cw_off[g] = tmp_i;
      TRY(upload_table(h, c.cw_shell[g].data(), c.cw_shell[g].size(), &tmp_i)); T.cw_shell[g] = tmp_i;
    }
    for (int s = 0; s < 2; ++s) { T.cpad[s] = h->d_cpad[t][s]; T.ldc[s] = 16 * h->nt[s]; }
    // k_orb_wide: all shells dealt to 64 lane groups (longest processing time first), tile row of a shell = its padded row
    const int tw = h->twist ? 2 : 1;
    const int ngrp = h->twist ? 32 : 64;  // lane groups of k_orb_wide (16 points per block, launch_orb_pbc: 512 / 1024 threads)
    std::vector<int> order((size_t)h->nshell), wrow((size_t)tw * h->nshell), woff(65, 0), wsh;
    auto cost = [&](int s) { return h->shell_cost[s]; };
    for (int s = 0; s < h->nshell; ++s) order[s] = s;
    std::stable_sort(order.begin(), order.end(), [&](int a, int b) { return cost(a) > cost(b); });
    std::vector<std::vector<int>> grp(64);
    std::vector<int> load(64, 0);
    for (int s : order) {
      int best = 0;
      for (int g = 1; g < ngrp; ++g)
        if (load[g] < load[best]) best = g;
      grp[best].push_back(s);
      load[best] += cost(s);
    }
    for (int g = 0; g < 64; ++g) {
      // shells of one atom next to each other: a thread re-reads the per-(point, atom) fold / mask only when the atom changes
      std::stable_sort(grp[g].begin(), grp[g].end(), [&](int a, int b) { return sys->shell_atom[a] < sys->shell_atom[b]; });
      for (int s : grp[g]) wsh.push_back(s);
      woff[g + 1] = (int)wsh.size();
    }
    for (int s = 0; s < tw * h->nshell; ++s) wrow[s] = c.row0[c.shell_chunk[s]] + c.shell_kb[s];
    TRY(upload_table(h, woff.data(), woff.size(), &tmp_i)); h->wide[t].off = tmp_i;
    TRY(upload_table(h, wsh.data(), wsh.size(), &tmp_i)); h->wide[t].shell = tmp_i;
    TRY(upload_table(h, wrow.data(), wrow.size(), &tmp_i)); h->wide[t].row = tmp_i;
    h->wide[t].rows_pad = c.rows_pad;
  }
  return 0;
}

// two- and three-body Jastrow: basis parameters, coefficient tables, the merged Pade numerators, the three-body LDS offset
static int create_jastrow(pqa_handle* h, const pqa_system_t* sys) {
  SysDev& S = h->S;
  S.na = h->na; S.nb = h->nb; S.rcut_a = sys->rcut_a; S.rcut_b = sys->rcut_b;
  for (int k = 0; k < h->na; ++k) { S.a_kind[k] = sys->a_kind[k]; S.a_param[k] = sys->a_param[k]; S.a_aux[k] = 1.0 / (3.0 + sys->a_param[k]); }
  for (int k = 0; k < h->nb; ++k) { S.b_kind[k] = sys->b_kind[k]; S.b_param[k] = sys->b_param[k]; S.b_aux[k] = 1.0 / (3.0 + sys->b_param[k]); }
  TRY(upload_table(h, sys->acoeff, (size_t)h->natom * h->na * 2, &h->d_acoeff)); S.acoeff = h->d_acoeff;
  TRY(upload_table(h, sys->bcoeff, (size_t)h->nb * 3, &h->d_bcoeff)); S.bcoeff = h->d_bcoeff;
  TRY(jas_merge_tables(h));
  S.na3 = h->na3; S.nb3 = h->nb3; S.rcut_a3 = sys->rcut_a3; S.rcut_b3 = sys->rcut_b3;
  for (int k = 0; k < h->na3; ++k) { S.a3_kind[k] = sys->a3_kind[k]; S.a3_param[k] = sys->a3_param[k]; S.a3_aux[k] = 1.0 / (3.0 + sys->a3_param[k]); }
  for (int k = 0; k < h->nb3; ++k) { S.b3_kind[k] = sys->b3_kind[k]; S.b3_param[k] = sys->b3_param[k]; S.b3_aux[k] = 1.0 / (3.0 + sys->b3_param[k]); }
  TRY(upload_table<double>(h, nullptr, (size_t)h->natom * h->na3 * h->na3 * h->nb3 * 3, &h->d_c3)); S.c3 = h->d_c3;
  if (h->has_j3 && sys->ccoeff) TRY(set_c3(h, sys->ccoeff));
  {  // the three-body scratch sits behind whatever else a kernel keeps in dynamic LDS
    const size_t n = std::max(sys->nelec_up, sys->nelec_dn);
    const size_t other = std::max((n > PQA_MAXN_FAST ? 3 * n + 64 : n * (n + 1) + 3 * n + 64) * sizeof(double),
                                  (size_t)std::max(sys->has_slater ? std::max(sys->ndet_up, sys->ndet_dn) : 1, 1) * 5 * sizeof(double));
    S.j3_off = (int)((other + 7) / 8);
  }
  return 0;
}

// ECP terms and ranges, the quadrature rules and the T-move candidate list
static int create_ecp(pqa_handle* h, const pqa_system_t* sys) {
  SysDev& S = h->S;
  double* tmp_d; int* tmp_i;
  S.necp = h->necp;
  if (h->necp > 0) {
    const int nchan = sys->ecp_chan_off[h->necp];
    const int nterm = sys->ecp_term_off[nchan];
    h->ecp_nchan = nchan; h->ecp_nterm = nterm;
    for (int k = 0; k < h->necp; ++k)
      if (sys->ecp_chan_off[k + 1] - sys->ecp_chan_off[k] > PQA_MAXCHAN) FAIL("ECP with more than 5 non-local channels (the reference's Legendre functions end at l = 4, eval_ecp.py:203-225)");
    TRY(upload_table(h, sys->ecp_atom, (size_t)h->necp, &tmp_i)); S.ecp_atom = tmp_i;
    TRY(upload_table(h, sys->ecp_chan_off, (size_t)h->necp + 1, &tmp_i)); S.ecp_chan_off = tmp_i;
    TRY(upload_table(h, sys->ecp_term_off, (size_t)nchan + 1, &tmp_i)); S.ecp_term_off = tmp_i;
    TRY(upload_table(h, sys->ecp_term_n, (size_t)nterm, &tmp_i)); S.ecp_term_n = tmp_i;
    TRY(upload_table(h, sys->ecp_term_exp, (size_t)nterm, &tmp_d)); S.ecp_term_exp = tmp_d;
    TRY(upload_table(h, sys->ecp_term_coef, (size_t)nterm, &tmp_d)); S.ecp_term_coef = tmp_d;
    {  // range of every ECP atom: r^2 beyond which all of its terms |c| r^n exp(-a r^2) stay below 1e-22 (k_ecp_count visits an
       // electron's near atoms only; what it leaves out is below the last bit of the local energy and can never pass the mask)
      std::vector<int> co((size_t)h->necp + 1), to((size_t)nchan + 1), tn((size_t)std::max(nterm, 1));
      std::vector<double> te(tn.size()), tc(tn.size()), rc2((size_t)std::max(h->necp, 1), 0.0);
      HIPCHK(hipMemcpy(co.data(), sys->ecp_chan_off, co.size() * sizeof(int), hipMemcpyDefault));
      HIPCHK(hipMemcpy(to.data(), sys->ecp_term_off, to.size() * sizeof(int), hipMemcpyDefault));
      if (nterm > 0) {
        HIPCHK(hipMemcpy(tn.data(), sys->ecp_term_n, (size_t)nterm * sizeof(int), hipMemcpyDefault));
        HIPCHK(hipMemcpy(te.data(), sys->ecp_term_exp, (size_t)nterm * sizeof(double), hipMemcpyDefault));
        HIPCHK(hipMemcpy(tc.data(), sys->ecp_term_coef, (size_t)nterm * sizeof(double), hipMemcpyDefault));
      }
      for (int k = 0; k < h->necp; ++k) {
        double rc = 0.0;
        for (int t = to[co[k]]; t < to[co[k + 1]]; ++t) {
          if (tc[t] == 0.0) continue;
          if (!(te[t] > 0.0)) { rc = 1e150; break; }  // no decay: never out of range
          double r = 60.0;  // walk inwards until the term is visible
          while (r > 0.02 && fabs(tc[t]) * std::pow(r, (double)tn[t]) * std::exp(-te[t] * r * r) < 1e-22) r -= 0.01;
          rc = std::max(rc, r + 0.02);
        }
        rc2[k] = rc * rc;
      }
      TRY(upload_table(h, rc2.data(), rc2.size(), &tmp_d)); S.ecp_rc2 = tmp_d;
    }
  }
  // quadrature grids (eval_ecp.py:278-336): all six rules of Mitas, Shirley & Ceperley in one table — rows 0-5 OA (6), 6-17 IAB (12),
  // 18-35 OAB (18), 36-61 OABC (26), 62-93 IABC (32), 94-143 OABCD (50) — in the reference's point order, with their weights
  {
    std::vector<double> quad, quadw;
    ecp_quadrature_tables(quad, quadw);
    TRY(upload_table(h, quad.data(), quad.size(), &h->d_quad));
    TRY(upload_table(h, quadw.data(), quadw.size(), &h->d_quadw));
    std::vector<int> na((size_t)std::max(h->necp, 1), 0), qo((size_t)std::max(h->necp, 1), 0);
    h->ecp_nch.assign((size_t)h->necp, 0);
    for (int k = 0; k < h->necp; ++k) {
      h->ecp_nch[k] = sys->ecp_chan_off[k + 1] - sys->ecp_chan_off[k];
      na[k] = h->ecp_nch[k] <= 2 ? 6 : 12;  // eval_ecp.py:239-240
      qo[k] = ecp_quadrature_offset(na[k]);
    }
    TRY(upload_table(h, na.data(), na.size(), &h->d_ecp_naip));
    TRY(upload_table(h, qo.data(), qo.size(), &h->d_ecp_qoff));
    S.ecp_naip = h->d_ecp_naip; S.ecp_qoff = h->d_ecp_qoff;
    S.ecp_naip_max = 0;
    for (int k = 0; k < h->necp; ++k) S.ecp_naip_max = std::max(S.ecp_naip_max, na[k]);
  }
  {  // flat (atom, quadrature index) list of the T-move candidates of one electron
    std::vector<int> ptk, pti;
    for (int k = 0; k < h->necp; ++k) {
      const int nch = sys->ecp_chan_off[k + 1] - sys->ecp_chan_off[k];
      const int naip = nch <= 2 ? 6 : 12;
      for (int i = 0; i < naip; ++i) { ptk.push_back(k); pti.push_back(i); }
    }
    h->dmc.tm_P = (int)ptk.size();
    TRY(upload_table(h, ptk.data(), ptk.size(), &h->dmc.d_ptk));
    TRY(upload_table(h, pti.data(), pti.size(), &h->dmc.d_pti));
  }
  return 0;
}

static int create_impl(pqa_handle* h, const pqa_system_t* sys) {
  HIPCHK(hipSetDevice(h->device));
  TRY(new_stream(h, &h->stream));
  TRY(new_event(h, &h->ev0));
  TRY(new_event(h, &h->ev1));
  PbcDev P{};
  TRY(create_switches(h, sys));
  TRY(create_lattice(h, sys, P));
  if (h->has_slater) {
    TRY(create_orbital_tables(h, sys, P));
    TRY(create_determinants(h, sys));
  }
  if (h->S.pbc) {  // all periodic tables sit behind one pointer (see SysDev)
    // (the resident sweep's in-block image lists need the mask tables, at most 128 candidates and a handful of shell cut-offs per atom)
    h->pbc_lists_ok = sys->nL > 0 && sys->nL <= 128 && (P.member == nullptr || P.memb_mask != nullptr) && h->pbc_mincls >= 1 && h->pbc_maxcls <= PQA_RES_NCUT;
    PbcDev* dp;
    TRY(upload_table(h, &P, (size_t)1, &dp));
    h->S.pb = dp;
  }
  TRY(create_jastrow(h, sys));
  return create_ecp(h, sys);
}

extern "C" int pqa_create(const pqa_system_t* sys, int device, pqa_handle_t** out) {
  *out = nullptr;
  pqa_handle* h = new pqa_handle();
  h->device = device;
  int rc = create_impl(h, sys);
  if (rc) {
    g_create_error = h->err;
    pqa_destroy(h);
    return rc;
  }
  *out = h;
  return 0;
}

// Frees what the handle recorded (pqa_internal.hpp: ensure, upload_table, new_pinned, new_stream, new_event), also for a handle
// whose create_impl failed half-way: device memory and pinned words once the main stream is idle, every auxiliary stream after
// its own work is done, the events, the main stream last.
extern "C" void pqa_destroy(pqa_handle_t* h) {
  if (!h) return;
  (void)hipSetDevice(h->device);
  if (h->stream) (void)hipStreamSynchronize(h->stream);
  for (void* p : h->owned) (void)hipFree(p);
  for (DevBuf* b : h->bufs) {  // (a buffer whose regrowth failed may be recorded twice: freed once)
    if (b->p) (void)hipFree(b->p);
    b->p = nullptr;
  }
  for (void* p : h->pinned) (void)hipHostFree(p);
  for (size_t k = h->streams.size(); k-- > 1;) {
    (void)hipStreamSynchronize(h->streams[k]);
    (void)hipStreamDestroy(h->streams[k]);
  }
  for (hipEvent_t e : h->events) (void)hipEventDestroy(e);
  if (!h->streams.empty()) (void)hipStreamDestroy(h->streams[0]);
  delete h;
}

// ---------------------------------------------------------------- merged Pade numerators
// Tables for pade_merged (pqa_jastrow.hpp): with D_k = 1 + beta_k p over the PolyPade functions k of a basis and a coefficient set c,
//   N1 = sum_k c_k prod_{j != k} D_j,  N2 = sum_k c_k (1 + beta_k) prod_{j != k} D_j^2,  N3 = sum_k c_k beta_k (1 + beta_k) prod_{j != k} D_j^3
// as ascending coefficients at offsets 0 / 4 / 11 of a PQA_JQ-double record, one record per (atom, spin of the electron) and per
// electron-electron spin channel; D = prod_k D_k in S.a_D / S.b_D.  Products in long double, rounded once.  Called at create and
// after every change of acoeff / bcoeff.  Route available (S.jq_on) when every non-empty basis is [cusp]? + 1..4 Pade functions.
typedef std::vector<long double> Poly;
static Poly poly_mul(const Poly& a, const Poly& b) {
  Poly c(a.size() + b.size() - 1, 0.0L);
  for (size_t i = 0; i < a.size(); ++i)
    for (size_t j = 0; j < b.size(); ++j) c[i + j] += a[i] * b[j];
  return c;
}
static void jas_merge_record(const std::vector<double>& beta, const double* c, size_t cstride, double* rec) {
  const int K = (int)beta.size();
  Poly n1(1, 0.0L), n2(1, 0.0L), n3(1, 0.0L);
  auto add = [](Poly& acc, const Poly& t, long double f) {
    if (acc.size() < t.size()) acc.resize(t.size(), 0.0L);
    for (size_t i = 0; i < t.size(); ++i) acc[i] += f * t[i];
  };
  for (int k = 0; k < K; ++k) {
    Poly o(1, 1.0L);
    for (int j = 0; j < K; ++j)
      if (j != k) o = poly_mul(o, Poly{1.0L, (long double)beta[j]});
    const Poly o2 = poly_mul(o, o), o3 = poly_mul(o2, o);
    const long double ck = c[(size_t)k * cstride], bk = beta[k];
    add(n1, o, ck); add(n2, o2, ck * (1.0L + bk)); add(n3, o3, ck * bk * (1.0L + bk));
  }
  for (int i = 0; i < PQA_JQ; ++i) rec[i] = 0.0;
  for (size_t i = 0; i < n1.size() && i < 4; ++i) rec[i] = (double)n1[i];
  for (size_t i = 0; i < n2.size() && i < 7; ++i) rec[4 + i] = (double)n2[i];
  for (size_t i = 0; i < n3.size() && i < 10; ++i) rec[11 + i] = (double)n3[i];
}
int jas_merge_tables(pqa_handle* h) {
  SysDev& S = h->S;
  S.jq_on = S.jq_a = S.jq_b = 0;
  if (!h->jas_merge || !h->has_j2 || (h->na == 0 && h->nb == 0)) return 0;
  auto pades = [](int n, const int* kind, const double* par, std::vector<double>& beta, int& first) {
    first = (n > 0 && kind[0] == 1) ? 1 : 0;
    beta.clear();
    for (int k = first; k < n; ++k) {
      if (kind[k] != 0 || !(par[k] > -1.0)) return false;
      beta.push_back(par[k]);
    }
    return n == 0 || (beta.size() >= 1 && beta.size() <= 4);
  };
  std::vector<double> ba, bb;
  int fa = 0, fb = 0;
  if (!pades(h->na, S.a_kind, S.a_param, ba, fa) || !pades(h->nb, S.b_kind, S.b_param, bb, fb)) return 0;
  auto denom = [](const std::vector<double>& beta, double* D) {
    Poly d(1, 1.0L);
    for (double b : beta) d = poly_mul(d, Poly{1.0L, (long double)b});
    for (int i = 0; i < 5; ++i) D[i] = i < (int)d.size() ? (double)d[i] : 0.0;
  };
  denom(ba, S.a_D); denom(bb, S.b_D);
  std::vector<double> ac((size_t)h->natom * h->na * 2 + 1), bc((size_t)h->nb * 3 + 1);
  HIPCHK(hipMemcpy(ac.data(), h->d_acoeff, (size_t)h->natom * h->na * 2 * sizeof(double), hipMemcpyDeviceToHost));
  HIPCHK(hipMemcpy(bc.data(), h->d_bcoeff, (size_t)h->nb * 3 * sizeof(double), hipMemcpyDeviceToHost));
  std::vector<double> aq((size_t)h->natom * 2 * PQA_JQ + PQA_JQ, 0.0), bq((size_t)3 * PQA_JQ, 0.0);
  if (h->na > 0)
    for (int I = 0; I < h->natom; ++I)
      for (int sp = 0; sp < 2; ++sp) jas_merge_record(ba, ac.data() + ((size_t)I * h->na + fa) * 2 + sp, 2, aq.data() + ((size_t)I * 2 + sp) * PQA_JQ);
  if (h->nb > 0)
    for (int ch = 0; ch < 3; ++ch) jas_merge_record(bb, bc.data() + (size_t)fb * 3 + ch, 3, bq.data() + (size_t)ch * PQA_JQ);
  if (!h->d_aq) {
    TRY(upload_table<double>(h, nullptr, aq.size(), &h->d_aq));
    TRY(upload_table<double>(h, nullptr, bq.size(), &h->d_bq));
  }
  HIPCHK(hipMemcpy(h->d_aq, aq.data(), aq.size() * sizeof(double), hipMemcpyHostToDevice));
  HIPCHK(hipMemcpy(h->d_bq, bq.data(), bq.size() * sizeof(double), hipMemcpyHostToDevice));
  S.aq = h->d_aq; S.bq = h->d_bq;
  S.jq_a = (int)ba.size(); S.jq_b = (int)bb.size(); S.jq_on = 1;
  return 0;
}
