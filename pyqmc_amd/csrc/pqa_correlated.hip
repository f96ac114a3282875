// Correlated evaluation of K Jastrow parameter sets on the resident walkers (correlated_compute_worker, pyqmc/method/linemin.py:378-409).
//
// The reference sets each parameter set, recomputes the whole wave function and runs the energy accumulator, with the random state
// reset before every set.  Only the two-body Jastrow coefficients differ between the sets here, and U is linear in them:
// U = sum_p c_p B_p(R), and so are grad_e U, lap_e U and the ECP exponent U(e -> q) - U(e).  The call therefore splits into
//   once per call   the Slater-only energy pass (energy_dev with the Jastrow switched off): Coulomb / Ewald, the local ECP channel and
//                   the ECP point lists with their Slater-weighted values s_q = (D(e -> q) / D) w_q (b_econ), the same draws for all
//                   sets; the log values from the basis sums the handle keeps (k_corr_u);
//   per walker      k_corr_energy: per electron grad D / D and lap D / D (from the orbital-row cache), the basis-resolved Jastrow rows
//                   (grad_e B_p, lap_e B_p) in LDS, and for every ECP point the row B_p(q) - B_p(r_e) (jas_rows / jas_diff_rows,
//                   pqa_estim.hpp); each row is contracted with the (P x K) coefficient matrix, one set per lane, and combined per set:
//                   ke_k = -1/2 sum_e [lap D/D + 2 grad D/D . grad U_k + lap U_k + |grad U_k|^2],  grad2_k = sum_e |grad D/D + grad U_k|^2,
//                   ecp_k = local + sum_q s_q exp(dU_k(q)),  total_k = ke_k + ee + ei + ecp_k + ii.
// The handle's coefficients are never changed.  Outputs are written per walker chunk of at most 256 MiB.
#include "pqa_estim.hpp"

namespace {

// U[k][w] = sum_i bvalues[w][i] c_b[k][i] + sum_i avalues[w][i] c_a[k][i] for k < K1: one wave per walker, the summation order of
// jas_value_wave (k_jastrow_value), so the row of the handle's own coefficients reproduces its Jastrow value bit for bit.
__global__ __launch_bounds__(64) void k_corr_u(const double* __restrict__ aval, const double* __restrict__ bval,
                                               const double* __restrict__ ca /*[K1][Pa]*/, const double* __restrict__ cb /*[K1][Pb]*/,
                                               int Pa, int Pb, int K1, long W, double* __restrict__ U /*[K1][W]*/) {
  const long w = blockIdx.x;
  const int lane = threadIdx.x;
  const double* bv = bval + (size_t)w * Pb;
  const double* av = aval + (size_t)w * Pa;
  for (int k = 0; k < K1; ++k) {
    double u = 0.0;
    for (int i = lane; i < Pb; i += 64) u += bv[i] * cb[(size_t)k * Pb + i];
    for (int i = lane; i < Pa; i += 64) u += av[i] * ca[(size_t)k * Pa + i];
    u = wave_sum(u);
    if (lane == 0) U[(size_t)k * W + w] = u;
  }
}

struct CorrArgs {
  long w0, Wc, W;           // first walker of the chunk, walkers in it, resident walkers
  int K, P, Pa;             // sets, coefficients per set (acoeff then bcoeff), of which acoeff
  const double* ct;         // [P][K] coefficient matrix
  const double* kc;         // [4][W] rows ke, ee, ei, grad2 of the Slater-only pass (ee, ei used)
  const double* local;      // [W] local ECP channel
  const double* econ[2];    // per spin: Slater-weighted point values
  const double* pts[2];     // per spin: point positions [n][3]
  const int* pte[2];        // per spin: electron of the point
  const long* off;          // [2][nseg W + 1] list offsets (k_ecp_sum's order)
  int nseg, has_ecp;
  double ii;
  double* out;              // [K][6][Wc]
};

// One wave per walker (grid.x), lanes = parameter sets kb + lane (grid.y: chunks of 64 sets).  LDS: rows R[4][P] (ke_electron).
template <bool PBC>
__global__ __launch_bounds__(64) void k_corr_energy(SysDev S, SlaterState st, JastrowState js, CorrArgs A) {
  extern __shared__ double R[];
  const int lane = threadIdx.x;
  const long bw = blockIdx.x, w = A.w0 + bw;
  const int k = blockIdx.y * 64 + lane;
  const bool act = k < A.K;
  const int P = A.P, Pa = A.Pa, N = S.nelec;
  const double* xw = js.x + (size_t)w * N * 3;
  const double irb = 1.0 / S.rcut_b, ira = 1.0 / S.rcut_a;
  double ke = 0.0, g2 = 0.0;
  for (int e = 0; e < N; ++e)
    ke_electron<PBC>(S, st, xw, w, e, P, Pa, ira, irb, R, A.ct, A.K, k, act, [&](double lap, double tx, double ty, double tz) {
      ke += -0.5 * lap;
      g2 += tx * tx + ty * ty + tz * tz;
    });
  // ECP: every point of the walker in k_ecp_sum's order (spin up then down, segment by segment); row B_p(q) - B_p(r_e)
  double tot = 0.0;
  if (A.has_ecp) {
    const size_t SS = (size_t)A.nseg * A.W + 1;
    for (int sp = 0; sp < 2; ++sp)
      for (int seg = 0; seg < A.nseg; ++seg) {
        const long* o = A.off + sp * SS + (size_t)seg * A.W + w;
        for (long pt = o[0]; pt < o[1]; ++pt) {
          const int e = A.pte[sp][pt], s = e >= S.nup;
          const double qx = A.pts[sp][3 * pt], qy = A.pts[sp][3 * pt + 1], qz = A.pts[sp][3 * pt + 2];
          jas_diff_rows<PBC>(S, xw, e, s, qx, qy, qz, P, Pa, ira, irb, R);
          if (act) {
            double du = 0.0;
            for (int q = 0; q < S.natom * S.na; ++q) { const int p = 2 * q + s; du += A.ct[(size_t)p * A.K + k] * R[p]; }
            for (int q = 0; q < 2 * S.nb; ++q) { const int p = Pa + (q >> 1) * 3 + s + (q & 1); du += A.ct[(size_t)p * A.K + k] * R[p]; }
            tot += A.econ[sp][pt] * exp(du);
          }
          __syncthreads();
        }
      }
  }
  if (!act) return;
  const double ee = A.kc[A.W + w], ei = A.kc[2 * A.W + w], ec = A.has_ecp ? A.local[w] + tot : 0.0;
  double* o = A.out + (size_t)k * 6 * A.Wc + bw;
  o[0] = ke; o[A.Wc] = ee; o[2 * A.Wc] = ei; o[3 * A.Wc] = ec; o[4 * A.Wc] = g2; o[5 * A.Wc] = ke + ee + ei + ec + A.ii;
}

}  // namespace

extern "C" int pqa_correlated(pqa_handle_t* h, int K, const double* acoeff, const double* bcoeff, double threshold, const double* rot,
                              const double* unif, uint64_t seed, double* logpsi, double* en) {
  HIPCHK(hipSetDevice(h->device));
  if (h->W == 0) FAIL("state not initialised (call pqa_wf_recompute)");
  if (K < 1) FAIL("pqa_correlated: K must be at least 1");
  if (!acoeff || !bcoeff || !logpsi || !en) FAIL("pqa_correlated: acoeff, bcoeff, logpsi and en must not be NULL");
  TRY(linear_jastrow_scope(h, "pqa_correlated"));
  if (h->ecpb_on || h->ecp_wave) FAIL("pqa_correlated: needs the semi-local ECP integrator's thread-per-point pass (evaluate per set)");
  const long W = h->W;
  const int Pa = h->natom * h->na * 2, Pb = h->nb * 3, P = Pa + Pb, K1 = K + 1;
  // log|Psi| at the handle's own coefficients (as pqa_wf_value: refreshes the basis sums a fused sweep left stale)
  std::vector<double> lg0((size_t)W);
  TRY(pqa_wf_value(h, nullptr, lg0.data()));
  std::vector<double> ca((size_t)K1 * Pa), cb((size_t)K1 * Pb);
  HIPCHK(hipStreamSynchronize(h->stream));
  if (Pa) HIPCHK(hipMemcpy(ca.data(), acoeff, (size_t)K * Pa * sizeof(double), hipMemcpyDefault));
  if (Pb) HIPCHK(hipMemcpy(cb.data(), bcoeff, (size_t)K * Pb * sizeof(double), hipMemcpyDefault));
  if (Pa) HIPCHK(hipMemcpy(ca.data() + (size_t)K * Pa, h->d_acoeff, Pa * sizeof(double), hipMemcpyDeviceToHost));
  if (Pb) HIPCHK(hipMemcpy(cb.data() + (size_t)K * Pb, h->d_bcoeff, Pb * sizeof(double), hipMemcpyDeviceToHost));
  const std::vector<double> ct = pack_coef_sets(ca.data(), cb.data(), K, Pa, Pb);
  // the Slater-only energy pass, once: the Jastrow switched off and the ECP totals read on the host (restored on every exit)
  struct Flags {
    pqa_handle* h; bool has_jastrow, has_j2; int defer;
    ~Flags() { h->has_jastrow = has_jastrow; h->has_j2 = has_j2; h->ecp_defer = defer; }
  } flags{h, h->has_jastrow, h->has_j2, h->ecp_defer};
  TRY(sync_aos(h));
  h->saved_valid = false;  // (as pqa_energy: the saved orbital rows of a gradient_value call are overwritten)
  h->has_jastrow = false; h->has_j2 = false; h->ecp_defer = 0;
  TRY(energy_dev(h, threshold, rot, unif, seed, 0u));
  h->has_jastrow = flags.has_jastrow; h->has_j2 = flags.has_j2; h->ecp_defer = flags.defer;
  const bool has_ecp = h->necp > 0;
  if (has_ecp && (h->ecp_last_tot[0] < 0 || h->ecp_last_tot[1] < 0)) FAIL("pqa_correlated: ECP point totals were left on the device");
  // device scratch (b_out is sized by every user on entry): coefficient rows for k_corr_u, U, the [P][K] matrix, a chunk of outputs
  const size_t nca = (size_t)K1 * std::max(Pa, 1), ncb = (size_t)K1 * std::max(Pb, 1), nu = (size_t)K1 * W, nct = (size_t)P * K;
  const long Wc = walker_chunk(W, (size_t)K * 6 * sizeof(double));
  TRY(ensure(h, h->b_out, (nca + ncb + nu + nct + (size_t)K * 6 * Wc) * sizeof(double)));
  double* d_ca = (double*)h->b_out.p;
  double* d_cb = d_ca + nca;
  double* d_u = d_cb + ncb;
  double* d_ct = d_u + nu;
  double* d_o = d_ct + nct;
  if (Pa) TRY(copy_in(h, d_ca, ca.data(), (size_t)K1 * Pa * sizeof(double)));
  if (Pb) TRY(copy_in(h, d_cb, cb.data(), (size_t)K1 * Pb * sizeof(double)));
  TRY(copy_in(h, d_ct, ct.data(), nct * sizeof(double)));
  hipLaunchKernelGGL(k_corr_u, dim3((unsigned)W), dim3(64), 0, h->stream, (const double*)h->js.avalues, (const double*)h->js.bvalues,
                     (const double*)d_ca, (const double*)d_cb, Pa, Pb, K1, W, d_u);
  TRY(check_launch(h, "k_corr_u"));
  CorrArgs A{};
  A.W = W; A.K = K; A.P = P; A.Pa = Pa; A.ct = d_ct; A.kc = (const double*)h->b_kc.p; A.ii = h->ii_energy; A.out = d_o;
  A.has_ecp = has_ecp;
  if (has_ecp) {
    A.local = (const double*)h->b_elocal.p; A.off = (const long*)h->b_eoff.p; A.nseg = h->ecp_last_nseg;
    for (int s = 0; s < 2; ++s) {
      A.econ[s] = (const double*)h->b_econ[s].p; A.pts[s] = (const double*)h->b_epts[s].p; A.pte[s] = (const int*)h->b_epte[s].p;
    }
  }
  const size_t lds = (size_t)4 * P * sizeof(double);
  for (long w0 = 0; w0 < W; w0 += Wc) {
    A.w0 = w0; A.Wc = std::min(Wc, W - w0);
    const dim3 g((unsigned)A.Wc, (unsigned)((K + 63) / 64));
    if (h->S.pbc) hipLaunchKernelGGL(k_corr_energy<true>, g, dim3(64), lds, h->stream, h->S, h->st, h->js, A);
    else hipLaunchKernelGGL(k_corr_energy<false>, g, dim3(64), lds, h->stream, h->S, h->st, h->js, A);
    TRY(check_launch(h, "k_corr_energy"));
    // [K][6][Wc] -> en [K][6][W] columns w0 ..
    HIPCHK(hipMemcpy2DAsync(en + w0, (size_t)W * sizeof(double), d_o, (size_t)A.Wc * sizeof(double), (size_t)A.Wc * sizeof(double),
                            (size_t)K * 6, hipMemcpyDefault, h->stream));
  }
  std::vector<double> u((size_t)K1 * W);
  TRY(copy_out(h, u.data(), d_u, u.size() * sizeof(double)));
  std::vector<double> lp((size_t)K * W);
  for (int k = 0; k < K; ++k)
    for (long w = 0; w < W; ++w) lp[(size_t)k * W + w] = lg0[w] - u[(size_t)K * W + w] + u[(size_t)k * W + w];
  HIPCHK(hipMemcpy(logpsi, lp.data(), lp.size() * sizeof(double), hipMemcpyDefault));
  return 0;
}
