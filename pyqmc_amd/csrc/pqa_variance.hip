// Variance of the local energy at K sets of two-body Jastrow coefficients on the resident walkers, with its exact gradient
// (variance_cost_function, pyqmc/method/optvariance.py:47-56).
//
// The reference keeps Enref total - Enref ke of one evaluation fixed (eoff, ECP included) and recomputes only the kinetic energy.  U is
// linear in the coefficients, U = sum_p c_p B_p(R), so with t_e = grad D / D + grad_e U_k
//   ke_k          = -1/2 sum_e [lap D/D + 2 grad D/D . grad_e U_k + lap_e U_k + |grad_e U_k|^2]   (k_corr_energy's contraction),
//   d ke_k / dc_p = -1/2 sum_e [lap_e B_p + 2 t_e . grad_e B_p],
//   var_k = 1/W sum_w (E_w - Ebar)^2,  dvar_k = 2/W sum_w (E_w - Ebar) d ke_k[w] / dc,  E_w = eoff_w + ke_k[w].
// k_var_ke runs one wave per walker over the electrons with k_corr_energy's per-electron terms (ke_electron, pqa_estim.hpp: grad D / D
// and lap D / D from the orbital-row cache, the Jastrow rows; no Coulomb, no ECP), so both kernels form the same ke bits.  Without
// the gradient the lanes are sets, as in k_corr_energy.  With it a block is one set: every lane forms that set's contraction and
// owns the coefficients p = lane + 64 j, accumulated over the electrons in registers.  The per-walker derivatives are written per
// walker chunk of at most 256 MiB; each chunk is reduced about its own mean m_c (A_c = sum_w d_w, B_c = sum_w (E_w - m_c) d_w) and
// the chunks are combined as sum_c B_c + (m_c - Ebar) A_c, so no two large sums are subtracted (E_w ~ -100 Ha, var ~ 1 Ha^2).
// Every walker reduction is a fixed-order tree (block_sum256): no atomics, and two calls give the same bits.  The handle is only read.
#include "pqa_estim.hpp"

namespace {

constexpr int kVarWB = 256;  // walkers per partial sum of k_var_dpart

struct VarArgs {
  long w0, Wc, W;     // first walker of the chunk, walkers in it, resident walkers
  int K, P, Pa;       // sets, coefficients per set (acoeff then bcoeff), of which acoeff
  const double* ct;   // [P][K] coefficient matrix
  double* ke;         // [K][W]
  double* dke;        // [K][Wc][P] (NS > 0)
};

// NS = 0: one wave per walker (grid.x), lanes = sets kb + lane (grid.y: chunks of 64 sets).  NS > 0: grid.y = set, and each lane
// keeps d ke / dc_p of p = lane + 64 j, j < NS (P <= 64 NS).  LDS: rows R[4][P].
template <bool PBC, int NS>
__global__ __launch_bounds__(64) void k_var_ke(SysDev S, SlaterState st, JastrowState js, VarArgs A) {
  constexpr int NR = NS > 0 ? NS : 1;
  extern __shared__ double R[];
  const int lane = threadIdx.x;
  const long bw = blockIdx.x, w = A.w0 + bw;
  const int k = NS ? (int)blockIdx.y : (int)blockIdx.y * 64 + lane;
  const bool act = k < A.K;
  const int P = A.P, Pa = A.Pa, N = S.nelec;
  const double* xw = js.x + (size_t)w * N * 3;
  const double irb = 1.0 / S.rcut_b, ira = 1.0 / S.rcut_a;
  double ke = 0.0;
  double dk[NR];
#pragma unroll
  for (int j = 0; j < NR; ++j) dk[j] = 0.0;
  for (int e = 0; e < N; ++e)
    ke_electron<PBC>(S, st, xw, w, e, P, Pa, ira, irb, R, A.ct, A.K, k, act, [&](double lap, double tx, double ty, double tz) {
      ke += -0.5 * lap;
      if (NS > 0) {
#pragma unroll
        for (int j = 0; j < NR; ++j) {
          const int p = lane + 64 * j;
          if (p < P) dk[j] += -0.5 * (R[3 * P + p] + 2.0 * (tx * R[p] + ty * R[P + p] + tz * R[2 * P + p]));
        }
      }
    });
  if (!act) return;
  if (NS == 0 || lane == 0) A.ke[(size_t)k * A.W + w] = ke;
  if (NS > 0) {
    double* d = A.dke + ((size_t)k * A.Wc + bw) * P;
#pragma unroll
    for (int j = 0; j < NR; ++j) {
      const int p = lane + 64 * j;
      if (p < P) d[p] = dk[j];
    }
  }
}

// mean[k] = 1/n sum_{w0 <= w < w0 + n} (eoff[w] + ke[k][w]): one block per set.
__global__ __launch_bounds__(256) void k_var_mean(const double* __restrict__ ke, const double* __restrict__ eoff, long W, long w0, long n,
                                                  double* __restrict__ mean) {
  __shared__ double sh[256];
  const int k = blockIdx.x;
  const double* kk = ke + (size_t)k * W;
  double s = 0.0;
  for (long w = w0 + threadIdx.x; w < w0 + n; w += 256) s += eoff[w] + kk[w];
  s = block_sum256(s, sh);
  if (threadIdx.x == 0) mean[k] = s / (double)n;
}

// var[k] = 1/W sum_w (eoff[w] + ke[k][w] - mean[k])^2 (mean of all walkers, k_var_mean): one block per set.
__global__ __launch_bounds__(256) void k_var_var(const double* __restrict__ ke, const double* __restrict__ eoff, long W,
                                                 const double* __restrict__ mean, double* __restrict__ var) {
  __shared__ double sh[256];
  const int k = blockIdx.x;
  const double* kk = ke + (size_t)k * W;
  const double m = mean[k];
  double s = 0.0;
  for (long w = threadIdx.x; w < W; w += 256) {
    const double d = eoff[w] + kk[w] - m;
    s += d * d;
  }
  s = block_sum256(s, sh);
  if (threadIdx.x == 0) var[k] = s / (double)W;
}

// Partial sums of one chunk (walkers w0 .. w0 + Wc): block (p tile, walker block b, set k) sums its kVarWB walkers in order,
// part[k][b][0][p] = sum_w d_w[p], part[k][b][1][p] = sum_w (E_w - m_c[k]) d_w[p].
__global__ __launch_bounds__(64) void k_var_dpart(const double* __restrict__ dke, const double* __restrict__ ke,
                                                  const double* __restrict__ eoff, const double* __restrict__ mc, long W, long w0, long Wc,
                                                  int P, double* __restrict__ part) {
  const int p = blockIdx.x * 64 + threadIdx.x, b = blockIdx.y, k = blockIdx.z, nb = gridDim.y;
  if (p >= P) return;
  const double m = mc[k];
  const double* kk = ke + (size_t)k * W + w0;
  const double* ek = eoff + w0;
  const double* d = dke + (size_t)k * Wc * P + p;
  double a = 0.0, c = 0.0;
  const long wb = (long)(b + 1) * kVarWB, wend = wb < Wc ? wb : Wc;
  for (long w = (long)b * kVarWB; w < wend; ++w) {
    const double v = d[(size_t)w * P];
    a += v;
    c += (ek[w] + kk[w] - m) * v;
  }
  double* o = part + ((size_t)k * nb + b) * 2 * P + p;
  o[0] = a;
  o[P] = c;
}

// The chunk's partials summed over its walker blocks in order -> ab[k][0 / 1][p] (A_c, B_c).
__global__ __launch_bounds__(64) void k_var_dchunk(const double* __restrict__ part, int nb, int P, double* __restrict__ ab) {
  const int p = blockIdx.x * 64 + threadIdx.x, k = blockIdx.y;
  if (p >= P) return;
  double a = 0.0, c = 0.0;
  for (int b = 0; b < nb; ++b) {
    const double* o = part + ((size_t)k * nb + b) * 2 * P + p;
    a += o[0];
    c += o[P];
  }
  ab[(size_t)k * 2 * P + p] = a;
  ab[((size_t)k * 2 + 1) * P + p] = c;
}

// dvar[k][p] = 2/W sum_c (B_c + (m_c - Ebar) A_c), chunks in order.  ab: [nc][K][2][P], mc: [nc][K], mean: Ebar [K].
__global__ __launch_bounds__(64) void k_var_dvar(const double* __restrict__ ab, const double* __restrict__ mc, const double* __restrict__ mean,
                                                 int nc, int K, int P, long W, double* __restrict__ dvar) {
  const int p = blockIdx.x * 64 + threadIdx.x, k = blockIdx.y;
  if (p >= P) return;
  const double m = mean[k];
  double s = 0.0;
  for (int c = 0; c < nc; ++c) {
    const double* o = ab + ((size_t)c * K + k) * 2 * P + p;
    s += o[P] + (mc[(size_t)c * K + k] - m) * o[0];
  }
  dvar[(size_t)k * P + p] = 2.0 * s / (double)W;
}

template <bool PBC>
void launch_var_ke(pqa_handle* h, dim3 g, size_t lds, int ns, const VarArgs& A) {
#define PQA_VK(NS) hipLaunchKernelGGL((k_var_ke<PBC, NS>), g, dim3(64), lds, h->stream, h->S, h->st, h->js, A)
  switch (ns) {
    case 0: PQA_VK(0); break;
    case 4: PQA_VK(4); break;
    case 8: PQA_VK(8); break;
    case 16: PQA_VK(16); break;
    default: PQA_VK(32); break;
  }
#undef PQA_VK
}

}  // namespace

extern "C" int pqa_variance(pqa_handle_t* h, int K, const double* acoeff, const double* bcoeff, const double* eoff, double* ke, double* var,
                            double* dvar) {
  HIPCHK(hipSetDevice(h->device));
  if (h->W == 0) FAIL("state not initialised (call pqa_wf_recompute)");
  if (K < 1) FAIL("pqa_variance: K must be at least 1");
  if (!acoeff || !bcoeff || !eoff || !var) FAIL("pqa_variance: acoeff, bcoeff, eoff and var must not be NULL");
  TRY(linear_jastrow_scope(h, "pqa_variance"));
  const long W = h->W;
  const int Pa = h->natom * h->na * 2, Pb = h->nb * 3, P = Pa + Pb;
  const bool grad = dvar != nullptr;
  const int ns = !grad ? 0 : P <= 256 ? 4 : P <= 512 ? 8 : P <= 1024 ? 16 : 32;
  TRY(sync_aos(h));  // (the walker-major coordinates and orbital rows the kernel reads)
  std::vector<double> ca((size_t)K * Pa), cb((size_t)K * Pb);
  HIPCHK(hipStreamSynchronize(h->stream));
  if (Pa) HIPCHK(hipMemcpy(ca.data(), acoeff, ca.size() * sizeof(double), hipMemcpyDefault));
  if (Pb) HIPCHK(hipMemcpy(cb.data(), bcoeff, cb.size() * sizeof(double), hipMemcpyDefault));
  const std::vector<double> ct = pack_coef_sets(ca.data(), cb.data(), K, Pa, Pb);
  // walker chunks: only the per-walker derivatives [K][Wc][P] scale with them
  const long Wc = grad ? walker_chunk(W, (size_t)K * P * sizeof(double)) : W;
  const int nc = (int)((W + Wc - 1) / Wc), nwb = (int)((Wc + kVarWB - 1) / kVarWB);
  // device scratch (b_out is sized by every user on entry): [P][K], eoff, ke [K][W], mean [K], var [K], chunk means [nc][K];
  // with the gradient: derivatives [K][Wc][P], partials [K][nwb][2][P], chunk sums [nc][K][2][P], dvar [K][P]
  const size_t nct = (size_t)P * K, nke = (size_t)K * W, nd = grad ? (size_t)K * Wc * P : 0, npart = grad ? (size_t)K * nwb * 2 * P : 0,
               nab = grad ? (size_t)nc * K * 2 * P : 0, ndv = grad ? (size_t)K * P : 0;
  TRY(ensure(h, h->b_out, (nct + W + nke + 2 * (size_t)K + (size_t)nc * K + nd + npart + nab + ndv) * sizeof(double)));
  double* d_ct = (double*)h->b_out.p;
  double* d_eoff = d_ct + nct;
  double* d_ke = d_eoff + W;
  double* d_mean = d_ke + nke;
  double* d_var = d_mean + K;
  double* d_mc = d_var + K;
  double* d_dke = d_mc + (size_t)nc * K;
  double* d_part = d_dke + nd;
  double* d_ab = d_part + npart;
  double* d_dvar = d_ab + nab;
  TRY(copy_in(h, d_ct, ct.data(), nct * sizeof(double)));
  TRY(copy_in(h, d_eoff, eoff, (size_t)W * sizeof(double)));
  VarArgs A{};
  A.W = W; A.K = K; A.P = P; A.Pa = Pa; A.ct = d_ct; A.ke = d_ke; A.dke = d_dke;
  const size_t lds = (size_t)4 * P * sizeof(double);
  const unsigned pt = (unsigned)((P + 63) / 64);
  for (int c = 0; c < nc; ++c) {
    A.w0 = (long)c * Wc; A.Wc = std::min(Wc, W - A.w0);
    const dim3 g((unsigned)A.Wc, grad ? (unsigned)K : (unsigned)((K + 63) / 64));
    if (h->S.pbc) launch_var_ke<true>(h, g, lds, ns, A);
    else launch_var_ke<false>(h, g, lds, ns, A);
    TRY(check_launch(h, "k_var_ke"));
    if (!grad) continue;
    const int nb = (int)((A.Wc + kVarWB - 1) / kVarWB);
    double* mc = d_mc + (size_t)c * K;
    hipLaunchKernelGGL(k_var_mean, dim3((unsigned)K), dim3(256), 0, h->stream, (const double*)d_ke, (const double*)d_eoff, W, A.w0, A.Wc, mc);
    hipLaunchKernelGGL(k_var_dpart, dim3(pt, (unsigned)nb, (unsigned)K), dim3(64), 0, h->stream, (const double*)d_dke, (const double*)d_ke,
                       (const double*)d_eoff, (const double*)mc, W, A.w0, A.Wc, P, d_part);
    hipLaunchKernelGGL(k_var_dchunk, dim3(pt, (unsigned)K), dim3(64), 0, h->stream, (const double*)d_part, nb, P, d_ab + (size_t)c * K * 2 * P);
    TRY(check_launch(h, "k_var_dchunk"));
  }
  hipLaunchKernelGGL(k_var_mean, dim3((unsigned)K), dim3(256), 0, h->stream, (const double*)d_ke, (const double*)d_eoff, W, 0L, W, d_mean);
  hipLaunchKernelGGL(k_var_var, dim3((unsigned)K), dim3(256), 0, h->stream, (const double*)d_ke, (const double*)d_eoff, W,
                     (const double*)d_mean, d_var);
  TRY(check_launch(h, "k_var_var"));
  if (grad) {
    hipLaunchKernelGGL(k_var_dvar, dim3(pt, (unsigned)K), dim3(64), 0, h->stream, (const double*)d_ab, (const double*)d_mc,
                       (const double*)d_mean, nc, K, P, W, d_dvar);
    TRY(check_launch(h, "k_var_dvar"));
    TRY(copy_in(h, dvar, d_dvar, ndv * sizeof(double)));
  }
  if (ke) TRY(copy_in(h, ke, d_ke, nke * sizeof(double)));
  return copy_out(h, var, d_var, (size_t)K * sizeof(double));
}
