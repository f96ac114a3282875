// v_mfma_f64_4x4x4_4b_f64 on gfx950 (round 8): the four-block 4x4x4 form beside the 16x16x4 form the contraction of k_sweep_r8 uses.
//   (a) layout: one instruction on small integer operands, the result compared EXACTLY with a host product under every assignment of the
//       three 2-bit lane fields (lane & 3, (lane >> 2) & 3, lane >> 4) to (row / column, k, block) of A, of B and of D;
//   (b) issue rate (s_memtime ticks and wall time per instruction): 4x4x4 with 1, 2, 4 accumulators, 16x16x4 with 1, 3 accumulators, and
//       the two k-step patterns of the contraction — three 16x16x4 against two 16x16x4 plus two 4x4x4 — each with 1 and 2 waves per SIMD.
// Build: hipcc --offload-arch=gfx950 -O3 tools/scratch/mfma4_probe.hip -o tools/scratch/bin/mfma4_probe ; run on the GPU box.
#include <hip/hip_runtime.h>
#include <cstdio>
#include <cstdlib>
#include <vector>
typedef double d4 __attribute__((ext_vector_type(4)));

__global__ void k_layout(const double* a, const double* b, double* d) {
  const int lane = threadIdx.x;
  d[lane] = __builtin_amdgcn_mfma_f64_4x4x4f64(a[lane], b[lane], 0.0, 0, 0, 0);
}

// N16 accumulators of the 16x16x4 form and N4 of the 4x4x4 form per iteration, all independent of each other
template <int N16, int N4>
__global__ void k_rate(double* out, unsigned long long* cyc, int iters) {
  d4 acc[N16 > 0 ? N16 : 1];
  double s4[N4 > 0 ? N4 : 1];
  for (int i = 0; i < (N16 > 0 ? N16 : 1); ++i) acc[i] = (d4){0, 0, 0, 0};
  for (int i = 0; i < (N4 > 0 ? N4 : 1); ++i) s4[i] = 0.0;
  const double a = threadIdx.x * 1e-3 + 1.0, b = blockIdx.x * 1e-3 + 1.0;
  const unsigned long long t0 = __builtin_readcyclecounter();
  for (int it = 0; it < iters; ++it) {
#pragma unroll
    for (int i = 0; i < N16; ++i) acc[i] = __builtin_amdgcn_mfma_f64_16x16x4f64(a, b, acc[i], 0, 0, 0);
#pragma unroll
    for (int i = 0; i < N4; ++i) s4[i] = __builtin_amdgcn_mfma_f64_4x4x4f64(a, b, s4[i], 0, 0, 0);
  }
  const unsigned long long t1 = __builtin_readcyclecounter();
  double s = 0;
  for (int i = 0; i < N16; ++i) s += acc[i][0] + acc[i][1] + acc[i][2] + acc[i][3];
  for (int i = 0; i < N4; ++i) s += s4[i];
  out[blockIdx.x * blockDim.x + threadIdx.x] = s;
  if (threadIdx.x == 0) cyc[blockIdx.x] = t1 - t0;
}

template <class K>
static void run(const char* name, K kern, int threads, int iters, double* out, unsigned long long* cyc) {
  const size_t lds = 100 * 1024;  // one block per CU
  hipFuncSetAttribute((const void*)kern, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024);
  hipEvent_t e0, e1; hipEventCreate(&e0); hipEventCreate(&e1);
  hipLaunchKernelGGL(kern, dim3(256), dim3(threads), lds, 0, out, cyc, iters);
  hipDeviceSynchronize();
  hipEventRecord(e0);
  hipLaunchKernelGGL(kern, dim3(256), dim3(threads), lds, 0, out, cyc, iters);
  hipEventRecord(e1); hipEventSynchronize(e1);
  float ms; hipEventElapsedTime(&ms, e0, e1);
  std::vector<unsigned long long> h(256);
  hipMemcpy(h.data(), cyc, 256 * 8, hipMemcpyDeviceToHost);
  double c = 0; for (auto v : h) c += (double)v; c /= 256;
  printf("%-52s %8.3f ms  %.2f ns per iteration per wave, %.2f ticks\n", name, ms, 1e6 * ms / iters, c / iters);
}

static const char* FN[3] = {"lane&3", "(lane>>2)&3", "lane>>4"};
int main() {
  // ---- (a) layout
  double *da, *db, *dd;
  hipMalloc(&da, 64 * 8); hipMalloc(&db, 64 * 8); hipMalloc(&dd, 64 * 8);
  const int perm[6][3] = {{0, 1, 2}, {0, 2, 1}, {1, 0, 2}, {1, 2, 0}, {2, 0, 1}, {2, 1, 0}};  // fields of (index, k, block) / (i, j, block)
  std::vector<int> alive(216, 1);
  srand(12345);
  for (int trial = 0; trial < 4; ++trial) {
    double ha[64], hb[64], hd[64];
    for (int l = 0; l < 64; ++l) { ha[l] = rand() % 17 - 8; hb[l] = rand() % 19 - 9; }
    hipMemcpy(da, ha, 512, hipMemcpyHostToDevice); hipMemcpy(db, hb, 512, hipMemcpyHostToDevice);
    hipLaunchKernelGGL(k_layout, dim3(1), dim3(64), 0, 0, da, db, dd);
    hipMemcpy(hd, dd, 512, hipMemcpyDeviceToHost);
    for (int pa = 0; pa < 6; ++pa) for (int pb = 0; pb < 6; ++pb) for (int pd = 0; pd < 6; ++pd) {
      auto at = [](const int* p, int x, int y, int blk) { return (x << (2 * p[0])) | (y << (2 * p[1])) | (blk << (2 * p[2])); };
      bool ok = true;
      for (int blk = 0; blk < 4 && ok; ++blk) for (int i = 0; i < 4 && ok; ++i) for (int j = 0; j < 4; ++j) {
        double s = 0;
        for (int k = 0; k < 4; ++k) s += ha[at(perm[pa], i, k, blk)] * hb[at(perm[pb], j, k, blk)];
        if (s != hd[at(perm[pd], i, j, blk)]) { ok = false; break; }
      }
      if (!ok) alive[(pa * 6 + pb) * 6 + pd] = 0;
    }
  }
  int nalive = 0;
  for (int c = 0; c < 216; ++c) if (alive[c]) {
    const int *pa = perm[c / 36], *pb = perm[(c / 6) % 6], *pd = perm[c % 6];
    ++nalive;
    printf("layout: A[blk][i][k] in lane with i = %s, k = %s, blk = %s;  B[blk][k][j]: j = %s, k = %s, blk = %s;  D[blk][i][j]: i = %s, j = %s, blk = %s\n",
           FN[pa[0]], FN[pa[1]], FN[pa[2]], FN[pb[0]], FN[pb[1]], FN[pb[2]], FN[pd[0]], FN[pd[1]], FN[pd[2]]);
  }
  printf("layout: %d of 216 field assignments reproduce the host product exactly in 4 trials of integer operands\n", nalive);

  // ---- (b) issue rate
  double* out; unsigned long long* cyc;
  hipMalloc(&out, 256 * 1024 * 8); hipMalloc(&cyc, 256 * 8);
  const int it = 20000;
#define R(N16, N4, T, nm) run(nm, k_rate<N16, N4>, T, it, out, cyc)
  R(1, 0, 256, "16x16x4 x1, 1 wave/SIMD");
  R(3, 0, 256, "16x16x4 x3, 1 wave/SIMD");
  R(0, 1, 256, "4x4x4 x1, 1 wave/SIMD");
  R(0, 2, 256, "4x4x4 x2, 1 wave/SIMD");
  R(0, 4, 256, "4x4x4 x4, 1 wave/SIMD");
  R(2, 2, 256, "16x16x4 x2 + 4x4x4 x2, 1 wave/SIMD");
  R(2, 0, 256, "16x16x4 x2, 1 wave/SIMD");
  R(1, 0, 512, "16x16x4 x1, 2 waves/SIMD");
  R(3, 0, 512, "16x16x4 x3, 2 waves/SIMD");
  R(0, 1, 512, "4x4x4 x1, 2 waves/SIMD");
  R(0, 2, 512, "4x4x4 x2, 2 waves/SIMD");
  R(0, 4, 512, "4x4x4 x4, 2 waves/SIMD");
  R(2, 2, 512, "16x16x4 x2 + 4x4x4 x2, 2 waves/SIMD");
  R(2, 0, 512, "16x16x4 x2, 2 waves/SIMD");
  return 0;
}
